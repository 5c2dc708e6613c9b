// rpkt_chain.h — device code of the parse over rpkt-dpdk's Pbuf (mbuf chains), shared by
// rpkt_parse.hip (rpkt_gpu_parse_chains) and rpkt_tunnel_chains.hip
// (rpkt_gpu_parse_tunnel_chains): the segment source, ChainView (the chain model of
// rpkt_common.h's view concept: chunk() at a logical cursor, the dword reader over segment
// 0's window), the lane-per-chain parse and the flattened (chain, segment) checksum stream.
#pragma once
#include "rpkt_common.h"

namespace {

// ---- mbuf chains: the same parse over rpkt-dpdk's Pbuf ----
// A chain is a list of (offset, data_len) segments of one arena.  Over a Pbuf the
// generic views test header sizes against chunk(), the rest of the segment that holds
// the header's first byte (pbuf.rs:48-57, 86-96), and totals against remaining()
// (pbuf.rs:98-101); trim_off cuts the packet end (pbuf.rs:117-140).  Segment 0 is
// windowed into LDS like a frame, so every header that starts inside it is parsed by
// the window path; a header that starts exactly at segment 0's end (the only way
// past it) is read from global memory byte-wise on a rare path.  The L4 bytes past
// the window are summed by the flattened chunk stream over (chain, segment) items,
// each item's sum brought to segment 0's byte phase before it is added.
struct ChainSrc {
    const uint2* segs;
    uint32_t fb;
    __device__ __forceinline__ Frame seg(uint32_t k) const {
        const uint2 v = segs[k];
        const uint32_t off = v.x < fb ? v.x : fb;
        const uint32_t len = v.y < fb - off ? v.y : fb - off;
        return Frame{off, len};
    }
};

// checksum::from_slice over n bytes at absolute `a` (rpkt/src/checksum.rs:33-62)
__device__ __forceinline__ uint32_t gsum_be(__amdgpu_buffer_rsrc_t rs, uint32_t a, uint32_t n) {
    uint32_t acc = 0, k = 0;
    for (; k + 1 < n; k += 2) acc += (gbyte(rs, a + k) << 8) | gbyte(rs, a + k + 1);
    if (k < n) acc += gbyte(rs, a + k) << 8;
    return fold16(acc);
}

// Chunk at logical cursor c > 0 of segments [a, b) under the packet end `limit`: the
// rest of the first segment whose end passes c (empty segments skipped, as
// advance_common walks), cut at limit.  `abs` = the chunk's first byte.
__device__ __forceinline__ uint32_t chain_chunk(const ChainSrc& S, uint32_t a, uint32_t b,
                                                uint32_t c, uint32_t limit, uint32_t& abs) {
    uint32_t cum = 0;
    for (uint32_t k = a; k < b; ++k) {
        const Frame s = S.seg(k);
        const uint32_t end = cum + s.len;
        if (end > c) {
            abs = s.off + (c - cum);
            return (end < limit ? end : limit) - c;
        }
        cum = end;
    }
    abs = S.fb;
    return 0;
}

// Chain bytes at absolute a..a+3 as a little-endian dword: from segment 0's LDS window
// when they lie in its windowed part (frame bytes [0, lim) of segment 0), else byte-wise
// from global memory.  A header lies inside the chunk it was tested against, i.e. in one
// segment, so its bytes are at consecutive absolute addresses.
struct ChainDw {
    const uint8_t* slot;
    uint32_t ph, off0, lim;
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ uint32_t operator()(uint32_t a) const {
        const uint32_t x = a - off0;                           // wraps for other segments
        if (x < lim && lim - x >= 4u) {
            const uint32_t y = ph + x, q = y & ~3u;
            return align_bytes(lds32(slot, q + 4), lds32(slot, q), y & 3u);
        }
        return gbyte(rs, a) | (gbyte(rs, a + 1) << 8) | (gbyte(rs, a + 2) << 16) |
               (gbyte(rs, a + 3) << 24);
    }
};

// The lane's chain as a Pbuf: the chain model of the view concept (rpkt_common.h).  chunk()
// at logical cursor c under the packet end lim (the trim of the views above it): below
// segment 0's end C the rest of segment 0; past it chain_chunk walks the segments (empty
// ones skipped, as advance_common).  at = the absolute address of the chunk's first byte
// (fb, where every load returns 0, when the chunk is empty); d reads there.
struct ChainView {
    ChainSrc S;
    uint32_t a, b, C;
    ChainDw d;
    __device__ __forceinline__ uint32_t chunk(uint32_t c, uint32_t lim, uint32_t& at) const {
        at = S.fb;
        if (c >= lim) return 0u;
        if (c < C) {
            at = d.off0 + c;
            return (C < lim ? C : lim) - c;
        }
        return chain_chunk(S, a, b, c, lim, at);
    }
    __device__ __forceinline__ uint32_t dw(uint32_t at) const { return d(at); }
    template <int N>
    __device__ __forceinline__ void read_words(uint32_t at, uint32_t (&F)[N]) const {
#pragma unroll
        for (int k = 0; k < N; ++k) F[k] = d(at + 4u * k);
    }
};

// The view of the lane's chain [a, b) whose segment 0 (s0) is in the lane's window slot.
__device__ __forceinline__ ChainView chain_view(const WaveScratch& W, int lane, Frame s0,
                                                const ChainSrc& S, uint32_t a, uint32_t b,
                                                __amdgpu_buffer_rsrc_t rs) {
    const uint32_t ph = s0.off & 15u, wl = (uint32_t)kWin - ph;
    return ChainView{S, a, b, s0.len,
                     ChainDw{&W.win[lane * kSlot], ph, s0.off, s0.len < wl ? s0.len : wl, rs}};
}

// Lane-per-chain parse: parse_lane with the chunk/remaining distinction of a Pbuf.
// C = segment 0's length: headers starting below C are read from the LDS window.
__device__ __forceinline__ void parse_chain_lane(const WaveScratch& W, int lane, Frame s0,
                                                 uint32_t pkt, const ChainSrc& S, uint32_t a,
                                                 uint32_t b, __amdgpu_buffer_rsrc_t rs,
                                                 uint32_t flags, LaneRec& L) {
    const uint32_t ph = s0.off & 15u;
    const uint8_t* slot = &W.win[lane * kSlot];
    uint32_t* w = L.w;
#pragma unroll
    for (int k = 0; k < 20; ++k) w[k] = 0;
    const uint32_t C = s0.len;                                 // Pbuf::new, pbuf.rs:19-34
    L.stream_s = L.stream_e = L.l4_part = L.l4_start_abs = L.pseudo = 0;
    L.want_l4 = false;
    L.is6 = false;
    w[19] = pkt;
    uint32_t status = RPKT_S_OK;

    uint32_t E[6];
    {
        const uint32_t a0 = ph & ~3u, sh = ph & 3u;
        uint32_t R[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) R[k] = lds32(slot, a0 + 4 * k);
#pragma unroll
        for (int k = 0; k < 6; ++k) E[k] = align_bytes(R[k + 1], R[k], sh);
    }
    if (C < 14) {                                              // ether/generated.rs:36
        L.status = RPKT_S_ETH_SHORT;
        w[0] = RPKT_S_ETH_SHORT;
        return;
    }
    w[1] = E[0];
    w[2] = E[1];
    w[3] = E[2];
    const uint32_t eth_et = be16_lo(E[3]);
    uint32_t nvlan = 0, et = eth_et, c = 14;
#pragma unroll
    for (int v = 0; v < RPKT_MAX_VLAN; ++v) {                  // vlan/generated.rs:32-61
        if (!is_tag(et)) break;
        uint32_t T = 0, ck = 0;
        if (c < C) {
            ck = C - c;
            T = v == 0 ? align_bytes(E[4], E[3], 2) : align_bytes(E[5], E[4], 2);
        } else if (c < pkt) {
            uint32_t ab;
            ck = chain_chunk(S, a, b, c, pkt, ab);
            T = gbyte(rs, ab) | (gbyte(rs, ab + 1) << 8) | (gbyte(rs, ab + 2) << 16) |
                (gbyte(rs, ab + 3) << 24);
        }
        if (ck < 4) {
            status = RPKT_S_VLAN_SHORT;
            break;
        }
        et = be16_hi(T);
        w[4] |= be16_lo(T) << (16 * v);
        w[5] |= et << (16 * v);
        nvlan += 1;
        c += 4;
    }
    w[0] = (nvlan << 8) | (eth_et << 16);
    const bool v6 = (flags & RPKT_F_IPV6) && status == RPKT_S_OK && et == 0x86ddu;
    if (status == RPKT_S_OK && et != 0x0800u && !v6) status = RPKT_S_NOT_IPV4;
    if (status != RPKT_S_OK) {
        w[0] |= status;
        L.status = status;
        return;
    }

    const uint32_t l3 = c;
    w[16] = l3;
    uint32_t l4, limit, l4rem, proto, paddr;
    if (v6) {
        L.is6 = true;
        status = parse_ip6(chain_view(W, lane, s0, S, a, b, rs), l3, pkt, w, l4, l4rem, proto,
                           paddr);
        if (status != RPKT_S_IP6_SHORT && status != RPKT_S_IP6_BAD_LEN) {
            w[16] |= l4 << 16;
            w[17] = (l4 & 0xffffu) | (l4rem << 16);
        }
        if (status != RPKT_S_OK) {
            w[0] |= status;
            L.status = status;
            return;
        }
        limit = l4 + l4rem;
    } else {
        // Ipv4::parse (ip4_rules): chunk vs remaining
        Hdr6 ip;
        uint32_t ck3 = 0, ab3 = 0;
        const bool fast3 = l3 < C;
        if (fast3) {
            ck3 = C - l3;
            read_hdr(slot, ph + l3, ip);
        } else {
            if (l3 < pkt) ck3 = chain_chunk(S, a, b, l3, pkt, ab3);
            gread20(rs, S.fb, ck3 ? ab3 : S.fb, ip.F);
        }
        const Ip4Out o = ip4_rules(ip.F, ck3, pkt - l3, w);
        status = o.status;
        if (status != RPKT_S_OK) {
            w[0] |= status;
            L.status = status;
            return;
        }
        if (flags & RPKT_F_IP_SUM)
            w[18] = fast3 ? be_sum(raw_range_sum(slot, ip.R, ip.a0, ph + l3, ph + l3 + o.ihl4),
                                   s0.off + l3)
                          : gsum_be(rs, ab3, o.ihl4);
        l4 = l3 + o.ihl4;                                      // Ipv4::payload :115-127
        limit = l3 + o.tot;
        l4rem = o.tot - o.ihl4;
        w[16] |= l4 << 16;
        w[17] = l4 | (l4rem << 16);
        proto = o.proto;
        paddr = o.paddr;
    }

    // Udp::parse / Tcp::parse (l4_rules) against the chunk at l4 under the trimmed end (an
    // IPv6 L4 header past segment 0's window is read from global memory)
    Hdr6 h4;
    uint32_t ck4 = 0, ab4 = 0;
    const bool fast4 = l4 < C && ph + l4 + 20u <= (uint32_t)kWin;
    if (fast4) {
        ck4 = (C < limit ? C : limit) - l4;
        read_hdr(slot, ph + l4, h4);
    } else {
        if (l4 < limit) ck4 = chain_chunk(S, a, b, l4, limit, ab4);
        gread20(rs, S.fb, ck4 ? ab4 : S.fb, h4.F);
    }
    const L4Out r4 = l4_rules(h4.F, ck4, l4rem, proto, v6, l4, w);
    status = r4.status;
    const uint32_t l4len = r4.l4len;
    const bool other_sum = r4.other_sum;
    w[0] |= status;
    L.status = status;
    if ((status == RPKT_S_OK || other_sum) && (flags & RPKT_F_L4_SUM)) {
        L.want_l4 = true;
        L.pseudo = other_sum ? 0u : paddr + proto + l4len;
        const uint32_t e = l4 + l4len;
        L.l4_start_abs = s0.off + l4;                          // segment 0's byte phase
        if (fast4) {
            const uint32_t win_end = kWin - ph;
            uint32_t e_in = e < win_end ? e : win_end;
            e_in = e_in < C ? e_in : C;
            L.l4_part = raw_range_sum(slot, h4.R, h4.a0, ph + l4, ph + e_in);
            L.stream_s = e_in;
        } else {
            L.stream_s = l4;
        }
        L.stream_e = e;                                        // logical, not absolute
    }
}

// Sum of the logical range [ss, se) of this lane's chain, in segment 0's byte phase,
// for every lane of the wave.  Items (chain, segment intersecting its range) are
// flattened in chain order; each round streams 64 of them with wave_stream_sum.
// An item's logical start is its owner's running cursor plus a segmented prefix sum
// of the round's segment lengths.  Scratch: the window area past the staged records
// (dwords [0, 513) of it; the caller keeps per-lane values at [513, 705)).
__device__ __forceinline__ uint32_t chain_stream(WaveScratch& W, __amdgpu_buffer_rsrc_t rs,
                                                 uint32_t fb, const ChainSrc& S, uint32_t a,
                                                 uint32_t b, uint32_t off0, uint32_t ss,
                                                 uint32_t se, int lane) {
    uint32_t k = 0, fi = 0, ls0 = 0;
    if (se > ss) {
        uint32_t cum = 0;
        for (uint32_t j = a; j < b; ++j) {
            const uint32_t len = S.seg(j).len;
            if (cum + len > ss && cum < se) {
                if (k == 0) {
                    fi = j;
                    ls0 = cum;
                }
                ++k;
            }
            cum += len;
            if (cum >= se) break;
        }
    }
    const uint32_t incl = wave_incl_scan(k);
    const uint32_t T = __builtin_amdgcn_readlane(incl, 63);
    if (T == 0) return 0;                                      // wave-uniform
    uint32_t* X = rec_stage(W) + kWave * 21;
    uint32_t* cb = X;                  // [65] first item of each lane
    uint32_t* cfi = X + 65;            // first segment index
    uint32_t* ccum = X + 129;          // logical start of the lane's next item
    uint32_t* css = X + 193;
    uint32_t* cse = X + 257;
    uint32_t* cacc = X + 321;
    uint32_t* citem = X + 385;         // [128] per-item state held over the stream
    cb[lane] = incl - k;
    if (lane == 63) cb[64] = incl;
    cfi[lane] = fi | (off0 << 31);     // segment 0's byte parity in bit 31
    ccum[lane] = ls0;
    css[lane] = ss;
    cse[lane] = se;
    cacc[lane] = 0;
    wave_sync();
    for (uint32_t r0 = 0; r0 < T; r0 += kWave) {
        const uint32_t g = r0 + lane;
        const bool v = g < T;
        uint32_t q = 0;
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1)
            if (cb[q + step] <= g) q += step;
        const uint32_t bq = cb[q];
        const uint32_t t = g - bq;
        const uint32_t fq = cfi[q];
        const Frame sg = v ? S.seg((fq & 0x7fffffffu) + t) : Frame{0, 0};
        const uint32_t x = sg.len;
        const uint32_t inc = wave_incl_scan(x);
        const uint32_t j0 = (bq > r0 ? bq : r0) - r0;          // owner's first lane this round
        const uint32_t base = (uint32_t)__shfl((int)(inc - x), (int)j0, kWave);
        const uint32_t ls = ccum[q] + (inc - x) - base;
        const uint32_t lo = ls > css[q] ? ls : css[q];
        const uint32_t he = ls + x, hi = he < cse[q] ? he : cse[q];
        uint32_t s_abs = 0, e_abs = 0;
        if (v && hi > lo) {
            s_abs = sg.off + (lo - ls);
            e_abs = sg.off + (hi - ls);
        }
        const uint32_t swap = ((sg.off - ls) ^ (fq >> 31)) & 1u;
        const uint32_t last = v && (lane == kWave - 1 || t + 1 == cb[q + 1] - bq);
        citem[lane] = q | (swap << 8) | (last << 9) | ((uint32_t)v << 10);   // kept in LDS
        citem[kWave + lane] = he;                                               // over the stream
        const uint32_t part = wave_stream_sum<2, kChainStreamUnroll>(rs, fb, s_abs, e_abs, W, lane);
        const uint32_t it = citem[lane];
        const uint32_t qq = it & 63u;
        if (it & (1u << 10)) {
            uint32_t c = fold16(part);
            atomicAdd(&cacc[qq], (it & (1u << 8)) ? bswap16(c) : c);
        }
        if (it & (1u << 9)) ccum[qq] = citem[kWave + lane];
        wave_sync();
    }
    return cacc[lane];
}

}  // namespace
