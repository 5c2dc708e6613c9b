// rpkt_tunnel_chains.hip — rpkt_gpu_parse_tunnel_chains: rpkt_gpu_parse_tunnel_batch's
// work (the outer parse, one VXLAN / GTP-U / GRE level, the parse of the inner frame, every
// sum of both levels) over mbuf chains, rpkt-dpdk's Pbuf (include/rpkt_gpu.h documents the
// records; tests/tunnel_chain_model.py restates the chunk()/remaining() rules on the CPU).
//
// One wavefront per 64 chains, as parse_chains_kernel: segment 0's 128-B window goes to LDS
// and each lane runs parse_chain_lane on its chain.  The lane then decodes the tunnel and
// parses the inner frame with logical cursors in the chain's bytes: every header-size test
// takes chunk() at the header's cursor under the current packet end (ChainView::chunk: the
// rest of segment 0 below its end, chain_chunk's segment walk past it), every total-length
// test takes remaining(), and header bytes come through ChainDw (LDS when they lie in
// segment 0's window, byte-wise global loads otherwise -- a header that starts past the
// window or in a later segment; there is no second inner window).  The outer record is
// staged in an LDS area of its own, the inner one in the window area, so chain_stream keeps
// its scratch.  One chain_stream pass sums the bytes the inner L4 range and the outer L4
// range (UDP, or GRE with its checksum) share; the outer range's bytes before the inner
// stream (inner headers past the window) and after the inner packet (padding, GTP trailing
// bytes) get a pass each, which returns at once when no lane of the wave has such bytes.
#include "rpkt_common.h"
#include "rpkt_args.h"
#include "rpkt_chain.h"
#include "rpkt_tunnel.h"

namespace {

// The lane's chain as a Pbuf: chunk() at logical cursor c under the packet end lim (the
// trim of the views above it).  Below segment 0's end C the chunk is the rest of segment
// 0; past it chain_chunk walks the segments (empty ones skipped, as advance_common).
// abs = the chunk's first byte (fb, where every load returns 0, when the chunk is empty).
struct ChainView {
    ChainSrc S;
    uint32_t a, b, off0, C;
    __device__ __forceinline__ uint32_t chunk(uint32_t c, uint32_t lim, uint32_t& abs) const {
        abs = S.fb;
        if (c >= lim) return 0u;
        if (c < C) {
            abs = off0 + c;
            return (C < lim ? C : lim) - c;
        }
        return chain_chunk(S, a, b, c, lim, abs);
    }
};

// decode_tunnel (rpkt_tunnel.h) over a Pbuf: the same dispatch and the same getters, with
// each parse's header-size tests against chunk() at its cursor and its total-length tests
// against remaining() (the views' own split: a header that straddles a segment boundary is
// Err there, T_BAD / T_EXT_BAD here).  ts, te, T.is, T.ie are logical positions in the chain.
__device__ __forceinline__ Tunnel decode_tunnel_chain(const LaneRec& L, const ChainDw& dw,
                                                      const ChainView& V, uint32_t flags) {
    Tunnel T;
    T.w[0] = RPKT_TUN_NONE | (RPKT_T_NONE << 8);
    T.w[1] = T.w[2] = T.w[3] = 0u;
    T.is = T.ie = T.start_et = 0u;
    T.ok = false;
    const uint32_t* w = L.w;
    const uint32_t proto = (w[8] >> 8) & 0xffu;              // ip_protocol (IPv4 and IPv6)
    uint32_t kind = RPKT_TUN_NONE, ts = 0u, te = 0u;
    if (L.status == RPKT_S_OK && proto == 17u) {
        // Udp::payload() (udp/generated.rs:66-76): [payload_off, + payload_len)
        const uint32_t dp = w[11] >> 16, sp = w[11] & 0xffffu;
        const uint32_t port = (dp == 4789u || dp == 2152u) ? dp
                            : ((sp == 4789u || sp == 2152u) ? sp : 0u);
        if (port != 0u) {
            kind = port == 4789u ? RPKT_TUN_VXLAN : RPKT_TUN_GTPU;
            ts = w[17] & 0xffffu;
            te = ts + (w[17] >> 16);
        }
    } else if (L.status == RPKT_S_L4_OTHER && proto == 47u &&
               (L.is6 || ((w[7] >> 16) & 0x1fffu) == 0u)) {
        // Ipv4|Ipv6::payload() of a first (or only) fragment: [l4_off, + payload_len)
        kind = RPKT_TUN_GRE;
        ts = w[16] >> 16;
        te = ts + (w[17] >> 16);
    }
    if (kind == RPKT_TUN_NONE) return T;
    uint32_t ab;
    const uint32_t cl = V.chunk(ts, te, ab), rm = te - ts;   // chunk().len(), remaining()
    tun_set(T, kind, RPKT_T_BAD, ts, 0u, 0u);
    if (kind == RPKT_TUN_VXLAN) {
        // Vxlan::parse (vxlan/generated.rs:32-39): chunk_len >= 8
        if (cl < 8u) return T;
        const uint32_t d0 = dw(ab), d1 = dw(ab + 4u);
        T.w[2] = bswap32(d1) >> 8;                            // vni, bytes 4..6
        T.w[3] = (d0 & 0xffffu) | (be16_hi(d0) << 16);        // flags bytes 0, 1; group_id
        tun_inner(T, kind, ts, ts + 8u, te, 0x6558u, flags);
        return T;
    }
    if (kind == RPKT_TUN_GTPU) {
        // Gtpv1::parse (gtpv1/generated.rs:33-49): chunk_len >= 8, header_len <= chunk_len,
        // header_len <= packet_len <= remaining
        if (cl < 8u) return T;
        const uint32_t d0 = dw(ab);
        const uint32_t b0 = d0 & 0xffu, msg = (d0 >> 8) & 0xffu;
        const uint32_t hl = (b0 & 7u) ? 12u : 8u;
        const uint32_t plen = be16_hi(d0) + 8u;
        if (hl > cl || plen < hl || plen > rm) return T;
        const uint32_t d2 = hl == 12u ? dw(ab + 8u) : 0u;
        T.w[2] = bswap32(dw(ab + 4u));                        // teid :74-76
        T.w[3] = (d0 & 0xffffu) | (be16_lo(d2) << 16);        // byte 0, message_type; sequence
        // payload() :98-108: trim to packet_len, advance header_len
        uint32_t c = ts + hl;
        const uint32_t end = ts + plen;
        if ((b0 >> 5) != 1u || msg != 255u) {                 // not a GTPv1 G-PDU
            tun_set(T, kind, RPKT_T_NOT_TPDU, ts, c, 0u);
            return T;
        }
        // the extension headers, each parsed against its own chunk (:336-341, :461-466,
        // :587-592, :747-752, :880-892 and the NrUp / PduSessionUp group parses)
        uint32_t nx = (b0 & 4u) ? (d2 >> 24) : 0u;
        for (int k = 0; k < RPKT_MAX_GTP_EXT && nx != 0u; ++k) {
            uint32_t ax;
            const uint32_t rem = V.chunk(c, end, ax), x = dw(ax);
            const uint32_t e0 = x & 0xffu, t = (x >> 12) & 0xfu;
            uint32_t need, mn, ehl;
            if (nx == 0x40u || nx == 0xc0u || nx == 0x20u) {
                need = 4u; mn = 4u; ehl = 4u;
            } else if (nx == 0x03u || nx == 0x82u) {
                need = 8u; mn = 8u; ehl = 8u;
            } else if (nx == 0x81u || nx == 0x83u) {
                need = 1u; mn = 1u; ehl = e0 * 4u;
            } else if (nx == 0x84u && t <= 2u) {
                need = 2u; mn = t == 0u ? 6u : (t == 1u ? 7u : 3u); ehl = e0 * 4u;
            } else if (nx == 0x85u && t <= 1u) {
                need = 2u; mn = 3u; ehl = e0 * 4u;
            } else {
                need = ~0u; mn = 0u; ehl = 0u;                // unknown type / group Err
            }
            if (rem < need || rem < mn || ehl < mn || ehl > rem) {
                tun_set(T, kind, RPKT_T_EXT_BAD, ts, c, 0u);
                return T;
            }
            nx = dw(ax + ehl - 1u) & 0xffu;                   // next_extention_header: last byte
            c += ehl;
        }
        if (nx != 0u) {
            tun_set(T, kind, RPKT_T_EXT_BAD, ts, c, 0u);
            return T;
        }
        // the T-PDU: Ipv4 / Ipv6 by the version nibble of the cursor's first byte
        uint32_t ax;
        const uint32_t v = V.chunk(c, end, ax) ? (dw(ax) >> 4) & 0xfu : 0u;
        tun_inner(T, kind, ts, c, end, v == 4u ? 0x0800u : (v == 6u ? 0x86ddu : 0u), flags);
        return T;
    }
    // GreGroup::group_parse (gre/generated.rs:800-820): chunk >= 4; GreForPPTP::parse
    // (:371-386): chunk >= 8, header_len <= chunk, payload_len + header_len <= remaining;
    // Gre::parse (:33-44): header_len in [4, chunk]
    if (cl < 4u) return T;
    const uint32_t d0 = dw(ab);
    const uint32_t b0 = d0 & 0xffu, b1 = (d0 >> 8) & 0xffu, pt = be16_hi(d0), ver = b1 & 7u;
    if ((b0 & 0xe0u) == 0x20u && ver == 1u && pt == 0x880bu) {
        if (cl < 8u) return T;
        const uint32_t d1 = dw(ab + 4u);
        const uint32_t phl = 8u + ((b0 & 0x10u) ? 4u : 0u) + ((b1 & 0x80u) ? 4u : 0u);
        if (phl > cl || be16_lo(d1) + phl > rm) return T;
        T.w[2] = bswap32(d1);                                 // payload_len, call_id
        T.w[3] = d0 & 0xffffu;
        tun_set(T, kind, RPKT_T_INNER_UNKNOWN, ts, ts + phl, pt);   // PPP, not IP
        return T;
    }
    if (ver != 0u) return T;
    const uint32_t cr = (b0 & 0xc0u) ? 4u : 0u;
    const uint32_t hl = 4u + cr + ((b0 & 0x20u) ? 4u : 0u) + ((b0 & 0x10u) ? 4u : 0u);
    if (hl > cl) return T;
    T.w[3] = (d0 & 0xffffu) | (cr ? be16_lo(dw(ab + 4u)) << 16 : 0u);   // checksum :236-241
    if (b0 & 0x20u) T.w[2] = bswap32(dw(ab + 4u + cr));        // key :260-267
    tun_inner(T, kind, ts, ts + hl, te, pt, flags);           // payload() advance header_len
    return T;
}

// Big-endian sum of the n <= chunk bytes of a header at absolute `ab`: from segment 0's
// window when they lie in it, else byte-wise (gsum_be).
__device__ __forceinline__ uint32_t header_sum(const ChainDw& dw, uint32_t ab, uint32_t n) {
    const uint32_t x = ab - dw.off0;
    if (x < dw.lim && dw.lim - x >= n)
        return be_sum(slot_range_sum(dw.slot, dw.ph + x, dw.ph + x + n), ab);
    return gsum_be(dw.rs, ab, n);
}

// parse_chain_lane for the inner frame: the sub-chain [T.is, T.ie) of the lane's chain,
// started at its Ethernet header (T.start_et 0) or at its IP header (GTP-U, GRE over IP:
// MACs 0, no tags, ethertype = the tunnel's dispatch value).  Cursors and the record's
// offsets are logical positions in the outer chain; frame_len is the sub-chain's length.
// The same tests as parse_chain_lane, each chunk taken by V.chunk at the header's cursor
// under the current end, each header read through dw.
__device__ __forceinline__ void parse_inner_lane(const ChainDw& dw, const ChainView& V,
                                                 const Tunnel& T, uint32_t flags, LaneRec& L) {
    uint32_t* w = L.w;
#pragma unroll
    for (int k = 0; k < 20; ++k) w[k] = 0;
    L.stream_s = L.stream_e = L.l4_part = L.l4_start_abs = L.pseudo = 0;
    L.want_l4 = false;
    L.is6 = false;
    const uint32_t pkt = T.ie;
    w[19] = T.ie - T.is;
    uint32_t status = RPKT_S_OK, et = T.start_et, c = T.is, ab;
    if (T.start_et == 0u) {
        if (V.chunk(c, pkt, ab) < 14u) {                       // ether/generated.rs:36
            L.status = RPKT_S_ETH_SHORT;
            w[0] = RPKT_S_ETH_SHORT;
            return;
        }
        w[1] = dw(ab);
        w[2] = dw(ab + 4u);
        w[3] = dw(ab + 8u);
        const uint32_t eth_et = be16_lo(dw(ab + 12u));
        uint32_t nvlan = 0;
        et = eth_et;
        c += 14u;
        for (int v = 0; v < RPKT_MAX_VLAN; ++v) {              // vlan/generated.rs:32-61
            if (!is_tag(et)) break;
            if (V.chunk(c, pkt, ab) < 4u) {
                status = RPKT_S_VLAN_SHORT;
                break;
            }
            const uint32_t t = dw(ab);
            et = be16_hi(t);
            w[4] |= be16_lo(t) << (16 * v);
            w[5] |= et << (16 * v);
            nvlan += 1;
            c += 4u;
        }
        w[0] = (nvlan << 8) | (eth_et << 16);
    } else {
        w[0] = T.start_et << 16;                               // the tunnel's dispatch value
    }
    const bool v6 = (flags & RPKT_F_IPV6) && status == RPKT_S_OK && et == 0x86ddu;
    if (status == RPKT_S_OK && et != 0x0800u && !v6) status = RPKT_S_NOT_IPV4;
    if (status != RPKT_S_OK) {
        w[0] |= status;
        L.status = status;
        return;
    }

    const uint32_t l3 = c;
    w[16] = l3 & 0xffffu;
    uint32_t l4, limit, l4rem, proto, paddr;
    if (v6) {
        L.is6 = true;
        status = parse_chain_ip6(dw, V.C, pkt, V.S, V.a, V.b, l3, w, l4, l4rem, proto, paddr);
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
        // Ipv4::parse (ipv4/generated.rs:35-51): chunk vs remaining
        const uint32_t ck3 = V.chunk(l3, pkt, ab);
        uint32_t F[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) F[k] = ck3 >= 20u ? dw(ab + 4u * k) : 0u;
        const uint32_t ihl4 = (F[0] & 0xfu) * 4u;
        const uint32_t tot = be16_hi(F[0]);
        if (ck3 < 20) status = RPKT_S_IP_SHORT;
        else if (ihl4 < 20) status = RPKT_S_IP_BAD_IHL;
        else if (ihl4 > ck3) status = RPKT_S_IP_IHL_GT_LEN;
        else if (tot < ihl4) status = RPKT_S_IP_TOT_LT_IHL;
        else if (tot > pkt - l3) status = RPKT_S_IP_TOT_GT_LEN;
        if (status != RPKT_S_OK) {
            w[0] |= status;
            L.status = status;
            return;
        }
        proto = (F[2] >> 8) & 0xffu;
        const uint32_t src = bswap32(F[3]), dst = bswap32(F[4]);
        w[6] = (F[0] & 0xffffu) | (tot << 16);
        w[7] = be16_lo(F[1]) | (be16_hi(F[1]) << 16);
        w[8] = (F[2] & 0xffffu) | (be16_hi(F[2]) << 16);
        w[9] = src;
        w[10] = dst;
        if (flags & RPKT_F_IP_SUM) w[18] = header_sum(dw, ab, ihl4);
        l4 = l3 + ihl4;                                        // Ipv4::payload :115-127
        limit = l3 + tot;
        l4rem = tot - ihl4;
        w[16] |= l4 << 16;
        w[17] = (l4 & 0xffffu) | (l4rem << 16);
        paddr = (src >> 16) + (src & 0xffffu) + (dst >> 16) + (dst & 0xffffu);
    }

    // Udp::parse / Tcp::parse against the chunk at l4 under the trimmed end
    uint32_t ab4;
    const uint32_t ck4 = V.chunk(l4, limit, ab4);
    uint32_t H[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) H[k] = dw(ab4 + 4u * k);
    uint32_t l4len = 0;
    bool other_sum = false;                                    // ICMP / GRE (parse_lane)
    if (proto == 17u) {
        const uint32_t ulen = be16_lo(H[1]);
        if (ck4 < 8) status = RPKT_S_UDP_SHORT;
        else if (ulen < 8 || ulen > l4rem) status = RPKT_S_UDP_BAD_LEN;
        else {
            w[11] = be16_lo(H[0]) | (be16_hi(H[0]) << 16);
            w[14] = ulen;
            w[15] = be16_hi(H[1]);
            w[17] = ((l4 + 8) & 0xffffu) | ((ulen - 8) << 16);
            l4len = ulen;
        }
    } else if (proto == 6u) {
        const uint32_t hl = ((H[3] >> 4) & 0xfu) * 4u;
        if (ck4 < 20) status = RPKT_S_TCP_SHORT;
        else if (hl < 20 || hl > ck4) status = RPKT_S_TCP_BAD_DOFF;
        else {
            w[11] = be16_lo(H[0]) | (be16_hi(H[0]) << 16);
            w[12] = bswap32(H[1]);
            w[13] = bswap32(H[2]);
            w[14] = be16_lo(H[3]) | (be16_hi(H[3]) << 16);
            w[15] = be16_lo(H[4]) | (be16_hi(H[4]) << 16);
            w[17] = ((l4 + hl) & 0xffffu) | ((l4rem - hl) << 16);
            l4len = l4rem;
        }
    } else {
        status = RPKT_S_L4_OTHER;
        if (!v6 && proto == 1u) {
            if (l4rem == 0u) status = RPKT_S_ICMP_EMPTY;
            else other_sum = true;
        } else if (proto == 47u && l4rem >= 4u && (H[0] & 0x80u)) {
            other_sum = true;
        }
        l4len = l4rem;
    }
    w[0] |= status;
    L.status = status;
    if ((status == RPKT_S_OK || other_sum) && (flags & RPKT_F_L4_SUM)) {
        L.want_l4 = true;
        L.pseudo = other_sum ? 0u : paddr + proto + l4len;
        const uint32_t e = l4 + l4len;
        L.l4_start_abs = dw.off0 + l4;                         // segment 0's byte phase
        // the part of [l4, e) segment 0's window holds (logical bytes [0, dw.lim))
        const uint32_t e_in = l4 < dw.lim ? (e < dw.lim ? e : dw.lim) : l4;
        L.l4_part = slot_range_sum(dw.slot, dw.ph + l4, dw.ph + e_in);
        L.stream_s = e_in;
        L.stream_e = e;                                        // logical, not absolute
    }
}

// WaveScratch (the window, then the inner records' stage and chain_stream's scratch past
// it) and a stage of its own for the outer records, which wait for the stream's sum too
struct TunChainScratch {
    WaveScratch W;
    uint32_t outer[kWave * 21];
};

// One wave per workgroup, as tunnel_kernel; registers, not waves, are the budget of the
// chain stream (parse_chains_kernel): 2 waves per SIMD, 15 KB of LDS per wave
template <bool L4>
__global__ __launch_bounds__(kWave, 2)
void tunnel_chains_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                          const uint2* __restrict__ segs, uint32_t n_segs,
                          const uint32_t* __restrict__ chain_first, uint32_t n, uint32_t flags,
                          rpkt_rec_t* __restrict__ outer, rpkt_tun_t* __restrict__ tun,
                          rpkt_rec_t* __restrict__ inner, uint64_t* __restrict__ flow_ev,
                          uint32_t n_buckets) {
    __shared__ __attribute__((aligned(16))) TunChainScratch scratch;
    WaveScratch& W = scratch.W;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t p0 = blockIdx.x * kWave;
    if (p0 >= n) return;                                          // wave-uniform exit
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
    const ChainSrc S{segs, fb};

    // chain bounds, segment 0 and pkt_len, as parse_chains_kernel
    uint32_t a = 0, b = 0;
    if (valid) {
        const uint32_t f0 = chain_first[i], f1 = chain_first[i + 1];
        a = f0 < n_segs ? f0 : n_segs;
        b = f1 > a ? f1 : a;
        b = b < n_segs ? b : n_segs;
    }
    Frame s0{0, 0};
    uint32_t pkt = 0;
    for (uint32_t k = a; k < b; ++k) {
        const Frame s = S.seg(k);
        if (k == a) s0 = s;
        pkt = pkt + s.len < pkt ? 0xffffffffu : pkt + s.len;
    }

    // 1. segment 0's header window -> LDS, the outer parse; the outer record to its stage
    {
        u32x4 d[kWinChunks];
        uint32_t addr[kWinChunks];
        const uint32_t fix = window_issue(rs, fb, s0, lane, d, addr);
        window_commit(W, rs, fb, d, addr, fix, lane);
    }
    wave_sync();
    LaneRec L;
    parse_chain_lane(W, lane, s0, pkt, S, a, b, rs, flags, L);
    uint32_t* ost = scratch.outer + lane * 21;
#pragma unroll
    for (int k = 0; k < 20; ++k) ost[k] = L.w[k];
    [[maybe_unused]] const uint32_t o_ss = L.stream_s, o_se = L.stream_e, o_part = L.l4_part;
    [[maybe_unused]] const uint32_t o_abs = L.l4_start_abs, o_pseudo = L.pseudo;
    [[maybe_unused]] const bool o_want = L.want_l4;

    // 2. the tunnel and the inner frame, from the same window (byte-wise past it)
    const uint32_t ph = s0.off & 15u, wl = (uint32_t)kWin - ph;
    const ChainDw dw{&W.win[lane * kSlot], ph, s0.off, s0.len < wl ? s0.len : wl, rs};
    const ChainView V{S, a, b, s0.off, s0.len};
    const Tunnel T = decode_tunnel_chain(L, dw, V, flags);
    if (T.ok) {
        parse_inner_lane(dw, V, T, flags, L);
    } else {
#pragma unroll
        for (int k = 0; k < 20; ++k) L.w[k] = 0u;
        L.w[0] = RPKT_S_NO_INNER;
        L.want_l4 = false;
        L.stream_s = L.stream_e = 0u;
    }
    stage_record(W, lane, L.w);

    // 3. L4 bytes past the window: the inner range (the outer one when there is no inner
    //    sum), which the outer range contains, then the outer range's other bytes
    if constexpr (L4) {
        const bool both = L.want_l4 && o_want;
        const uint32_t i_ss = L.stream_s, i_se = L.stream_e;
        const uint32_t ms = L.want_l4 ? i_ss : (o_want ? o_ss : 0u);
        const uint32_t me = L.want_l4 ? i_se : (o_want ? o_se : 0u);
        const uint32_t sp_m = chain_stream(W, rs, fb, S, a, b, s0.off, ms, me, lane);
        // outer [o_ss, o_se) = [o_ss, i_ss) + the inner stream + [i_se, o_se); an inner
        // range that ends inside the window has no stream and leaves the outer one whole
        const uint32_t pre_e = i_ss > o_ss ? i_ss : o_ss, tail_s = i_se > o_ss ? i_se : o_ss;
        uint32_t sp_o = sp_m;
        sp_o += chain_stream(W, rs, fb, S, a, b, s0.off, both ? o_ss : 0u, both ? pre_e : 0u, lane);
        sp_o += chain_stream(W, rs, fb, S, a, b, s0.off, both ? tail_s : 0u, both ? o_se : 0u, lane);
        if (L.want_l4)
            rec_stage(W)[lane * 21 + 18] |=
                fold16(L.pseudo + be_sum(L.l4_part + sp_m, L.l4_start_abs)) << 16;
        if (o_want) ost[18] |= fold16(o_pseudo + be_sum(o_part + sp_o, o_abs)) << 16;
    }

    // 4. the flow event (the inner record's when the tunnel decoded, else the outer's), the
    //    records (1-KiB wave stores), the tunnel record (16 B per lane)
    if ((flags & RPKT_F_FLOW_EV) && valid) {
        const uint32_t* rw = T.ok ? rec_stage(W) + lane * 21 : ost;
        __builtin_nontemporal_store(record_event(rw, n_buckets), &flow_ev[i]);
    }
    flush_stage(rec_stage(W), lane, inner, p0, n);
    flush_stage(scratch.outer, lane, outer, p0, n);
    if (valid) __builtin_nontemporal_store(u32x4{T.w[0], T.w[1], T.w[2], T.w[3]},
                                           reinterpret_cast<u32x4*>(tun) + i);
}

}  // namespace

extern "C" {

int rpkt_gpu_parse_tunnel_chains(const rpkt_chains_t* c, uint32_t flags, rpkt_rec_t* outer_dev,
                                 rpkt_tun_t* tun_dev, rpkt_rec_t* inner_dev,
                                 rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream) {
    if (!c) return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, kRxFlags));
    if (c->n_chains == 0) return RPKT_OK;
    if (any_null(outer_dev, tun_dev, inner_dev)) return RPKT_E_INVAL;
    RPKT_TRY(chains_ok(*c));
    if (misaligned(15, outer_dev, tun_dev, inner_dev) || misaligned(7, c->segs_dev))
        return RPKT_E_ALIGN;
    RPKT_TRY(events_ok(flags, flow_ev_dev, n_buckets));
    const uint32_t grid = (c->n_chains + kWave - 1) / kWave;
    auto k = (flags & RPKT_F_L4_SUM) ? tunnel_chains_kernel<true> : tunnel_chains_kernel<false>;
    return launch(k, dim3(grid), dim3(kWave), 0, (hipStream_t)stream, c->buf_dev,
                  (uint32_t)c->buf_bytes, (const uint2*)c->segs_dev, c->n_segs,
                  c->chain_first_dev, c->n_chains, flags, outer_dev, tun_dev, inner_dev,
                  (uint64_t*)flow_ev_dev, n_buckets);
}

}  // extern "C"
