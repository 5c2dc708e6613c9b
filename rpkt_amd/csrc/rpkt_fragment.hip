// rpkt_fragment.hip — rpkt_gpu_fragment_batch: IPv4 (RFC 791, the Linux ip_do_fragment slow
// path with ip_options_fragment) and IPv6 (RFC 8200 section 4.5) fragmentation of a
// device-resident batch at an L3 MTU (include/rpkt_gpu.h has the semantics).
//
// One more re-framing of a batch into a packed batch with other offsets, so it is the third
// user of the plan -> scan -> write structure of rpkt_segcopy.h (rpkt_segment.hip has the
// description): the same four launches on the stream with no host step between them, the
// same two scan kernels, the same search of the write's waves for their input frame.  What
// differs is the header rule, and that no payload byte is summed: fragmentation fills no L4
// checksum, so the slice goes through wave_copy<false> and the header waits for nothing.
//   plan   one lane per input frame.  It reads the record through the LDS stage for status,
//          the dispatch ethertype, l3_off and l4_off, and everything else from the frame: the
//          IPv4 header's ihl, packet_len and frag word, then a walk of its options (at most 40
//          bytes) for the bytes that turn into NOOPs in the fragments after the first; or the
//          IPv6 payload_len and a walk of the extension headers (at most RPKT_MAX_IP6_EXT) for
//          the end of the per-fragment headers.  The 32-B plan of a frame that is cut holds
//          the offsets, the slice size c and, for IPv4, the two header sums that are constant
//          over its fragments: with the options as they are (fragment 0) and with the NOOPs
//          (the others), both without packet_len, frag word and checksum.
//   write  one wave per run of kSegRun outputs.  Fragment k of a frame is `H + c` bytes after
//          fragment k - 1 (H: the bytes before the slice), so its place needs no search.  The
//          header goes out a lane per dword with patches: length, frag word and checksum for
//          IPv4 (the NOOP mask applied where the dword is fetched); payload_len, the
//          next-header byte and the 8-byte Fragment header (two 4-byte patches over bytes the
//          fetch read from the payload's start and does not keep) for IPv6.
// c, k and the plan are wave-uniform: every branch on them is.
// Every load goes through the frames buffer resource and every store through one over
// [out_frames_dev, + out_bytes); an overflowing batch writes its totals and frag_first and
// nothing else.  A record whose offsets do not nest makes its frame pass through.
//
// rpkt_gpu_fragment_chains is the same cut over mbuf chains (rpkt_chains_t), the frame being the
// chain's bytes in order, put together from rpkt_chaincopy.h as rpkt_gpu_segment_chains is
// (rpkt_segment.hip has the description): a plan and a write kernel of its own, everything
// else shared, the scan kernels included.  The plan's lane walks its chain's segments for
// pkt_len and the first non-empty segment, and reads the header [0, l4_off) as a flat frame's
// when it lies in that segment (the mbuf layout, and nearly every chain rpkt_gpu_parse_chains
// accepts) and byte by byte through the segment list otherwise; the rules are the ones above,
// templated on the header reader.  The write copies each slice as one wave copy per segment it
// touches and carries its place in the segment list from one fragment of a chain to the next:
// slices ascend, so the cursor only moves forward.
//
// rpkt_gpu_fragment_tunnel_batch cuts the inner IPv4 packet of a tunnelled frame before the
// encapsulation: the IPv4 rule above with the inner record, the outer headers as tunnel
// segmentation writes them ("tunnels" below has the description).
#include "rpkt_chaincopy.h"

namespace {

// plan words: 0 frame offset (chains: the chain's first segment, clamped), 1 frame length
// (chains: pkt_len), 2 l3 | hs << 16 (hs: the header bytes copied from
// the frame, l4_off for IPv4 and U for IPv6), 3 c | P << 16 (P: the bytes all the fragments
// carry together), 7 bit 0 cut, bit 1 IPv6;
//   IPv4: 4 header sum with the original options | with the NOOP-ed ones << 16, 5 the frame's
//         frag word | NOOP mask bits 32..39 << 16, 6 NOOP mask bits 0..31 (bit b: option byte
//         l3 + 20 + b becomes 0x01 in fragments k > 0);
//   IPv6: 4 offset of the next-header byte that becomes 44 | its old value << 16, 5 the
//         Fragment header's identification
constexpr uint32_t kFragOn = 1u, kFragV6 = 2u;
constexpr int kFragPatches = 4;

// the big-endian 16-bit words of a little-endian dword of header bytes, added
__device__ __forceinline__ uint32_t be_words(uint32_t d) { return be16_lo(d) + be16_hi(d); }

// nibble m (bit b: byte b) spread to a byte mask
__device__ __forceinline__ uint32_t nibble_bytes(uint32_t m) {
    return ((m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21)) * 0xffu;
}

// The IPv4 rule for the frame at H (record offsets l3, l4; len: the frame's length): true when
// it is cut, then cnt fragments and their bytes, plan words 2..7.
template <class Header>
__device__ __forceinline__ bool plan_ip4(const Header& H, uint32_t l3, uint32_t l4, uint32_t len,
                                         uint32_t mtu, bool ignore_df, uint32_t (&p)[8],
                                         uint64_t& cnt, uint64_t& bytes) {
    const uint32_t ip0 = H.dw(l3), ip1 = H.dw(l3 + 4u);
    const uint32_t ihl = (ip0 & 0xfu) * 4u, L = be16_hi(ip0), fw = be16_hi(ip1);
    if (ihl < 20u || l4 != l3 + ihl || L > len || l3 > len - L || L <= mtu) return false;
    if ((fw & 0x4000u) && !ignore_df) return false;
    if (mtu < ihl + 8u) return false;
    const uint32_t c = (mtu - ihl) & ~7u, P = L - ihl;            // c >= 8, P > c
    const uint32_t n = (P + c - 1u) / c;
    if ((fw & 0x1fffu) + (n - 1u) * (c >> 3) > 0x1fffu) return false;

    // ip_options_fragment: the option bytes that become NOOPs after the first fragment
    uint64_t mask = 0;
    const uint32_t olen = ihl - 20u;
    for (uint32_t x = 0; x < olen;) {
        const uint32_t d = H.dw(l3 + 20u + x);
        const uint32_t type = d & 0xffu, ol = (d >> 8) & 0xffu;
        if (type == 0u) break;
        if (type == 1u) {
            ++x;
            continue;
        }
        if (x + 1u >= olen || ol < 2u || ol > olen - x) break;
        if (!(type & 0x80u)) mask |= ((1ull << ol) - 1ull) << x;  // ol <= 40
        x += ol;
    }
    // the header's words without packet_len, frag word and checksum
    const uint32_t ip2 = H.dw(l3 + 8u);
    uint32_t s0 = be16_lo(ip0) + be16_lo(ip1) + be16_lo(ip2) + H.sum(l3 + 12u, l3 + 20u), s1 = s0;
    for (uint32_t x = 0; x < olen; x += 4u) {
        const uint32_t d = H.dw(l3 + 20u + x);
        const uint32_t bm = nibble_bytes((uint32_t)(mask >> x) & 0xfu);
        s0 += be_words(d);
        s1 += be_words((d & ~bm) | (0x01010101u & bm));
    }
    p[2] = l3 | (l4 << 16);
    p[3] = c | (P << 16);
    p[4] = fold16(s0) | (fold16(s1) << 16);
    p[5] = fw | ((uint32_t)(mask >> 32) << 16);
    p[6] = (uint32_t)mask;
    p[7] = kFragOn;
    cnt = n;
    bytes = (uint64_t)n * l4 + P;
    return true;
}

// The IPv6 rule, likewise; ident: the Fragment header's identification for this frame.
template <class Header>
__device__ __forceinline__ bool plan_ip6(const Header& H, uint32_t l3, uint32_t l4, uint32_t len,
                                         uint32_t mtu, uint32_t ident, uint32_t (&p)[8],
                                         uint64_t& cnt, uint64_t& bytes) {
    const uint32_t ip1 = H.dw(l3 + 4u);
    const uint32_t plen = be16_lo(ip1);
    const uint32_t E = l3 + 40u + plen;
    if (l4 < l3 + 40u || l4 > E || E > len || 40u + plen <= mtu) return false;
    // the extension headers up to l4: a Fragment header anywhere forbids the cut; the
    // per-fragment headers end after the last Routing header, else after a leading Hop-by-Hop
    uint32_t nh = (ip1 >> 16) & 0xffu, x = l3 + 40u, U = x, nhoff = l3 + 6u;
    for (int k = 0; k < RPKT_MAX_IP6_EXT && x < l4; ++k) {
        if (nh == 44u) return false;
        const uint32_t d = H.dw(x);
        uint32_t hl;
        if (nh == 0u || nh == 43u || nh == 60u) hl = 8u * (1u + ((d >> 8) & 0xffu));
        else if (nh == 51u) hl = 4u * (2u + ((d >> 8) & 0xffu));
        else break;
        if (hl > l4 - x) return false;
        if (nh == 43u || (nh == 0u && x == l3 + 40u)) {
            U = x + hl;
            nhoff = x;
        }
        nh = d & 0xffu;
        x += hl;
    }
    const uint32_t uh = U - l3;                                   // 40 .. l4 - l3
    if (mtu < uh + 16u) return false;
    const uint32_t c = (mtu - uh - 8u) & ~7u, F = E - U;          // c >= 8, F > c + 8
    const uint32_t n = (F + c - 1u) / c;
    p[2] = l3 | (U << 16);
    p[3] = c | (F << 16);
    p[4] = nhoff | ((H.dw(nhoff) & 0xffu) << 16);
    p[5] = ident;
    p[7] = kFragOn | kFragV6;
    cnt = n;
    bytes = (uint64_t)n * (U + 8u) + F;
    return true;
}

// What a staged record says about a frame: which rule applies and the offsets it reads.
struct FragWhere {
    bool v4, v6;
    uint32_t l3, l4;
};
__device__ __forceinline__ FragWhere frag_where(const uint32_t* w) {
    const uint32_t w0 = w[0], w5 = w[5], w16 = w[16];
    const uint32_t status = w0 & 0xffu, nv = (w0 >> 8) & 0xffu;
    const uint32_t det = nv == 0u ? w0 >> 16 : (nv == 1u ? w5 & 0xffffu : w5 >> 16);
    // the statuses under which the IP header parsed (IPv6: and its extension headers)
    const bool l4_status = status == RPKT_S_OK ||
                           (status >= RPKT_S_L4_OTHER && status <= RPKT_S_TCP_BAD_DOFF);
    return FragWhere{det == 0x0800u && (l4_status || status == RPKT_S_ICMP_EMPTY),
                     det == 0x86ddu && l4_status, w16 & 0xffffu, w16 >> 16};
}

__global__ __launch_bounds__(kSegBlock)
void fragment_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                          const uint32_t* __restrict__ offsets, uint32_t stride, uint32_t frame_len,
                          uint32_t n, const rpkt_rec_t* __restrict__ recs, uint32_t mtu,
                          uint32_t ignore_df, uint32_t ip6_ident, u32x4* __restrict__ plan,
                          uint32_t* __restrict__ frag_first, uint64_t* __restrict__ obase,
                          uint64_t* __restrict__ part) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    uint64_t cnt = 0, bytes = 0;
    uint32_t p[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

    if (p0 < n) {                                                 // wave-uniform
        uint32_t* st = stage[wave];
        stage_records_tile(st, recs, p0, n, lane);
        const uint32_t* w = st + lane * 21;
        const Frame fr = valid ? frame_span(offsets, stride, frame_len, fb, i) : Frame{0u, 0u};
        p[0] = fr.off;
        p[1] = fr.len;
        if (valid) {
            cnt = 1;
            bytes = fr.len;
            const FragWhere f = frag_where(w);
            const FlatHeader H{make_rsrc(frames, fb), fb, fr.off};
            if (f.v4)
                plan_ip4(H, f.l3, f.l4, fr.len, mtu, ignore_df != 0u, p, cnt, bytes);
            else if (f.v6)
                plan_ip6(H, f.l3, f.l4, fr.len, mtu, ip6_ident + i, p, cnt, bytes);
        }
    }
    plan_store(valid, i, p, cnt, bytes, plan, frag_first, obase, part, red);
}

// Fragment k of a cut frame with plan (pa, pb) and output byte base `base`: where it goes
// (d0), the H bytes before its slice (hs of them the frame's), the slice [done, + pk) of the
// bytes after the frame's hs, the header's patches (Pt) and its NOOP mask.  Wave-uniform.
struct FragOut {
    uint32_t l3, hs, H, done, pk, d0;
    uint64_t mask;
};
__device__ __forceinline__ FragOut frag_out(u32x4 pa, u32x4 pb, uint32_t k, uint32_t base,
                                            SegPatch (&Pt)[kFragPatches]) {
    const bool v6 = (pb.w & kFragV6) != 0u;
    const uint32_t l3 = pa.z & 0xffffu, hs = pa.z >> 16, c = pa.w & 0xffffu, P = pa.w >> 16;
    const uint32_t H = v6 ? hs + 8u : hs;                         // the bytes before the slice
    const uint32_t done = k * c;                                  // < P: k < ceil(P / c)
    const uint32_t left = done < P ? P - done : 0u;
    const uint32_t pk = left < c ? left : c;
    const bool last = left <= c;
    const uint32_t d0 = base + k * (H + c);
    const uint64_t mask = (v6 || k == 0u) ? 0ull : ((uint64_t)(pb.y >> 16) << 32) | pb.z;
    if (!v6) {
        const uint32_t fw0 = pb.y & 0xffffu;
        const uint32_t tot = hs - l3 + pk;
        const uint32_t fw = ((fw0 & 0x1fffu) + (done >> 3)) | ((!last || (fw0 & 0x2000u)) ? 0x2000u : 0u);
        const uint32_t sum = k == 0u ? pb.x & 0xffffu : pb.x >> 16;
        const uint32_t ck = ~fold16(sum + tot + fw) & 0xffffu;
        Pt[0] = SegPatch{l3 + 2u, 2u, bswap16(tot)};
        Pt[1] = SegPatch{l3 + 6u, 2u, bswap16(fw)};
        Pt[2] = SegPatch{l3 + 10u, 2u, bswap16(ck)};
        Pt[3] = SegPatch{0u, 0u, 0u};
    } else {
        const uint32_t nhoff = pb.x & 0xffffu, nh = pb.x >> 16;
        Pt[0] = SegPatch{l3 + 4u, 2u, bswap16((hs - l3 - 40u + 8u + pk) & 0xffffu)};
        Pt[1] = SegPatch{nhoff, 1u, 44u};
        Pt[2] = SegPatch{hs, 4u, nh | (bswap16(done | (last ? 0u : 1u)) << 16)};
        Pt[3] = SegPatch{hs + 4u, 4u, bswap32(pb.y)};
    }
    return FragOut{l3, hs, H, done, pk, d0, mask};
}

// The header's source bytes v of destination dword q with the NOOP mask applied: the dword's
// byte b is option byte rel + b - (l3 + 20)
__device__ __forceinline__ uint32_t noop_dword(const FragOut& o, uint32_t q, uint32_t v) {
    if (o.mask != 0ull) {
        const int x = (int)((o.d0 & ~3u) + 4u * q - o.d0) - (int)(o.l3 + 20u);
        if (x > -4 && x < 40) {
            const uint32_t bm = nibble_bytes((uint32_t)(x >= 0 ? o.mask >> x : o.mask << -x) & 0xfu);
            v = (v & ~bm) | (0x01010101u & bm);
        }
    }
    return v;
}

// Output j, fragment k of the input frame with plan (pa, pb) and output byte base `base`: its
// offset entry and its bytes, the whole wave.
__device__ __forceinline__ void write_fragment(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                               __amdgpu_buffer_rsrc_t ro,
                                               uint32_t* __restrict__ out_offsets, uint32_t j,
                                               uint32_t k, u32x4 pa, u32x4 pb, uint32_t base,
                                               int lane) {
    const uint32_t foff = pa.x, flen = pa.y;
    if (!(pb.w & kFragOn)) {                                      // pass-through: a byte copy
        if (lane == 0) out_offsets[j + 1] = base + flen;
        wave_copy<false>(rs, fb, ro, foff, base, flen, lane);
        return;
    }
    SegPatch Pt[kFragPatches];
    const FragOut o = frag_out(pa, pb, k, base, Pt);              // wave-uniform
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.H + o.pk;
    auto fetch = [&](uint32_t q) -> uint32_t {
        return noop_dword(o, q, header_dword(rs, fb, foff, o.d0, q));
    };
    const uint32_t hfirst = fetch((uint32_t)lane);
    wave_copy<false>(rs, fb, ro, foff + o.hs + o.done, o.d0 + o.H, o.pk, lane);
    wave_copy_header_from(ro, o.d0, o.H, hfirst, Pt, lane, fetch);
}

__global__ __launch_bounds__(kSegBlock)
void fragment_write_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                           const u32x4* __restrict__ plan, const uint32_t* __restrict__ frag_first,
                           const uint64_t* __restrict__ obase, const uint64_t* __restrict__ totals,
                           uint8_t* __restrict__ out, uint32_t out_bytes,
                           uint32_t* __restrict__ out_offsets, uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, frag_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = frag_first[i], nxt = frag_first[i + 1];
    u32x4 pa = plan[2 * (size_t)i], pb = plan[2 * (size_t)i + 1];
    uint32_t base = (uint32_t)obase[i];                           // < need <= out_bytes < 4 GiB
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next frame's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = frag_first[i + 1];
            }
            pa = plan[2 * (size_t)i];
            pb = plan[2 * (size_t)i + 1];
            base = (uint32_t)obase[i];
        }
        write_fragment(rs, fb, ro, out_offsets, j, j - cur, pa, pb, base, lane);
    }
}

// ---- mbuf chains -------------------------------------------------------------------------

__global__ __launch_bounds__(kSegBlock)
void fragment_chains_plan_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                                 const uint32_t* __restrict__ segs, uint32_t n_segs,
                                 const uint32_t* __restrict__ chain_first, uint32_t n,
                                 const rpkt_rec_t* __restrict__ recs, uint32_t mtu,
                                 uint32_t ignore_df, uint32_t ip6_ident, u32x4* __restrict__ plan,
                                 uint32_t* __restrict__ frag_first, uint64_t* __restrict__ obase,
                                 uint64_t* __restrict__ part) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    uint64_t cnt = 0, bytes = 0;
    uint32_t p[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

    if (p0 < n) {                                                 // wave-uniform
        uint32_t* st = stage[wave];
        stage_records_tile(st, recs, p0, n, lane);
        const SegTable S{segs, fb};
        // pkt_len in 64 bits (segments may overlap: no bound but n_segs * buf_bytes), and the
        // first non-empty segment, where the header starts
        uint32_t a = 0, b = 0;
        if (valid) chain_range(chain_first, n_segs, i, a, b);
        uint64_t pkt = 0;
        Frame s0{fb, 0u};
        for (uint32_t k = a; k < b; ++k) {
            const Frame s = S.seg(k);
            if (pkt == 0) s0 = s;
            pkt += s.len;
        }
        // a chain of 4 GiB or more cannot fit out_bytes: the call overflows and the write
        // never sees this plan; the IP lengths are 16 bits wide, so saturating is exact
        const uint32_t len = pkt < 0xffffffffull ? (uint32_t)pkt : 0xffffffffu;
        p[0] = a;
        p[1] = len;
        if (valid) {
            cnt = 1;
            bytes = pkt;
            const FragWhere f = frag_where(st + lane * 21);
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
            if (f.v4 || f.v6) {
                if (__builtin_expect(f.l4 <= s0.len, 1)) {
                    const FlatHeader H{rs, fb, s0.off};
                    if (f.v4) plan_ip4(H, f.l3, f.l4, len, mtu, ignore_df != 0u, p, cnt, bytes);
                    else plan_ip6(H, f.l3, f.l4, len, mtu, ip6_ident + i, p, cnt, bytes);
                } else {
                    const GatheredHeader H{S, rs, a, b, f.l4};
                    if (f.v4) plan_ip4(H, f.l3, f.l4, len, mtu, ignore_df != 0u, p, cnt, bytes);
                    else plan_ip6(H, f.l3, f.l4, len, mtu, ip6_ident + i, p, cnt, bytes);
                }
            }
        }
    }
    plan_store(valid, i, p, cnt, bytes, plan, frag_first, obase, part, red);
}

// The chain a wave is writing fragments of: its plan, its output byte base, the cursor, and
// where the header is (hdr: the first non-empty segment's offset when the copied header
// [0, hs) lies in it, `flat`).
struct FragChainState {
    u32x4 pa, pb;
    uint32_t base, hdr;
    bool flat;
    ChainCursor c;
};
__device__ __forceinline__ FragChainState frag_chain_state(const u32x4* __restrict__ plan,
                                                           const uint64_t* __restrict__ obase,
                                                           uint32_t i, const SegTable& S,
                                                           uint32_t n_segs) {
    FragChainState st;
    st.pa = plan[2 * (size_t)i];
    st.pb = plan[2 * (size_t)i + 1];
    st.base = (uint32_t)obase[i];                                 // < need <= out_bytes < 4 GiB
    st.c = ChainCursor{st.pa.x, 0u};
    st.hdr = S.fb;
    st.flat = true;
    if (st.pb.w & kFragOn) {                            // pkt_len >= hs > 0: a segment has bytes
        Frame s{S.fb, 0u};
        while (st.c.k < n_segs && (s = S.seg(st.c.k)).len == 0u) ++st.c.k;
        st.hdr = s.off;
        st.flat = (st.pa.z >> 16) <= s.len;
    }
    return st;
}

// write_fragment over a chain: the slice and the pass-through copy through the cursor, the
// header from the first non-empty segment or gathered
__device__ __forceinline__ void write_chain_fragment(__amdgpu_buffer_rsrc_t rs, const SegTable& S,
                                                     uint32_t n_segs, __amdgpu_buffer_rsrc_t ro,
                                                     uint32_t* __restrict__ out_offsets, uint32_t j,
                                                     uint32_t k, FragChainState& st, int lane) {
    const uint32_t fb = S.fb;
    if (!(st.pb.w & kFragOn)) {                                   // pass-through: a byte copy
        if (lane == 0) out_offsets[j + 1] = st.base + st.pa.y;
        chain_copy<false>(rs, S, n_segs, ro, st.c, 0u, st.base, st.pa.y, lane);
        return;
    }
    SegPatch Pt[kFragPatches];
    const FragOut o = frag_out(st.pa, st.pb, k, st.base, Pt);     // wave-uniform
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.H + o.pk;
    // IPv6: the 8 bytes after [0, hs) are the Fragment header's, all of them patched
    const GatheredHeader G{S, rs, st.pa.x, n_segs, o.hs};
    const uint32_t hdr = st.hdr;
    const bool flat = st.flat;                                    // wave-uniform
    auto fetch = [&](uint32_t q) -> uint32_t {
        return noop_dword(o, q, flat ? header_dword(rs, fb, hdr, o.d0, q)
                                     : G.dw((o.d0 & ~3u) + 4u * q - o.d0));
    };
    const uint32_t hfirst = fetch((uint32_t)lane);
    chain_copy<false>(rs, S, n_segs, ro, st.c, o.hs + o.done, o.d0 + o.H, o.pk, lane);
    wave_copy_header_from(ro, o.d0, o.H, hfirst, Pt, lane, fetch);
}

__global__ __launch_bounds__(kSegBlock)
void fragment_chains_write_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                                  const uint32_t* __restrict__ segs, uint32_t n_segs, uint32_t n,
                                  const u32x4* __restrict__ plan,
                                  const uint32_t* __restrict__ frag_first,
                                  const uint64_t* __restrict__ obase,
                                  const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                                  uint32_t out_bytes, uint32_t* __restrict__ out_offsets,
                                  uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, frag_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = frag_first[i], nxt = frag_first[i + 1];
    const SegTable S{segs, fb};
    FragChainState st = frag_chain_state(plan, obase, i, S, n_segs);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next chain's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = frag_first[i + 1];
            }
            st = frag_chain_state(plan, obase, i, S, n_segs);
        }
        write_chain_fragment(rs, S, n_segs, ro, out_offsets, j, j - cur, st, lane);
    }
}

// ---- tunnels: the inner IPv4 packet of VXLAN, GTP-U and GRE frames ------------------------
//
// rpkt_gpu_fragment_tunnel_batch cuts the inner IPv4 packet of a decoded tunnel before the
// encapsulation (RFC 4459 section 3.2): the inner record's offsets are positions in the outer
// frame, so the cut is plan_ip4 with the inner record at mtu - over (over: the bytes from the
// outer IP header to the inner one), the copied header is [0, inner l4_off), and the outer
// headers follow as rpkt_gpu_segment_tunnel_batch writes them.  The plan is 64 B a frame: words
// 0..7 as above for the packet that is cut (the inner one; the frame's own for a frame without
// a tunnel or, with RPKT_FRAGMENT_TUNNEL_OUTER, one whose inner packet is not cut), then words
// 8..11 and the kTun* bits of word 7 as rpkt_segment.hip ("tunnels") has them.
// The constant under the outer checksum (word 11) must not depend on k, and the inner header's
// packet_len, frag word, checksum and NOOP-ed options do.  The rule, once: a filled IPv4 header
// sums to 0xffff, which is 0 in one's complement, at either parity; so the constant is the
// pseudo header and [origin, inner l3) without the outer fields the write patches, the inner
// header [inner l3, inner l4) adds nothing, and the slice's sum enters at the parity of inner
// l4 - origin.  (What is summed is never all zero -- the pseudo header's 17, GRE's protocol --
// so the sum stays in the class of the full one and 0 / 0xffff come out as they would.)  The
// slice is summed in its copy, wave_copy<true>, only where the outer checksum is filled
// (kTunCsum); every other output goes through wave_copy<false> as the flat write's.

__global__ __launch_bounds__(kSegBlock)
void fragment_tunnel_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                                 const uint32_t* __restrict__ offsets, uint32_t stride,
                                 uint32_t frame_len, uint32_t n, const rpkt_rec_t* __restrict__ outer,
                                 const rpkt_tun_t* __restrict__ tun, const rpkt_rec_t* __restrict__ inner,
                                 uint32_t mtu, uint32_t ignore_df, uint32_t outer_fallback,
                                 uint32_t ip6_ident, u32x4* __restrict__ plan,
                                 uint32_t* __restrict__ frag_first, uint64_t* __restrict__ obase,
                                 uint64_t* __restrict__ part) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    uint64_t cnt = 0, bytes = 0;
    uint32_t p[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};

    if (p0 < n) {                                                 // wave-uniform
        // the tile's outer records through the stage, then its inner records through the same
        uint32_t* st = stage[wave];
        const uint32_t* w = st + lane * 21;
        stage_records_tile(st, outer, p0, n, lane);
        const uint32_t o0 = w[0], o5 = w[5], o7 = w[7], o8 = w[8], o16 = w[16];
        const FragWhere fo = frag_where(w);
        wave_sync();
        stage_records_tile(st, inner, p0, n, lane);
        const u32x4 t = valid ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tun) + i)
                              : u32x4{0u, 0u, 0u, 0u};
        const Frame fr = valid ? frame_span(offsets, stride, frame_len, fb, i) : Frame{0u, 0u};
        p[0] = fr.off;
        p[1] = fr.len;
        if (valid) {
            cnt = 1;
            bytes = fr.len;
            const FlatHeader H{make_rsrc(frames, fb), fb, fr.off};
            // no tunnel: the frame's own packet under its outer record; so is a tunnelled frame
            // whose inner packet is not cut, when the caller asks for it
            bool own = (t.x & 0xffu) == RPKT_TUN_NONE;
            if (!own) {
                const FragWhere fi = frag_where(w);
                L4Where in{};
                in.l3 = fi.l3;
                const TunWhere tw = tun_where(o0, o5, o7, o8, o16, t, in);
                const uint32_t over = fi.l3 - tw.l3;              // tw.ok: outer l3 <= inner l3
                uint32_t bits = 0;
                // the cut is decided first: a frame whose inner packet fits or has DF set (most
                // of a transmit batch) does not pay for the outer constants
                bool cut = ((t.x >> 8) & 0xffu) == RPKT_T_OK && tw.ok && fi.v4 && mtu > over &&
                           plan_ip4(H, fi.l3, fi.l4, fr.len, mtu - over, ignore_df != 0u, p, cnt,
                                    bytes);
                if (cut && !tunnel_constants_to(H, tw, fi.l3, q, bits, [](auto) {})) {
                    // the GRE header forbids it after all: the plan as it was before plan_ip4
                    cut = false;
                    p[2] = p[3] = p[4] = p[5] = p[6] = p[7] = 0u;
                    q[0] = q[1] = q[2] = q[3] = 0u;
                    cnt = 1;
                    bytes = fr.len;
                }
                if (cut) p[7] |= bits;
                else own = outer_fallback != 0u;
            }
            if (own) {
                if (fo.v4)
                    plan_ip4(H, fo.l3, fo.l4, fr.len, mtu, ignore_df != 0u, p, cnt, bytes);
                else if (fo.v6)
                    plan_ip6(H, fo.l3, fo.l4, fr.len, mtu, ip6_ident + i, p, cnt, bytes);
            }
        }
    }
    if (valid) {
        plan[4 * (size_t)i + 2] = u32x4{q[0], q[1], q[2], q[3]};
        plan[4 * (size_t)i + 3] = u32x4{0u, 0u, 0u, 0u};
    }
    plan_store<4>(valid, i, p, cnt, bytes, plan, frag_first, obase, part, red);
}

// write_fragment for the 64-B plan (pa, pb, pc): an inner cut's fragment k, everything else as
// the flat write has it
__device__ __forceinline__ void write_tunnel_fragment(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                      __amdgpu_buffer_rsrc_t ro,
                                                      uint32_t* __restrict__ out_offsets, uint32_t j,
                                                      uint32_t k, u32x4 pa, u32x4 pb, u32x4 pc,
                                                      uint32_t base, int lane) {
    if (!(pb.w & kTunOn)) {                                       // wave-uniform
        write_fragment(rs, fb, ro, out_offsets, j, k, pa, pb, base, lane);
        return;
    }
    const uint32_t foff = pa.x;
    SegPatch Pt[kFragPatches];
    const FragOut o = frag_out(pa, pb, k, base, Pt);              // the inner IPv4 rule: H == hs
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.H + o.pk;
    auto fetch = [&](uint32_t c) -> uint32_t {
        return noop_dword(o, c, header_dword(rs, fb, foff, o.d0, c));
    };
    const uint32_t hfirst = fetch((uint32_t)lane);
    uint32_t pay = 0;
    if (pb.w & kTunCsum) {                                        // wave-uniform
        const uint32_t part = wave_copy<true>(rs, fb, ro, foff + o.hs + o.done, o.d0 + o.H, o.pk, lane);
        pay = be_sum(wave_sum(fold16(part)), o.d0 + o.H);
    } else {
        wave_copy<false>(rs, fb, ro, foff + o.hs + o.done, o.d0 + o.H, o.pk, lane);
    }
    // the outer patches over an output whose payload starts at inner l4; no inner patch enters
    // the outer sum (the rule above), so they are set after it is formed
    SegPatch P[kTunPatches];
#pragma unroll
    for (int u = 0; u < kSegPatches; ++u) P[u] = SegPatch{0u, 0u, 0u};
    const SegOut so{false, false, o.l3, o.hs, o.hs, o.done, o.pk, o.d0};
    tunnel_patches(so, pb, pc, k, pay, P);
#pragma unroll
    for (int u = 0; u < 3; ++u) P[u] = Pt[u];
    wave_copy_header_from(ro, o.d0, o.H, hfirst, P, lane, fetch);
}

__global__ __launch_bounds__(kSegBlock)
void fragment_tunnel_write_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                                  const u32x4* __restrict__ plan,
                                  const uint32_t* __restrict__ frag_first,
                                  const uint64_t* __restrict__ obase,
                                  const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                                  uint32_t out_bytes, uint32_t* __restrict__ out_offsets,
                                  uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, frag_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = frag_first[i], nxt = frag_first[i + 1];
    u32x4 pa = plan[4 * (size_t)i], pb = plan[4 * (size_t)i + 1], pc = plan[4 * (size_t)i + 2];
    uint32_t base = (uint32_t)obase[i];                           // < need <= out_bytes < 4 GiB
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next frame's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = frag_first[i + 1];
            }
            pa = plan[4 * (size_t)i];
            pb = plan[4 * (size_t)i + 1];
            pc = plan[4 * (size_t)i + 2];
            base = (uint32_t)obase[i];
        }
        write_tunnel_fragment(rs, fb, ro, out_offsets, j, j - cur, pa, pb, pc, base, lane);
    }
}

}  // namespace

extern "C" {

size_t rpkt_gpu_fragment_tunnel_workspace_bytes(uint32_t n) { return seg_ws(nullptr, n, 4).bytes; }

int rpkt_gpu_fragment_tunnel_batch(const rpkt_batch_t* b, const rpkt_rec_t* outer_dev,
                                   const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                   uint32_t mtu, uint32_t flags, uint32_t ip6_ident,
                                   uint8_t* out_frames_dev, uint64_t out_bytes,
                                   uint32_t* out_offsets_dev, uint32_t out_cap,
                                   uint32_t* frag_first_dev, uint64_t* totals_dev,
                                   void* workspace_dev, void* stream) {
    RPKT_TRY(reframe_args_ok(b, outer_dev, mtu, flags,
                             RPKT_FRAGMENT_IGNORE_DF | RPKT_FRAGMENT_TUNNEL_OUTER, out_frames_dev,
                             out_bytes, out_offsets_dev, out_cap, frag_first_dev, totals_dev,
                             workspace_dev, tun_dev, inner_dev));
    if (b->n == 0) return RPKT_OK;

    const SegWs ws = seg_ws(workspace_dev, b->n, 4);
    RPKT_TRY(launch_batch(fragment_tunnel_plan_kernel, kSegBlock, 0, stream, *b, outer_dev, tun_dev,
                          inner_dev, mtu, flags & RPKT_FRAGMENT_IGNORE_DF,
                          flags & RPKT_FRAGMENT_TUNNEL_OUTER, ip6_ident, ws.plan, frag_first_dev,
                          ws.obase, ws.part));
    return scan_and_write(fragment_tunnel_write_kernel, ws, b->n, out_cap, frag_first_dev,
                          totals_dev, (hipStream_t)stream, b->frames_dev,
                          (uint32_t)b->frames_bytes, b->n, ws.plan, frag_first_dev, ws.obase,
                          totals_dev, out_frames_dev, (uint32_t)out_bytes, out_offsets_dev, out_cap);
}

size_t rpkt_gpu_fragment_workspace_bytes(uint32_t n) { return seg_ws(nullptr, n).bytes; }

int rpkt_gpu_fragment_batch(const rpkt_batch_t* b, const rpkt_rec_t* recs_dev, uint32_t mtu,
                            uint32_t flags, uint32_t ip6_ident, uint8_t* out_frames_dev,
                            uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                            uint32_t* frag_first_dev, uint64_t* totals_dev, void* workspace_dev,
                            void* stream) {
    RPKT_TRY(reframe_args_ok(b, recs_dev, mtu, flags, RPKT_FRAGMENT_IGNORE_DF, out_frames_dev,
                             out_bytes, out_offsets_dev, out_cap, frag_first_dev, totals_dev,
                             workspace_dev));
    if (b->n == 0) return RPKT_OK;

    const SegWs ws = seg_ws(workspace_dev, b->n);
    RPKT_TRY(launch_batch(fragment_plan_kernel, kSegBlock, 0, stream, *b, recs_dev, mtu,
                          flags & RPKT_FRAGMENT_IGNORE_DF, ip6_ident, ws.plan, frag_first_dev,
                          ws.obase, ws.part));
    return scan_and_write(fragment_write_kernel, ws, b->n, out_cap, frag_first_dev, totals_dev,
                          (hipStream_t)stream, b->frames_dev, (uint32_t)b->frames_bytes, b->n,
                          ws.plan, frag_first_dev, ws.obase, totals_dev, out_frames_dev,
                          (uint32_t)out_bytes, out_offsets_dev, out_cap);
}

size_t rpkt_gpu_fragment_chains_workspace_bytes(uint32_t n) { return seg_ws(nullptr, n).bytes; }

int rpkt_gpu_fragment_chains(const rpkt_chains_t* c, const rpkt_rec_t* recs_dev, uint32_t mtu,
                             uint32_t flags, uint32_t ip6_ident, uint8_t* out_frames_dev,
                             uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                             uint32_t* frag_first_dev, uint64_t* totals_dev, void* workspace_dev,
                             void* stream) {
    RPKT_TRY(reframe_args_ok(c, recs_dev, mtu, flags, RPKT_FRAGMENT_IGNORE_DF, out_frames_dev,
                             out_bytes, out_offsets_dev, out_cap, frag_first_dev, totals_dev,
                             workspace_dev));
    if (c->n_chains == 0) return RPKT_OK;

    const uint32_t n = c->n_chains, fb = (uint32_t)c->buf_bytes;
    const uint32_t* segs = c->segs_dev;
    const SegWs ws = seg_ws(workspace_dev, n);
    RPKT_TRY(launch(fragment_chains_plan_kernel, dim3(blocks(n)), dim3(kSegBlock), 0,
                    (hipStream_t)stream, c->buf_dev, fb, segs, c->n_segs, c->chain_first_dev, n,
                    recs_dev, mtu, flags & RPKT_FRAGMENT_IGNORE_DF, ip6_ident, ws.plan,
                    frag_first_dev, ws.obase, ws.part));
    return scan_and_write(fragment_chains_write_kernel, ws, n, out_cap, frag_first_dev, totals_dev,
                          (hipStream_t)stream, c->buf_dev, fb, segs, c->n_segs, n, ws.plan,
                          frag_first_dev, ws.obase, totals_dev, out_frames_dev, (uint32_t)out_bytes,
                          out_offsets_dev, out_cap);
}

}  // extern "C"
