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
#include "rpkt_segcopy.h"

namespace {

// plan words: 0 frame offset, 1 frame length, 2 l3 | hs << 16 (hs: the header bytes copied from
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
__device__ __forceinline__ bool plan_ip4(const FlatHeader& H, uint32_t l3, uint32_t l4, uint32_t len,
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
__device__ __forceinline__ bool plan_ip6(const FlatHeader& H, uint32_t l3, uint32_t l4, uint32_t len,
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
            const uint32_t w0 = w[0], w5 = w[5], w16 = w[16];
            const uint32_t status = w0 & 0xffu, nv = (w0 >> 8) & 0xffu;
            const uint32_t det = nv == 0u ? w0 >> 16 : (nv == 1u ? w5 & 0xffffu : w5 >> 16);
            const uint32_t l3 = w16 & 0xffffu, l4 = w16 >> 16;
            // the statuses under which the IP header parsed (IPv6: and its extension headers)
            const bool l4_status = status == RPKT_S_OK ||
                                   (status >= RPKT_S_L4_OTHER && status <= RPKT_S_TCP_BAD_DOFF);
            const FlatHeader H{make_rsrc(frames, fb), fb, fr.off};
            if (det == 0x0800u && (l4_status || status == RPKT_S_ICMP_EMPTY))
                plan_ip4(H, l3, l4, fr.len, mtu, ignore_df != 0u, p, cnt, bytes);
            else if (det == 0x86ddu && l4_status)
                plan_ip6(H, l3, l4, fr.len, mtu, ip6_ident + i, p, cnt, bytes);
        }
    }
    plan_store(valid, i, p, cnt, bytes, plan, frag_first, obase, part, red);
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
    const bool v6 = (pb.w & kFragV6) != 0u;                       // wave-uniform, as all below
    const uint32_t l3 = pa.z & 0xffffu, hs = pa.z >> 16, c = pa.w & 0xffffu, P = pa.w >> 16;
    const uint32_t H = v6 ? hs + 8u : hs;                         // the bytes before the slice
    const uint32_t done = k * c;                                  // < P: k < ceil(P / c)
    const uint32_t left = done < P ? P - done : 0u;
    const uint32_t pk = left < c ? left : c;
    const bool last = left <= c;
    const uint32_t d0 = base + k * (H + c);
    if (lane == 0) out_offsets[j + 1] = d0 + H + pk;

    SegPatch Pt[kFragPatches];
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
    // the header's source bytes of destination dword q, the NOOP mask applied: the dword's
    // byte b is option byte rel + b - (l3 + 20)
    auto fetch = [&](uint32_t q) -> uint32_t {
        uint32_t v = header_dword(rs, fb, foff, d0, q);
        if (mask != 0ull) {
            const int o = (int)((d0 & ~3u) + 4u * q - d0) - (int)(l3 + 20u);
            if (o > -4 && o < 40) {
                const uint32_t bm = nibble_bytes((uint32_t)(o >= 0 ? mask >> o : mask << -o) & 0xfu);
                v = (v & ~bm) | (0x01010101u & bm);
            }
        }
        return v;
    };
    const uint32_t hfirst = fetch((uint32_t)lane);
    wave_copy<false>(rs, fb, ro, foff + hs + done, d0 + H, pk, lane);
    wave_copy_header_from(ro, d0, H, hfirst, Pt, lane, fetch);
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

}  // namespace

extern "C" {

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

}  // extern "C"
