// rpkt_segment.hip — rpkt_gpu_segment_batch and rpkt_gpu_segment_chains: TCP segmentation
// (TSO) of a device-resident batch, flat or in mbuf chains, the TCP_SEG transmit offload of
// rpkt-dpdk/examples/tso_tx.rs:128-134 under the Linux tcp_gso_segment / DPDK rte_gso rules,
// and with RPKT_SEGMENT_UDP UDP segmentation under the Linux __udp_gso_segment rules
// (include/rpkt_gpu.h has the semantics).  UDP is a second L4 header rule in the same
// kernels: another constant sum in the plan, one patch (length and checksum) where TCP has
// three (seq, flags, checksum) in the write.  The kernels that test the protocol take the flag
// as a template argument <kUdp>: a call with the flag clear launches the code without the
// test, so the TCP-only call costs what it did before the flag existed.
//
// The output batch has another frame count and other offsets than the input, so the work
// is planned from the input and split by the output.  Four launches on the stream, no host
// step between them:
//   1. plan   one lane per input frame: its record (coalesced through an LDS stage) says
//             whether it is segmented; n_i outputs and their bytes go to seg_first / the
//             workspace, with the block's sums, and for a segmented frame the constants
//             every one of its segments shares (the IPv4 header sum without packet_len /
//             ident / checksum, the TCP header + pseudo header sum without seq / flags /
//             checksum / length, or the UDP one without length / checksum), read from the
//             frame once per super-frame;
//   2. scan   exclusive prefix sums of counts and bytes: one block over the block sums
//             (with a carry from each 256 to the next), then one block per 256 frames;
//   3. write  one wavefront per run of kSegRun consecutive OUTPUT frames: it finds the first
//             one's input frame by a 64-way search of seg_first and steps along seg_first
//             for the others.  Per output it copies the payload slice in 16-B chunks of the
//             destination (source and destination at any two byte phases: two aligned 16-B
//             loads and a byte funnel shift per chunk), sums the bytes it copies (absolute
//             destination phase, be_sum), and then writes the header with the patched fields
//             and the two checksums.  A pass-through frame is the same copy without the sum.
// What a record says about a TCP or UDP frame (l4_where), the record stage, the block scan and
// the kernel over the block sums, the copy, the header write, the entries' argument checks and
// the workspace carving are in rpkt_segcopy.h, which rpkt_coalesce.hip (the inverse entry)
// shares; the workspace layout (seg_ws), the plan's end (plan_store), the scan over frames, the
// write's run of outputs (output_run, kSegRun) and scan_and_write are there too, shared with
// rpkt_fragment.hip (IP fragmentation: the same structure with another header rule).
// Every load goes through the frames buffer resource and every store through one over
// [out_frames_dev, + out_bytes); an overflowing batch (totals past the capacities) writes
// its totals and seg_first and nothing else.
//
// Over mbuf chains (rpkt_chains_t) the frame is the chain's bytes in order.  The plan and the
// write have a kernel of their own there and share everything else, the scan kernels
// included: the plan's lane walks its chain's segments for pkt_len; the write copies a slice
// of the logical bytes as one wave copy per segment it touches (their sums add: each is over
// destination-aligned words) and carries its place in the segment list from one output of a
// chain to the next.  The header [0, payload_off) is read as a flat frame's when it lies in
// the chain's first non-empty segment (the mbuf layout, and nearly every chain that
// rpkt_gpu_parse_chains calls TCP: there a header may start where a segment ends but never
// straddles an end), and byte by byte through the segment list otherwise, its sums then
// taken at the logical position's parity.
//
// rpkt_gpu_segment_tunnel_batch (the inner TCP / UDP of VXLAN, GTP-U and GRE frames, flat
// batches) is the flat cut with the inner record plus the outer headers' fix-ups: a plan and a
// write kernel of its own with a 64-B plan and nine patches, everything else shared; see
// "tunnels" below.  rpkt_gpu_segment_tunnel_chains is that cut over mbuf chains: the chain
// kernels' walk, cursor and gathered header with the tunnel kernels' plan and patches.
#include "rpkt_chaincopy.h"

namespace {

// plan words: 0 frame offset (chains: the chain's first segment, clamped), 1 frame length
// (chains: pkt_len), 2 l3 | l4 << 16, 3 payload_off | payload_len << 16, 4 IPv4 constant sum |
// ident << 16, 5 L4 constant sum | be16 of TCP bytes 12..13 << 16 (UDP: 0), 6 seq (UDP: 0),
// 7 bit 0 segmented, bit 1 IPv6, bit 2 UDP
constexpr uint32_t kSegOn = 1u, kSegV6 = 2u, kSegUdp = 4u;

// ---- 1. plan ---------------------------------------------------------------------------

// The header bytes of a flat frame: FlatHeader (rpkt_segcopy.h).

// Plan words 2..7 of a segmented frame from its header H: the constants all its segments
// share.
template <class Header>
__device__ __forceinline__ void seg_constants(const Header& H, const L4Where& s, uint32_t (&p)[8]) {
    const uint32_t l3 = s.l3, l4 = s.l4, po = s.po;
    // a field leaves a sum by adding its complement (one's complement arithmetic;
    // the sums stay positive, so the folded values are the plain sums')
    uint32_t ipc = 0, pseudo;
    const uint32_t ip0 = H.dw(l3);
    uint32_t ident = 0;
    if (!s.v6) {
        const uint32_t ip1 = H.dw(l3 + 4u), ip2 = H.dw(l3 + 8u);
        ident = be16_lo(ip1);
        ipc = H.sum(l3, l4) + (0xffffu ^ be16_hi(ip0)) + (0xffffu ^ ident) + (0xffffu ^ be16_hi(ip2));
        pseudo = H.sum(l3 + 12u, l3 + 20u);
    } else {
        const uint32_t pd = ip6_pseudo_dst(s.pdst, l3, l4);
        pseudo = H.sum(l3 + 8u, l3 + 24u) + H.sum(pd, pd + 16u);
    }
    // bytes l4 + 4..7 leave the L4 sum whole: TCP's seq, UDP's length and checksum
    const uint32_t t1 = H.dw(l4 + 4u);
    uint32_t l4c = H.sum(l4, po) + pseudo + (0xffffu ^ be16_lo(t1)) + (0xffffu ^ be16_hi(t1));
    uint32_t seq = 0, w12 = 0;
    if (s.udp) {
        l4c += 17u;
    } else {
        const uint32_t t3 = H.dw(l4 + 12u), t4 = H.dw(l4 + 16u);
        seq = bswap32(t1);
        w12 = be16_lo(t3);
        l4c += 6u + (0xffffu ^ w12) + (0xffffu ^ be16_lo(t4));
    }
    p[2] = l3 | (l4 << 16);
    p[3] = po | (s.pl << 16);
    p[4] = fold16(ipc) | (ident << 16);
    p[5] = fold16(l4c) | (w12 << 16);
    p[6] = seq;
    p[7] = kSegOn | (s.v6 ? kSegV6 : 0u) | (s.udp ? kSegUdp : 0u);
}

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                         const uint32_t* __restrict__ offsets, uint32_t stride, uint32_t frame_len,
                         uint32_t n, const rpkt_rec_t* __restrict__ recs, uint32_t mss,
                         u32x4* __restrict__ plan, uint32_t* __restrict__ seg_first,
                         uint64_t* __restrict__ obase, uint64_t* __restrict__ part) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    uint64_t cnt = 0, bytes = 0;
    uint32_t p[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

    if (p0 < n) {                                                 // wave-uniform
        // the tile's records, coalesced through the stage (stride 21 dwords)
        uint32_t* st = stage[wave];
        stage_records_tile(st, recs, p0, n, lane);
        const Frame fr = valid ? frame_span(offsets, stride, frame_len, fb, i) : Frame{0u, 0u};
        const L4Where s = l4_where(st + lane * 21, fr.len, kUdp);
        p[0] = fr.off;
        p[1] = fr.len;
        if (valid) {
            cnt = 1;
            bytes = fr.len;
        }
        if (valid && s.on && s.pl > mss) {                       // segmented
            cnt = (s.pl + mss - 1u) / mss;
            bytes = cnt * s.po + s.pl;
            seg_constants(FlatHeader{make_rsrc(frames, fb), fb, fr.off}, s, p);
        }
    }
    plan_store(valid, i, p, cnt, bytes, plan, seg_first, obase, part, red);
}

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_chains_plan_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                                const uint32_t* __restrict__ segs, uint32_t n_segs,
                                const uint32_t* __restrict__ chain_first, uint32_t n,
                                const rpkt_rec_t* __restrict__ recs, uint32_t mss,
                                u32x4* __restrict__ plan, uint32_t* __restrict__ seg_first,
                                uint64_t* __restrict__ obase, uint64_t* __restrict__ part) {
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
        // never sees this plan; the record's offsets are 16 bits wide, so saturating is exact
        const uint32_t len = pkt < 0xffffffffull ? (uint32_t)pkt : 0xffffffffu;
        const L4Where s = l4_where(st + lane * 21, len, kUdp);
        p[0] = a;
        p[1] = len;
        if (valid) {
            cnt = 1;
            bytes = pkt;
        }
        if (valid && s.on && s.pl > mss) {                       // segmented
            cnt = (s.pl + mss - 1u) / mss;
            bytes = cnt * s.po + s.pl;
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
            if (__builtin_expect(s.po <= s0.len, 1))
                seg_constants(FlatHeader{rs, fb, s0.off}, s, p);
            else
                seg_constants(GatheredHeader{S, rs, a, n_segs, s.po}, s, p);
        }
    }
    plan_store(valid, i, p, cnt, bytes, plan, seg_first, obase, part, red);
}

// ---- 2. scan: scan_parts_kernel and segment_scan_frames_kernel (rpkt_segcopy.h) -------------

// ---- 3. write --------------------------------------------------------------------------

// Output k of a segmented frame with plan (pa, pb) and output byte base `base`: where it
// goes and which payload bytes it carries (SegOut: rpkt_segcopy.h).
__device__ __forceinline__ SegOut seg_out(u32x4 pa, u32x4 pb, uint32_t mss, uint32_t k,
                                          uint32_t base) {
    SegOut o;
    o.v6 = (pb.w & kSegV6) != 0u;
    o.l3 = pa.z & 0xffffu;
    o.l4 = pa.z >> 16;
    o.po = pa.w & 0xffffu;
    const uint32_t pl = pa.w >> 16;
    o.done = k * mss;                                             // < pl: k < ceil(pl / mss)
    const uint32_t left = o.done < pl ? pl - o.done : 0u;
    o.pk = left < mss ? left : mss;
    o.last = left <= mss;
    o.d0 = base + k * (o.po + mss);
    return o;
}

// The fields output k's header differs in, `pay` the big-endian sum of its payload.
template <bool kUdp>
__device__ __forceinline__ void seg_patches(const SegOut& o, u32x4 pb, uint32_t k, uint32_t pay,
                                            SegPatch (&P)[kSegPatches]) {
    const uint32_t l3 = o.l3, l4 = o.l4, po = o.po, pk = o.pk;
    if (!o.v6) {
        const uint32_t tot = po - l3 + pk, ident = ((pb.x >> 16) + k) & 0xffffu;
        const uint32_t ck = ~fold16((pb.x & 0xffffu) + tot + ident) & 0xffffu;
        P[0] = SegPatch{l3 + 2u, 4u, bswap16(tot) | (bswap16(ident) << 16)};
        P[1] = SegPatch{l3 + 10u, 2u, bswap16(ck)};
    } else {
        P[0] = SegPatch{l3 + 4u, 2u, bswap16((po - l3 - 40u + pk) & 0xffffu)};
        P[1] = SegPatch{0u, 0u, 0u};
    }
    if (kUdp && (pb.w & kSegUdp)) {                               // wave-uniform: one output a wave
        // length and checksum, one patch; the length is in the pseudo header and in the header
        const uint32_t ulen = 8u + pk;
        const uint32_t uck = udp_csum_field((pb.y & 0xffffu) + 2u * ulen + pay);
        P[2] = SegPatch{l4 + 4u, 4u, bswap16(ulen) | (bswap16(uck) << 16)};
        P[3] = P[4] = SegPatch{0u, 0u, 0u};
        return;
    }
    const uint32_t seq = pb.z + o.done;
    uint32_t w12 = pb.y >> 16;
    if (!o.last) w12 &= ~0x09u;                                   // FIN, PSH: the last segment's
    if (k != 0u) w12 &= ~0x80u;                                   // CWR: the first segment's
    const uint32_t tlen = po - l4 + pk;
    const uint32_t tck = ~fold16((pb.y & 0xffffu) + (seq >> 16) + (seq & 0xffffu) + w12 + tlen + pay) &
                         0xffffu;
    P[2] = SegPatch{l4 + 4u, 4u, bswap32(seq)};
    P[3] = SegPatch{l4 + 13u, 1u, w12 & 0xffu};
    P[4] = SegPatch{l4 + 16u, 2u, bswap16(tck)};
}

// Output j, the k-th of the input frame with plan (pa, pb) and output byte base `base`: its
// offset entry and its bytes, the whole wave.
template <bool kUdp>
__device__ __forceinline__ void write_output(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                             __amdgpu_buffer_rsrc_t ro,
                                             uint32_t* __restrict__ out_offsets, uint32_t mss,
                                             uint32_t j, uint32_t k, u32x4 pa, u32x4 pb,
                                             uint32_t base, int lane) {
    const uint32_t foff = pa.x, flen = pa.y;
    if (!(pb.w & kSegOn)) {                                       // pass-through: a byte copy
        if (lane == 0) out_offsets[j + 1] = base + flen;
        wave_copy<false>(rs, fb, ro, foff, base, flen, lane);
        return;
    }
    const SegOut o = seg_out(pa, pb, mss, k, base);
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.po + o.pk;
    // the payload slice first: its sum goes into the header, whose bytes are fetched along
    // with it (a lane past the header reads a dword it does not keep)
    const uint32_t hfirst = header_dword(rs, fb, foff, o.d0, (uint32_t)lane);
    const uint32_t part = wave_copy<true>(rs, fb, ro, foff + o.po + o.done, o.d0 + o.po, o.pk, lane);
    const uint32_t pay = be_sum(wave_sum(fold16(part)), o.d0 + o.po);
    SegPatch P[kSegPatches];
    seg_patches<kUdp>(o, pb, k, pay, P);
    wave_copy_header(rs, fb, ro, foff, o.d0, o.po, hfirst, P, lane);
}

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_write_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n, uint32_t mss,
                          const u32x4* __restrict__ plan, const uint32_t* __restrict__ seg_first,
                          const uint64_t* __restrict__ obase, const uint64_t* __restrict__ totals,
                          uint8_t* __restrict__ out, uint32_t out_bytes,
                          uint32_t* __restrict__ out_offsets, uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, seg_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = seg_first[i], nxt = seg_first[i + 1];
    u32x4 pa = plan[2 * (size_t)i], pb = plan[2 * (size_t)i + 1];
    uint32_t base = (uint32_t)obase[i];                           // < need <= out_bytes < 4 GiB
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next frame's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = seg_first[i + 1];
            }
            pa = plan[2 * (size_t)i];
            pb = plan[2 * (size_t)i + 1];
            base = (uint32_t)obase[i];
        }
        write_output<kUdp>(rs, fb, ro, out_offsets, mss, j, j - cur, pa, pb, base, lane);
    }
}

// The chain a wave is writing outputs of: its plan, its output byte base, the cursor, and
// where the header is (hdr: the first non-empty segment's offset when [0, payload_off) lies
// in it, `flat`).
struct ChainState {
    u32x4 pa, pb;
    uint32_t base, hdr;
    bool flat;
    ChainCursor c;
};
__device__ __forceinline__ ChainState chain_state(const u32x4* __restrict__ plan,
                                                  const uint64_t* __restrict__ obase, uint32_t i,
                                                  const SegTable& S, uint32_t n_segs) {
    ChainState st;
    st.pa = plan[2 * (size_t)i];
    st.pb = plan[2 * (size_t)i + 1];
    st.base = (uint32_t)obase[i];                                 // < need <= out_bytes < 4 GiB
    st.c = ChainCursor{st.pa.x, 0u};
    st.hdr = S.fb;
    st.flat = true;
    if (st.pb.w & kSegOn) {                     // pkt_len >= payload_off > 0: a segment has bytes
        Frame s{S.fb, 0u};
        while (st.c.k < n_segs && (s = S.seg(st.c.k)).len == 0u) ++st.c.k;
        st.hdr = s.off;
        st.flat = (st.pa.w & 0xffffu) <= s.len;
    }
    return st;
}

template <bool kUdp>
__device__ __forceinline__ void write_chain_output(__amdgpu_buffer_rsrc_t rs, const SegTable& S,
                                                   uint32_t n_segs, __amdgpu_buffer_rsrc_t ro,
                                                   uint32_t* __restrict__ out_offsets, uint32_t mss,
                                                   uint32_t j, uint32_t k, ChainState& st, int lane) {
    const uint32_t fb = S.fb;
    if (!(st.pb.w & kSegOn)) {                                    // pass-through: a byte copy
        if (lane == 0) out_offsets[j + 1] = st.base + st.pa.y;
        chain_copy<false>(rs, S, n_segs, ro, st.c, 0u, st.base, st.pa.y, lane);
        return;
    }
    const SegOut o = seg_out(st.pa, st.pb, mss, k, st.base);
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.po + o.pk;
    const GatheredHeader G{S, rs, st.pa.x, n_segs, o.po};
    const uint32_t hdr = st.hdr, d0 = o.d0;
    const bool flat = st.flat;                                    // wave-uniform
    auto fetch = [&](uint32_t c) -> uint32_t {
        return flat ? header_dword(rs, fb, hdr, d0, c) : G.dw((d0 & ~3u) + 4u * c - d0);
    };
    const uint32_t hfirst = fetch((uint32_t)lane);
    const uint32_t part = chain_copy<true>(rs, S, n_segs, ro, st.c, o.po + o.done, o.d0 + o.po,
                                           o.pk, lane);
    const uint32_t pay = be_sum(wave_sum(fold16(part)), o.d0 + o.po);
    SegPatch P[kSegPatches];
    seg_patches<kUdp>(o, st.pb, k, pay, P);
    wave_copy_header_from(ro, o.d0, o.po, hfirst, P, lane, fetch);
}

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_chains_write_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                                 const uint32_t* __restrict__ segs, uint32_t n_segs, uint32_t n,
                                 uint32_t mss, const u32x4* __restrict__ plan,
                                 const uint32_t* __restrict__ seg_first,
                                 const uint64_t* __restrict__ obase,
                                 const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                                 uint32_t out_bytes, uint32_t* __restrict__ out_offsets,
                                 uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, seg_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = seg_first[i], nxt = seg_first[i + 1];
    const SegTable S{segs, fb};
    ChainState st = chain_state(plan, obase, i, S, n_segs);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next chain's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = seg_first[i + 1];
            }
            st = chain_state(plan, obase, i, S, n_segs);
        }
        write_chain_output<kUdp>(rs, S, n_segs, ro, out_offsets, mss, j, j - cur, st, lane);
    }
}

// ---- tunnels: the inner TCP / UDP of VXLAN, GTP-U and GRE frames ------------------------
//
// rpkt_gpu_segment_tunnel_batch cuts the inner frame of a decoded tunnel: the inner record's
// offsets are positions in the outer frame, so the cut is the flat one with the inner record
// -- the same copy, the same inner patches -- and the outer headers follow: the outer IP
// length / ident / checksum, the outer UDP length and checksum (or the GRE checksum), the
// GTP-U length.  The plan is 64 B a frame: words 0..7 as above for the inner frame (a frame
// without a tunnel: for the frame itself, and the rest 0), then
//   8 outer l3 | outer l4 << 16, 9 tun_off, 10 outer IPv4 constant sum | outer ident << 16,
//   11 the outer L4 constant: the pseudo header (UDP) and [origin, payload_off) without the
//      bytes the write patches, origin the outer UDP header or (GRE with C) the GRE header;
//   word 7 also bit 3 a tunnel, bit 4 outer IPv6, bit 5 outer UDP (VXLAN, GTP-U; clear: GRE),
//   bit 6 GTP-U, bit 7 the outer checksum is filled (UDP: the input's field is not 0; GRE: C).
// The write forms the outer checksum from that constant, the values of the patches that lie
// under it and the payload sum the copy returned for the inner checksum: the payload is
// summed once.  A patch or the payload at an odd distance from the origin enters byte-swapped
// (it cannot happen in a frame that parsed: every header in between is even).
// The kTun* bits, the carrier rule (TunWhere, tun_where), the constants (tunnel_constants) and
// the outer patches (tunnel_patches) are in rpkt_segcopy.h: rpkt_gpu_coalesce_tunnel_batch
// (rpkt_coalesce.hip) judges a carrier by the same rule and writes a merged frame's outer
// headers as segment 0 of a cut.

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_tunnel_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                                const uint32_t* __restrict__ offsets, uint32_t stride,
                                uint32_t frame_len, uint32_t n, const rpkt_rec_t* __restrict__ outer,
                                const rpkt_tun_t* __restrict__ tun, const rpkt_rec_t* __restrict__ inner,
                                uint32_t mss, u32x4* __restrict__ plan,
                                uint32_t* __restrict__ seg_first, uint64_t* __restrict__ obase,
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
        const uint32_t o0 = w[0], o5 = w[5], o7 = w[7], o8 = w[8], o16 = w[16], o17 = w[17];
        wave_sync();
        stage_records_tile(st, inner, p0, n, lane);
        const u32x4 t = valid ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tun) + i)
                              : u32x4{0u, 0u, 0u, 0u};
        const Frame fr = valid ? frame_span(offsets, stride, frame_len, fb, i) : Frame{0u, 0u};
        // no tunnel: the frame itself under its outer record; a decoded one: its inner frame
        const bool tunnel = (t.x & 0xffu) != RPKT_TUN_NONE;
        L4Where s = l4_where(o0, o5, o7, o8, o16, o17, fr.len, kUdp);
        TunWhere tw{};
        if (tunnel) {
            s = l4_where(w, fr.len, kUdp);
            tw = tun_where(o0, o5, o7, o8, o16, t, s);
            s.on = s.on && ((t.x >> 8) & 0xffu) == RPKT_T_OK && tw.ok;
        }
        p[0] = fr.off;
        p[1] = fr.len;
        if (valid) {
            cnt = 1;
            bytes = fr.len;
        }
        if (valid && s.on && s.pl > mss) {
            const FlatHeader H{make_rsrc(frames, fb), fb, fr.off};
            uint32_t bits = 0;
            if (!tunnel || tunnel_constants(H, s, tw, q, bits)) {  // segmented
                cnt = (s.pl + mss - 1u) / mss;
                bytes = cnt * s.po + s.pl;
                seg_constants(H, s, p);
                p[7] |= bits;
            }
        }
    }
    if (valid) {
        plan[4 * (size_t)i + 2] = u32x4{q[0], q[1], q[2], q[3]};
        plan[4 * (size_t)i + 3] = u32x4{0u, 0u, 0u, 0u};
    }
    plan_store<4>(valid, i, p, cnt, bytes, plan, seg_first, obase, part, red);
}

// write_output for the 64-B plan (pa, pb, pc)
template <bool kUdp>
__device__ __forceinline__ void write_tunnel_output(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                    __amdgpu_buffer_rsrc_t ro,
                                                    uint32_t* __restrict__ out_offsets,
                                                    uint32_t mss, uint32_t j, uint32_t k, u32x4 pa,
                                                    u32x4 pb, u32x4 pc, uint32_t base, int lane) {
    const uint32_t foff = pa.x, flen = pa.y;
    if (!(pb.w & kSegOn)) {                                       // pass-through: a byte copy
        if (lane == 0) out_offsets[j + 1] = base + flen;
        wave_copy<false>(rs, fb, ro, foff, base, flen, lane);
        return;
    }
    const SegOut o = seg_out(pa, pb, mss, k, base);
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.po + o.pk;
    const uint32_t hfirst = header_dword(rs, fb, foff, o.d0, (uint32_t)lane);
    const uint32_t part = wave_copy<true>(rs, fb, ro, foff + o.po + o.done, o.d0 + o.po, o.pk, lane);
    const uint32_t pay = be_sum(wave_sum(fold16(part)), o.d0 + o.po);
    SegPatch Pi[kSegPatches], P[kTunPatches];
    seg_patches<kUdp>(o, pb, k, pay, Pi);
#pragma unroll
    for (int u = 0; u < kSegPatches; ++u) P[u] = Pi[u];
    tunnel_patches(o, pb, pc, k, pay, P);
    wave_copy_header(rs, fb, ro, foff, o.d0, o.po, hfirst, P, lane);
}

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_tunnel_write_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                                 uint32_t mss, const u32x4* __restrict__ plan,
                                 const uint32_t* __restrict__ seg_first,
                                 const uint64_t* __restrict__ obase,
                                 const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                                 uint32_t out_bytes, uint32_t* __restrict__ out_offsets,
                                 uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, seg_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = seg_first[i], nxt = seg_first[i + 1];
    u32x4 pa = plan[4 * (size_t)i], pb = plan[4 * (size_t)i + 1], pc = plan[4 * (size_t)i + 2];
    uint32_t base = (uint32_t)obase[i];                           // < need <= out_bytes < 4 GiB
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next frame's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = seg_first[i + 1];
            }
            pa = plan[4 * (size_t)i];
            pb = plan[4 * (size_t)i + 1];
            pc = plan[4 * (size_t)i + 2];
            base = (uint32_t)obase[i];
        }
        write_tunnel_output<kUdp>(rs, fb, ro, out_offsets, mss, j, j - cur, pa, pb, pc, base, lane);
    }
}

// ---- tunnels over mbuf chains ----------------------------------------------------------
//
// rpkt_gpu_segment_tunnel_chains is the two above put together: the chain plan's walk for
// pkt_len and the first non-empty segment with the tunnel plan's three records and 64-B plan,
// the chain write's cursor and flat-or-gathered header with the tunnel write's nine patches.
// The header here is [0, inner payload_off): the outer, tunnel and inner headers together.

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_tunnel_chains_plan_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                                       const uint32_t* __restrict__ segs, uint32_t n_segs,
                                       const uint32_t* __restrict__ chain_first, uint32_t n,
                                       const rpkt_rec_t* __restrict__ outer,
                                       const rpkt_tun_t* __restrict__ tun,
                                       const rpkt_rec_t* __restrict__ inner, uint32_t mss,
                                       u32x4* __restrict__ plan, uint32_t* __restrict__ seg_first,
                                       uint64_t* __restrict__ obase, uint64_t* __restrict__ part) {
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
        const uint32_t o0 = w[0], o5 = w[5], o7 = w[7], o8 = w[8], o16 = w[16], o17 = w[17];
        wave_sync();
        stage_records_tile(st, inner, p0, n, lane);
        const u32x4 t = valid ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tun) + i)
                              : u32x4{0u, 0u, 0u, 0u};
        // pkt_len in 64 bits and the first non-empty segment, as segment_chains_plan_kernel
        const SegTable S{segs, fb};
        uint32_t a = 0, b = 0;
        if (valid) chain_range(chain_first, n_segs, i, a, b);
        uint64_t pkt = 0;
        Frame s0{fb, 0u};
        for (uint32_t k = a; k < b; ++k) {
            const Frame sg = S.seg(k);
            if (pkt == 0) s0 = sg;
            pkt += sg.len;
        }
        const uint32_t len = pkt < 0xffffffffull ? (uint32_t)pkt : 0xffffffffu;
        // no tunnel: the chain itself under its outer record; a decoded one: its inner frame
        const bool tunnel = (t.x & 0xffu) != RPKT_TUN_NONE;
        L4Where s = l4_where(o0, o5, o7, o8, o16, o17, len, kUdp);
        TunWhere tw{};
        if (tunnel) {
            s = l4_where(w, len, kUdp);
            tw = tun_where(o0, o5, o7, o8, o16, t, s);
            s.on = s.on && ((t.x >> 8) & 0xffu) == RPKT_T_OK && tw.ok;
        }
        p[0] = a;
        p[1] = len;
        if (valid) {
            cnt = 1;
            bytes = pkt;
        }
        if (valid && s.on && s.pl > mss) {
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
            uint32_t bits = 0;
            bool cut;
            if (__builtin_expect(s.po <= s0.len, 1)) {
                const FlatHeader H{rs, fb, s0.off};
                cut = !tunnel || tunnel_constants(H, s, tw, q, bits);
                if (cut) seg_constants(H, s, p);
            } else {
                const GatheredHeader H{S, rs, a, n_segs, s.po};
                cut = !tunnel || tunnel_constants(H, s, tw, q, bits);
                if (cut) seg_constants(H, s, p);
            }
            if (cut) {                                            // segmented
                cnt = (s.pl + mss - 1u) / mss;
                bytes = cnt * s.po + s.pl;
                p[7] |= bits;
            }
        }
    }
    if (valid) {
        plan[4 * (size_t)i + 2] = u32x4{q[0], q[1], q[2], q[3]};
        plan[4 * (size_t)i + 3] = u32x4{0u, 0u, 0u, 0u};
    }
    plan_store<4>(valid, i, p, cnt, bytes, plan, seg_first, obase, part, red);
}

// chain_state for the 64-B plan: ChainState and plan words 8..11
struct TunnelChainState {
    ChainState s;
    u32x4 pc;
};
__device__ __forceinline__ TunnelChainState tunnel_chain_state(const u32x4* __restrict__ plan,
                                                               const uint64_t* __restrict__ obase,
                                                               uint32_t i, const SegTable& S,
                                                               uint32_t n_segs) {
    TunnelChainState t;
    ChainState& st = t.s;
    st.pa = plan[4 * (size_t)i];
    st.pb = plan[4 * (size_t)i + 1];
    t.pc = plan[4 * (size_t)i + 2];
    st.base = (uint32_t)obase[i];                                 // < need <= out_bytes < 4 GiB
    st.c = ChainCursor{st.pa.x, 0u};
    st.hdr = S.fb;
    st.flat = true;
    if (st.pb.w & kSegOn) {                     // pkt_len >= payload_off > 0: a segment has bytes
        Frame s{S.fb, 0u};
        while (st.c.k < n_segs && (s = S.seg(st.c.k)).len == 0u) ++st.c.k;
        st.hdr = s.off;
        st.flat = (st.pa.w & 0xffffu) <= s.len;
    }
    return t;
}

// write_chain_output for the 64-B plan
template <bool kUdp>
__device__ __forceinline__ void write_tunnel_chain_output(__amdgpu_buffer_rsrc_t rs, const SegTable& S,
                                                          uint32_t n_segs, __amdgpu_buffer_rsrc_t ro,
                                                          uint32_t* __restrict__ out_offsets,
                                                          uint32_t mss, uint32_t j, uint32_t k,
                                                          TunnelChainState& t, int lane) {
    ChainState& st = t.s;
    const uint32_t fb = S.fb;
    if (!(st.pb.w & kSegOn)) {                                    // pass-through: a byte copy
        if (lane == 0) out_offsets[j + 1] = st.base + st.pa.y;
        chain_copy<false>(rs, S, n_segs, ro, st.c, 0u, st.base, st.pa.y, lane);
        return;
    }
    const SegOut o = seg_out(st.pa, st.pb, mss, k, st.base);
    if (lane == 0) out_offsets[j + 1] = o.d0 + o.po + o.pk;
    const GatheredHeader G{S, rs, st.pa.x, n_segs, o.po};
    const uint32_t hdr = st.hdr, d0 = o.d0;
    const bool flat = st.flat;                                    // wave-uniform
    auto fetch = [&](uint32_t c) -> uint32_t {
        return flat ? header_dword(rs, fb, hdr, d0, c) : G.dw((d0 & ~3u) + 4u * c - d0);
    };
    const uint32_t hfirst = fetch((uint32_t)lane);
    // the payload is summed once: for the inner checksum and under the outer one
    const uint32_t part = chain_copy<true>(rs, S, n_segs, ro, st.c, o.po + o.done, o.d0 + o.po,
                                           o.pk, lane);
    const uint32_t pay = be_sum(wave_sum(fold16(part)), o.d0 + o.po);
    SegPatch Pi[kSegPatches], P[kTunPatches];
    seg_patches<kUdp>(o, st.pb, k, pay, Pi);
#pragma unroll
    for (int u = 0; u < kSegPatches; ++u) P[u] = Pi[u];
    tunnel_patches(o, st.pb, t.pc, k, pay, P);
    wave_copy_header_from(ro, o.d0, o.po, hfirst, P, lane, fetch);
}

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void segment_tunnel_chains_write_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                                        const uint32_t* __restrict__ segs, uint32_t n_segs,
                                        uint32_t n, uint32_t mss, const u32x4* __restrict__ plan,
                                        const uint32_t* __restrict__ seg_first,
                                        const uint64_t* __restrict__ obase,
                                        const uint64_t* __restrict__ totals,
                                        uint8_t* __restrict__ out, uint32_t out_bytes,
                                        uint32_t* __restrict__ out_offsets, uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t j0, jend, i;
    if (!output_run(n, seg_first, totals, out_bytes, out_offsets, out_cap, lane, j0, jend, i)) return;
    uint32_t cur = seg_first[i], nxt = seg_first[i + 1];
    const SegTable S{segs, fb};
    TunnelChainState t = tunnel_chain_state(plan, obase, i, S, n_segs);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < jend; ++j) {
        if (j >= nxt) {                                           // the next chain's first output
            while (j >= nxt && i + 1u < n) {
                ++i;
                cur = nxt;
                nxt = seg_first[i + 1];
            }
            t = tunnel_chain_state(plan, obase, i, S, n_segs);
        }
        write_tunnel_chain_output<kUdp>(rs, S, n_segs, ro, out_offsets, mss, j, j - cur, t, lane);
    }
}

}  // namespace

extern "C" {

size_t rpkt_gpu_segment_workspace_bytes(uint32_t n) { return seg_ws(nullptr, n).bytes; }

int rpkt_gpu_segment_batch(const rpkt_batch_t* b, const rpkt_rec_t* recs_dev, uint32_t mss,
                           uint32_t flags, uint8_t* out_frames_dev, uint64_t out_bytes,
                           uint32_t* out_offsets_dev, uint32_t out_cap, uint32_t* seg_first_dev,
                           uint64_t* totals_dev, void* workspace_dev, void* stream) {
    RPKT_TRY(reframe_args_ok(b, recs_dev, mss, flags, RPKT_SEGMENT_UDP, out_frames_dev, out_bytes,
                             out_offsets_dev, out_cap, seg_first_dev, totals_dev, workspace_dev));
    if (b->n == 0) return RPKT_OK;

    const SegWs ws = seg_ws(workspace_dev, b->n);
    const bool udp = (flags & RPKT_SEGMENT_UDP) != 0u;
    RPKT_TRY(launch_batch(udp ? segment_plan_kernel<true> : segment_plan_kernel<false>, kSegBlock, 0,
                          stream, *b, recs_dev, mss, ws.plan, seg_first_dev, ws.obase, ws.part));
    return scan_and_write(udp ? segment_write_kernel<true> : segment_write_kernel<false>, ws, b->n, out_cap, seg_first_dev, totals_dev,
                          (hipStream_t)stream, b->frames_dev, (uint32_t)b->frames_bytes, b->n, mss,
                          ws.plan, seg_first_dev, ws.obase, totals_dev, out_frames_dev,
                          (uint32_t)out_bytes, out_offsets_dev, out_cap);
}

size_t rpkt_gpu_segment_chains_workspace_bytes(uint32_t n) { return seg_ws(nullptr, n).bytes; }

int rpkt_gpu_segment_chains(const rpkt_chains_t* c, const rpkt_rec_t* recs_dev, uint32_t mss,
                            uint32_t flags, uint8_t* out_frames_dev, uint64_t out_bytes,
                            uint32_t* out_offsets_dev, uint32_t out_cap, uint32_t* seg_first_dev,
                            uint64_t* totals_dev, void* workspace_dev, void* stream) {
    RPKT_TRY(reframe_args_ok(c, recs_dev, mss, flags, RPKT_SEGMENT_UDP, out_frames_dev, out_bytes,
                             out_offsets_dev, out_cap, seg_first_dev, totals_dev, workspace_dev));
    if (c->n_chains == 0) return RPKT_OK;

    const uint32_t n = c->n_chains, fb = (uint32_t)c->buf_bytes;
    const uint32_t* segs = c->segs_dev;
    const SegWs ws = seg_ws(workspace_dev, n);
    const bool udp = (flags & RPKT_SEGMENT_UDP) != 0u;
    RPKT_TRY(launch(udp ? segment_chains_plan_kernel<true> : segment_chains_plan_kernel<false>,
                    dim3(blocks(n)), dim3(kSegBlock), 0, (hipStream_t)stream, c->buf_dev, fb, segs,
                    c->n_segs, c->chain_first_dev, n, recs_dev, mss, ws.plan, seg_first_dev, ws.obase,
                    ws.part));
    return scan_and_write(udp ? segment_chains_write_kernel<true> : segment_chains_write_kernel<false>, ws, n, out_cap, seg_first_dev, totals_dev,
                          (hipStream_t)stream, c->buf_dev, fb, segs, c->n_segs, n, mss, ws.plan,
                          seg_first_dev, ws.obase, totals_dev, out_frames_dev, (uint32_t)out_bytes,
                          out_offsets_dev, out_cap);
}

size_t rpkt_gpu_segment_tunnel_workspace_bytes(uint32_t n) { return seg_ws(nullptr, n, 4).bytes; }

int rpkt_gpu_segment_tunnel_batch(const rpkt_batch_t* b, const rpkt_rec_t* outer_dev,
                                  const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                  uint32_t mss, uint32_t flags, uint8_t* out_frames_dev,
                                  uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                                  uint32_t* seg_first_dev, uint64_t* totals_dev, void* workspace_dev,
                                  void* stream) {
    RPKT_TRY(reframe_args_ok(b, outer_dev, mss, flags, RPKT_SEGMENT_UDP, out_frames_dev, out_bytes,
                             out_offsets_dev, out_cap, seg_first_dev, totals_dev, workspace_dev,
                             tun_dev, inner_dev));
    if (b->n == 0) return RPKT_OK;

    const SegWs ws = seg_ws(workspace_dev, b->n, 4);
    const bool udp = (flags & RPKT_SEGMENT_UDP) != 0u;
    RPKT_TRY(launch_batch(udp ? segment_tunnel_plan_kernel<true> : segment_tunnel_plan_kernel<false>,
                          kSegBlock, 0, stream, *b, outer_dev, tun_dev, inner_dev, mss, ws.plan,
                          seg_first_dev, ws.obase, ws.part));
    return scan_and_write(udp ? segment_tunnel_write_kernel<true> : segment_tunnel_write_kernel<false>,
                          ws, b->n, out_cap, seg_first_dev, totals_dev, (hipStream_t)stream,
                          b->frames_dev, (uint32_t)b->frames_bytes, b->n, mss, ws.plan, seg_first_dev,
                          ws.obase, totals_dev, out_frames_dev, (uint32_t)out_bytes, out_offsets_dev,
                          out_cap);
}

size_t rpkt_gpu_segment_tunnel_chains_workspace_bytes(uint32_t n) {
    return seg_ws(nullptr, n, 4).bytes;
}

int rpkt_gpu_segment_tunnel_chains(const rpkt_chains_t* c, const rpkt_rec_t* outer_dev,
                                   const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                   uint32_t mss, uint32_t flags, uint8_t* out_frames_dev,
                                   uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                                   uint32_t* seg_first_dev, uint64_t* totals_dev,
                                   void* workspace_dev, void* stream) {
    RPKT_TRY(reframe_args_ok(c, outer_dev, mss, flags, RPKT_SEGMENT_UDP, out_frames_dev, out_bytes,
                             out_offsets_dev, out_cap, seg_first_dev, totals_dev, workspace_dev,
                             tun_dev, inner_dev));
    if (c->n_chains == 0) return RPKT_OK;

    const uint32_t n = c->n_chains, fb = (uint32_t)c->buf_bytes;
    const uint32_t* segs = c->segs_dev;
    const SegWs ws = seg_ws(workspace_dev, n, 4);
    const bool udp = (flags & RPKT_SEGMENT_UDP) != 0u;
    RPKT_TRY(launch(udp ? segment_tunnel_chains_plan_kernel<true>
                        : segment_tunnel_chains_plan_kernel<false>,
                    dim3(blocks(n)), dim3(kSegBlock), 0, (hipStream_t)stream, c->buf_dev, fb, segs,
                    c->n_segs, c->chain_first_dev, n, outer_dev, tun_dev, inner_dev, mss, ws.plan,
                    seg_first_dev, ws.obase, ws.part));
    return scan_and_write(udp ? segment_tunnel_chains_write_kernel<true>
                              : segment_tunnel_chains_write_kernel<false>,
                          ws, n, out_cap, seg_first_dev, totals_dev, (hipStream_t)stream, c->buf_dev,
                          fb, segs, c->n_segs, n, mss, ws.plan, seg_first_dev, ws.obase, totals_dev,
                          out_frames_dev, (uint32_t)out_bytes, out_offsets_dev, out_cap);
}

}  // extern "C"
