// rpkt_coalesce.hip — rpkt_gpu_coalesce_batch: TCP receive coalescing (GRO / LRO) of a
// device-resident batch, what the port's LRO offload does for rpkt-dpdk/examples/lro_rx.rs
// and the inverse of rpkt_gpu_segment_batch (include/rpkt_gpu.h has the semantics).  With
// RPKT_COALESCE_UDP also UDP datagrams (the Linux udp_gro_receive_segment rules): a second L4
// rule in the plan's eligibility, the link's predicate and the header patches.
//
// Many input positions make one output, so the work is planned per position and the bytes
// are placed by prefix sums.  Eight launches on the stream, no host step between them:
//   1. plan    one lane per position: its frame (through order_dev), its record (coalesced
//              through an LDS stage, or gathered under an order) and the three header dwords
//              eligibility and the predicate need (ident / DF, seq, the flags; UDP: the
//              checksum field);
//   2. link    one lane per position: B(i), the masked compare of its header with its
//              predecessor's, a dword of each per step through the buffer resource; B(i - 1)
//              from the neighbouring lane (the block's first lane computes it); link and
//              short; the block's max-scan of run heads;
//   3. heads   one block: the max-scan of the blocks' last run heads, with a carry;
//   4. group   one lane per position: its run head, so its place in the run, K and whether
//              it opens a group, is merged, or is a member; its byte contribution;
//   5. sums    one block: exclusive prefix sums of the blocks' (outputs, bytes); the totals;
//   6. place   one lane per position: its output index and destination; src_first, out_mss
//              and the offsets;
//   7. copy    one wavefront per run of kCoRun consecutive POSITIONS: a lone frame is copied
//              whole, a member's (and a merged head's) payload goes to its destination with
//              the funnel-shift copy of rpkt_segcopy.h, which sums what it copies at the
//              absolute destination phase; the sum goes to the workspace;
//   8. header  one wavefront per run of kCoHdrRun OUTPUTS: for a merged one it adds its
//              members' sums (a lane each), sums the head's headers and writes them with the
//              patched lengths, flags and checksums.
// The split by input position keeps every wave's work a few frames whatever the group
// sizes (one output of 65,495 one-byte members is 8,187 copy waves, not one wave's loop);
// its price is the second pass over the merged outputs' headers.  No kernel waits on
// another workgroup and every loop is bounded by a count from the plan.
// Shared with rpkt_segment.hip through rpkt_segcopy.h: which records are the TCP frames that
// segmentation cuts (l4_where), the record stage, the block scans and launches 3 and 5, the walk
// of a header's dwords, the copy, the header write, the entry's argument checks and the
// workspace carving (rpkt_reassemble.hip follows the same launches with a fragment rule).
// Every load of frame bytes goes through the frames buffer resource and every store of
// output bytes through one over [out_frames_dev, + out_bytes); an overflowing call (totals
// past the capacities) writes its totals, src_first and out_mss and nothing else.
//
// rpkt_gpu_coalesce_tunnel_batch (the inner TCP / UDP of VXLAN, GTP-U and GRE frames) is the
// same eight launches with the inner record: a plan kernel of its own that also judges the
// carrier and writes 16 B more per position, <kTun> instantiations of link, group and header,
// and heads, sums, place and copy as they are; see "tunnels" below.
#include "rpkt_segcopy.h"

namespace {

// the workspace: per-position plans (32 B), destinations (u64), a u32 per position (link
// bits and the block-local run head, later the payload sum), the block sums (outputs,
// bytes: u64 pairs) and the blocks' run heads
struct CoWs {
    u32x4*    plan;
    uint64_t* obase;
    uint32_t* aux;
    uint64_t* part;
    uint32_t* pmax;
    u32x4*    tplan;      // the tunnel entry's: 16 B more per position ("tunnels" below)
    size_t    bytes;
};
inline CoWs co_ws(void* ws, uint32_t n, bool tunnel = false) {
    Carve c(ws);
    CoWs w;
    w.plan = c.take<u32x4>(2 * (size_t)n);
    w.obase = c.take<uint64_t>(n);
    w.aux = c.take<uint32_t>(n);
    w.part = c.take<uint64_t>(2 * (size_t)blocks(n));
    w.pmax = c.take<uint32_t>(blocks(n));
    w.tplan = tunnel ? c.take<u32x4>(n) : nullptr;
    w.bytes = c.used();
    return w;
}

// plan words: 0 frame offset, 1 frame length, 2 l3 | l4 << 16, 3 payload_off | payload_len
// << 16 (2 and 3: 0 unless eligible), 4 seq (UDP: 0), 5 ident | TCP byte 13 << 16 (UDP: 0),
// 6 kCoElig | kCoV6 | kCoDF | kCoUdp | ip6_pdst_off << 16, 7 (from group on) kCoHead |
// kCoMerged | the run head's payload_len << 16
constexpr uint32_t kCoElig = 1u, kCoV6 = 2u, kCoDF = 4u, kCoUdp = 8u;
constexpr uint32_t kCoHead = 1u, kCoMerged = 2u;
// aux (link .. group): the block-local index + 1 of the position's run head (0: in an earlier
// block) | kCoLink | kCoShort
constexpr uint32_t kCoLink = 1u << 16, kCoShort = 1u << 17;

constexpr uint32_t kFin = 0x01u, kSyn = 0x02u, kRst = 0x04u, kPsh = 0x08u, kUrg = 0x20u, kCwr = 0x80u;

// ---- 1. plan ---------------------------------------------------------------------------

// What the header of a frame that may be eligible (`s`) adds to its plan: seq, ident | TCP byte
// 13 << 16, kCoDF; ok: its flags (UDP: its checksum field) allow a merge.
struct CoLook {
    uint32_t seq, idfl, df;
    bool ok;
};
__device__ __forceinline__ CoLook co_look(__amdgpu_buffer_rsrc_t rs, uint32_t fb, uint32_t foff,
                                          const L4Where& s) {
    const uint32_t a3 = foff + s.l3, a4 = foff + s.l4;
    // t1: TCP's seq, UDP's length and checksum; a UDP frame has no byte 13 (t3 is payload)
    const uint32_t t1 = gdword(rs, fb, a4 + 4u), t3 = gdword(rs, fb, a4 + 12u);
    const uint32_t tf = s.udp ? 0u : (t3 >> 8) & 0xffu;           // TCP byte 13
    CoLook k{s.udp ? 0u : bswap32(t1), tf << 16, 0u, false};
    if (!s.v6) {
        const uint32_t ip1 = gdword(rs, fb, a3 + 4u);
        k.idfl |= be16_lo(ip1);
        k.df = (be16_hi(ip1) & 0x4000u) ? kCoDF : 0u;
    }
    // a UDP datagram sent without a checksum (field 0) is not merged, sums trusted or not
    k.ok = s.udp ? be16_hi(t1) != 0u : (tf & (kSyn | kRst | kUrg)) == 0u;
    return k;
}

// position i's plan words 0..7
__device__ __forceinline__ void plan_store(u32x4* __restrict__ plan, uint32_t i, Frame fr,
                                           const L4Where& s, bool elig, const CoLook& k) {
    plan[2 * (size_t)i] = u32x4{fr.off, fr.len, elig ? s.l3 | (s.l4 << 16) : 0u,
                                elig ? s.po | (s.pl << 16) : 0u};
    const uint32_t bits = kCoElig | (s.v6 ? kCoV6 : 0u) | k.df | (s.udp ? kCoUdp : 0u);
    plan[2 * (size_t)i + 1] = u32x4{k.seq, k.idfl, elig ? bits | (s.pdst << 16) : 0u, 0u};
}

// <kUdp>: the entry's RPKT_COALESCE_UDP.  The kernels that test the protocol (plan, link,
// header) take it as a template argument, so a call without the flag launches the code
// without the tests.
template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void coalesce_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                          const uint32_t* __restrict__ offsets, uint32_t stride, uint32_t frame_len,
                          uint32_t n, const rpkt_rec_t* __restrict__ recs,
                          const uint32_t* __restrict__ order, uint32_t trust,
                          u32x4* __restrict__ plan) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    if (p0 >= n) return;                                          // wave-uniform

    uint32_t f = valid ? i : n;                                   // the position's frame
    uint32_t w0 = 0, w5 = 0, w7 = 0, w8 = 0, w16 = 0, w17 = 0, w18 = 0;
    if (!order) {
        uint32_t* st = stage[wave];
        stage_records_tile(st, recs, p0, n, lane);
        const uint32_t* w = st + lane * 21;
        w0 = w[0], w5 = w[5], w7 = w[7], w8 = w[8], w16 = w[16], w17 = w[17], w18 = w[18];
    } else {
        if (valid) f = order[i];
        if (f < n) {                                              // an entry >= n: an empty frame
            const u32x4* r = reinterpret_cast<const u32x4*>(recs + f);
            const u32x4 q0 = r[0], q1 = r[1], q2 = r[2], q4 = r[4];
            w0 = q0.x, w5 = q1.y, w7 = q1.w, w8 = q2.x, w16 = q4.x, w17 = q4.y, w18 = q4.z;
        }
    }
    const bool present = f < n;
    const Frame fr = present ? frame_span(offsets, stride, frame_len, fb, f) : Frame{0u, 0u};
    // the frames segmentation cuts, with a payload and sums that verified
    const L4Where s = l4_where(w0, w5, w7, w8, w16, w17, fr.len, kUdp);
    const bool sums = trust || ((w18 >> 16) == 0xffffu && (s.v6 || (w18 & 0xffffu) == 0xffffu));
    bool elig = present && s.on && s.pl >= 1u && sums;
    CoLook k{0u, 0u, 0u, false};
    if (elig) {
        k = co_look(make_rsrc(frames, fb), fb, fr.off, s);
        elig = k.ok;
    }
    if (valid) plan_store(plan, i, fr, s, elig, k);
}

// ---- tunnels: the inner TCP / UDP of VXLAN, GTP-U and GRE frames ------------------------
//
// rpkt_gpu_coalesce_tunnel_batch merges the inner frames of decoded tunnels: the inner
// record's offsets are positions in the outer frame, so a tunnelled position's 32-B plan is
// the flat one under the inner record -- group, place and copy do not know the difference --
// and 16 B more per position (tplan) carry the carrier:
//   x outer l3 | outer l4 << 16, y tun_off | inner_off << 16, z outer ident | outer
//   ip6_pdst_off << 16, w kTunOn | kTunV6 | kTunUdp | kTunGtp | kTunCsum (the outer UDP
//   checksum field is not 0; GRE: C) | kTunDF (all 0 unless an eligible tunnelled position).
// The carrier rule is segmentation's (tun_where, rpkt_segcopy.h); the plan adds the length
// fields that must agree and the outer sums, the link the outer bytes that may differ, the
// outer ident and the zero / non-zero outer checksum, the group the outer IP's limit, the
// header the outer patches (tunnel_constants and tunnel_patches, as segment 0 of a cut).
// These take <kTun>: the flat entry launches the code without any of it.
constexpr uint32_t kTunDF = 256u;

template <bool kUdp>
__global__ __launch_bounds__(kSegBlock)
void coalesce_tunnel_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                                 const uint32_t* __restrict__ offsets, uint32_t stride,
                                 uint32_t frame_len, uint32_t n, const rpkt_rec_t* __restrict__ outer,
                                 const rpkt_tun_t* __restrict__ tun, const rpkt_rec_t* __restrict__ inner,
                                 const uint32_t* __restrict__ order, uint32_t trust,
                                 u32x4* __restrict__ plan, u32x4* __restrict__ tplan) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    if (p0 >= n) return;                                          // wave-uniform

    uint32_t f = valid ? i : n;                                   // the position's frame
    uint32_t o[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u}, in[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    u32x4 t = {0u, 0u, 0u, 0u};
    const u32x4* tq = reinterpret_cast<const u32x4*>(tun);
    if (!order) {
        // the tile's outer records through the stage, then its inner records through the same
        uint32_t* st = stage[wave];
        const uint32_t* w = st + lane * 21;
        stage_records_tile(st, outer, p0, n, lane);
        o[0] = w[0], o[1] = w[5], o[2] = w[7], o[3] = w[8], o[4] = w[16], o[5] = w[17], o[6] = w[18];
        wave_sync();
        stage_records_tile(st, inner, p0, n, lane);
        in[0] = w[0], in[1] = w[5], in[2] = w[7], in[3] = w[8], in[4] = w[16], in[5] = w[17], in[6] = w[18];
        if (valid) t = __builtin_nontemporal_load(tq + i);
    } else {
        if (valid) f = order[i];
        if (f < n) {                                              // an entry >= n: an empty frame
            const u32x4* r = reinterpret_cast<const u32x4*>(outer + f);
            const u32x4 q0 = r[0], q1 = r[1], q2 = r[2], q4 = r[4];
            o[0] = q0.x, o[1] = q1.y, o[2] = q1.w, o[3] = q2.x, o[4] = q4.x, o[5] = q4.y, o[6] = q4.z;
            t = tq[f];
            if ((t.x & 0xffu) != RPKT_TUN_NONE) {
                const u32x4* ri = reinterpret_cast<const u32x4*>(inner + f);
                const u32x4 j0 = ri[0], j1 = ri[1], j2 = ri[2], j4 = ri[4];
                in[0] = j0.x, in[1] = j1.y, in[2] = j1.w, in[3] = j2.x, in[4] = j4.x, in[5] = j4.y,
                in[6] = j4.z;
            }
        }
    }
    const bool present = f < n;
    const Frame fr = present ? frame_span(offsets, stride, frame_len, fb, f) : Frame{0u, 0u};
    // no tunnel: the frame itself under its outer record; a decoded one: its inner frame, with
    // the inner record's verdicts
    const bool tunnel = (t.x & 0xffu) != RPKT_TUN_NONE;
    L4Where s = l4_where(o[0], o[1], o[2], o[3], o[4], o[5], fr.len, kUdp);
    uint32_t w18 = o[6];
    TunWhere tw{};
    if (tunnel) {
        s = l4_where(in[0], in[1], in[2], in[3], in[4], in[5], fr.len, kUdp);
        tw = tun_where(o[0], o[1], o[2], o[3], o[4], t, s);
        s.on = s.on && ((t.x >> 8) & 0xffu) == RPKT_T_OK && tw.ok;
        w18 = in[6];
    }
    const bool sums = trust || ((w18 >> 16) == 0xffffu && (s.v6 || (w18 & 0xffffu) == 0xffffu));
    bool elig = present && s.on && s.pl >= 1u && sums;
    CoLook k{0u, 0u, 0u, false};
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    if (elig) {
        k = co_look(rs, fb, fr.off, s);
        elig = k.ok;
    }
    u32x4 pt = {0u, 0u, 0u, 0u};
    if (elig && tunnel) {
        // the length fields a merge rewrites say tot already; the GRE bits; the outer sums
        const FlatHeader H{rs, fb, fr.off};
        const uint32_t tot = s.po + s.pl;                         // >= every offset below: they nest
        bool ok, csum;
        if (tw.udp) {
            const uint32_t u1 = H.dw(tw.l4 + 4u);
            csum = be16_hi(u1) != 0u;
            ok = be16_lo(u1) == tot - tw.l4;
            if (tw.gtp) ok = ok && be16_hi(H.dw(tw.toff)) == tot - tw.toff - 8u;
        } else {
            const uint32_t g0 = H.dw(tw.toff) & 0xffu;            // C 0x80, R 0x40, K 0x20, S 0x10
            csum = (g0 & 0x80u) != 0u;
            ok = !(g0 & 0x50u) && !(csum && tw.toff + 8u > tw.ioff);
        }
        uint32_t oident = 0, odf = 0;
        if (!tw.v6) {
            const uint32_t ip0 = H.dw(tw.l3), ip1 = H.dw(tw.l3 + 4u);
            ok = ok && be16_hi(ip0) == tot - tw.l3;
            oident = be16_lo(ip1);
            odf = (be16_hi(ip1) & 0x4000u) ? kTunDF : 0u;
        } else {
            ok = ok && be16_lo(H.dw(tw.l3 + 4u)) == tot - tw.l3 - 40u;
        }
        if (!trust)
            ok = ok && (tw.v6 || (o[6] & 0xffffu) == 0xffffu) && (!csum || (o[6] >> 16) == 0xffffu);
        elig = ok;
        if (ok)
            pt = u32x4{tw.l3 | (tw.l4 << 16), tw.toff | (tw.ioff << 16), oident | (tw.pdst << 16),
                       kTunOn | (tw.v6 ? kTunV6 : 0u) | (tw.udp ? kTunUdp : 0u) |
                           (tw.gtp ? kTunGtp : 0u) | (csum ? kTunCsum : 0u) | odf};
    }
    if (valid) {
        plan_store(plan, i, fr, s, elig, k);
        tplan[i] = pt;
    }
}

// ---- 2. link ---------------------------------------------------------------------------

// which bits of the header dword at frame offset x enter the compare.  One mask serves both
// protocols: UDP's ignored bytes l4+4..7 (length, checksum) are where TCP's seq is, and its
// header ends (po = l4 + 8) before the other TCP fields.
__device__ __forceinline__ uint32_t header_keep(uint32_t x, uint32_t l3, uint32_t l4, uint32_t po,
                                                bool v6) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t y = x + b, d3 = y - l3, d4 = y - l4;
        uint32_t keep = 0xffu;
        if (y >= po) keep = 0u;
        else if (!v6 && ((d3 >= 2u && d3 <= 5u) || d3 == 10u || d3 == 11u)) keep = 0u;
        else if (v6 && (d3 == 4u || d3 == 5u)) keep = 0u;
        else if ((d4 >= 4u && d4 <= 7u) || d4 == 16u || d4 == 17u) keep = 0u;
        else if (d4 == 13u) keep = 0xffu & ~(kFin | kPsh | kCwr);
        m |= keep << (8u * b);
    }
    return m;
}

// the same for the outer headers of a tunnelled position with tplan words `t`: the outer IP's
// length, ident and checksum bytes, the outer UDP's length and checksum, the GTP-U length, the
// GRE checksum.  They lie before the inner headers, so the two masks are ANDed.
__device__ __forceinline__ uint32_t outer_keep(uint32_t x, u32x4 t) {
    const uint32_t l3 = t.x & 0xffffu, l4 = t.x >> 16, toff = t.y & 0xffffu;
    const bool v6 = (t.w & kTunV6) != 0u, udp = (t.w & kTunUdp) != 0u;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t y = x + b, d3 = y - l3, d4 = y - l4, dt = y - toff;
        uint32_t keep = 0xffu;
        if (!v6 && ((d3 >= 2u && d3 <= 5u) || d3 == 10u || d3 == 11u)) keep = 0u;
        else if (v6 && (d3 == 4u || d3 == 5u)) keep = 0u;
        else if (udp && d4 >= 4u && d4 <= 7u) keep = 0u;
        else if ((t.w & kTunGtp) && (dt == 2u || dt == 3u)) keep = 0u;
        else if (!udp && (t.w & kTunCsum) && (dt == 4u || dt == 5u)) keep = 0u;
        m |= keep << (8u * b);
    }
    return m;
}

// B(i), i >= 1: the frame at position i continues the one at i - 1
template <bool kUdp, bool kTun>
__device__ __forceinline__ bool base_pred(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                          const u32x4* __restrict__ plan,
                                          const u32x4* __restrict__ tplan, uint32_t i) {
    const u32x4 pa = plan[2 * (size_t)i], pb = plan[2 * (size_t)i + 1];
    const u32x4 qa = plan[2 * (size_t)i - 2], qb = plan[2 * (size_t)i - 1];
    if (!(pb.z & qb.z & kCoElig) || ((pb.z ^ qb.z) & (kCoV6 | (kUdp ? kCoUdp : 0u))))
        return false;
    u32x4 pt = {0u, 0u, 0u, 0u};
    if (kTun) {
        // a tunnelled position continues one in the same kind of tunnel over the same outer IP
        // version at the same offsets, both outer checksums filled or both 0; the outer ident
        pt = tplan[i];
        const u32x4 qt = tplan[i - 1u];
        if (((pt.w ^ qt.w) & (kTunOn | kTunV6 | kTunUdp | kTunGtp | kTunCsum)) || pt.x != qt.x ||
            pt.y != qt.y)
            return false;
        if ((pt.w & kTunOn) && !(pt.w & (kTunV6 | kTunDF)) && ((pt.z ^ (qt.z + 1u)) & 0xffffu))
            return false;
    }
    if (pa.z != qa.z || ((pa.w ^ qa.w) & 0xffffu)) return false;          // l3, l4, payload_off
    const bool v6 = (pb.z & kCoV6) != 0u;
    // seq; UDP has no sequence and no flag condition (its flag words are 0)
    if (!(kUdp && (pb.z & kCoUdp)) && pb.x != qb.x + (qa.w >> 16)) return false;
    if (!v6 && !(pb.z & kCoDF) && ((pb.y ^ (qb.y + 1u)) & 0xffffu)) return false;   // ident
    if (((qb.y >> 16) & (kFin | kPsh)) || ((pb.y >> 16) & kCwr)) return false;
    const uint32_t l3 = pa.z & 0xffffu, l4 = pa.z >> 16, po = pa.w & 0xffffu;
    HeaderWalk a(rs, fb, pa.x), b(rs, fb, qa.x);
    if constexpr (!kTun) {
        for (uint32_t x = 0; x < po; x += 4u)                             // po <= 65535
            if ((a.next(rs, fb) ^ b.next(rs, fb)) & header_keep(x, l3, l4, po, v6)) return false;
    } else {
        const bool outer = (pt.w & kTunOn) != 0u;
        for (uint32_t x = 0; x < po; x += 4u) {
            const uint32_t d = a.next(rs, fb) ^ b.next(rs, fb);
            if (d & header_keep(x, l3, l4, po, v6) & (outer ? outer_keep(x, pt) : ~0u)) return false;
        }
    }
    return true;
}

// tplan: the tunnel entry's (<kTun>), else unused
template <bool kUdp, bool kTun>
__global__ __launch_bounds__(kSegBlock)
void coalesce_link_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                          const u32x4* __restrict__ plan, uint32_t* __restrict__ aux,
                          uint32_t* __restrict__ pmax, const u32x4* __restrict__ tplan) {
    __shared__ uint32_t bs[kSegBlock];
    __shared__ uint32_t red[kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    const bool valid = i < n;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const bool bi = valid && i >= 1u && base_pred<kUdp, kTun>(rs, fb, plan, tplan, i);
    bs[threadIdx.x] = bi ? 1u : 0u;
    __syncthreads();
    bool bp;                                                      // B(i - 1)
    if (threadIdx.x != 0u) bp = bs[threadIdx.x - 1u] != 0u;
    else bp = valid && i >= 2u && base_pred<kUdp, kTun>(rs, fb, plan, tplan, i - 1u);
    const uint32_t p = valid ? plan[2 * (size_t)i].w >> 16 : 0u;
    const uint32_t p1 = (valid && i >= 1u) ? plan[2 * (size_t)i - 2].w >> 16 : 0u;
    const uint32_t p2 = (valid && i >= 2u) ? plan[2 * (size_t)i - 4].w >> 16 : 0u;
    const bool short_prev = bp && p1 < p2;
    const bool sh = bi && p < p1;
    const bool link = bi && p <= p1 && !short_prev;
    const uint32_t hl = block_incl_max(valid && !link ? threadIdx.x + 1u : 0u, red);
    if (valid) aux[i] = hl | (link ? kCoLink : 0u) | (sh ? kCoShort : 0u);
    if (threadIdx.x == kSegBlock - 1)
        pmax[blockIdx.x] = hl ? blockIdx.x * kSegBlock + hl : 0u; // global index + 1
}

// ---- 3. heads --------------------------------------------------------------------------

// the blocks' run heads' scan: scan_heads_kernel (rpkt_segcopy.h)

// ---- 4. group --------------------------------------------------------------------------

template <bool kTun>
__global__ __launch_bounds__(kSegBlock)
void coalesce_group_kernel(uint32_t n, uint32_t max_payload, u32x4* __restrict__ plan,
                           const uint32_t* __restrict__ aux, const uint32_t* __restrict__ pmax,
                           uint64_t* __restrict__ obase, uint64_t* __restrict__ part,
                           const u32x4* __restrict__ tplan) {
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    uint64_t cnt = 0, bytes = 0;
    if (i < n) {
        const uint32_t a = aux[i], hl = a & 0xffffu;
        const bool link = (a & kCoLink) != 0u;
        const uint32_t hp = hl ? blockIdx.x * kSegBlock + hl : (blockIdx.x ? pmax[blockIdx.x - 1u] : 0u);
        const uint32_t h = hp ? hp - 1u : 0u;                     // the run's head, <= i
        const u32x4 pa = plan[2 * (size_t)i];
        const uint32_t z = plan[2 * (size_t)i + 1].z;
        const uint32_t l3 = pa.z & 0xffffu, po = pa.w & 0xffffu, p = pa.w >> 16;
        const uint32_t ph = plan[2 * (size_t)h].w >> 16;
        // a linked frame has its head's offsets and IP version
        const uint32_t iph = po - l3 - ((z & kCoV6) ? 40u : 0u);
        const uint32_t room = 65535u - (iph < 65535u ? iph : 65535u);
        uint32_t limit = max_payload < room ? max_payload : room;
        if (kTun) {
            // the outer IP's length field too (a linked frame has its head's outer offsets)
            const u32x4 t = tplan[i];
            if (t.w & kTunOn) {
                const uint32_t oph = po - (t.x & 0xffffu) - ((t.w & kTunV6) ? 40u : 0u);
                const uint32_t oroom = 65535u - (oph < 65535u ? oph : 65535u);
                limit = limit < oroom ? limit : oroom;
            }
        }
        uint32_t K = ph ? limit / ph : 0u;
        if (K == 0u) K = 1u;
        const uint32_t r = i - h;
        const bool ghead = !link || (r % K == 0u && K * ph + p > limit);
        bool nhead = true;                                        // does i + 1 open a group
        if (i + 1u < n && (aux[i + 1u] & kCoLink)) {
            const uint32_t pn = plan[2 * (size_t)i + 2].w >> 16;
            nhead = (r + 1u) % K == 0u && K * ph + pn > limit;
        }
        const bool merged = ghead && !nhead;
        cnt = ghead ? 1u : 0u;
        bytes = !ghead ? p : (merged ? po + p : pa.y);
        plan[2 * (size_t)i + 1].w = (ghead ? kCoHead : 0u) | (merged ? kCoMerged : 0u) | (ph << 16);
        obase[i] = bytes;
    }
    block_sums_to_part(cnt, bytes, part, red);
}

// ---- 5. sums ---------------------------------------------------------------------------

// the block sums' scan: scan_parts_kernel (rpkt_segcopy.h)

// ---- 6. place --------------------------------------------------------------------------

__global__ __launch_bounds__(kSegBlock)
void coalesce_place_kernel(uint32_t n, const u32x4* __restrict__ plan,
                           const uint64_t* __restrict__ part, const uint64_t* __restrict__ totals,
                           uint64_t* __restrict__ obase, uint32_t* __restrict__ src_first,
                           uint16_t* __restrict__ out_mss, uint32_t* __restrict__ out_offsets,
                           uint32_t out_cap, uint32_t out_bytes) {
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    const bool valid = i < n;
    const uint32_t role = valid ? plan[2 * (size_t)i + 1].w : 0u;
    uint64_t a = role & kCoHead, b = valid ? obase[i] : 0;
    uint64_t ta, tb;
    block_excl_scan2(a, b, ta, tb, red);
    const uint64_t n_out = totals[0], need = totals[1];
    const bool fits = n_out <= out_cap && need <= out_bytes;
    if (valid) {
        const uint64_t j = part[2 * (size_t)blockIdx.x] + a;      // < n_out <= n
        const uint64_t dest = part[2 * (size_t)blockIdx.x + 1] + b;
        obase[i] = dest;
        if (role & kCoHead) {
            src_first[j] = i;
            if (out_mss) out_mss[j] = (role & kCoMerged) ? (uint16_t)(role >> 16) : (uint16_t)0;
            if (fits) out_offsets[j] = (uint32_t)dest;            // j < n_out <= out_cap
        }
        if (i >= n_out) {
            src_first[i] = n;
            if (out_mss) out_mss[i] = 0;
        }
        if (i == 0u) src_first[n] = n;
    }
    // the end of the last output and the spare slots: empty frames at the end
    if (fits) {
        const uint64_t step = (uint64_t)gridDim.x * kSegBlock;
        for (uint64_t k = n_out + i; k <= out_cap; k += step) out_offsets[k] = (uint32_t)need;
    }
}

// ---- 7. copy ---------------------------------------------------------------------------

// A wave copies kCoRun consecutive positions (rpkt_segment.hip's kSegRun: what precedes a
// position's first copy load is a chain of dependent loads, here the plans and destinations
// of the whole run fetched at once, a lane each).
#ifndef RPKT_CO_RUN
#define RPKT_CO_RUN 8
#endif
constexpr uint32_t kCoRun = RPKT_CO_RUN;
static_assert(kCoRun <= (uint32_t)kWave, "a lane per position of the run");

__global__ __launch_bounds__(kSegBlock)
void coalesce_copy_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                          const u32x4* __restrict__ plan, const uint64_t* __restrict__ obase,
                          const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                          uint32_t out_bytes, uint32_t out_cap, uint32_t* __restrict__ aux) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t i64 = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kCoRun;
    if (i64 >= n) return;                                         // wave-uniform, as all below
    if (totals[0] > out_cap || totals[1] > out_bytes) return;     // overflow: the totals say so
    const uint32_t i0 = (uint32_t)i64;
    const uint32_t cnt = n - i0 < kCoRun ? n - i0 : kCoRun;
    u32x4 la = {0u, 0u, 0u, 0u};
    uint32_t lrole = 0, ldst = 0;
    if ((uint32_t)lane < cnt) {
        la = plan[2 * (size_t)(i0 + lane)];
        lrole = plan[2 * (size_t)(i0 + lane) + 1].w;
        ldst = (uint32_t)obase[i0 + lane];                        // < need <= out_bytes < 4 GiB
    }
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t foff = (uint32_t)__shfl((int)la.x, (int)k, kWave);
        const uint32_t flen = (uint32_t)__shfl((int)la.y, (int)k, kWave);
        const uint32_t pw = (uint32_t)__shfl((int)la.w, (int)k, kWave);
        const uint32_t role = (uint32_t)__shfl((int)lrole, (int)k, kWave);
        const uint32_t dst = (uint32_t)__shfl((int)ldst, (int)k, kWave);
        if ((role & (kCoHead | kCoMerged)) == kCoHead) {          // a lone frame: a byte copy
            wave_copy<false>(rs, fb, ro, foff, dst, flen, lane);
            continue;
        }
        // a merged head's payload follows its header; a member's is at its destination
        const uint32_t po = pw & 0xffffu, p = pw >> 16;
        const uint32_t d = dst + ((role & kCoHead) ? po : 0u);
        const uint32_t part = wave_copy<true>(rs, fb, ro, foff + po, d, p, lane);
        const uint32_t s = fold16(wave_sum(fold16(part)));
        if (lane == 0) aux[i0 + k] = s;
    }
}

// ---- 8. header -------------------------------------------------------------------------

#ifndef RPKT_CO_HDR_RUN
#define RPKT_CO_HDR_RUN 4
#endif
constexpr uint32_t kCoHdrRun = RPKT_CO_HDR_RUN;

template <bool kUdp, bool kTun>
__global__ __launch_bounds__(kSegBlock)
void coalesce_header_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                            const u32x4* __restrict__ plan, const uint64_t* __restrict__ obase,
                            const uint32_t* __restrict__ aux, const uint32_t* __restrict__ src_first,
                            const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                            uint32_t out_bytes, uint32_t out_cap, const u32x4* __restrict__ tplan) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t j64 = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kCoHdrRun;
    const uint64_t n_out = totals[0], need = totals[1];
    if (j64 >= n_out || n_out > out_cap || need > out_bytes) return;      // wave-uniform
    const uint32_t j0 = (uint32_t)j64;
    const uint32_t j1 = n_out - j0 < kCoHdrRun ? (uint32_t)n_out : j0 + kCoHdrRun;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t i0 = src_first[j], i1 = src_first[j + 1u];        // j + 1 <= n_out <= n
        if (i1 > n || i1 - i0 < 2u || i1 < i0) continue;                  // one frame: copied
        const u32x4 pa = plan[2 * (size_t)i0], pb = plan[2 * (size_t)i0 + 1];
        const uint32_t lastf = plan[2 * (size_t)i1 - 1].y >> 16;          // the last member's flags
        const uint32_t d0 = (uint32_t)obase[i0];
        const uint32_t end = i1 < n ? (uint32_t)obase[i1] : (uint32_t)need;
        const uint32_t foff = pa.x, l3 = pa.z & 0xffffu, l4 = pa.z >> 16, po = pa.w & 0xffffu;
        const bool v6 = (pb.z & kCoV6) != 0u, udp = kUdp && (pb.z & kCoUdp);   // wave-uniform
        const uint32_t pdst = pb.z >> 16;
        u32x4 pt = {0u, 0u, 0u, 0u};
        if (kTun) pt = tplan[i0];
        const bool tun = kTun && (pt.w & kTunOn);                         // wave-uniform
        const uint32_t P = end - d0 - po;                                 // the merged payload
        // the members' payload sums, all at the absolute destination phase
        uint32_t s = 0;
        for (uint32_t m = i0 + (uint32_t)lane; m < i1; m += kWave) s += aux[m];   // <= 1024 each
        const uint32_t pay = be_sum(wave_sum(fold16(s)), d0 + po);
        // the head's header sums, a lane each: IPv4 header, TCP (without flags and checksum) or
        // UDP (without length and checksum) header, pseudo addresses.  A field leaves a sum by
        // adding its complement.
        const uint32_t a3 = foff + l3, a4 = foff + l4;
        uint32_t x = 0, y = 0;
        if (lane == 0 && !v6) {
            const uint32_t ip0 = gdword(rs, fb, a3), ip2 = gdword(rs, fb, a3 + 8u);
            x = range_be_sum(rs, fb, a3, a4) + (0xffffu ^ be16_hi(ip0)) + (0xffffu ^ be16_hi(ip2));
        } else if (lane == 1) {
            x = range_be_sum(rs, fb, a4, foff + po);
            if (udp) {
                const uint32_t t1 = gdword(rs, fb, a4 + 4u);
                x += (0xffffu ^ be16_lo(t1)) + (0xffffu ^ be16_hi(t1));
            } else {
                const uint32_t t3 = gdword(rs, fb, a4 + 12u), t4 = gdword(rs, fb, a4 + 16u);
                y = be16_lo(t3);
                x += (0xffffu ^ y) + (0xffffu ^ be16_lo(t4));
            }
        } else if (lane == 2) {
            if (!v6) {
                x = range_be_sum(rs, fb, a3 + 12u, a3 + 20u);
            } else {
                const uint32_t pd = ip6_pseudo_dst(pdst, l3, l4);
                x = range_be_sum(rs, fb, a3 + 8u, a3 + 24u) +
                    range_be_sum(rs, fb, foff + pd, foff + pd + 16u);
            }
        } else if (kTun && lane == 3 && tun) {
            // the outer constants of the head as segmentation plans them: x the outer IPv4 sum
            // | ident << 16, y the outer checksum's sum without the patched bytes
            const L4Where s{true, udp, v6, l3, l4, po, 0u, pdst};
            const TunWhere w{true, (pt.w & kTunV6) != 0u, (pt.w & kTunUdp) != 0u,
                             (pt.w & kTunGtp) != 0u, pt.x & 0xffffu, pt.x >> 16, pt.y & 0xffffu,
                             pt.y >> 16, pt.z >> 16};
            uint32_t q[4] = {0u, 0u, 0u, 0u}, bits = 0;
            tunnel_constants(FlatHeader{rs, fb, foff}, s, w, q, bits);
            x = q[2];
            y = q[3];
        }
        const uint32_t ipc = (uint32_t)__builtin_amdgcn_readlane((int)x, 0);
        const uint32_t l4c = (uint32_t)__builtin_amdgcn_readlane((int)x, 1);
        const uint32_t pseudo = (uint32_t)__builtin_amdgcn_readlane((int)x, 2);
        uint32_t w12 = (uint32_t)__builtin_amdgcn_readlane((int)y, 1);
        w12 |= lastf & (kFin | kPsh);

        // A tunnelled head (<kTun>): the outer patches follow the inner ones, which then cover
        // every byte tunnel_constants takes out of the outer checksum's sum: the head's own
        // ident and seq are written again.
        SegPatch Pt[kTun ? kTunPatches : kSegPatches];
        if (!v6) {
            const uint32_t tot = po - l3 + P;
            const uint32_t ck = ~fold16(fold16(ipc) + tot) & 0xffffu;
            Pt[0] = SegPatch{l3 + 2u, 2u, bswap16(tot & 0xffffu)};
            if (tun) Pt[0] = SegPatch{l3 + 2u, 4u, bswap16(tot & 0xffffu) | (bswap16(pb.y & 0xffffu) << 16)};
            Pt[1] = SegPatch{l3 + 10u, 2u, bswap16(ck)};
        } else {
            Pt[0] = SegPatch{l3 + 4u, 2u, bswap16((po - l3 - 40u + P) & 0xffffu)};
            Pt[1] = SegPatch{0u, 0u, 0u};
        }
        const uint32_t tlen = po - l4 + P;                                // UDP: 8 + P
        if (udp) {
            // the length is in the pseudo header and in the header; a result of 0 goes as 0xffff
            const uint32_t uck = udp_csum_field(fold16(l4c) + fold16(pseudo) + 17u + 2u * tlen + pay);
            Pt[2] = SegPatch{l4 + 4u, 4u, bswap16(tlen & 0xffffu) | (bswap16(uck) << 16)};
            Pt[3] = SegPatch{0u, 0u, 0u};
        } else {
            const uint32_t tck = ~fold16(fold16(l4c) + fold16(pseudo) + 6u + w12 + tlen + pay) & 0xffffu;
            Pt[2] = SegPatch{l4 + 13u, 1u, w12 & 0xffu};
            Pt[3] = SegPatch{l4 + 16u, 2u, bswap16(tck)};
        }
        Pt[4] = SegPatch{0u, 0u, 0u};
        if constexpr (kTun) {
            if (tun && !udp) Pt[4] = SegPatch{l4 + 4u, 4u, bswap32(pb.x)};
            const uint32_t oq2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 3);
            const uint32_t oq3 = (uint32_t)__builtin_amdgcn_readlane((int)y, 3);
            const SegOut o{v6, true, l3, l4, po, 0u, P, d0};
            tunnel_patches(o, u32x4{0u, 0u, 0u, pt.w}, u32x4{pt.x, pt.y, oq2, oq3}, 0u, pay, Pt);
        }
        const uint32_t hfirst = header_dword(rs, fb, foff, d0, (uint32_t)lane);
        wave_copy_header(rs, fb, ro, foff, d0, po, hfirst, Pt, lane);
    }
}

// launches 2..8 for the `n` positions planned into ws (ws.tplan with <kTun>)
template <bool kUdp, bool kTun>
int link_and_write(const rpkt_batch_t* b, const CoWs& ws, uint32_t max_payload,
                   uint8_t* out_frames_dev, uint64_t out_bytes, uint32_t* out_offsets_dev,
                   uint32_t out_cap, uint32_t* src_first_dev, uint16_t* out_mss_dev,
                   uint64_t* totals_dev, hipStream_t st) {
    const uint32_t n = b->n, nb = blocks(n), fb = (uint32_t)b->frames_bytes;
    const dim3 blk(kSegBlock), per(nb);
    const u32x4* tplan = ws.tplan;
    RPKT_TRY(launch(coalesce_link_kernel<kUdp, kTun>, per, blk, 0, st, b->frames_dev, fb, n, ws.plan,
                    ws.aux, ws.pmax, tplan));
    RPKT_TRY(launch(scan_heads_kernel, dim3(1), blk, 0, st, ws.pmax, nb));
    RPKT_TRY(launch(coalesce_group_kernel<kTun>, per, blk, 0, st, n, max_payload, ws.plan, ws.aux,
                    ws.pmax, ws.obase, ws.part, tplan));
    RPKT_TRY(launch(scan_parts_kernel, dim3(1), blk, 0, st, ws.part, nb, totals_dev,
                    (uint32_t*)nullptr));
    RPKT_TRY(launch(coalesce_place_kernel, per, blk, 0, st, n, ws.plan, ws.part, totals_dev, ws.obase,
                    src_first_dev, out_mss_dev, out_offsets_dev, out_cap, (uint32_t)out_bytes));
    const uint64_t cper = (uint64_t)kWavesPerBlock * kCoRun;             // positions a block
    RPKT_TRY(launch(coalesce_copy_kernel, dim3((uint32_t)(((uint64_t)n + cper - 1) / cper)), blk, 0,
                    st, b->frames_dev, fb, n, ws.plan, ws.obase, totals_dev, out_frames_dev,
                    (uint32_t)out_bytes, out_cap, ws.aux));
    const uint64_t hper = (uint64_t)kWavesPerBlock * kCoHdrRun;          // outputs a block
    const uint32_t outs = n < out_cap ? n : out_cap;                     // n_out <= both, or overflow
    return launch(coalesce_header_kernel<kUdp, kTun>, dim3((uint32_t)(((uint64_t)outs + hper - 1) / hper)),
                  blk, 0, st, b->frames_dev, fb, n, ws.plan, ws.obase, ws.aux, src_first_dev,
                  totals_dev, out_frames_dev, (uint32_t)out_bytes, out_cap, tplan);
}

}  // namespace

extern "C" {

size_t rpkt_gpu_coalesce_workspace_bytes(uint32_t n) { return co_ws(nullptr, n).bytes; }

int rpkt_gpu_coalesce_batch(const rpkt_batch_t* b, const rpkt_rec_t* recs_dev,
                            const uint32_t* order_dev, uint32_t max_payload, uint32_t flags,
                            uint8_t* out_frames_dev, uint64_t out_bytes, uint32_t* out_offsets_dev,
                            uint32_t out_cap, uint32_t* src_first_dev, uint16_t* out_mss_dev,
                            uint64_t* totals_dev, void* workspace_dev, void* stream) {
    RPKT_TRY(reframe_args_ok(b, recs_dev, max_payload, flags,
                             RPKT_COALESCE_TRUST_SUMS | RPKT_COALESCE_UDP, out_frames_dev, out_bytes,
                             out_offsets_dev, out_cap, src_first_dev, totals_dev, workspace_dev));
    if (b->n == 0) return RPKT_OK;

    const CoWs ws = co_ws(workspace_dev, b->n);
    const bool udp = (flags & RPKT_COALESCE_UDP) != 0u;
    RPKT_TRY(launch_batch(udp ? coalesce_plan_kernel<true> : coalesce_plan_kernel<false>, kSegBlock, 0,
                          stream, *b, recs_dev, order_dev, flags & RPKT_COALESCE_TRUST_SUMS, ws.plan));
    return (udp ? link_and_write<true, false> : link_and_write<false, false>)(
        b, ws, max_payload, out_frames_dev, out_bytes, out_offsets_dev, out_cap, src_first_dev,
        out_mss_dev, totals_dev, (hipStream_t)stream);
}

size_t rpkt_gpu_coalesce_tunnel_workspace_bytes(uint32_t n) { return co_ws(nullptr, n, true).bytes; }

int rpkt_gpu_coalesce_tunnel_batch(const rpkt_batch_t* b, const rpkt_rec_t* outer_dev,
                                   const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                   const uint32_t* order_dev, uint32_t max_payload, uint32_t flags,
                                   uint8_t* out_frames_dev, uint64_t out_bytes,
                                   uint32_t* out_offsets_dev, uint32_t out_cap,
                                   uint32_t* src_first_dev, uint16_t* out_mss_dev,
                                   uint64_t* totals_dev, void* workspace_dev, void* stream) {
    RPKT_TRY(reframe_args_ok(b, outer_dev, max_payload, flags,
                             RPKT_COALESCE_TRUST_SUMS | RPKT_COALESCE_UDP, out_frames_dev, out_bytes,
                             out_offsets_dev, out_cap, src_first_dev, totals_dev, workspace_dev,
                             tun_dev, inner_dev));
    if (b->n == 0) return RPKT_OK;

    const CoWs ws = co_ws(workspace_dev, b->n, true);
    const bool udp = (flags & RPKT_COALESCE_UDP) != 0u;
    RPKT_TRY(launch_batch(udp ? coalesce_tunnel_plan_kernel<true> : coalesce_tunnel_plan_kernel<false>,
                          kSegBlock, 0, stream, *b, outer_dev, tun_dev, inner_dev, order_dev,
                          flags & RPKT_COALESCE_TRUST_SUMS, ws.plan, ws.tplan));
    return (udp ? link_and_write<true, true> : link_and_write<false, true>)(
        b, ws, max_payload, out_frames_dev, out_bytes, out_offsets_dev, out_cap, src_first_dev,
        out_mss_dev, totals_dev, (hipStream_t)stream);
}

}  // extern "C"
