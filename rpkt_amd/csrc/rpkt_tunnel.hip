// rpkt_tunnel.hip — rpkt_gpu_parse_tunnel_batch: the outer parse, one tunnel level
// (VXLAN, GTP-U with its extension headers, GRE) and the parse of the inner frame, with
// every sum of both levels, in one pass per 64-frame tile (include/rpkt_gpu.h documents
// the records and the dispatch; oracle/rpkt_oracle_tunnel.c restates it on the CPU).
//
// One wavefront per tile, as parse_kernel: the outer header windows go to LDS (on long
// tiles together with each frame's tail line, whose sum is taken there and then) and each
// lane runs parse_lane on its frame; the lane then decodes the tunnel header(s) from the
// same window (FlatView: global memory past it).  The outer record waits in registers (its
// words 0..11 in LDS past the inner record's stage once that is written: 128 VGPRs and
// 9.7 KB of LDS per wave, 16 waves per CU), and the inner frame's window is made from the
// outer one: the chunks they share move down the lane's slot and only the chunks past the
// outer window are loaded.  parse_lane runs again from the inner frame's first byte (its
// IP header for GTP-U and GRE).  One flattened chunk stream (rpkt_common.h) then sums each
// lane's main range -- the inner L4 bytes past the inner window, or the outer L4 range
// without a tunnel -- and the outer L4 sum (UDP, or GRE with its checksum), whose range
// contains the inner one, is composed from the outer window's part, the inner window's
// part (LDS), the main stream's sum when the rest of the two ranges is the same, and a
// rare stream for bytes before the inner window or a trailer after the inner packet.
// Each payload byte leaves HBM about once for all four sums (config 13: reads 1.09x the
// frame bytes, the excess the line the outer window ends in).
#include "rpkt_common.h"
#include "rpkt_args.h"
#include "rpkt_tunnel.h"

namespace {

// The outer header windows, and with them (joint) each frame's tail line [tb, fend): the
// line the next frame's window starts in, fetched in the same load group as that window
// (the cooperative mapping of window_with_edges: chunk k of lane l is piece l % 8 of frame
// 8 k + l / 8), so the stream never fetches it a second time.  Returns this lane's tail sum.
__device__ __forceinline__ uint32_t outer_window_tail(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                      WaveScratch& W, int lane, Frame fr,
                                                      uint32_t tb, uint32_t fend) {
    const int j = lane & 7;
    constexpr int kHalf = kWinChunks / 2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        u32x4 dw[kHalf], dt[kHalf];
        uint32_t aw[kHalf], at[kHalf], lt[kHalf];
#pragma unroll
        for (int i = 0; i < kHalf; ++i) {
            const int k = h * kHalf + i;
            const int q = (k * kWave + lane) >> 3;
            const uint32_t qo = (uint32_t)__shfl((int)fr.off, q, kWave);
            const uint32_t qn = (uint32_t)__shfl((int)fr.len, q, kWave);
            const uint32_t qt = (uint32_t)__shfl((int)tb, q, kWave);
            const uint32_t qe = (uint32_t)__shfl((int)fend, q, kWave);
            const uint32_t a = (qo & ~15u) + 16u * j, y = qt + 16u * j;
            aw[i] = a < qo + qn ? a : fb;
            const bool tin = y < qe;
            at[i] = tin ? y : fb;
            lt[i] = tin ? (qe - y < 16u ? qe - y : 16u) : 0u;
        }
#pragma unroll
        for (int i = 0; i < kHalf; ++i) {
            dw[i] = load16_fast<0>(rs, aw[i]);
            dt[i] = load16_fast<0>(rs, at[i]);
        }
#pragma unroll
        for (int i = 0; i < kHalf; ++i) {
            const int k = h * kHalf + i;
            u32x4 v = dw[i], vt = dt[i];
            if (__builtin_expect(straddles(aw[i], fb), 0)) v = load16(rs, aw[i], fb);
            if (__builtin_expect(lt[i] != 0 && straddles(at[i], fb), 0)) vt = load16(rs, at[i], fb);
            put_chunk(W, k * kWave + lane, v);
            const uint32_t xt = sum8_lanes(lt[i] ? chunk_sum(vt, 0, (int)lt[i]) : 0u);
            if (j == 0) W.last[(k * kWave + lane) >> 3] = xt;
        }
    }
    wave_sync();
    return W.last[lane];
}

// The inner window from the outer one: a lane whose inner frame starts d chunks into its
// outer window moves chunks d.. of its slot down to 0.. (its own slot: no other lane reads
// it), then the wave loads only the chunks past the outer window (cooperatively, the
// window_issue mapping) and writes them into the slots.  Lanes without a tunnel keep
// their outer window.
__device__ __forceinline__ void inner_window_reuse(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                   WaveScratch& W, int lane, uint32_t a1,
                                                   uint32_t keep, uint32_t lim) {
    u32x4 d[kWinChunks];
    uint32_t addr[kWinChunks];
    uint32_t fix = 0;
#pragma unroll
    for (int k = 0; k < kWinChunks; ++k) {
        const int c = k * kWave + lane;
        const int q = c / kWinChunks, j = c % kWinChunks;
        const uint32_t qa = (uint32_t)__shfl((int)a1, q, kWave);
        const uint32_t qk = (uint32_t)__shfl((int)keep, q, kWave);
        const uint32_t ql = (uint32_t)__shfl((int)lim, q, kWave);
        const uint32_t a = qa + 16u * j;
        addr[k] = ((uint32_t)j >= qk && a < ql) ? a : fb;
        fix |= (uint32_t)straddles(addr[k], fb) << k;
    }
#pragma unroll
    for (int k = 0; k < kWinChunks; ++k) d[k] = load16_fast<0>(rs, addr[k]);
    const uint32_t sh = (uint32_t)kWinChunks - keep;              // chunks moved down
    if (keep != (uint32_t)kWinChunks && keep != 0u) {
        uint32_t* sl = reinterpret_cast<uint32_t*>(&W.win[lane * kSlot]);
        for (uint32_t j = 0; j < keep; ++j) {
            const uint32_t x0 = sl[4 * (j + sh)], x1 = sl[4 * (j + sh) + 1];
            const uint32_t x2 = sl[4 * (j + sh) + 2], x3 = sl[4 * (j + sh) + 3];
            sl[4 * j] = x0;
            sl[4 * j + 1] = x1;
            sl[4 * j + 2] = x2;
            sl[4 * j + 3] = x3;
        }
    }
    wave_sync();                                      // every slot moved before the writes
#pragma unroll
    for (int k = 0; k < kWinChunks; ++k) {
        if (addr[k] == fb) continue;
        u32x4 v = d[k];
        if (__builtin_expect(fix & (1u << k), 0)) v = load16(rs, addr[k], fb);
        put_chunk(W, k * kWave + lane, v);
    }
    wave_sync();
}

// chunk loads in flight per lane in the main stream (2: 1-2 % faster than 3 and 4, the
// fewer lines in flight the fewer window lines evicted before their reuse; 6 and 8: no gain,
// and 8 costs occupancy)
#ifndef RPKT_TUN_UNROLL
#define RPKT_TUN_UNROLL 2
#endif
constexpr int kTunUnroll = RPKT_TUN_UNROLL;

template <bool L4>
__device__ __forceinline__ void tunnel_tile(WaveScratch& W,
                                            const uint8_t* __restrict__ frames, uint32_t fb,
                                            const uint32_t* __restrict__ offsets, uint32_t stride,
                                            uint32_t frame_len, uint32_t n, uint32_t flags,
                                            rpkt_rec_t* __restrict__ outer, rpkt_tun_t* __restrict__ tun,
                                            rpkt_rec_t* __restrict__ inner,
                                            uint64_t* __restrict__ flow_ev, uint32_t n_buckets,
                                            uint32_t p0, int lane) {
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const SpanSrc spans{offsets, stride, frame_len, fb, n};
    // header-only batches read each line once: non-temporal window loads (as parse_tile)
    constexpr int kWinAux = L4 ? 0 : 2;

    // 1. the outer header windows -> LDS (with the frames' tail lines on long tiles), the
    // outer parse
    const Frame fr = spans.get(i);
    const uint32_t a0 = fr.off & ~15u, fend = fr.off + (valid ? fr.len : 0u);
    [[maybe_unused]] uint32_t tb = fend, tail_sum = 0u;
    bool joint = false;
    if constexpr (L4) {
        const uint32_t wend0 = a0 + kWin;
        if (fend > wend0) tb = max(fend & ~127u, wend0);
        joint = wave_sum(fend > wend0 ? fend - wend0 : 0u) > kEdgeWindowBytes;   // uniform
    }
    if (joint) {
        tail_sum = outer_window_tail(rs, fb, W, lane, fr, tb, fend);
    } else {
        u32x4 d[kWinChunks];
        uint32_t addr[kWinChunks];
        const uint32_t fix = window_issue<kWinAux>(rs, fb, fr, lane, d, addr);
        window_commit(W, rs, fb, d, addr, fix, lane);
        wave_sync();
    }
    LaneRec L;
    parse_lane(W, lane, fr, valid, flags, L, rs, fb);

    // 2. the tunnel, from the outer window
    const Tunnel T = decode_tunnel(L, FlatView{{&W.win[lane * kSlot], fr.off & 15u, fr.off, fb, rs}},
                                   flags);

    // 3. the outer record in registers through the inner parse (a second LDS stage for it
    // held the kernel at 10 waves per CU), its L4 sum state kept for the streams
    uint32_t ow[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) ow[k] = L.w[k];
    [[maybe_unused]] const uint32_t o_ss = L.stream_s, o_se = L.stream_e, o_part = L.l4_part;
    [[maybe_unused]] const uint32_t o_abs = L.l4_start_abs, o_pseudo = L.pseudo;
    [[maybe_unused]] const bool o_want = L.want_l4;

    // 4. the inner header windows -> LDS (the outer ones are no longer read), inner parse
    const Frame fi = T.ok ? Frame{fr.off + T.is, T.ie - T.is} : Frame{0u, 0u};
    const uint32_t a1 = T.ok ? fi.off & ~15u : a0;
    const uint32_t dch = (a1 - a0) >> 4;
    const uint32_t keep = dch < (uint32_t)kWinChunks ? (uint32_t)kWinChunks - dch : 0u;
    // (chunks loaded up to the outer frame's end: the outer L4 range's part in this window
    // is summed from it below, and it can run past the inner frame)
    inner_window_reuse(rs, fb, W, lane, a1, T.ok ? keep : (uint32_t)kWinChunks, fend);
    parse_lane(W, lane, fi, T.ok, flags, L, rs, fb, T.start_et, T.is);
    if (!T.ok) no_inner(L);
    // the outer L4 range's bytes the inner window holds: [max(o_ss, a1), min(o_se, a1 + 128))
    [[maybe_unused]] uint32_t o_lds = 0u;
    if constexpr (L4) {
        if (T.ok && o_want) {
            const uint32_t ls = o_ss > a1 ? o_ss : a1, le = o_se < a1 + kWin ? o_se : a1 + kWin;
            o_lds = slot_range_sum(&W.win[lane * kSlot], ls - a1, le > ls ? le - a1 : ls - a1);
        }
    }
    stage_record(W, lane, L.w);
    // the outer record's words 0..11 wait in the window area past the inner stage (free
    // now: 3072 B, word-major), so the streams hold 8 of its words in registers, not 20
    static_assert(kWave * 21 * 4 + 12 * kWave * 4 <= kWinArea, "parked words fit past the stage");
    uint32_t* park = reinterpret_cast<uint32_t*>(&W.win[kWave * 21 * 4]);
#pragma unroll
    for (int k = 0; k < 12; ++k) park[k * kWave + lane] = ow[k];

    // 5. L4 bytes past the windows: the inner stream, then the outer range's other bytes
    if constexpr (L4) {
        // one main stream per lane: the inner L4 range (the outer one without a tunnel),
        // less the tail line summed with the windows when the range runs to the frame end
        const uint32_t ms = T.ok ? L.stream_s : (o_want ? o_ss : 0u);
        const uint32_t me = T.ok ? L.stream_e : (o_want ? o_se : 0u);
        const bool use_tail = joint && me > ms && me == fend && tb < fend && tb >= ms;
        const uint32_t sp_m = wave_stream_sum<2, kTunUnroll>(rs, fb, ms, use_tail ? tb : me, W, lane) +
                              (use_tail ? tail_sum : 0u);
        // the outer range of a tunnel frame: [o_ss, a1) streamed (an inner window past the
        // outer one), the inner window's part from LDS, [a1 + 128, o_se) the main stream when
        // it is the same range, else streamed
        const uint32_t w1 = a1 + kWin;
        const uint32_t p3s = o_ss > w1 ? o_ss : w1;
        const bool shared = T.ok && o_want && p3s == ms && o_se == me && me > ms;
        const bool rest = T.ok && o_want;
        uint32_t sp_o = wave_stream_sum<2>(rs, fb, rest ? o_ss : 0u,
                                           rest ? (o_se < a1 ? o_se : a1) : 0u, W, lane);
        sp_o += wave_stream_sum<2>(rs, fb, rest && !shared ? p3s : 0u,
                                   rest && !shared ? o_se : 0u, W, lane);
        sp_o += T.ok ? o_lds + (shared ? sp_m : 0u) : sp_m;
        if (L.want_l4)
            rec_stage(W)[lane * 21 + 18] |= fold16(L.pseudo + be_sum(L.l4_part + sp_m, L.l4_start_abs)) << 16;
        if (o_want) ow[18] |= fold16(o_pseudo + be_sum(o_part + sp_o, o_abs)) << 16;
    }

    // 6. records: the inner one, then the outer one staged where it was (1-KiB wave stores),
    // the tunnel record (16 B per lane); the flow event from the inner record when the
    // tunnel decoded, else from the outer one (include/rpkt_gpu.h)
    const bool ev = (flags & RPKT_F_FLOW_EV) && valid;
    if (ev && T.ok) __builtin_nontemporal_store(record_event(rec_stage(W) + lane * 21, n_buckets),
                                                &flow_ev[i]);
    flush_stage(rec_stage(W), lane, inner, p0, n);
#pragma unroll
    for (int k = 0; k < 12; ++k) ow[k] = park[k * kWave + lane];
    if (ev && !T.ok) __builtin_nontemporal_store(record_event(ow, n_buckets), &flow_ev[i]);
    stage_record(W, lane, ow);
    flush_stage(rec_stage(W), lane, outer, p0, n);
    if (valid) store_tun(tun, i, T);
}

// One wave per workgroup (as the parse: a CU slot frees when its wave ends); 9.7 KB of LDS
// and 128 VGPRs per wave: 16 waves per CU
template <bool L4>
__global__ __launch_bounds__(kWave, 2)
void tunnel_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                   const uint32_t* __restrict__ offsets, uint32_t stride, uint32_t frame_len,
                   uint32_t n, uint32_t flags, rpkt_rec_t* __restrict__ outer,
                   rpkt_tun_t* __restrict__ tun, rpkt_rec_t* __restrict__ inner,
                   uint64_t* __restrict__ flow_ev, uint32_t n_buckets) {
    __shared__ __attribute__((aligned(16))) WaveScratch scratch;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t p0 = blockIdx.x * kWave;
    if (p0 >= n) return;                                          // wave-uniform exit
    tunnel_tile<L4>(scratch, frames, fb, offsets, stride, frame_len, n, flags, outer, tun,
                    inner, flow_ev, n_buckets, p0, lane);
}

// A ring of tunnelled bursts in one launch (rpkt_gpu_parse_tunnel_ring): wave t takes
// tile t of the ring's tiles, numbered slot after slot (tile0[k] = the first tile of slot
// k), and parses it exactly as tunnel_kernel parses that tile of the slot's own batch.  The
// slot descriptors are kernel arguments (2.2 KB), read with scalar loads.
constexpr uint32_t kTunRingMax = RPKT_RING_MAX_SLOTS;
struct TunRingSlot {
    const uint8_t* frames;
    const uint32_t* offsets;
    rpkt_rec_t* outer;
    rpkt_tun_t* tun;
    rpkt_rec_t* inner;
    uint64_t* flow_ev;
    uint32_t frames_bytes, stride, frame_len, n;
};
struct TunRingArgs {
    uint32_t n_slots;
    uint32_t tile0[kTunRingMax + 1];
    TunRingSlot s[kTunRingMax];
};

template <bool L4>
__global__ __launch_bounds__(kWave, 2)
void tunnel_ring_kernel(const TunRingArgs A, uint32_t flags, uint32_t n_buckets) {
    __shared__ __attribute__((aligned(16))) WaveScratch scratch;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t t = blockIdx.x;
    if (t >= A.tile0[A.n_slots]) return;                         // wave-uniform exit
    uint32_t k = 0;                                               // the slot holding tile t
    for (uint32_t j = 1; j < A.n_slots; ++j) k = A.tile0[j] <= t ? j : k;
    const TunRingSlot& S = A.s[k];
    tunnel_tile<L4>(scratch, S.frames, S.frames_bytes, S.offsets, S.stride, S.frame_len, S.n,
                    flags, S.outer, S.tun, S.inner, S.flow_ev, n_buckets,
                    (t - A.tile0[k]) * kWave, lane);
}

// one batch's argument checks (rpkt_gpu_parse_tunnel_batch's, and each slot's of a ring;
// RPKT_OK for an empty batch too: the caller returns before it launches)
int tunnel_args_ok(const rpkt_batch_t& b, uint32_t flags, const void* outer, const void* tun,
                   const void* inner, const void* flow_ev, uint32_t n_buckets) {
    RPKT_TRY(events_ok(flags, flow_ev, n_buckets));     // not the family order: before n == 0
    if (b.n == 0) return RPKT_OK;
    if (any_null(b.frames_dev, outer, tun, inner)) return RPKT_E_INVAL;
    RPKT_TRY(size_ok(b.frames_bytes));
    RPKT_TRY(layout_ok(b));
    return misaligned(15, outer, tun, inner) ? RPKT_E_ALIGN : RPKT_OK;
}

}  // namespace

extern "C" {

int rpkt_gpu_parse_tunnel_batch(const rpkt_batch_t* b, uint32_t flags, rpkt_rec_t* outer_dev,
                                rpkt_tun_t* tun_dev, rpkt_rec_t* inner_dev,
                                rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream) {
    if (!b) return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, kRxFlags));
    RPKT_TRY(tunnel_args_ok(*b, flags, outer_dev, tun_dev, inner_dev, flow_ev_dev, n_buckets));
    if (b->n == 0) return RPKT_OK;
    auto k = (flags & RPKT_F_L4_SUM) ? tunnel_kernel<true> : tunnel_kernel<false>;
    return launch_batch(k, kWave, 0, stream, *b, flags, outer_dev, tun_dev, inner_dev, flow_ev_dev,
                        n_buckets);
}

int rpkt_gpu_parse_tunnel_ring(const rpkt_tun_ring_slot_t* slots, uint32_t n_slots,
                               uint32_t flags, uint32_t n_buckets, void* stream) {
    if (n_slots && !slots) return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, kRxFlags));
    for (uint32_t k = 0; k < n_slots; ++k) {                      // all checked, then launched
        const rpkt_tun_ring_slot_t& q = slots[k];
        if (q.batch.n == 0) continue;
        RPKT_TRY(tunnel_args_ok(q.batch, flags, q.outer_dev, q.tun_dev, q.inner_dev, q.flow_ev_dev,
                                n_buckets));
    }
    const bool fev = (flags & RPKT_F_FLOW_EV) != 0;
    auto kern = (flags & RPKT_F_L4_SUM) ? tunnel_ring_kernel<true> : tunnel_ring_kernel<false>;
    TunRingArgs A;
    auto outputs = [fev](TunRingSlot& S, const rpkt_tun_ring_slot_t& q) {
        S.outer = q.outer_dev;
        S.tun = q.tun_dev;
        S.inner = q.inner_dev;
        S.flow_ev = fev ? q.flow_ev_dev : nullptr;
    };
    for (uint32_t k0 = 0; pack_ring(A, slots, n_slots, k0, outputs);)
        RPKT_TRY(launch(kern, dim3(A.tile0[A.n_slots]), dim3(kWave), 0, (hipStream_t)stream, A,
                        flags, n_buckets));
    return RPKT_OK;
}

}  // extern "C"
