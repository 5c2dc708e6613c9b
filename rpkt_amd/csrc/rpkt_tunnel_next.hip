// rpkt_tunnel_next.hip — rpkt_gpu_parse_tunnel_next: the next tunnel level of a batch
// whose level-k tunnel and inner records exist (rpkt_gpu_parse_tunnel_batch's, or an
// earlier call's of this entry).  The level-k inner record plays the outer record's part:
// decode_tunnel (rpkt_tunnel.h) dispatches and decodes from it, parse_lane parses the
// level-k+1 inner frame, and every offset written is a position in the outermost frame,
// because the level-k record's offsets already are (include/rpkt_gpu.h).
//
// One wavefront per 64-frame tile.  The tile's records come in with coalesced 16-B loads
// through the LDS stage, so a tile none of whose records dispatches to a tunnel writes its
// NONE / NO_INNER records and ends without reading a frame byte.  Otherwise the tunnel
// header is decoded from global memory (a few dwords per frame, in the lines the innermost
// window fetches next), the innermost header windows go to LDS, and one chunk stream sums
// the innermost L4 bytes past the window.  The mid-level sums are in the level-k record;
// for a nested frame the innermost L4 bytes were streamed once by level 1 (for the
// mid-level sum) and are read here a second time.
#include "rpkt_common.h"
#include "rpkt_args.h"
#include "rpkt_tunnel.h"

namespace {

// chunk loads in flight per lane in the stream (as tunnel_kernel's main stream)
constexpr int kNextUnroll = 2;

// the tile's 80-B records -> the LDS stage (stride 21 dwords): flush_stage's mapping,
// the other way
__device__ __forceinline__ void load_stage(uint32_t* rl, int lane, const rpkt_rec_t* recs,
                                           uint32_t p0, uint32_t n) {
    const uint32_t nrec = n - p0 < (uint32_t)kWave ? n - p0 : (uint32_t)kWave;
    const u32x4* in = reinterpret_cast<const u32x4*>(recs + p0);
    u32x4 v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t c = k * kWave + lane;
        v[k] = c / 5 < nrec ? __builtin_nontemporal_load(&in[c]) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t c = k * kWave + lane, r = c / 5, pc = c % 5;
        uint32_t* dst = rl + r * 21 + pc * 4;
        dst[0] = v[k].x;
        dst[1] = v[k].y;
        dst[2] = v[k].z;
        dst[3] = v[k].w;
    }
    wave_sync();
}

template <bool L4>
__global__ __launch_bounds__(kWave, 2)
void tunnel_next_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                        const uint32_t* __restrict__ offsets, uint32_t stride, uint32_t frame_len,
                        uint32_t n, uint32_t flags, const rpkt_tun_t* __restrict__ tun,
                        const rpkt_rec_t* __restrict__ inner, rpkt_tun_t* __restrict__ tun_next,
                        rpkt_rec_t* __restrict__ inner_next, uint64_t* __restrict__ flow_ev,
                        uint32_t n_buckets) {
    __shared__ __attribute__((aligned(16))) WaveScratch W;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t p0 = blockIdx.x * kWave;
    if (p0 >= n) return;                                          // wave-uniform exit
    const uint32_t i = p0 + lane;
    const bool valid = i < n;

    // 1. the level-k records: the tunnel record (16 B per lane), the inner record's words
    // through the stage
    u32x4 tw = {0u, 0u, 0u, 0u};
    if (valid) tw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tun) + i);
    load_stage(rec_stage(W), lane, inner, p0, n);
    const bool have = valid && ((tw.x >> 8) & 0xffu) == RPKT_T_OK;
    LaneRec L;
    {
        const uint32_t* rl = rec_stage(W) + lane * 21;
#pragma unroll
        for (int k = 0; k < 20; ++k) L.w[k] = rl[k];
    }
    wave_sync();                                     // every lane has its words: the stage is free
    // status and is6 from the words; a frame without a level-k inner frame gets a status
    // that dispatches to nothing
    rec_status_is6(L.w, L.status, L.is6);
    if (!have) {
        L.status = RPKT_S_ETH_SHORT;
        L.is6 = false;
    }
    const uint32_t k_off = tw.y & 0xffffu, k_len = L.w[19];       // level k: inner_off, frame_len

    // 2. the tunnel of the level-k frame.  decode_tunnel returns before its first read for
    // a record that dispatches to nothing; the others read the outer frame's bytes through
    // the buffer resource (no window: ph past it sends every read to global memory).
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const SpanSrc spans{offsets, stride, frame_len, fb, n};
    const Frame fr = spans.get(i);
    Tunnel T = decode_tunnel(L, FlatView{{W.win, (uint32_t)kWin, fr.off, fb, rs}}, flags);

    // 3. no tunnel in the tile: its NONE / NO_INNER records, no frame byte read
    if (__ballot((T.w[0] & 0xffu) != RPKT_TUN_NONE) == 0) {       // wave-uniform
        const uint32_t nrec = n - p0 < (uint32_t)kWave ? n - p0 : (uint32_t)kWave;
        u32x4* out = reinterpret_cast<u32x4*>(inner_next + p0);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint32_t c = k * kWave + lane;
            const u32x4 v = {c % 5 == 0 ? (uint32_t)RPKT_S_NO_INNER : 0u, 0u, 0u, 0u};
            if (c / 5 < nrec) __builtin_nontemporal_store(v, &out[c]);
        }
        if (valid) store_tun(tun_next, i, T);
        return;
    }

    // 4. the innermost frame, inside the level-k frame's bytes and those inside frame i's
    // span (records of this batch keep both; others give wrong records, never a fault)
    const uint32_t k_s = k_off < fr.len ? k_off : fr.len;
    const uint32_t k_e = k_len < fr.len - k_s ? k_s + k_len : fr.len;
    const uint32_t is = T.is < k_s ? k_s : (T.is < k_e ? T.is : k_e);
    const uint32_t ie = T.ie < is ? is : (T.ie < k_e ? T.ie : k_e);
    const Frame fi = T.ok ? Frame{fr.off + is, ie - is} : Frame{0u, 0u};
    // header-only batches read each line once: non-temporal window loads (as tunnel_kernel)
    constexpr int kWinAux = L4 ? 0 : 2;
    {
        u32x4 d[kWinChunks];
        uint32_t addr[kWinChunks];
        const uint32_t fix = window_issue<kWinAux>(rs, fb, fi, lane, d, addr);
        window_commit(W, rs, fb, d, addr, fix, lane);
        wave_sync();
    }
    parse_lane(W, lane, fi, T.ok, flags, L, rs, fb, T.start_et, is);
    if (!T.ok) no_inner(L);
    stage_record(W, lane, L.w);

    // 5. the innermost L4 bytes past the window
    if constexpr (L4) {
        const uint32_t sp = wave_stream_sum<2, kNextUnroll>(rs, fb, L.stream_s, L.stream_e, W, lane);
        if (L.want_l4)
            rec_stage(W)[lane * 21 + 18] |= fold16(L.pseudo + be_sum(L.l4_part + sp, L.l4_start_abs)) << 16;
    }

    // 6. the event of a decoded tunnel's inner record (other entries stay), the records
    if ((flags & RPKT_F_FLOW_EV) && valid && T.ok)
        __builtin_nontemporal_store(record_event(rec_stage(W) + lane * 21, n_buckets), &flow_ev[i]);
    flush_stage(rec_stage(W), lane, inner_next, p0, n);
    if (valid) store_tun(tun_next, i, T);
}

}  // namespace

extern "C" {

int rpkt_gpu_parse_tunnel_next(const rpkt_batch_t* b, uint32_t flags, const rpkt_tun_t* tun_dev,
                               const rpkt_rec_t* inner_dev, rpkt_tun_t* tun_next_dev,
                               rpkt_rec_t* inner_next_dev, rpkt_flow_ev_t* flow_ev_dev,
                               uint32_t n_buckets, void* stream) {
    if (!b) return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, kRxFlags));
    if (b->n == 0) return RPKT_OK;
    if (any_null(b->frames_dev, tun_dev, inner_dev, tun_next_dev, inner_next_dev))
        return RPKT_E_INVAL;
    RPKT_TRY(layout_ok(*b));                // not the family order: layout and aliasing before size
    if (tun_next_dev == tun_dev || inner_next_dev == inner_dev) return RPKT_E_INVAL;
    RPKT_TRY(size_ok(b->frames_bytes));
    if (misaligned(15, tun_dev, inner_dev, tun_next_dev, inner_next_dev)) return RPKT_E_ALIGN;
    RPKT_TRY(events_ok(flags, flow_ev_dev, n_buckets));
    auto k = (flags & RPKT_F_L4_SUM) ? tunnel_next_kernel<true> : tunnel_next_kernel<false>;
    return launch_batch(k, kWave, 0, stream, *b, flags, tun_dev, inner_dev, tun_next_dev,
                        inner_next_dev, flow_ev_dev, n_buckets);
}

}  // extern "C"
