// rpkt_args.h — the host prologue of the C ABI entry points (include/rpkt_gpu.h), in
// pieces: argument checks that return RPKT_OK or the status to return, the frame length
// and window fit of a batch, the launch of a kernel over a batch and the packing of ring
// slots.  Host only, no device code; included after rpkt_common.h by the units that have
// entry points.
//
// An entry is its checks in order, a kernel choice and one launch.  The family order is:
// null arguments, flags, n == 0 (RPKT_OK), the batch (frames pointer, size, layout),
// alignment, flow events.  An entry whose order differs composes the finer pieces in its
// own order and says so in a comment; include/rpkt_gpu.h (at enum rpkt_err) documents those
// and tests/test_abi_status_matrix.py pins every order.
#pragma once
#include "rpkt_common.h"

// return a check's status unless it is RPKT_OK
#define RPKT_TRY(check)                 \
    do {                                \
        const int rc_ = (check);        \
        if (rc_ != RPKT_OK) return rc_; \
    } while (0)

namespace {

// flags the receive-side entries (batch, ring, options, chains, tunnel) accept
constexpr uint32_t kRxFlags = RPKT_F_IP_SUM | RPKT_F_L4_SUM | RPKT_F_FLOW_EV | RPKT_F_IPV6;

inline int flags_ok(uint32_t flags, uint32_t allowed) {
    return (flags & ~allowed) ? RPKT_E_INVAL : RPKT_OK;
}

template <typename... P>
inline bool any_null(const P*... p) {
    return (... || (p == nullptr));
}

// any pointer with a bit of `mask` set (15: 16-byte alignment)
template <typename... P>
inline bool misaligned(uintptr_t mask, const P*... p) {
    return ((... | (uintptr_t)p) & mask) != 0;
}

// the batch check and its three parts
inline int frames_ok(const rpkt_batch_t& b) { return b.frames_dev ? RPKT_OK : RPKT_E_INVAL; }
inline int size_ok(uint64_t bytes) { return bytes > kMaxFrameBytes ? RPKT_E_TOO_LARGE : RPKT_OK; }
inline int layout_ok(const rpkt_batch_t& b) {
    return (!b.offsets_dev && b.stride == 0) ? RPKT_E_INVAL : RPKT_OK;
}
inline int batch_ok(const rpkt_batch_t& b) {
    RPKT_TRY(frames_ok(b));
    RPKT_TRY(size_ok(b.frames_bytes));
    return layout_ok(b);
}

// rpkt_chains_t: pointers, then sizes (segs_dev's alignment goes with the alignment step)
inline int chains_ok(const rpkt_chains_t& c) {
    if (!c.chain_first_dev || (c.n_segs && any_null(c.buf_dev, c.segs_dev))) return RPKT_E_INVAL;
    RPKT_TRY(size_ok(c.buf_bytes));
    return c.n_segs >= 0x80000000u ? RPKT_E_TOO_LARGE : RPKT_OK;
}

inline int buckets_ok(uint32_t n_buckets) {
    return (n_buckets == 0 || n_buckets > RPKT_FLOW_MAX_BUCKETS) ? RPKT_E_INVAL : RPKT_OK;
}

// RPKT_F_FLOW_EV: an event buffer, 8-byte aligned, and 1..RPKT_FLOW_MAX_BUCKETS buckets
inline int events_ok(uint32_t flags, const void* flow_ev_dev, uint32_t n_buckets) {
    if (!(flags & RPKT_F_FLOW_EV)) return RPKT_OK;
    if (!flow_ev_dev || buckets_ok(n_buckets) != RPKT_OK) return RPKT_E_INVAL;
    return misaligned(7, flow_ev_dev) ? RPKT_E_ALIGN : RPKT_OK;
}

// the frame_len kernel argument: 0 for a packed batch, else the frames' length
inline uint32_t batch_flen(const rpkt_batch_t& b) {
    return b.offsets_dev ? 0u : (b.frame_len ? b.frame_len : b.stride);
}

// every frame of a strided batch inside a `win`-byte header window from its 16-B boundary
// (the frame at i * stride has phase (i * stride) & 15: 0 for strides of 16-B multiples)
inline bool fits_window(const rpkt_batch_t& b, uint32_t win) {
    const uint32_t flen = batch_flen(b);
    if (b.offsets_dev || b.stride == 0 || flen == 0) return false;
    return flen + ((b.stride & 15u) ? 15u : 0u) <= win;
}

// Launch `kernel` over batch `b`, `per_block` threads a block and one thread a frame: the
// six leading kernel arguments every batch kernel takes, then `args`.
template <typename F, typename... KArgs, typename... Args>
int launch_batch(void (*kernel)(F, uint32_t, const uint32_t*, uint32_t, uint32_t, uint32_t, KArgs...),
                 uint32_t per_block, size_t lds, void* stream, const rpkt_batch_t& b,
                 Args... args) {
    return launch(kernel, dim3((b.n + per_block - 1) / per_block), dim3(per_block), lds,
                  (hipStream_t)stream, const_cast<F>(b.frames_dev), (uint32_t)b.frames_bytes,
                  b.offsets_dev, b.stride, batch_flen(b), b.n, args...);
}

// the batch fields of a ring kernel's slot (RingSlot, TunRingSlot)
template <typename Slot>
inline void slot_batch(Slot& S, const rpkt_batch_t& b) {
    S.frames = b.frames_dev;
    S.offsets = b.offsets_dev;
    S.frames_bytes = (uint32_t)b.frames_bytes;
    S.stride = b.stride;
    S.frame_len = batch_flen(b);
    S.n = b.n;
}

// Pack the next non-empty slots of a ring, from slot k0 on and at most RPKT_RING_MAX_SLOTS,
// into the kernel arguments A (RingArgs, TunRingArgs); outputs(S, q) sets slot S's output
// pointers from the caller's slot q.  False when no slot is left.
template <typename A, typename Q, typename Outputs>
bool pack_ring(A& args, const Q* slots, uint32_t n_slots, uint32_t& k0, Outputs outputs) {
    args.n_slots = 0;
    args.tile0[0] = 0;
    for (; k0 < n_slots && args.n_slots < RPKT_RING_MAX_SLOTS; ++k0) {
        const rpkt_batch_t& b = slots[k0].batch;
        if (b.n == 0) continue;
        auto& S = args.s[args.n_slots];
        slot_batch(S, b);
        outputs(S, slots[k0]);
        args.tile0[args.n_slots + 1] = args.tile0[args.n_slots] + (b.n + kWave - 1) / kWave;
        ++args.n_slots;
    }
    return args.n_slots != 0;
}

}  // namespace
