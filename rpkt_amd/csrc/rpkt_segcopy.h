// rpkt_segcopy.h — what the units that re-frame a batch share (rpkt_segment.hip and
// rpkt_fragment.hip: one frame into many; rpkt_coalesce.hip and rpkt_reassemble.hip: many into
// one).  Host: the entries' argument checks, the carving of their workspaces and, for the two
// that cut, the launch of the scans and the write.  Device: what a record says about a TCP or UDP frame, a
// tile's records staged through LDS, header sums by one lane, the block scans of the plan ->
// scan -> write structure, the end of a plan kernel and the start of a write kernel's wave
// (its run of outputs and their input frame), for runs of positions the block max-scan, the
// scan of the blocks' run heads and the walk of a header's dwords, and the wave copy between
// any two byte phases that sums what it copies.
// Everything is inline in an anonymous namespace.
#pragma once
#include "rpkt_common.h"
#include "rpkt_args.h"

namespace {

constexpr int kSegBlock = kWave * kWavesPerBlock;   // frames per block in plan and scan

// The source of a re-framing call, a flat batch or mbuf chains: its input count, its checks
// with out_bytes' in its documented place, and whether a pointer of its own is misaligned.
inline uint32_t source_n(const rpkt_batch_t& b) { return b.n; }
inline uint32_t source_n(const rpkt_chains_t& c) { return c.n_chains; }
inline int source_ok(const rpkt_batch_t& b, uint64_t out_bytes) {
    RPKT_TRY(frames_ok(b));
    RPKT_TRY(size_ok(b.frames_bytes));
    RPKT_TRY(size_ok(out_bytes));
    return layout_ok(b);
}
inline int source_ok(const rpkt_chains_t& c, uint64_t out_bytes) {
    RPKT_TRY(chains_ok(c));
    return size_ok(out_bytes);
}
inline bool source_misaligned(const rpkt_batch_t&) { return false; }
inline bool source_misaligned(const rpkt_chains_t& c) { return misaligned(7, c.segs_dev); }

// The checks of a re-framing entry in the documented order: required pointers, flags, `limit`
// (mss, max_payload) in 1..65535, no inputs (RPKT_OK: the entry then returns), the source with
// out_bytes, out_cap, alignment.  more_recs: an entry's further record arrays (the tunnel and
// inner records of a tunnel entry), required and 16-byte aligned as recs is.
template <class Source, typename... More>
inline int reframe_args_ok(const Source* src, const rpkt_rec_t* recs, uint32_t limit,
                           uint32_t flags, uint32_t allowed, const uint8_t* out_frames,
                           uint64_t out_bytes, const uint32_t* out_offsets, uint32_t out_cap,
                           const uint32_t* first, const uint64_t* totals, const void* workspace,
                           const More*... more_recs) {
    if (!src || any_null(recs, out_frames, out_offsets, first, totals, more_recs...) || !workspace)
        return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, allowed));
    if (limit == 0u || limit > 65535u) return RPKT_E_INVAL;
    if (source_n(*src) == 0) return RPKT_OK;
    RPKT_TRY(source_ok(*src, out_bytes));
    if (out_cap == 0u) return RPKT_E_INVAL;
    if (source_misaligned(*src) || misaligned(15, recs, out_frames, more_recs...) ||
        misaligned(15, (const uint8_t*)workspace) || misaligned(7, totals))
        return RPKT_E_ALIGN;
    return RPKT_OK;
}

inline uint32_t blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kSegBlock - 1) / kSegBlock); }
inline size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }

// A workspace handed out in regions rounded up to 16 bytes.  From a null base used() is the
// size the layout needs: a unit states its layout once, for its pointers and its byte count.
struct Carve {
    uintptr_t base, at;
    explicit Carve(void* ws) : base((uintptr_t)ws), at(base) {}
    template <class T>
    T* take(size_t count) {
        T* r = reinterpret_cast<T*>(at);
        at += up16(count * sizeof(T));
        return r;
    }
    size_t used() const { return (size_t)(at - base); }
};

// the workspace: per-frame plans (32 B: `quads` 2; the tunnel entry's 64 B: 4), per-frame
// output byte bases (u64), block sums (count, bytes: u64 pairs)
struct SegWs {
    u32x4*    plan;
    uint64_t* obase;
    uint64_t* part;
    size_t    bytes;
};
inline SegWs seg_ws(void* ws, uint32_t n, uint32_t quads = 2) {
    Carve c(ws);
    SegWs w;
    w.plan = c.take<u32x4>(quads * (size_t)n);
    w.obase = c.take<uint64_t>(n);
    w.part = c.take<uint64_t>(2 * (size_t)blocks(n));
    w.bytes = c.used();
    return w;
}

// What the record's dwords 0, 5, 7, 8, 16, 17 say about a frame of `len` bytes: `on`, status
// OK and an unfragmented TCP packet (or, with `with_udp`, UDP datagram: `udp`) over IPv4 or
// IPv6 whose offsets nest; pl clamped to the frame.  Without `with_udp` a UDP frame is as any
// other protocol's: not `on`.
struct L4Where {
    bool on, udp, v6;
    uint32_t l3, l4, po, pl, pdst;
};
__device__ __forceinline__ L4Where l4_where(uint32_t w0, uint32_t w5, uint32_t w7, uint32_t w8,
                                            uint32_t w16, uint32_t w17, uint32_t len, bool with_udp) {
    const uint32_t status = w0 & 0xffu, nv = (w0 >> 8) & 0xffu;
    const uint32_t det = nv == 0u ? w0 >> 16 : (nv == 1u ? w5 & 0xffffu : w5 >> 16);
    const bool v6 = det == 0x86ddu;
    const uint32_t proto = (w8 >> 8) & 0xffu, frag = w7 >> 16, pdst = w8 >> 16;
    const uint32_t l3 = w16 & 0xffffu, l4 = w16 >> 16, po = w17 & 0xffffu;
    const bool udp = with_udp && proto == 17u;
    // offsets that nest as a parse of this frame leaves them (the L4 header: TCP's 20..60
    // bytes, UDP's 8); [po, + pl) inside the frame
    const bool nest = l4 >= l3 && po >= l4 && po <= len &&
                      (udp ? po - l4 == 8u : (po - l4 >= 20u && po - l4 <= 60u)) &&
                      (v6 ? l4 - l3 >= 40u : (l4 - l3 >= 20u && l4 - l3 <= 60u));
    uint32_t pl = w17 >> 16;
    if (nest && pl > len - po) pl = len - po;
    const bool on = status == RPKT_S_OK && (proto == 6u || udp) && (v6 || det == 0x0800u) &&
                    (v6 || (frag & 0x3fffu) == 0u) && nest;
    return L4Where{on, udp, v6, l3, l4, po, pl, pdst};
}
// the same from a staged record (stage_records_tile)
__device__ __forceinline__ L4Where l4_where(const uint32_t* w, uint32_t len, bool with_udp) {
    return l4_where(w[0], w[5], w[7], w[8], w[16], w[17], len, with_udp);
}

// The UDP checksum field for a one's complement sum over pseudo header, header and payload:
// a result of 0 is sent as 0xffff (RFC 768), the opposite of TCP's, where 0 stays 0.
__device__ __forceinline__ uint32_t udp_csum_field(uint32_t sum) {
    const uint32_t ck = ~fold16(sum) & 0xffffu;
    return ck ? ck : 0xffffu;
}

// The IPv6 pseudo header's destination: the routing header's final address when ip6_pdst_off
// lies in [l3 + 24, l4 - 16], else the fixed header's (rpkt_gpu_build_batch's rule, rpkt_tx.hip).
__device__ __forceinline__ uint32_t ip6_pseudo_dst(uint32_t pdst, uint32_t l3, uint32_t l4) {
    return (pdst >= l3 + 24u && pdst + 16u <= l4) ? pdst : l3 + 24u;
}

// the aligned dword at x (bytes past the buffer read as 0: its last, partial dword by bytes)
__device__ __forceinline__ uint32_t ldw(__amdgpu_buffer_rsrc_t rs, uint32_t fb, uint32_t x) {
    if (__builtin_expect(x + 4u <= fb, 1))
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)x, 0, 0);
    return gbyte(rs, x) | (gbyte(rs, x + 1u) << 8) | (gbyte(rs, x + 2u) << 16) |
           (gbyte(rs, x + 3u) << 24);
}

// big-endian RFC 1071 sum (folded) of buffer bytes [a, b), one lane: headers, addresses
__device__ __forceinline__ uint32_t range_be_sum(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                 uint32_t a, uint32_t b) {
    if (b <= a) return 0u;
    uint32_t acc = 0;
    for (uint32_t x = a & ~3u; x < b; x += 4u) {
        const uint32_t lo = a > x ? a - x : 0u, hi = b - x < 4u ? b - x : 4u;
        acc = hsum(ldw(rs, fb, x) & byte_mask((int)lo, (int)hi), acc);
    }
    return be_sum(acc, a);
}

// The records of the wave's tile [p0, p0 + 64) of n, coalesced: 5 dwordx4 per lane over its
// contiguous 5 KiB into the stage `st` (64 * 21 dwords: record r at stride 21 dwords), as
// rpkt_tx.hip's load_records_tile
__device__ __forceinline__ void stage_records_tile(uint32_t* st, const rpkt_rec_t* __restrict__ recs,
                                                   uint32_t p0, uint32_t n, int lane) {
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
        const uint32_t c = k * kWave + lane;
        uint32_t* d = st + (c / 5) * 21 + (c % 5) * 4;
        d[0] = v[k].x;
        d[1] = v[k].y;
        d[2] = v[k].z;
        d[3] = v[k].w;
    }
    wave_sync();
}

// 64-bit inclusive scan over the wave
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t x, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)x, d, kWave);
        if (lane >= d) x += y;
    }
    return x;
}

// Exclusive scan of (a, b) over the block's kSegBlock threads; tot_*: the block's sums.
// red: 4 * kWavesPerBlock u64 of LDS.
__device__ __forceinline__ void block_excl_scan2(uint64_t& a, uint64_t& b, uint64_t& tot_a,
                                                 uint64_t& tot_b, uint64_t* red) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint64_t ia = wave_incl_scan64(a, lane), ib = wave_incl_scan64(b, lane);
    if (lane == kWave - 1) {
        red[2 * wave] = ia;
        red[2 * wave + 1] = ib;
    }
    __syncthreads();
    uint64_t ba = 0, bb = 0;
    tot_a = tot_b = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
        if (w < wave) {
            ba += red[2 * w];
            bb += red[2 * w + 1];
        }
        tot_a += red[2 * w];
        tot_b += red[2 * w + 1];
    }
    __syncthreads();                                   // red is free for the next call
    a = ba + ia - a;
    b = bb + ib - b;
}

// The end of a planning kernel: the block's sums of (cnt, bytes) to part[blockIdx.x].
__device__ __forceinline__ void block_sums_to_part(uint64_t cnt, uint64_t bytes,
                                                   uint64_t* __restrict__ part, uint64_t* red) {
    uint64_t tc, tb;
    block_excl_scan2(cnt, bytes, tc, tb, red);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = tc;
        part[2 * (size_t)blockIdx.x + 1] = tb;
    }
}

// The plan's end: frame i's plan (words 0..7 of its kQuads * 16 bytes), count and bytes to the
// workspace, the block's sums to part.
template <int kQuads = 2>
__device__ __forceinline__ void plan_store(bool valid, uint32_t i, const uint32_t (&p)[8],
                                           uint64_t cnt, uint64_t bytes, u32x4* __restrict__ plan,
                                           uint32_t* __restrict__ seg_first,
                                           uint64_t* __restrict__ obase, uint64_t* __restrict__ part,
                                           uint64_t* red) {
    if (valid) {
        plan[kQuads * (size_t)i] = u32x4{p[0], p[1], p[2], p[3]};
        plan[kQuads * (size_t)i + 1] = u32x4{p[4], p[5], p[6], p[7]};
        seg_first[i] = (uint32_t)cnt;
        obase[i] = bytes;
    }
    block_sums_to_part(cnt, bytes, part, red);
}

// one block: the nb block sums -> their exclusive prefixes, kSegBlock at a time with a carry;
// the totals, and the total count as a u32 to `count` unless that is null
__global__ __launch_bounds__(kSegBlock)
void scan_parts_kernel(uint64_t* __restrict__ part, uint32_t nb, uint64_t* __restrict__ totals,
                       uint32_t* __restrict__ count) {
    __shared__ uint64_t red[2 * kWavesPerBlock];
    uint64_t ca = 0, cb = 0;
    for (uint32_t base = 0; base < nb; base += kSegBlock) {
        const uint32_t k = base + threadIdx.x;
        uint64_t a = k < nb ? part[2 * (size_t)k] : 0, b = k < nb ? part[2 * (size_t)k + 1] : 0;
        uint64_t ta, tb;
        block_excl_scan2(a, b, ta, tb, red);
        if (k < nb) {
            part[2 * (size_t)k] = ca + a;
            part[2 * (size_t)k + 1] = cb + b;
        }
        ca += ta;
        cb += tb;
    }
    if (threadIdx.x == 0) {
        totals[0] = ca;
        totals[1] = cb;
        if (count) *count = (uint32_t)ca;
    }
}

// after scan_parts_kernel over the block sums, which also stores seg_first[n]:
// one block per kSegBlock frames: counts and bytes -> seg_first and the output byte bases
__attribute__((unused))          // rpkt_coalesce.hip places its outputs with a scan of its own
__global__ __launch_bounds__(kSegBlock)
void segment_scan_frames_kernel(uint32_t n, const uint64_t* __restrict__ part,
                                uint32_t* __restrict__ seg_first, uint64_t* __restrict__ obase) {
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    uint64_t a = i < n ? seg_first[i] : 0, b = i < n ? obase[i] : 0;
    uint64_t ta, tb;
    block_excl_scan2(a, b, ta, tb, red);
    if (i < n) {
        seg_first[i] = (uint32_t)(part[2 * (size_t)blockIdx.x] + a);
        obase[i] = part[2 * (size_t)blockIdx.x + 1] + b;
    }
}

// ---- runs of positions (rpkt_coalesce.hip, rpkt_reassemble.hip) ---------------------------

// inclusive max-scan over the block's kSegBlock threads; red: kWavesPerBlock u32 of LDS
__device__ __forceinline__ uint32_t block_incl_max(uint32_t v, uint32_t* red) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t x = wave_incl_max(v);
    if (lane == kWave - 1) red[wave] = x;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w)
        if (w < wave) x = max(x, red[w]);
    __syncthreads();                                              // red is free for the next call
    return x;
}

// one block: pmax[b] becomes the index + 1 of the last run head in blocks 0..b
__attribute__((unused))          // the units that cut have no runs of positions
__global__ __launch_bounds__(kSegBlock)
void scan_heads_kernel(uint32_t* __restrict__ pmax, uint32_t nb) {
    __shared__ uint32_t red[kWavesPerBlock];
    __shared__ uint32_t last;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kSegBlock) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t x = max(block_incl_max(k < nb ? pmax[k] : 0u, red), carry);
        if (k < nb) pmax[k] = x;
        if (threadIdx.x == kSegBlock - 1) last = x;
        __syncthreads();
        carry = last;
        __syncthreads();
    }
}

// the frame-relative dwords of a header in turn: one aligned load a step
struct HeaderWalk {
    uint32_t a4, sh, lo;
    __device__ __forceinline__ HeaderWalk(__amdgpu_buffer_rsrc_t rs, uint32_t fb, uint32_t s)
        : a4(s & ~3u), sh(s & 3u), lo(ldw(rs, fb, s & ~3u)) {}
    __device__ __forceinline__ uint32_t next(__amdgpu_buffer_rsrc_t rs, uint32_t fb) {
        const uint32_t hi = ldw(rs, fb, a4 + 4u);
        const uint32_t v = align_bytes(hi, lo, sh);
        lo = hi;
        a4 += 4u;
        return v;
    }
};

// bytes [lo, hi) of dword v to the output at x (4-B aligned): one dword store, or bytes
__device__ __forceinline__ void store_dword_part(__amdgpu_buffer_rsrc_t ro, uint32_t x, uint32_t v,
                                                 int lo, int hi) {
    if (hi <= 0 || lo >= 4) return;
    if (lo <= 0 && hi >= 4) {
        __builtin_amdgcn_raw_buffer_store_b32(v, ro, (int)x, 0, 0);
        return;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b >= lo && b < hi)
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v >> (8 * b)), ro, (int)(x + b), 0, 0);
}

// Copy src [s0, s0 + len) of the frames buffer to dst [d0, d0 + len) of the output, the
// whole wave: lane l of pass t owns the 16-B aligned destination chunk t * 64 + l.  The
// chunk's source bytes start at phase sh = (s0 - d0) & 15 of an aligned source chunk
// (wave-uniform), so they are that chunk and the next, shifted.  Whole chunks go out as one
// dwordx4 store, the (at most two) partial ones as dwords and bytes: their other bytes belong
// to the neighbouring output frames, which other waves write.  Returns this lane's part of
// the word sum of the bytes copied, over absolute-destination-aligned LE words (SUM).
constexpr int kCopyUnroll = 2;     // destination chunks (and their loads) in flight per lane
#ifndef RPKT_SEG_NT
#define RPKT_SEG_NT 0              // 2: non-temporal copy loads and dwordx4 stores
#endif
constexpr int kCopyAux = RPKT_SEG_NT;
template <bool SUM>
__device__ __forceinline__ uint32_t wave_copy(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                              __amdgpu_buffer_rsrc_t ro, uint32_t s0, uint32_t d0,
                                              uint32_t len, int lane) {
    uint32_t acc = 0;
    if (len == 0) return acc;
    const uint32_t dbase = d0 & ~15u, dend = d0 + len;
    const uint32_t sh = (s0 - d0) & 15u, q = sh >> 2, r = sh & 3u;       // wave-uniform
    const uint32_t nchunk = (dend - dbase + 15u) >> 4;                   // counted: dc never wraps
    for (uint32_t c0 = (uint32_t)lane; c0 < nchunk; c0 += kCopyUnroll * kWave) {
        u32x4 A[kCopyUnroll], B[kCopyUnroll];
        uint32_t sa[kCopyUnroll];
        // every load of the pass first, unconditional (a chunk past the end reads the
        // descriptor's out-of-range offset: zeros, no traffic)
#pragma unroll
        for (int u = 0; u < kCopyUnroll; ++u) {
            const uint32_t c = c0 + u * kWave;
            // source address of destination byte dc (before the frame's start for the first
            // chunk: those addresses wrap past the range and read as 0; their bytes are not
            // kept)
            sa[u] = c < nchunk ? (s0 + (dbase + 16u * c - d0)) & ~15u : fb;
            A[u] = load16_fast<kCopyAux>(rs, sa[u]);
            B[u] = load16_fast<kCopyAux>(rs, sh != 0u && c < nchunk ? sa[u] + 16u : fb);
        }
#pragma unroll
        for (int u = 0; u < kCopyUnroll; ++u) {
            const uint32_t c = c0 + u * kWave;
            if (c >= nchunk) break;
            const uint32_t dc = dbase + 16u * c;
            u32x4 a = A[u], b = B[u];
            // a chunk that straddles the buffer's end was dropped whole: re-read it (rare)
            if (__builtin_expect(straddles(sa[u], fb), 0)) a = load16(rs, sa[u], fb);
            if (__builtin_expect(sh != 0u && straddles(sa[u] + 16u, fb), 0))
                b = load16(rs, sa[u] + 16u, fb);
            const uint32_t W[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t T[5];
#pragma unroll
            for (int m = 0; m < 5; ++m)
                T[m] = q == 0u ? W[m] : (q == 1u ? W[m + 1] : (q == 2u ? W[m + 2] : W[m + 3]));
            u32x4 v;
            v.x = align_bytes(T[1], T[0], r);
            v.y = align_bytes(T[2], T[1], r);
            v.z = align_bytes(T[3], T[2], r);
            v.w = align_bytes(T[4], T[3], r);
            const int lo = dc < d0 ? (int)(d0 - dc) : 0;
            const int hi = dend - dc < 16u ? (int)(dend - dc) : 16;
            if (SUM) acc += chunk_sum(v, lo, hi);
            if (lo == 0 && hi == 16) {
                __builtin_amdgcn_raw_buffer_store_b128(v, ro, (int)dc, 0, kCopyAux);
            } else {
                store_dword_part(ro, dc, v.x, lo, hi);
                store_dword_part(ro, dc + 4u, v.y, lo - 4, hi - 4);
                store_dword_part(ro, dc + 8u, v.z, lo - 8, hi - 8);
                store_dword_part(ro, dc + 12u, v.w, lo - 12, hi - 12);
            }
        }
    }
    return acc;
}

// the fields an output's header differs in: n bytes at frame offset off, value in memory order
struct SegPatch {
    uint32_t off, n, val;
};
constexpr int kSegPatches = 5;     // a header's patches; an entry with more sizes its own array

// The header [s0, s0 + len) goes to [d0, d0 + len) a lane per 4-B aligned destination dword
// (headers are a few dwords: one pass as a rule).  header_dword: the source bytes of
// destination dword c.
__device__ __forceinline__ uint32_t header_dword(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                 uint32_t s0, uint32_t d0, uint32_t c) {
    return gdword(rs, fb, s0 + ((d0 & ~3u) + 4u * c - d0));
}

// Copy a `len`-byte header to [d0, d0 + len) with the patches applied.  fetch(c): the source
// bytes of destination dword c, as header_dword gives them; `first`: fetch(lane), which the
// caller loaded along with the payload.
template <int N, class Fetch>
__device__ __forceinline__ void wave_copy_header_from(__amdgpu_buffer_rsrc_t ro, uint32_t d0,
                                                      uint32_t len, uint32_t first,
                                                      const SegPatch (&P)[N], int lane, Fetch fetch) {
    const uint32_t dend = d0 + len;
    const uint32_t ndw = (dend - (d0 & ~3u) + 3u) >> 2;
    for (uint32_t c = (uint32_t)lane; c < ndw; c += kWave) {
        const uint32_t dd = (d0 & ~3u) + 4u * c;
        const int rel = (int)(dd - d0);                 // header offset of the dword's byte 0
        uint32_t v = c < (uint32_t)kWave ? first : fetch(c);
#pragma unroll
        for (int k = 0; k < N; ++k) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t idx = (uint32_t)(rel + b) - P[k].off;
                if (idx < P[k].n)
                    v = (v & ~(0xffu << (8 * b))) | (((P[k].val >> (8u * idx)) & 0xffu) << (8 * b));
            }
        }
        store_dword_part(ro, dd, v, rel < 0 ? -rel : 0, dend - dd < 4u ? (int)(dend - dd) : 4);
    }
}

// The same for a header that lies at [s0, s0 + len) of the frames buffer.
template <int N>
__device__ __forceinline__ void wave_copy_header(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                                 __amdgpu_buffer_rsrc_t ro, uint32_t s0,
                                                 uint32_t d0, uint32_t len, uint32_t first,
                                                 const SegPatch (&P)[N], int lane) {
    wave_copy_header_from(ro, d0, len, first, P, lane,
                          [&](uint32_t c) { return header_dword(rs, fb, s0, d0, c); });
}

// The header bytes of a flat frame at `off` of the frames buffer: dw(x), header bytes
// x .. x + 3 as a little-endian dword; sum(a, b), the big-endian RFC 1071 sum of [a, b).
struct FlatHeader {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t fb, off;
    __device__ __forceinline__ uint32_t dw(uint32_t x) const { return gdword(rs, fb, off + x); }
    __device__ __forceinline__ uint32_t sum(uint32_t a, uint32_t b) const {
        return range_be_sum(rs, fb, off + a, off + b);
    }
};

// One output of a re-framed frame: its offsets, the payload bytes it carries ([done, + pk) of
// the frame's payload) and where it goes (d0).  Segmentation fills it per output k (seg_out);
// coalescing for a merged frame (done 0, pk the merged payload).
struct SegOut {
    bool v6, last;
    uint32_t l3, l4, po, done, pk, d0;
};

// A wave writes kSegRun consecutive outputs.  What precedes an output's first copy load is a
// chain of dependent loads (the totals, the search, the plan), microseconds against the
// fraction of one that 1.5 KB take to copy; with one output a wave that chain bounded the
// kernel at 0.55 of the same bytes' device copy.  Here the search is done once for the run,
// and the outputs after the first find their frame by stepping along seg_first.
#ifndef RPKT_SEG_RUN
#define RPKT_SEG_RUN 8
#endif
constexpr uint32_t kSegRun = RPKT_SEG_RUN;

// The wave's run of outputs [j0, jend) and the input frame i of output j0; false when the
// wave has nothing to write (past out_cap, an overflowing batch, only spare slots, whose
// offsets it fills).  Wave-uniform throughout.
__device__ __forceinline__ bool output_run(uint32_t n, const uint32_t* __restrict__ seg_first,
                                           const uint64_t* __restrict__ totals, uint32_t out_bytes,
                                           uint32_t* __restrict__ out_offsets, uint32_t out_cap,
                                           int lane, uint32_t& j0, uint32_t& jend, uint32_t& i) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t j64 = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kSegRun;
    if (j64 >= out_cap) return false;
    j0 = (uint32_t)j64;
    const uint32_t j1 = out_cap - j0 < kSegRun ? out_cap : j0 + kSegRun;   // outputs [j0, j1)
    const uint64_t n_out = totals[0], need = totals[1];
    if (n_out > out_cap || need > out_bytes) return false;        // overflow: the totals say so
    // spare slots are empty frames at the end
    if ((uint32_t)lane < j1 - j0 && j0 + (uint32_t)lane >= n_out)
        out_offsets[j0 + (uint32_t)lane + 1u] = (uint32_t)need;
    if (j0 >= n_out) return false;
    if (j0 == 0u && lane == 0) out_offsets[0] = 0u;
    // the input frame of output j0: the last i with seg_first[i] <= j0 (every frame has an
    // output, so i <= j0).  64 probes a round, one per lane: three dependent loads at
    // n = 32,768 where a binary search has fifteen.
    uint32_t lo = 0, hi = j0 < n - 1u ? j0 : n - 1u;
    while (lo < hi) {
        const uint32_t step = (hi - lo) / kWave + 1u;
        const uint64_t at = (uint64_t)lo + (uint64_t)(lane + 1) * step;
        const bool le = at <= hi && seg_first[at] <= j0;          // true on the first c lanes
        const uint32_t c = (uint32_t)__popcll(__ballot(le));
        lo += c * step;
        hi = hi - lo < step - 1u ? hi : lo + step - 1u;
    }
    i = lo;
    jend = j1 < n_out ? j1 : (uint32_t)n_out;
    return true;
}

// the scans and the write's grid, the same for both entries: `n` inputs planned into ws
template <typename... KArgs, typename... Args>
int scan_and_write(void (*write_kernel)(KArgs...), const SegWs& ws, uint32_t n, uint32_t out_cap,
                   uint32_t* seg_first_dev, uint64_t* totals_dev, hipStream_t st, Args... args) {
    const uint32_t nb = blocks(n);
    RPKT_TRY(launch(scan_parts_kernel, dim3(1), dim3(kSegBlock), 0, st, ws.part, nb, totals_dev,
                    seg_first_dev + n));
    RPKT_TRY(launch(segment_scan_frames_kernel, dim3(nb), dim3(kSegBlock), 0, st, n, ws.part,
                    seg_first_dev, ws.obase));
    const uint64_t per_block = (uint64_t)kWavesPerBlock * kSegRun;        // outputs a block
    const uint32_t wb = (uint32_t)(((uint64_t)out_cap + per_block - 1) / per_block);
    return launch(write_kernel, dim3(wb), dim3(kSegBlock), 0, st, args...);
}

// ---- tunnels: the carrier of an inner TCP / UDP frame -----------------------------------
//
// What rpkt_gpu_segment_tunnel_batch (rpkt_segment.hip, "tunnels"),
// rpkt_gpu_coalesce_tunnel_batch (rpkt_coalesce.hip) and rpkt_gpu_fragment_tunnel_batch
// (rpkt_fragment.hip, "tunnels": the carrier of an inner IPv4 packet) share: the bits that say which outer
// headers a frame has, the rule for a carrier whose headers can be fixed up, the constants of
// its outer checksums and the outer patches of an output.
constexpr uint32_t kTunOn = 8u, kTunV6 = 16u, kTunUdp = 32u, kTunGtp = 64u, kTunCsum = 128u;
constexpr int kTunPatches = 9;

// What the outer record (dwords 0, 5, 7, 8, 16) and the tunnel record say about the carrier of
// an inner frame at `in`: ok, the outer headers are ones the write can fix up and the offsets
// nest (outer l3 + 20 (IPv6: 40) <= l4; VXLAN / GTP-U: status OK, protocol 17, l4 + 8 <=
// tun_off; GRE: protocol 47, l4 == tun_off; tun_off + 8 (GRE: 4) <= inner_off <= inner l3).
struct TunWhere {
    bool ok, v6, udp, gtp;
    uint32_t l3, l4, toff, ioff, pdst;
};
__device__ __forceinline__ TunWhere tun_where(uint32_t w0, uint32_t w5, uint32_t w7, uint32_t w8,
                                              uint32_t w16, u32x4 t, const L4Where& in) {
    const uint32_t status = w0 & 0xffu, nv = (w0 >> 8) & 0xffu;
    const uint32_t det = nv == 0u ? w0 >> 16 : (nv == 1u ? w5 & 0xffffu : w5 >> 16);
    const bool v6 = det == 0x86ddu;
    const uint32_t proto = (w8 >> 8) & 0xffu, frag = w7 >> 16, pdst = w8 >> 16;
    const uint32_t l3 = w16 & 0xffffu, l4 = w16 >> 16;
    const uint32_t kind = t.x & 0xffu, toff = t.x >> 16, ioff = t.y & 0xffffu;
    const bool gre = kind == RPKT_TUN_GRE, gtp = kind == RPKT_TUN_GTPU;
    const bool carrier = gre ? (proto == 47u && l4 == toff)
                             : ((kind == RPKT_TUN_VXLAN || gtp) && status == RPKT_S_OK &&
                                proto == 17u && l4 + 8u <= toff);
    const bool nest = l4 >= l3 && (v6 ? l4 - l3 >= 40u : (l4 - l3 >= 20u && l4 - l3 <= 60u)) &&
                      toff + (gre ? 4u : 8u) <= ioff && ioff <= in.l3;
    const bool ok = carrier && (v6 || det == 0x0800u) && (v6 || (frag & 0x3fffu) == 0u) && nest;
    return TunWhere{ok, v6, !gre, gtp, l3, l4, toff, ioff, pdst};
}

// Plan words 8..11 (q[0..3]) and the tunnel bits of word 7 for a frame whose inner packet is
// cut; false when the GRE header forbids it (the S or R bit, or C without room for its word).
// The constant under the outer checksum is [origin, end) without the outer fields the write
// patches and without what `inner(drop)` drops: the inner fields the caller's write patches.
template <class Header, class InnerDrops>
__device__ __forceinline__ bool tunnel_constants_to(const Header& H, const TunWhere& w,
                                                    uint32_t end, uint32_t (&q)[4],
                                                    uint32_t& bits, InnerDrops inner) {
    const uint32_t l3 = w.l3, l4 = w.l4, toff = w.toff, po = end;
    bool csum;
    uint32_t origin, c = 0;
    if (w.udp) {
        csum = (H.dw(l4 + 4u) >> 16) != 0u;                      // a zero checksum stays zero
        origin = l4;
        if (csum) {
            if (!w.v6) {
                c = 17u + H.sum(l3 + 12u, l3 + 20u);
            } else {
                const uint32_t pd = ip6_pseudo_dst(w.pdst, l3, l4);
                c = 17u + H.sum(l3 + 8u, l3 + 24u) + H.sum(pd, pd + 16u);
            }
        }
    } else {
        const uint32_t g0 = H.dw(toff) & 0xffu;                  // C 0x80, R 0x40, K 0x20, S 0x10
        csum = (g0 & 0x80u) != 0u;
        if ((g0 & 0x50u) || (csum && toff + 8u > w.ioff)) return false;
        origin = toff;
    }
    if (csum) {
        // [origin, po) without the bytes the write patches: each leaves by its complement
        c += H.sum(origin, po);
        auto drop = [&](uint32_t off, uint32_t n) {
            const uint32_t v = H.sum(off, off + n);
            c += 0xffffu ^ (((off - origin) & 1u) ? bswap16(v) : v);
        };
        if (w.udp) drop(l4 + 4u, 4u); else drop(toff + 4u, 2u);
        if (w.gtp) drop(toff + 2u, 2u);
        inner(drop);
    }
    uint32_t opc = 0, oident = 0;
    if (!w.v6) {
        const uint32_t ip0 = H.dw(l3), ip1 = H.dw(l3 + 4u), ip2 = H.dw(l3 + 8u);
        oident = be16_lo(ip1);
        opc = H.sum(l3, l4) + (0xffffu ^ be16_hi(ip0)) + (0xffffu ^ oident) + (0xffffu ^ be16_hi(ip2));
    }
    q[0] = l3 | (l4 << 16);
    q[1] = toff;
    q[2] = fold16(opc) | (oident << 16);
    q[3] = fold16(c);
    bits = kTunOn | (w.v6 ? kTunV6 : 0u) | (w.udp ? kTunUdp : 0u) | (w.gtp ? kTunGtp : 0u) |
           (csum ? kTunCsum : 0u);
    return true;
}

// The same for a frame whose inner TCP / UDP frame `s` is segmented or merged: the constant
// runs to the inner payload and drops the inner IP length (IPv4: and ident, checksum), and the
// L4 fields seg_patches writes.
template <class Header>
__device__ __forceinline__ bool tunnel_constants(const Header& H, const L4Where& s,
                                                 const TunWhere& w, uint32_t (&q)[4],
                                                 uint32_t& bits) {
    return tunnel_constants_to(H, w, s.po, q, bits, [&](auto drop) {
        if (s.v6) {
            drop(s.l3 + 4u, 2u);
        } else {
            drop(s.l3 + 2u, 4u);
            drop(s.l3 + 10u, 2u);
        }
        drop(s.l4 + 4u, 4u);
        if (!s.udp) {
            drop(s.l4 + 13u, 1u);
            drop(s.l4 + 16u, 2u);
        }
    });
}

// The outer headers' patches of output k, P[5..8], after the inner ones P[0..4]; pc: plan
// words 8..11, `pay` the payload's big-endian sum.
__device__ __forceinline__ void tunnel_patches(const SegOut& o, u32x4 pb, u32x4 pc, uint32_t k,
                                               uint32_t pay, SegPatch (&P)[kTunPatches]) {
    P[5] = P[6] = P[7] = P[8] = SegPatch{0u, 0u, 0u};
    if (!(pb.w & kTunOn)) return;                                 // wave-uniform
    const uint32_t l3 = pc.x & 0xffffu, l4 = pc.x >> 16, toff = pc.y & 0xffffu;
    const uint32_t tot = o.po + o.pk;
    if (!(pb.w & kTunV6)) {
        const uint32_t tlen = (tot - l3) & 0xffffu, ident = ((pc.z >> 16) + k) & 0xffffu;
        const uint32_t ck = ~fold16((pc.z & 0xffffu) + tlen + ident) & 0xffffu;
        P[5] = SegPatch{l3 + 2u, 4u, bswap16(tlen) | (bswap16(ident) << 16)};
        P[6] = SegPatch{l3 + 10u, 2u, bswap16(ck)};
    } else {
        P[5] = SegPatch{l3 + 4u, 2u, bswap16((tot - l3 - 40u) & 0xffffu)};
    }
    if (pb.w & kTunGtp) P[7] = SegPatch{toff + 2u, 2u, bswap16((tot - toff - 8u) & 0xffffu)};
    const bool udp = (pb.w & kTunUdp) != 0u, csum = (pb.w & kTunCsum) != 0u;
    const uint32_t origin = udp ? l4 : toff;
    uint32_t sum = 0;
    if (csum) {
        sum = pc.w + (((o.po - origin) & 1u) ? bswap16(pay) : pay);
        // the inner patches and the GTP-U length lie under the outer checksum
        const int under[6] = {0, 1, 2, 3, 4, 7};
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const SegPatch& x = P[under[u]];
            const uint32_t v = x.n >= 4u ? x.val : x.val & ((1u << (8u * x.n)) - 1u);
            sum += be_sum((v & 0xffffu) + (v >> 16), x.off - origin);
        }
    }
    if (udp) {
        // the length is in the pseudo header and in the header
        const uint32_t ulen = (tot - l4) & 0xffffu;
        const uint32_t uck = csum ? udp_csum_field(sum + 2u * ulen) : 0u;
        P[8] = SegPatch{l4 + 4u, 4u, bswap16(ulen) | (bswap16(uck) << 16)};
    } else if (csum) {
        P[8] = SegPatch{toff + 4u, 2u, bswap16(~fold16(sum) & 0xffffu)};   // RFC 2784: 0 stays 0
    }
}

}  // namespace
