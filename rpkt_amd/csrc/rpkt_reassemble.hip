// rpkt_reassemble.hip — rpkt_gpu_reassemble_batch: IPv4 (RFC 791) and IPv6 (RFC 8200 section
// 4.5) reassembly of the fragments of one device-resident batch, the inverse of
// rpkt_gpu_fragment_batch, and rpkt_gpu_reassemble_keys, the sort keys that bring a datagram's
// fragments together (include/rpkt_gpu.h has the semantics).
//
// Many positions make one output, so this is rpkt_coalesce.hip's structure with a fragment rule
// in the place of the TCP / UDP one: the work is planned per position and the bytes are placed
// by prefix sums.  Eight launches on the stream, no host step between them:
//   1. plan    one lane per position: its frame (through order_dev), its record (coalesced
//              through an LDS stage, or gathered under an order) for status, the dispatch
//              ethertype, l3_off, l4_off and ip_sum, and from the frame the words eligibility
//              needs: ihl, packet_len and the frag word, or payload_len, a walk of the extension
//              headers (at most RPKT_MAX_IP6_EXT) and the Fragment header;
//   2. link    one lane per position: B(i), the offsets' arithmetic on plan words and the
//              masked compare of its header with its predecessor's, a dword of each per step
//              through the buffer resource; the block's max-scan of run heads;
//   3. heads   one block: the max-scan of the blocks' last run heads, with a carry;
//   4. group   one lane per position: its run head, whether it opens an output, is merged or
//              is a member, and its byte contribution.  A run is one group: there is no cut.
//              The last member of a run knows the head's offset through the run head and its
//              own M: it says in done[head] whether the group is a complete IPv6 datagram, and
//              then contributes 8 bytes less, the Fragment header the output drops, so every
//              later output's start is exact;
//   5. sums    one block: exclusive prefix sums of the blocks' (outputs, bytes); the totals;
//   6. place   one lane per position: its output index and destination (its own exclusive
//              prefix is header bytes + off_i - off_head past the output's start; 8 less for
//              the members of a complete group, read from done[head]); src_first, the offsets;
//   7. copy    one wavefront per run of kRaRun consecutive POSITIONS: a lone frame is copied
//              whole, a member's (and a merged head's) payload goes to its destination with
//              wave_copy<false>: no payload byte is summed;
//   8. header  one wavefront per run of kRaHdrRun OUTPUTS: a merged one's header with the
//              patched lengths, frag word and checksum, or without its Fragment header.
// No kernel waits on another workgroup (done[] is written in launch 4 and read from launch 6
// on), every loop is bounded by a count from the plan, and the wave-uniform branches of copy
// and header are made on plan words.  Every load of frame bytes goes through the frames buffer
// resource and every store of output bytes through one over [out_frames_dev, + out_bytes); an
// overflowing call writes its totals and src_first and nothing else.
#include "rpkt_segcopy.h"

namespace {

// the workspace: per-position plans (32 B), destinations (u64), a u32 per position for the link
// bit and the block-local run head, a u32 per position that a run's last member writes for its
// head, the block sums (outputs, bytes: u64 pairs) and the blocks' run heads
struct RaWs {
    u32x4*    plan;
    uint64_t* obase;
    uint32_t* aux;
    uint32_t* done;
    uint64_t* part;
    uint32_t* pmax;
    size_t    bytes;
};
inline RaWs ra_ws(void* ws, uint32_t n) {
    Carve c(ws);
    RaWs w;
    w.plan = c.take<u32x4>(2 * (size_t)n);
    w.obase = c.take<uint64_t>(n);
    w.aux = c.take<uint32_t>(n);
    w.done = c.take<uint32_t>(n);
    w.part = c.take<uint64_t>(2 * (size_t)blocks(n));
    w.pmax = c.take<uint32_t>(blocks(n));
    w.bytes = c.used();
    return w;
}

// plan words: 0 frame offset, 1 frame length, 2 l3 | l4 << 16, 3 P | off << 16 (P: the payload
// bytes the fragment carries, off: their byte offset in the datagram), 4 kRaElig | kRaV6 |
// kRaMore (MF / M), 5 IPv6: the offset of the next-header byte that says 44 | the Fragment
// header's next_header << 16 (words 2..5: 0 unless eligible), 7 (from group on) kRaHead |
// kRaMerged, (from place on) | kRaWhole: a complete IPv6 datagram
constexpr uint32_t kRaElig = 1u, kRaV6 = 2u, kRaMore = 4u;
constexpr uint32_t kRaHead = 1u, kRaMerged = 2u, kRaWhole = 4u;
// aux: the block-local index + 1 of the position's run head (0: in an earlier block) | kRaLink
constexpr uint32_t kRaLink = 1u << 16;

// ---- the fragment rule -------------------------------------------------------------------

// What a record's dwords 0, 5, 16, 18 and the frame at H (len bytes) say: `on`, an eligible
// fragment; then its offsets, payload, and what the key hashes (ident, proto: 44 for IPv6).
struct FragWhere {
    bool on, v6, more;
    uint32_t l3, l4, P, off, nh, ident, proto;
};
__device__ __forceinline__ FragWhere frag_where(const FlatHeader& H, uint32_t w0, uint32_t w5,
                                                uint32_t w16, uint32_t w18, uint32_t len,
                                                bool trust) {
    const uint32_t status = w0 & 0xffu, nv = (w0 >> 8) & 0xffu;
    const uint32_t det = nv == 0u ? w0 >> 16 : (nv == 1u ? w5 & 0xffffu : w5 >> 16);
    const uint32_t l3 = w16 & 0xffffu, l4 = w16 >> 16;
    FragWhere f{false, det == 0x86ddu, false, l3, l4, 0u, 0u, 0u, 0u, 0u};
    const bool ip4_status = status == RPKT_S_OK || status == RPKT_S_ICMP_EMPTY ||
                            (status >= RPKT_S_L4_OTHER && status <= RPKT_S_TCP_BAD_DOFF);
    if (det == 0x0800u && ip4_status) {
        const uint32_t ip0 = H.dw(l3), ip1 = H.dw(l3 + 4u);
        const uint32_t ihl = (ip0 & 0xfu) * 4u, L = be16_hi(ip0), fw = be16_hi(ip1);
        if (ihl < 20u || l4 != l3 + ihl || L > len || l3 > len - L || L <= ihl) return f;
        if ((fw & 0x3fffu) == 0u) return f;                        // neither MF nor an offset
        f.P = L - ihl;
        f.off = (fw & 0x1fffu) * 8u;
        if (ihl + f.off + f.P > 65535u) return f;
        if (!trust && (w18 & 0xffffu) != 0xffffu) return f;
        f.more = (fw & 0x2000u) != 0u;
        f.ident = be16_lo(ip1);
        f.proto = (H.dw(l3 + 8u) >> 8) & 0xffu;
        f.on = true;
    } else if (f.v6 && status == RPKT_S_IP6_FRAGMENT) {
        if (l4 < l3 + 48u) return f;
        const uint32_t x = l4 - 8u;                                // the Fragment header
        const uint32_t ip1 = H.dw(l3 + 4u);
        uint32_t nh = (ip1 >> 16) & 0xffu, y = l3 + 40u, nhoff = l3 + 6u;
        for (int k = 0; k < RPKT_MAX_IP6_EXT && y < x; ++k) {
            const uint32_t d = H.dw(y);
            uint32_t hl;
            if (nh == 0u || nh == 43u || nh == 60u) hl = 8u * (1u + ((d >> 8) & 0xffu));
            else if (nh == 51u) hl = 4u * (2u + ((d >> 8) & 0xffu));
            else return f;
            if (hl > x - y) return f;
            nhoff = y;
            nh = d & 0xffu;
            y += hl;
        }
        if (y != x || nh != 44u) return f;
        const uint32_t E = l3 + 40u + be16_lo(ip1);
        if (E > len || E <= l4) return f;
        const uint32_t fh = H.dw(x), ow = be16_hi(fh);
        f.P = E - l4;
        f.off = ow & 0xfff8u;
        if ((x - l3 - 40u) + 8u + f.off + f.P > 65535u) return f;
        f.more = (ow & 1u) != 0u;
        f.nh = nhoff | ((fh & 0xffu) << 16);
        f.ident = bswap32(H.dw(x + 4u));
        f.proto = 44u;
        f.on = true;
    }
    return f;
}

// The record dwords the rule and the key read (0, 5, 9, 10, 16, 18) of the position's frame f,
// through the LDS stage `st` (no order: f is the wave's tile p0 + lane) or gathered.
struct RecWords {
    uint32_t w0, w5, w9, w10, w16, w18;
};
__device__ __forceinline__ RecWords rec_words(uint32_t* st, const rpkt_rec_t* __restrict__ recs,
                                              uint32_t p0, uint32_t n, int lane, bool staged,
                                              uint32_t f) {
    RecWords r{0u, 0u, 0u, 0u, 0u, 0u};
    if (staged) {
        stage_records_tile(st, recs, p0, n, lane);
        const uint32_t* w = st + lane * 21;
        r = RecWords{w[0], w[5], w[9], w[10], w[16], w[18]};
    } else if (f < n) {                                            // an entry >= n: an empty frame
        const u32x4* q = reinterpret_cast<const u32x4*>(recs + f);
        const u32x4 q0 = q[0], q1 = q[1], q2 = q[2], q4 = q[4];
        r = RecWords{q0.x, q1.y, q2.y, q2.z, q4.x, q4.z};
    }
    return r;
}

// ---- keys ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kSegBlock)
void reassemble_keys_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
                            const uint32_t* __restrict__ offsets, uint32_t stride, uint32_t frame_len,
                            uint32_t n, const rpkt_rec_t* __restrict__ recs, uint32_t trust,
                            uint64_t* __restrict__ keys) {
    __shared__ uint32_t stage[kWavesPerBlock][kWave * 21];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t p0 = blockIdx.x * kSegBlock + wave * kWave;
    const uint32_t i = p0 + lane;
    if (p0 >= n) return;                                          // wave-uniform
    const RecWords r = rec_words(stage[wave], recs, p0, n, lane, true, i);
    if (i >= n) return;
    const Frame fr = frame_span(offsets, stride, frame_len, fb, i);
    const FragWhere f = frag_where(FlatHeader{make_rsrc(frames, fb), fb, fr.off}, r.w0, r.w5, r.w16,
                                   r.w18, fr.len, trust != 0u);
    uint64_t key = (1ull << 63) | i;
    if (f.on) {
        const uint32_t h = flow_hash(r.w9, r.w10, f.ident & 0xffffu, f.ident >> 16, f.proto);
        key = ((uint64_t)(h & 0x7fffffffu) << 32) | (f.off >> 3);
    }
    keys[i] = key;
}

// ---- 1. plan -------------------------------------------------------------------------------

__global__ __launch_bounds__(kSegBlock)
void reassemble_plan_kernel(const uint8_t* __restrict__ frames, uint32_t fb,
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
    if (order && valid) f = order[i];
    const RecWords r = rec_words(stage[wave], recs, p0, n, lane, order == nullptr, f);
    if (!valid) return;
    const bool present = f < n;
    const Frame fr = present ? frame_span(offsets, stride, frame_len, fb, f) : Frame{0u, 0u};
    FragWhere w{};
    if (present)
        w = frag_where(FlatHeader{make_rsrc(frames, fb), fb, fr.off}, r.w0, r.w5, r.w16, r.w18,
                       fr.len, trust != 0u);
    const bool e = w.on;
    plan[2 * (size_t)i] = u32x4{fr.off, fr.len, e ? w.l3 | (w.l4 << 16) : 0u,
                                e ? w.P | (w.off << 16) : 0u};
    const uint32_t bits = kRaElig | (w.v6 ? kRaV6 : 0u) | (w.more ? kRaMore : 0u);
    plan[2 * (size_t)i + 1] = u32x4{e ? bits : 0u, e ? w.nh : 0u, 0u, 0u};
}

// ---- 2. link -------------------------------------------------------------------------------

// which bits of the header dword at frame offset x enter the compare.  IPv4: the bytes before
// l3, ident, protocol and the addresses.  IPv6: everything before l4 (the Fragment header's end)
// but payload_len and the Fragment header's offset / M.
__device__ __forceinline__ uint32_t frag_keep(uint32_t x, uint32_t l3, uint32_t l4, bool v6) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t y = x + b, d3 = y - l3, dx = y - (l4 - 8u);
        bool keep;
        if (v6) keep = y < l4 && !(d3 == 4u || d3 == 5u || dx == 2u || dx == 3u);
        else keep = y < l3 || d3 == 4u || d3 == 5u || d3 == 9u || (d3 >= 12u && d3 < 20u);
        m |= (keep ? 0xffu : 0u) << (8u * b);
    }
    return m;
}

// B(i), i >= 1: the fragment at position i continues the one at i - 1
__device__ __forceinline__ bool frag_pred(__amdgpu_buffer_rsrc_t rs, uint32_t fb,
                                          const u32x4* __restrict__ plan, uint32_t i) {
    const u32x4 pa = plan[2 * (size_t)i], qa = plan[2 * (size_t)i - 2];
    const uint32_t pz = plan[2 * (size_t)i + 1].x, qz = plan[2 * (size_t)i - 1].x;
    if (!(pz & qz & kRaElig) || ((pz ^ qz) & kRaV6) || pa.z != qa.z) return false;
    const uint32_t pq = qa.w & 0xffffu;                            // off + P <= 65535 each
    if (!(qz & kRaMore) || (pq & 7u) || (pa.w >> 16) != (qa.w >> 16) + pq) return false;
    const bool v6 = (pz & kRaV6) != 0u;
    const uint32_t l3 = pa.z & 0xffffu, l4 = pa.z >> 16;
    const uint32_t end = v6 ? l4 : l3 + 20u;                       // <= 65555
    HeaderWalk a(rs, fb, pa.x), b(rs, fb, qa.x);
    for (uint32_t x = 0; x < end; x += 4u)
        if ((a.next(rs, fb) ^ b.next(rs, fb)) & frag_keep(x, l3, l4, v6)) return false;
    return true;
}

__global__ __launch_bounds__(kSegBlock)
void reassemble_link_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                            const u32x4* __restrict__ plan, uint32_t* __restrict__ aux,
                            uint32_t* __restrict__ pmax) {
    __shared__ uint32_t red[kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    const bool valid = i < n;
    const bool link = valid && i >= 1u && frag_pred(make_rsrc(frames, fb), fb, plan, i);
    const uint32_t hl = block_incl_max(valid && !link ? threadIdx.x + 1u : 0u, red);
    if (valid) aux[i] = hl | (link ? kRaLink : 0u);
    if (threadIdx.x == kSegBlock - 1)
        pmax[blockIdx.x] = hl ? blockIdx.x * kSegBlock + hl : 0u; // global index + 1
}

// ---- 3. heads: scan_heads_kernel (rpkt_segcopy.h) --------------------------------------------

// position i's run head (<= i) from its aux word and the blocks' scanned run heads
__device__ __forceinline__ uint32_t run_head(uint32_t a, const uint32_t* __restrict__ pmax) {
    const uint32_t hl = a & 0xffffu;
    const uint32_t hp = hl ? blockIdx.x * kSegBlock + hl : (blockIdx.x ? pmax[blockIdx.x - 1u] : 0u);
    return hp ? hp - 1u : 0u;
}

// ---- 4. group ------------------------------------------------------------------------------

__global__ __launch_bounds__(kSegBlock)
void reassemble_group_kernel(uint32_t n, u32x4* __restrict__ plan, const uint32_t* __restrict__ aux,
                             const uint32_t* __restrict__ pmax, uint32_t* __restrict__ done,
                             uint64_t* __restrict__ obase, uint64_t* __restrict__ part) {
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    uint64_t cnt = 0, bytes = 0;
    if (i < n) {
        const uint32_t a = aux[i];
        const bool head = !(a & kRaLink);
        const bool last = !(i + 1u < n && (aux[i + 1u] & kRaLink));       // of its run
        const u32x4 pa = plan[2 * (size_t)i];
        const uint32_t P = pa.w & 0xffffu, l4 = pa.z >> 16;
        cnt = head ? 1u : 0u;
        bytes = !head ? P : (last ? pa.y : l4 + P);                // a linked position is eligible
        if (last) {
            const uint32_t h = run_head(a, pmax);
            bool whole = false;
            if (!head) {
                const uint32_t z = plan[2 * (size_t)i + 1].x;
                whole = (z & kRaV6) && !(z & kRaMore) && (plan[2 * (size_t)h].w >> 16) == 0u;
            }
            // the Fragment header a complete datagram drops; u64 sums wrap, and the head's l4
            // bytes precede this position's, so every prefix is exact
            if (whole) bytes -= 8u;
            done[h] = whole ? 1u : 0u;
        }
        plan[2 * (size_t)i + 1].w = (head ? kRaHead : 0u) | (head && !last ? kRaMerged : 0u);
        obase[i] = bytes;
    }
    block_sums_to_part(cnt, bytes, part, red);
}

// ---- 5. sums: scan_parts_kernel (rpkt_segcopy.h) ----------------------------------------------

// ---- 6. place ------------------------------------------------------------------------------

__global__ __launch_bounds__(kSegBlock)
void reassemble_place_kernel(uint32_t n, u32x4* __restrict__ plan, const uint32_t* __restrict__ aux,
                             const uint32_t* __restrict__ pmax, const uint32_t* __restrict__ done,
                             const uint64_t* __restrict__ part, const uint64_t* __restrict__ totals,
                             uint64_t* __restrict__ obase, uint32_t* __restrict__ src_first,
                             uint32_t* __restrict__ out_offsets, uint32_t out_cap,
                             uint32_t out_bytes) {
    __shared__ uint64_t red[2 * kWavesPerBlock];
    const uint32_t i = blockIdx.x * kSegBlock + threadIdx.x;
    const bool valid = i < n;
    const uint32_t role = valid ? plan[2 * (size_t)i + 1].w : 0u;
    uint64_t a = role & kRaHead, b = valid ? obase[i] : 0;
    uint64_t ta, tb;
    block_excl_scan2(a, b, ta, tb, red);
    const uint64_t n_out = totals[0], need = totals[1];
    const bool fits = n_out <= out_cap && need <= out_bytes;
    if (valid) {
        const uint64_t j = part[2 * (size_t)blockIdx.x] + a;      // < n_out <= n
        uint64_t dest = part[2 * (size_t)blockIdx.x + 1] + b;
        if ((role & (kRaHead | kRaMerged)) != kRaHead && done[run_head(aux[i], pmax)]) {
            if (!(role & kRaHead)) dest -= 8u;                    // after l4 - 8 header bytes
            plan[2 * (size_t)i + 1].w = role | kRaWhole;
        }
        obase[i] = dest;
        if (role & kRaHead) {
            src_first[j] = i;
            if (fits) out_offsets[j] = (uint32_t)dest;            // j < n_out <= out_cap
        }
        if (i >= n_out) src_first[i] = n;
        if (i == 0u) src_first[n] = n;
    }
    // the end of the last output and the spare slots: empty frames at the end
    if (fits) {
        const uint64_t step = (uint64_t)gridDim.x * kSegBlock;
        for (uint64_t k = n_out + i; k <= out_cap; k += step) out_offsets[k] = (uint32_t)need;
    }
}

// ---- 7. copy -------------------------------------------------------------------------------

// A wave copies kRaRun consecutive positions (rpkt_coalesce.hip's kCoRun: the plans and
// destinations of the whole run are fetched at once, a lane each).
#ifndef RPKT_RA_RUN
#define RPKT_RA_RUN 8
#endif
constexpr uint32_t kRaRun = RPKT_RA_RUN;
static_assert(kRaRun <= (uint32_t)kWave, "a lane per position of the run");

__global__ __launch_bounds__(kSegBlock)
void reassemble_copy_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                            const u32x4* __restrict__ plan, const uint64_t* __restrict__ obase,
                            const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                            uint32_t out_bytes, uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t i64 = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kRaRun;
    if (i64 >= n) return;                                         // wave-uniform, as all below
    if (totals[0] > out_cap || totals[1] > out_bytes) return;     // overflow: the totals say so
    const uint32_t i0 = (uint32_t)i64;
    const uint32_t cnt = n - i0 < kRaRun ? n - i0 : kRaRun;
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
        const uint32_t l4 = (uint32_t)__shfl((int)la.z, (int)k, kWave) >> 16;
        const uint32_t P = (uint32_t)__shfl((int)la.w, (int)k, kWave) & 0xffffu;
        const uint32_t role = (uint32_t)__shfl((int)lrole, (int)k, kWave);
        const uint32_t dst = (uint32_t)__shfl((int)ldst, (int)k, kWave);
        if ((role & (kRaHead | kRaMerged)) == kRaHead) {          // a lone frame: a byte copy
            wave_copy<false>(rs, fb, ro, foff, dst, flen, lane);
            continue;
        }
        // a merged head's payload follows its header; a member's is at its destination
        const uint32_t hdr = (role & kRaHead) ? l4 - ((role & kRaWhole) ? 8u : 0u) : 0u;
        wave_copy<false>(rs, fb, ro, foff + l4, dst + hdr, P, lane);
    }
}

// ---- 8. header -----------------------------------------------------------------------------

#ifndef RPKT_RA_HDR_RUN
#define RPKT_RA_HDR_RUN 4
#endif
constexpr uint32_t kRaHdrRun = RPKT_RA_HDR_RUN;
constexpr int kRaPatches = 3;

__global__ __launch_bounds__(kSegBlock)
void reassemble_header_kernel(const uint8_t* __restrict__ frames, uint32_t fb, uint32_t n,
                              const u32x4* __restrict__ plan, const uint64_t* __restrict__ obase,
                              const uint32_t* __restrict__ src_first,
                              const uint64_t* __restrict__ totals, uint8_t* __restrict__ out,
                              uint32_t out_bytes, uint32_t out_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t j64 = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) * kRaHdrRun;
    const uint64_t n_out = totals[0], need = totals[1];
    if (j64 >= n_out || n_out > out_cap || need > out_bytes) return;      // wave-uniform
    const uint32_t j0 = (uint32_t)j64;
    const uint32_t j1 = n_out - j0 < kRaHdrRun ? (uint32_t)n_out : j0 + kRaHdrRun;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(frames, fb);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, out_bytes);
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t i0 = src_first[j], i1 = src_first[j + 1u];        // j + 1 <= n_out <= n
        if (i1 > n || i1 - i0 < 2u || i1 < i0) continue;                  // one frame: copied
        const u32x4 pa = plan[2 * (size_t)i0], pb = plan[2 * (size_t)i0 + 1];
        // the last member: the fragments of a run are contiguous, so its end is the group's
        const u32x4 qa = plan[2 * (size_t)i1 - 2];
        const bool more = (plan[2 * (size_t)i1 - 1].x & kRaMore) != 0u;
        const uint32_t d0 = (uint32_t)obase[i0];
        const uint32_t foff = pa.x, l3 = pa.z & 0xffffu, l4 = pa.z >> 16, off0 = pa.w >> 16;
        const uint32_t total = (qa.w >> 16) + (qa.w & 0xffffu) - off0;    // <= 65535
        const bool v6 = (pb.x & kRaV6) != 0u, whole = (pb.w & kRaWhole) != 0u;   // wave-uniform
        SegPatch Pt[kRaPatches];
        uint32_t hlen = l4;
        if (!v6) {
            // the header's sum without packet_len, frag word and checksum: a field leaves a sum
            // by adding its complement
            uint32_t x = 0, y = 0;
            if (lane == 0) {
                const uint32_t a3 = foff + l3;
                const uint32_t ip0 = gdword(rs, fb, a3), ip1 = gdword(rs, fb, a3 + 4u),
                               ip2 = gdword(rs, fb, a3 + 8u);
                y = be16_hi(ip1);
                x = range_be_sum(rs, fb, a3, foff + l4) + (0xffffu ^ be16_hi(ip0)) + (0xffffu ^ y) +
                    (0xffffu ^ be16_hi(ip2));
            }
            const uint32_t ipc = (uint32_t)__builtin_amdgcn_readlane((int)x, 0);
            const uint32_t fw0 = (uint32_t)__builtin_amdgcn_readlane((int)y, 0);
            const uint32_t fw = (fw0 & ~0x2000u) | (more ? 0x2000u : 0u);
            const uint32_t tot = l4 - l3 + total;
            const uint32_t ck = ~fold16(fold16(ipc) + tot + fw) & 0xffffu;
            Pt[0] = SegPatch{l3 + 2u, 2u, bswap16(tot & 0xffffu)};
            Pt[1] = SegPatch{l3 + 6u, 2u, bswap16(fw)};
            Pt[2] = SegPatch{l3 + 10u, 2u, bswap16(ck)};
        } else if (!whole) {
            Pt[0] = SegPatch{l3 + 4u, 2u, bswap16((l4 - l3 - 40u + total) & 0xffffu)};
            Pt[1] = SegPatch{l4 - 6u, 2u, bswap16(off0 | (more ? 1u : 0u))};
            Pt[2] = SegPatch{0u, 0u, 0u};
        } else {
            hlen = l4 - 8u;
            Pt[0] = SegPatch{l3 + 4u, 2u, bswap16((hlen - l3 - 40u + total) & 0xffffu)};
            Pt[1] = SegPatch{pb.y & 0xffffu, 1u, pb.y >> 16};
            Pt[2] = SegPatch{0u, 0u, 0u};
        }
        const uint32_t hfirst = header_dword(rs, fb, foff, d0, (uint32_t)lane);
        wave_copy_header(rs, fb, ro, foff, d0, hlen, hfirst, Pt, lane);
    }
}

}  // namespace

extern "C" {

size_t rpkt_gpu_reassemble_workspace_bytes(uint32_t n) { return ra_ws(nullptr, n).bytes; }

int rpkt_gpu_reassemble_batch(const rpkt_batch_t* b, const rpkt_rec_t* recs_dev,
                              const uint32_t* order_dev, uint32_t flags, uint8_t* out_frames_dev,
                              uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                              uint32_t* src_first_dev, uint64_t* totals_dev, void* workspace_dev,
                              void* stream) {
    // no limit argument: a constant in range in its place
    RPKT_TRY(reframe_args_ok(b, recs_dev, 65535u, flags, RPKT_REASSEMBLE_TRUST_SUMS, out_frames_dev,
                             out_bytes, out_offsets_dev, out_cap, src_first_dev, totals_dev,
                             workspace_dev));
    if (b->n == 0) return RPKT_OK;

    const RaWs ws = ra_ws(workspace_dev, b->n);
    const uint32_t n = b->n, nb = blocks(n), fb = (uint32_t)b->frames_bytes;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 blk(kSegBlock), per(nb);
    RPKT_TRY(launch_batch(reassemble_plan_kernel, kSegBlock, 0, stream, *b, recs_dev, order_dev,
                          flags & RPKT_REASSEMBLE_TRUST_SUMS, ws.plan));
    RPKT_TRY(launch(reassemble_link_kernel, per, blk, 0, st, b->frames_dev, fb, n, ws.plan, ws.aux,
                    ws.pmax));
    RPKT_TRY(launch(scan_heads_kernel, dim3(1), blk, 0, st, ws.pmax, nb));
    RPKT_TRY(launch(reassemble_group_kernel, per, blk, 0, st, n, ws.plan, ws.aux, ws.pmax, ws.done,
                    ws.obase, ws.part));
    RPKT_TRY(launch(scan_parts_kernel, dim3(1), blk, 0, st, ws.part, nb, totals_dev,
                    (uint32_t*)nullptr));
    RPKT_TRY(launch(reassemble_place_kernel, per, blk, 0, st, n, ws.plan, ws.aux, ws.pmax, ws.done,
                    ws.part, totals_dev, ws.obase, src_first_dev, out_offsets_dev, out_cap,
                    (uint32_t)out_bytes));
    const uint64_t cper = (uint64_t)kWavesPerBlock * kRaRun;             // positions a block
    RPKT_TRY(launch(reassemble_copy_kernel, dim3((uint32_t)(((uint64_t)n + cper - 1) / cper)), blk, 0,
                    st, b->frames_dev, fb, n, ws.plan, ws.obase, totals_dev, out_frames_dev,
                    (uint32_t)out_bytes, out_cap));
    const uint64_t hper = (uint64_t)kWavesPerBlock * kRaHdrRun;          // outputs a block
    const uint32_t outs = n < out_cap ? n : out_cap;                     // n_out <= both, or overflow
    return launch(reassemble_header_kernel, dim3((uint32_t)(((uint64_t)outs + hper - 1) / hper)), blk,
                  0, st, b->frames_dev, fb, n, ws.plan, ws.obase, src_first_dev, totals_dev,
                  out_frames_dev, (uint32_t)out_bytes, out_cap);
}

int rpkt_gpu_reassemble_keys(const rpkt_batch_t* b, const rpkt_rec_t* recs_dev, uint32_t flags,
                             uint64_t* keys_dev, void* stream) {
    if (!b || any_null(recs_dev, keys_dev)) return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, RPKT_REASSEMBLE_TRUST_SUMS));
    if (b->n == 0) return RPKT_OK;
    RPKT_TRY(batch_ok(*b));
    if (misaligned(15, recs_dev) || misaligned(7, keys_dev)) return RPKT_E_ALIGN;
    return launch_batch(reassemble_keys_kernel, kSegBlock, 0, stream, *b, recs_dev,
                        flags & RPKT_REASSEMBLE_TRUST_SUMS, keys_dev);
}

}  // extern "C"
