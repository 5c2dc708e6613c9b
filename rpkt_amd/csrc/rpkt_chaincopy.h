// rpkt_chaincopy.h — what the units that read mbuf chains (rpkt_chains_t) as a re-framing
// source share (rpkt_segment.hip: rpkt_gpu_segment_chains, rpkt_gpu_segment_tunnel_chains;
// rpkt_fragment.hip: rpkt_gpu_fragment_chains): the segment table under the chain parse's
// clamps, a chain's range of it, the header bytes of a chain whose header crosses segments, and
// the copy of a slice of a chain's logical bytes by a wave that carries its place in the
// segment list from one output to the next.
// Everything is inline in an anonymous namespace.
#pragma once
#include "rpkt_segcopy.h"

namespace {

// The segment table of rpkt_chains_t: segment k = (offset, length), clamped to the arena as
// the chain parse clamps it.  The table is only read, so it is read through the constant
// address space: with a wave-uniform k (the write's cursor) the load then stays on the
// scalar side whatever vector stores surround it, and does not wait for them.
struct SegTable {
    const uint32_t* segs;
    uint32_t fb;
    __device__ __forceinline__ Frame seg(uint32_t k) const {
        typedef __attribute__((address_space(4))) const uint32_t* cptr;
        const cptr p = (cptr)(segs + 2 * (size_t)k);
        const uint32_t x = p[0], y = p[1];
        const uint32_t off = x < fb ? x : fb;
        return Frame{off, y < fb - off ? y : fb - off};
    }
};

// The header bytes of a chain whose [0, lim) crosses segments (first segment `a`): each
// byte through a walk of the segment list, sums at the logical position's parity.
struct GatheredHeader {
    SegTable S;
    __amdgpu_buffer_rsrc_t rs;
    uint32_t a, n_segs, lim;
    // logical bytes x .. x + 3 (x may lie before 0, as a wrapped value); bytes outside
    // [0, lim) read as 0
    __device__ __forceinline__ uint32_t dw(uint32_t x) const {
        uint32_t v = 0, cum = 0;
        for (uint32_t k = a; k < n_segs && cum < lim; ++k) {
            const Frame s = S.seg(k);
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) {
                const uint32_t y = x + b;
                if (y < lim && y - cum < s.len) v |= gbyte(rs, s.off + (y - cum)) << (8u * b);
            }
            cum += s.len;
        }
        return v;
    }
    __device__ __forceinline__ uint32_t sum(uint32_t lo, uint32_t hi) const {
        hi = hi < lim ? hi : lim;
        uint32_t acc = 0, cum = 0;
        for (uint32_t k = a; k < n_segs && cum < hi; ++k) {
            const Frame s = S.seg(k);
            const uint32_t e = s.len < hi - cum ? cum + s.len : hi;
            for (uint32_t y = lo > cum ? lo : cum; y < e; ++y)
                acc += gbyte(rs, s.off + (y - cum)) << (((y - lo) & 1u) ? 0u : 8u);
            cum += s.len;
        }
        return fold16(acc);
    }
};

// chain p's first segment and the end of its list, under rpkt_chains_t's clamps
__device__ __forceinline__ void chain_range(const uint32_t* __restrict__ chain_first,
                                            uint32_t n_segs, uint32_t p, uint32_t& a, uint32_t& b) {
    const uint32_t f0 = chain_first[p], f1 = chain_first[p + 1];
    a = f0 < n_segs ? f0 : n_segs;
    b = f1 > a ? f1 : a;
    b = b < n_segs ? b : n_segs;
}

// A wave's place in a chain's segment list: segment k starts at logical byte `cum`.  The
// values are wave-uniform, so the segment table is read on the scalar side.
struct ChainCursor {
    uint32_t k, cum;
};

// Copy logical bytes [pos, pos + len) of the chain under the cursor (pos >= c.cum) to the
// output at d, one wave copy per segment they touch; the cursor moves to the segment that
// holds the slice's end.  Pieces that meet inside a 16-B destination chunk write disjoint
// bytes, and each piece's sum is over destination-aligned words, so the sums add.
template <bool SUM>
__device__ __forceinline__ uint32_t chain_copy(__amdgpu_buffer_rsrc_t rs, const SegTable& S,
                                               uint32_t n_segs, __amdgpu_buffer_rsrc_t ro,
                                               ChainCursor& c, uint32_t pos, uint32_t d,
                                               uint32_t len, int lane) {
    uint32_t acc = 0;
    while (len != 0u && c.k < n_segs) {
        const Frame s = S.seg(c.k);
        const uint32_t in = pos - c.cum;
        if (in >= s.len) {                                        // pos is past this segment
            c.cum += s.len;
            ++c.k;
            continue;
        }
        const uint32_t take = s.len - in < len ? s.len - in : len;
        acc += wave_copy<SUM>(rs, S.fb, ro, s.off + in, d, take, lane);
        pos += take;
        d += take;
        len -= take;
    }
    return acc;
}

}  // namespace
