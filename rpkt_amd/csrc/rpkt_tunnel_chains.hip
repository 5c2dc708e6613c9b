// rpkt_tunnel_chains.hip — rpkt_gpu_parse_tunnel_chains: rpkt_gpu_parse_tunnel_batch's
// work (the outer parse, one VXLAN / GTP-U / GRE level, the parse of the inner frame, every
// sum of both levels) over mbuf chains, rpkt-dpdk's Pbuf (include/rpkt_gpu.h documents the
// records; tests/tunnel_chain_model.py restates the chunk()/remaining() rules on the CPU).
//
// One wavefront per 64 chains, as parse_chains_kernel: segment 0's 128-B window goes to LDS
// and each lane runs parse_chain_lane on its chain.  The lane then decodes the tunnel and
// parses the inner frame with logical cursors in the chain's bytes: every header-size test
// takes chunk() at the header's cursor under the current packet end (ChainView, rpkt_chain.h:
// the rest of segment 0 below its end, chain_chunk's segment walk past it), every
// total-length test takes remaining(), and header bytes come through ChainDw (LDS when they lie in
// segment 0's window, byte-wise global loads otherwise -- a header that starts past the
// window or in a later segment; there is no second inner window).  The outer record is
// staged in an LDS area of its own, the inner one in the window area, so chain_stream keeps
// its scratch.  One chain_stream pass sums the bytes the inner L4 range and the outer L4
// range (UDP, or GRE with its checksum) share; the outer range's bytes before the inner
// stream (inner headers past the window) and after the inner packet (padding, GTP trailing
// bytes) get a pass each, which returns at once when no lane of the wave has such bytes.
#include "rpkt_common.h"
#include "rpkt_args.h"
#include "rpkt_chain.h"
#include "rpkt_tunnel.h"

namespace {

// Big-endian sum of the n <= chunk bytes of a header at absolute `ab`: from segment 0's
// window when they lie in it, else byte-wise (gsum_be).
__device__ __forceinline__ uint32_t header_sum(const ChainDw& dw, uint32_t ab, uint32_t n) {
    const uint32_t x = ab - dw.off0;
    if (x < dw.lim && dw.lim - x >= n)
        return be_sum(slot_range_sum(dw.slot, dw.ph + x, dw.ph + x + n), ab);
    return gsum_be(dw.rs, ab, n);
}

// parse_chain_lane for the inner frame: the sub-chain [T.is, T.ie) of the lane's chain,
// started at its Ethernet header (T.start_et 0) or at its IP header (GTP-U, GRE over IP:
// MACs 0, no tags, ethertype = the tunnel's dispatch value).  Cursors and the record's
// offsets are logical positions in the outer chain; frame_len is the sub-chain's length.
// The rules are the shared ones (parse_ip6, ip4_rules, l4_rules); what is here is the link
// layer and the cursors, every header read through the view: parse_chain_lane's own rounds
// are built on segment 0's window at cursor 0 (bulk LDS reads, raw_range_sum on them), and
// an inner frame starts anywhere in the chain.
__device__ __forceinline__ void parse_inner_lane(const ChainView& V, const Tunnel& T,
                                                 uint32_t flags, LaneRec& L) {
    uint32_t* w = L.w;
#pragma unroll
    for (int k = 0; k < 20; ++k) w[k] = 0;
    L.stream_s = L.stream_e = L.l4_part = L.l4_start_abs = L.pseudo = 0;
    L.want_l4 = false;
    L.is6 = false;
    const uint32_t pkt = T.ie;
    w[19] = T.ie - T.is;
    uint32_t status = RPKT_S_OK, et = T.start_et, c = T.is, ab;
    if (T.start_et == 0u) {
        if (V.chunk(c, pkt, ab) < 14u) {                       // ether/generated.rs:36
            L.status = RPKT_S_ETH_SHORT;
            w[0] = RPKT_S_ETH_SHORT;
            return;
        }
        w[1] = V.dw(ab);
        w[2] = V.dw(ab + 4u);
        w[3] = V.dw(ab + 8u);
        const uint32_t eth_et = be16_lo(V.dw(ab + 12u));
        uint32_t nvlan = 0;
        et = eth_et;
        c += 14u;
        for (int v = 0; v < RPKT_MAX_VLAN; ++v) {              // vlan/generated.rs:32-61
            if (!is_tag(et)) break;
            if (V.chunk(c, pkt, ab) < 4u) {
                status = RPKT_S_VLAN_SHORT;
                break;
            }
            const uint32_t t = V.dw(ab);
            et = be16_hi(t);
            w[4] |= be16_lo(t) << (16 * v);
            w[5] |= et << (16 * v);
            nvlan += 1;
            c += 4u;
        }
        w[0] = (nvlan << 8) | (eth_et << 16);
    } else {
        w[0] = T.start_et << 16;                               // the tunnel's dispatch value
    }
    const bool v6 = (flags & RPKT_F_IPV6) && status == RPKT_S_OK && et == 0x86ddu;
    if (status == RPKT_S_OK && et != 0x0800u && !v6) status = RPKT_S_NOT_IPV4;
    if (status != RPKT_S_OK) {
        w[0] |= status;
        L.status = status;
        return;
    }

    const uint32_t l3 = c;
    w[16] = l3 & 0xffffu;
    uint32_t l4, limit, l4rem, proto, paddr;
    if (v6) {
        L.is6 = true;
        status = parse_ip6(V, l3, pkt, w, l4, l4rem, proto, paddr);
        if (status != RPKT_S_IP6_SHORT && status != RPKT_S_IP6_BAD_LEN) {
            w[16] |= l4 << 16;
            w[17] = (l4 & 0xffffu) | (l4rem << 16);
        }
        if (status != RPKT_S_OK) {
            w[0] |= status;
            L.status = status;
            return;
        }
        limit = l4 + l4rem;
    } else {
        const uint32_t ck3 = V.chunk(l3, pkt, ab);
        uint32_t F[5] = {0u, 0u, 0u, 0u, 0u};
        if (ck3 >= 20u) V.read_words(ab, F);
        const Ip4Out o = ip4_rules(F, ck3, pkt - l3, w);
        status = o.status;
        if (status != RPKT_S_OK) {
            w[0] |= status;
            L.status = status;
            return;
        }
        if (flags & RPKT_F_IP_SUM) w[18] = header_sum(V.d, ab, o.ihl4);
        l4 = l3 + o.ihl4;                                      // Ipv4::payload :115-127
        limit = l3 + o.tot;
        l4rem = o.tot - o.ihl4;
        w[16] |= l4 << 16;
        w[17] = (l4 & 0xffffu) | (l4rem << 16);
        proto = o.proto;
        paddr = o.paddr;
    }

    // the L4 header against the chunk at l4 under the trimmed end
    uint32_t ab4, H[5];
    const uint32_t ck4 = V.chunk(l4, limit, ab4);
    V.read_words(ab4, H);
    const L4Out r4 = l4_rules(H, ck4, l4rem, proto, v6, l4, w);
    status = r4.status;
    const uint32_t l4len = r4.l4len;
    const bool other_sum = r4.other_sum;                       // ICMP / GRE
    w[0] |= status;
    L.status = status;
    if ((status == RPKT_S_OK || other_sum) && (flags & RPKT_F_L4_SUM)) {
        const ChainDw& dw = V.d;
        L.want_l4 = true;
        L.pseudo = other_sum ? 0u : paddr + proto + l4len;
        const uint32_t e = l4 + l4len;
        L.l4_start_abs = dw.off0 + l4;                         // segment 0's byte phase
        // the part of [l4, e) segment 0's window holds (logical bytes [0, dw.lim))
        const uint32_t e_in = l4 < dw.lim ? (e < dw.lim ? e : dw.lim) : l4;
        L.l4_part = slot_range_sum(dw.slot, dw.ph + l4, dw.ph + e_in);
        L.stream_s = e_in;
        L.stream_e = e;                                        // logical, not absolute
    }
}

// WaveScratch (the window, then the inner records' stage and chain_stream's scratch past
// it) and a stage of its own for the outer records, which wait for the stream's sum too
struct TunChainScratch {
    WaveScratch W;
    uint32_t outer[kWave * 21];
};

// One wave per workgroup, as tunnel_kernel; registers, not waves, are the budget of the
// chain stream (parse_chains_kernel): 2 waves per SIMD, 15 KB of LDS per wave
template <bool L4>
__global__ __launch_bounds__(kWave, 2)
void tunnel_chains_kernel(const uint8_t* __restrict__ buf, uint32_t fb,
                          const uint2* __restrict__ segs, uint32_t n_segs,
                          const uint32_t* __restrict__ chain_first, uint32_t n, uint32_t flags,
                          rpkt_rec_t* __restrict__ outer, rpkt_tun_t* __restrict__ tun,
                          rpkt_rec_t* __restrict__ inner, uint64_t* __restrict__ flow_ev,
                          uint32_t n_buckets) {
    __shared__ __attribute__((aligned(16))) TunChainScratch scratch;
    WaveScratch& W = scratch.W;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t p0 = blockIdx.x * kWave;
    if (p0 >= n) return;                                          // wave-uniform exit
    const uint32_t i = p0 + lane;
    const bool valid = i < n;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(buf, fb);
    const ChainSrc S{segs, fb};

    // chain bounds, segment 0 and pkt_len, as parse_chains_kernel
    uint32_t a = 0, b = 0;
    if (valid) {
        const uint32_t f0 = chain_first[i], f1 = chain_first[i + 1];
        a = f0 < n_segs ? f0 : n_segs;
        b = f1 > a ? f1 : a;
        b = b < n_segs ? b : n_segs;
    }
    Frame s0{0, 0};
    uint32_t pkt = 0;
    for (uint32_t k = a; k < b; ++k) {
        const Frame s = S.seg(k);
        if (k == a) s0 = s;
        pkt = pkt + s.len < pkt ? 0xffffffffu : pkt + s.len;
    }

    // 1. segment 0's header window -> LDS, the outer parse; the outer record to its stage
    {
        u32x4 d[kWinChunks];
        uint32_t addr[kWinChunks];
        const uint32_t fix = window_issue(rs, fb, s0, lane, d, addr);
        window_commit(W, rs, fb, d, addr, fix, lane);
    }
    wave_sync();
    LaneRec L;
    parse_chain_lane(W, lane, s0, pkt, S, a, b, rs, flags, L);
    uint32_t* ost = scratch.outer + lane * 21;
#pragma unroll
    for (int k = 0; k < 20; ++k) ost[k] = L.w[k];
    [[maybe_unused]] const uint32_t o_ss = L.stream_s, o_se = L.stream_e, o_part = L.l4_part;
    [[maybe_unused]] const uint32_t o_abs = L.l4_start_abs, o_pseudo = L.pseudo;
    [[maybe_unused]] const bool o_want = L.want_l4;

    // 2. the tunnel and the inner frame, from the same window (byte-wise past it)
    const ChainView V = chain_view(W, lane, s0, S, a, b, rs);
    const Tunnel T = decode_tunnel(L, V, flags);
    if (T.ok) parse_inner_lane(V, T, flags, L);
    else no_inner(L);
    stage_record(W, lane, L.w);

    // 3. L4 bytes past the window: the inner range (the outer one when there is no inner
    //    sum), which the outer range contains, then the outer range's other bytes
    if constexpr (L4) {
        const bool both = L.want_l4 && o_want;
        const uint32_t i_ss = L.stream_s, i_se = L.stream_e;
        const uint32_t ms = L.want_l4 ? i_ss : (o_want ? o_ss : 0u);
        const uint32_t me = L.want_l4 ? i_se : (o_want ? o_se : 0u);
        const uint32_t sp_m = chain_stream(W, rs, fb, S, a, b, s0.off, ms, me, lane);
        // outer [o_ss, o_se) = [o_ss, i_ss) + the inner stream + [i_se, o_se); an inner
        // range that ends inside the window has no stream and leaves the outer one whole
        const uint32_t pre_e = i_ss > o_ss ? i_ss : o_ss, tail_s = i_se > o_ss ? i_se : o_ss;
        uint32_t sp_o = sp_m;
        sp_o += chain_stream(W, rs, fb, S, a, b, s0.off, both ? o_ss : 0u, both ? pre_e : 0u, lane);
        sp_o += chain_stream(W, rs, fb, S, a, b, s0.off, both ? tail_s : 0u, both ? o_se : 0u, lane);
        if (L.want_l4)
            rec_stage(W)[lane * 21 + 18] |=
                fold16(L.pseudo + be_sum(L.l4_part + sp_m, L.l4_start_abs)) << 16;
        if (o_want) ost[18] |= fold16(o_pseudo + be_sum(o_part + sp_o, o_abs)) << 16;
    }

    // 4. the flow event (the inner record's when the tunnel decoded, else the outer's), the
    //    records (1-KiB wave stores), the tunnel record (16 B per lane)
    if ((flags & RPKT_F_FLOW_EV) && valid) {
        const uint32_t* rw = T.ok ? rec_stage(W) + lane * 21 : ost;
        __builtin_nontemporal_store(record_event(rw, n_buckets), &flow_ev[i]);
    }
    flush_stage(rec_stage(W), lane, inner, p0, n);
    flush_stage(scratch.outer, lane, outer, p0, n);
    if (valid) store_tun(tun, i, T);
}

}  // namespace

extern "C" {

int rpkt_gpu_parse_tunnel_chains(const rpkt_chains_t* c, uint32_t flags, rpkt_rec_t* outer_dev,
                                 rpkt_tun_t* tun_dev, rpkt_rec_t* inner_dev,
                                 rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream) {
    if (!c) return RPKT_E_INVAL;
    RPKT_TRY(flags_ok(flags, kRxFlags));
    if (c->n_chains == 0) return RPKT_OK;
    if (any_null(outer_dev, tun_dev, inner_dev)) return RPKT_E_INVAL;
    RPKT_TRY(chains_ok(*c));
    if (misaligned(15, outer_dev, tun_dev, inner_dev) || misaligned(7, c->segs_dev))
        return RPKT_E_ALIGN;
    RPKT_TRY(events_ok(flags, flow_ev_dev, n_buckets));
    const uint32_t grid = (c->n_chains + kWave - 1) / kWave;
    auto k = (flags & RPKT_F_L4_SUM) ? tunnel_chains_kernel<true> : tunnel_chains_kernel<false>;
    return launch(k, dim3(grid), dim3(kWave), 0, (hipStream_t)stream, c->buf_dev,
                  (uint32_t)c->buf_bytes, (const uint2*)c->segs_dev, c->n_segs,
                  c->chain_first_dev, c->n_chains, flags, outer_dev, tun_dev, inner_dev,
                  (uint64_t*)flow_ev_dev, n_buckets);
}

}  // extern "C"
