// frag_tx_chains.cpp — an over-MTU datagram as the mbuf chain a DPDK port holds it in, cut into
// IP fragments without leaving the device, through the C ABI only (include/rpkt_gpu.h).
// rpkt-dpdk/examples/jumboframe_tx.rs sends 8000-byte frames; with 2048-byte data rooms
// (Mbuf::from_slice, rpkt-dpdk/src/mbuf.rs:261-312) such a frame is a chain of four segments,
// each at byte 128 (the headroom) of its own mempool slot.  A link with an MTU of 1500 wants
// that UDP/IPv4 datagram (DF clear) as six fragments.  The chain stays in HBM:
// rpkt_gpu_parse_chains locates the headers, rpkt_gpu_fragment_chains cuts the chain at 1500
// into flat wire frames, rpkt_gpu_parse_batch of the output with the IP sum plays the receiving
// port's checksum offload, and rpkt_gpu_reassemble_batch plays the receiver: the frame it gives
// back must be the chain's bytes.
//   hipcc -O2 -Iinclude examples/frag_tx_chains.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/frag_tx_chains && ./examples/frag_tx_chains
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rpkt_gpu.h"

#define HIP_OK(call)                                              \
    do {                                                          \
        if ((call) != hipSuccess) {                               \
            fprintf(stderr, "%s failed\n", #call);                \
            return 2;                                             \
        }                                                         \
    } while (0)
#define RPKT_OK_OR_FAIL(call)                                                                  \
    do {                                                                                       \
        const int rc_ = (call);                                                                \
        if (rc_ != RPKT_OK) {                                                                  \
            fprintf(stderr, "%s failed rc=%d hip=%d\n", #call, rc_, rpkt_gpu_last_hip_error()); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

template <class T>
static bool dev_alloc(T** p, size_t bytes) {
    return hipMalloc((void**)p, bytes ? bytes : 16) == hipSuccess;
}

static void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }

// the RFC 1071 checksum field of [p, p + n), n even
static uint32_t csum(const uint8_t* p, uint32_t n, uint32_t acc = 0) {
    for (uint32_t k = 0; k + 1 < n; k += 2) acc += ((uint32_t)p[k] << 8) | p[k + 1];
    while (acc >> 16) acc = (acc & 0xffff) + (acc >> 16);
    return ~acc & 0xffff;
}

int main() {
    const uint32_t flen = 8000, hdr = 14 + 20, mtu = 1500;        // the frame: an IP packet of 7986
    const uint32_t P = flen - hdr, c = (mtu - 20) & ~7u, nf = (P + c - 1) / c;   // 7966, 1480, 6
    const uint32_t head_room = 128, data_room = 2048, slot = head_room + data_room;
    const uint32_t n_segs = (flen + data_room - 1) / data_room;   // 4
    const uint32_t out_cap = 8;
    const uint64_t out_bytes = P + nf * hdr + 64;

    // the frame: Ether / IPv4 (DF clear) / UDP with both sums filled / a counting payload
    std::vector<uint8_t> frame(flen, 0);
    uint8_t* h = frame.data();
    const uint8_t dmac[6] = {0xac, 0xdc, 0xca, 0x79, 0xe5, 0xc6};
    const uint8_t smac[6] = {0xac, 0xdc, 0xca, 0x79, 0xca, 0x86};
    memcpy(h, dmac, 6);
    memcpy(h + 6, smac, 6);
    put16(h + 12, 0x0800);
    uint8_t* ip = h + 14;
    ip[0] = 0x45;
    put16(ip + 2, flen - 14);
    put16(ip + 4, 0x2bad);
    ip[8] = 64;
    ip[9] = 17;
    const uint8_t sip[4] = {172, 0, 10, 17}, dip[4] = {192, 168, 23, 2};
    memcpy(ip + 12, sip, 4);
    memcpy(ip + 16, dip, 4);
    put16(ip + 10, csum(ip, 20));
    uint8_t* udp = ip + 20;
    put16(udp, 60376);
    put16(udp + 2, 9000);
    put16(udp + 4, P);
    for (uint32_t k = 8; k < P; k++) udp[k] = (uint8_t)(k * 7 + (k >> 8));
    uint32_t pseudo = 17 + P;
    for (uint32_t k = 12; k < 20; k += 2) pseudo += ((uint32_t)ip[k] << 8) | ip[k + 1];
    put16(udp + 6, csum(udp, P, pseudo));

    // four mempool slots, handed out last first; every segment starts after its slot's headroom
    std::vector<uint8_t> arena(n_segs * slot + 16, 0x11);
    std::vector<uint32_t> segs_host(2 * n_segs);
    for (uint32_t k = 0; k < n_segs; k++) {
        const uint32_t at = (n_segs - 1 - k) * slot + head_room, from = k * data_room;
        const uint32_t len = flen - from < data_room ? flen - from : data_room;
        memcpy(arena.data() + at, frame.data() + from, len);
        segs_host[2 * k] = at;
        segs_host[2 * k + 1] = len;
    }
    const uint32_t first_host[2] = {0, n_segs};

    uint8_t *buf = nullptr, *frags = nullptr, *out = nullptr;
    uint32_t *segs = nullptr, *chain_first = nullptr, *frag_offsets = nullptr, *frag_first = nullptr;
    uint32_t *out_offsets = nullptr, *src_first = nullptr;
    rpkt_rec_t *recs = nullptr, *f_recs = nullptr;
    uint64_t *totals = nullptr, *r_totals = nullptr;
    void *ws = nullptr, *ws_re = nullptr;
    const size_t rb = sizeof(rpkt_rec_t);
    if (!(dev_alloc(&buf, arena.size()) && dev_alloc(&frags, out_bytes) && dev_alloc(&out, out_bytes) &&
          dev_alloc(&segs, segs_host.size() * 4) && dev_alloc(&chain_first, sizeof(first_host)) &&
          dev_alloc(&frag_offsets, (out_cap + 1) * 4) && dev_alloc(&frag_first, 2 * 4) &&
          dev_alloc(&out_offsets, (out_cap + 1) * 4) && dev_alloc(&src_first, (out_cap + 1) * 4) &&
          dev_alloc(&recs, rb) && dev_alloc(&f_recs, out_cap * rb) && dev_alloc(&totals, 16) &&
          dev_alloc(&r_totals, 16) && dev_alloc(&ws, rpkt_gpu_fragment_chains_workspace_bytes(1)) &&
          dev_alloc(&ws_re, rpkt_gpu_reassemble_workspace_bytes(out_cap)))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(buf, arena.data(), arena.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(segs, segs_host.data(), segs_host.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(chain_first, first_host, sizeof(first_host), hipMemcpyHostToDevice));

    // parse the chain, fragment it, parse the flat output, reassemble: one stream, no host step
    const rpkt_chains_t ch = {buf, arena.size(), segs, chain_first, n_segs, 1};
    const rpkt_batch_t fb = {frags, out_bytes, frag_offsets, 0, 0, out_cap, 0};
    RPKT_OK_OR_FAIL(rpkt_gpu_parse_chains(&ch, 0, recs, nullptr, 0, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_fragment_chains(&ch, recs, mtu, 0, 0, frags, out_bytes, frag_offsets,
                                             out_cap, frag_first, totals, ws, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_parse_batch(&fb, RPKT_F_IP_SUM, f_recs, nullptr, 0, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_reassemble_batch(&fb, f_recs, nullptr, 0, out, out_bytes, out_offsets,
                                              out_cap, src_first, r_totals, ws_re, nullptr));
    HIP_OK(hipDeviceSynchronize());

    rpkt_rec_t in, fr[8];
    uint64_t tot[2], rtot[2];
    uint32_t first[2], offs[9], roffs[9];
    std::vector<uint8_t> wire(out_bytes), back(out_bytes);
    HIP_OK(hipMemcpy(&in, recs, sizeof(in), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(fr, f_recs, sizeof(fr), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rtot, r_totals, sizeof(rtot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first, frag_first, sizeof(first), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs, frag_offsets, sizeof(offs), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(roffs, out_offsets, sizeof(roffs), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(wire.data(), frags, out_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(back.data(), out, out_bytes, hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    printf("in : %s pkt_len=%u in %u segments of up to %u, ip_packet_len=%u frag=0x%04x\n",
           rpkt_gpu_status_name(in.status), in.frame_len, n_segs, data_room, in.ip_packet_len,
           in.ip_frag);
    printf("out: %llu frames, %llu bytes; chain 0 -> outputs [%u, %u)\n",
           (unsigned long long)tot[0], (unsigned long long)tot[1], first[0], first[1]);
    bool ok = in.status == RPKT_S_OK && in.frame_len == flen && in.ip_packet_len == flen - 14 &&
              tot[0] == nf && tot[1] == P + nf * hdr && first[0] == 0 && first[1] == nf && offs[0] == 0;
    for (uint32_t k = 0; k < out_cap && ok; k++) {
        const rpkt_rec_t& s = fr[k];
        if (k >= nf) {                                            // the spare slots: empty frames
            ok = ok && s.frame_len == 0 && offs[k + 1] == tot[1];
            continue;
        }
        const uint32_t pk = k + 1 < nf ? c : P - k * c;
        const uint32_t want_fw = (k * c / 8) | (k + 1 < nf ? 0x2000u : 0u);
        printf("  %u: %s len=%u frag=0x%04x ident=0x%04x ip_sum=0x%04x\n", k,
               rpkt_gpu_status_name(s.status), s.frame_len, s.ip_frag, s.ip_ident, s.ip_sum);
        // offsets and MF run in order, every header sum is valid, the slice is the chain's
        ok = ok && s.frame_len == hdr + pk && offs[k + 1] - offs[k] == hdr + pk &&
             s.ip_packet_len == 20 + pk && s.ip_frag == want_fw && s.ip_ident == 0x2bad &&
             s.ip_sum == 0xffff && s.ip_protocol == 17 &&
             memcmp(wire.data() + offs[k] + hdr, frame.data() + hdr + k * c, pk) == 0;
    }
    printf("reassembled: %llu frame(s), %llu bytes\n", (unsigned long long)rtot[0],
           (unsigned long long)rtot[1]);
    ok = ok && rtot[0] == out_cap - nf + 1 && rtot[1] == flen && roffs[0] == 0 && roffs[1] == flen &&
         memcmp(back.data(), frame.data(), flen) == 0;
    printf("%s\n", ok ? "ok: 6 fragments from a 4-segment chain, header sums valid, reassembled"
                      : "MISMATCH");
    (void)hipFree(buf); (void)hipFree(frags); (void)hipFree(out); (void)hipFree(segs);
    (void)hipFree(chain_first); (void)hipFree(frag_offsets); (void)hipFree(frag_first);
    (void)hipFree(out_offsets); (void)hipFree(src_first); (void)hipFree(recs); (void)hipFree(f_recs);
    (void)hipFree(totals); (void)hipFree(r_totals); (void)hipFree(ws); (void)hipFree(ws_re);
    return ok ? 0 : 1;
}
