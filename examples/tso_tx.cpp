// tso_tx.cpp — rpkt-dpdk/examples/tso_tx.rs through the C ABI only (include/rpkt_gpu.h).
// The reference builds one Ether/IPv4/TCP frame around a 4000-byte payload of 0xae
// (tso_tx.rs:36-78), asks the port for the IP_CKSUM, TCP_CKSUM and TCP_SEG offloads with
// set_tso_segsz(1024) (:128-134) and sends it: the NIC cuts it into four TCP segments.  Here
// the frame stays in HBM: rpkt_gpu_build_batch writes the same headers from a record,
// rpkt_gpu_segment_batch cuts the frame at mss 1024, and a parse of the output with both
// sums plays the receiving port's RX checksum offload.
//   hipcc -O2 -Iinclude examples/tso_tx.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/tso_tx && ./examples/tso_tx
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

int main() {
    const uint32_t hdr = 14 + 20 + 20, payload = 4000, mss = 1024, out_cap = 8;
    const uint64_t out_bytes = 8192;
    std::vector<uint8_t> host(hdr + payload + 16, 0);
    memset(host.data() + hdr, 0xae, payload);                     // PAYLOAD_BYTE x PAYLOAD_LEN

    // the header values of tso_tx.rs:36-75, as the record rpkt_gpu_build_batch builds from
    rpkt_rec_t r;
    memset(&r, 0, sizeof(r));
    const uint8_t dmac[6] = {0xac, 0xdc, 0xca, 0x79, 0xe5, 0xc6};
    const uint8_t smac[6] = {0xac, 0xdc, 0xca, 0x79, 0xca, 0x86};
    memcpy(r.dst_addr, dmac, 6);
    memcpy(r.src_addr, smac, 6);
    r.ethertype = 0x0800;
    r.ip_vhl = 0x45;
    r.ip_ttl = 128;
    r.ip_protocol = 6;
    r.ip_src = (172u << 24) | (0u << 16) | (10u << 8) | 17u;
    r.ip_dst = (192u << 24) | (168u << 16) | (23u << 8) | 2u;
    r.src_port = 60376;
    r.dst_port = 161;
    r.tcp_seq = 0x8e501902u;
    r.tcp_ack = 0xc7529d89u;
    r.l4_word6 = 0x5000 | 0x10 | 0x08;                            // header_len 20, ACK, PSH
    r.tcp_window = 46;

    uint8_t *frames = nullptr, *out = nullptr, *built = nullptr;
    rpkt_rec_t *rec_build = nullptr, *recs = nullptr, *out_recs = nullptr;
    uint32_t *out_offsets = nullptr, *seg_first = nullptr;
    uint64_t* totals = nullptr;
    void* ws = nullptr;
    HIP_OK(hipMalloc(&frames, host.size()));
    HIP_OK(hipMalloc(&out, out_bytes));
    HIP_OK(hipMalloc(&built, 16));
    HIP_OK(hipMalloc(&rec_build, sizeof(r)));
    HIP_OK(hipMalloc(&recs, sizeof(r)));
    HIP_OK(hipMalloc(&out_recs, out_cap * sizeof(r)));
    HIP_OK(hipMalloc(&out_offsets, (out_cap + 1) * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&seg_first, 2 * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&totals, 2 * sizeof(uint64_t)));
    HIP_OK(hipMalloc(&ws, rpkt_gpu_segment_workspace_bytes(1) + 16));
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(rec_build, &r, sizeof(r), hipMemcpyHostToDevice));

    // build (both checksum offloads), parse, segment, parse the output: one stream, no host step
    const rpkt_batch_t b = {frames, host.size(), nullptr, hdr + payload, 0, 1, 0};
    int rc = rpkt_gpu_build_batch(&b, rec_build, RPKT_BUILD_IP_CSUM | RPKT_BUILD_L4_CSUM, built,
                                  nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_parse_batch(&b, RPKT_F_IP_SUM | RPKT_F_L4_SUM, recs, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_segment_batch(&b, recs, mss, 0, out, out_bytes, out_offsets, out_cap, seg_first,
                                    totals, ws, nullptr);
    const rpkt_batch_t ob = {out, out_bytes, out_offsets, 0, 0, out_cap, 0};
    if (rc == RPKT_OK)
        rc = rpkt_gpu_parse_batch(&ob, RPKT_F_IP_SUM | RPKT_F_L4_SUM, out_recs, nullptr, 0, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }

    rpkt_rec_t in, seg[8];
    uint64_t tot[2];
    uint32_t first[2], offs[9];
    HIP_OK(hipMemcpy(&in, recs, sizeof(in), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(seg, out_recs, sizeof(seg), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first, seg_first, sizeof(first), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs, out_offsets, sizeof(offs), hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    printf("in : %s len=%u payload=%u seq=0x%08x flags=0x%02x ip_sum=0x%04x l4_sum=0x%04x\n",
           rpkt_gpu_status_name(in.status), in.frame_len, in.payload_len, in.tcp_seq,
           in.l4_word6 & 0xff, in.ip_sum, in.l4_sum);
    printf("out: %llu frames, %llu bytes; frame 0 -> outputs [%u, %u)\n",
           (unsigned long long)tot[0], (unsigned long long)tot[1], first[0], first[1]);
    const uint32_t want[4] = {1024, 1024, 1024, 928};
    bool ok = in.status == RPKT_S_OK && in.ip_sum == 0xffff && in.l4_sum == 0xffff &&
              in.payload_len == payload && tot[0] == 4 && tot[1] == payload + 4 * hdr &&
              first[0] == 0 && first[1] == 4 && offs[0] == 0;
    for (uint32_t k = 0; k < out_cap; k++) {
        const rpkt_rec_t& s = seg[k];
        if (k >= 4) {                                             // the spare slots: empty frames
            ok = ok && s.frame_len == 0 && offs[k + 1] == tot[1];
            continue;
        }
        printf("  %u: %s len=%u payload=%u ident=%u seq=0x%08x flags=0x%02x ip_sum=0x%04x "
               "l4_sum=0x%04x\n", k, rpkt_gpu_status_name(s.status), s.frame_len, s.payload_len,
               s.ip_ident, s.tcp_seq, s.l4_word6 & 0xff, s.ip_sum, s.l4_sum);
        ok = ok && s.status == RPKT_S_OK && s.payload_len == want[k] &&
             s.frame_len == hdr + want[k] && s.tcp_seq == r.tcp_seq + k * mss && s.ip_ident == k &&
             ((s.l4_word6 & 0x08) != 0) == (k == 3) && (s.l4_word6 & 0x10) != 0 &&
             s.ip_sum == 0xffff && s.l4_sum == 0xffff && s.src_port == 60376 && s.dst_port == 161;
    }
    printf("%s\n", ok ? "ok: 4 segments, sums valid" : "MISMATCH");
    (void)hipFree(frames); (void)hipFree(out); (void)hipFree(built); (void)hipFree(rec_build);
    (void)hipFree(recs); (void)hipFree(out_recs); (void)hipFree(out_offsets); (void)hipFree(seg_first);
    (void)hipFree(totals); (void)hipFree(ws);
    return ok ? 0 : 1;
}
