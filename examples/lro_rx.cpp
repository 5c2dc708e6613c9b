// lro_rx.cpp — rpkt-dpdk/examples/lro_rx.rs through the C ABI only (include/rpkt_gpu.h).
// The reference turns on the port's LRO offload (rx_offloads bit 4, with scatter) and prints,
// for each COALESCED TCP frame, its ports, seq_num, ack_num, the ACK / PSH flags, window_size,
// payload length and checksum (lro_rx.rs:81-99).  Here the frames stay in HBM.  A few TCP
// streams are built (rpkt_gpu_build_batch), cut into wire segments on the device
// (rpkt_gpu_segment_batch) and interleaved round robin as a shared wire would deliver them;
// then the receive side: parse with flow events, order the burst by flow bucket, coalesce
// (rpkt_gpu_coalesce_batch) and parse again.  Exits non-zero unless every stream came back
// whole with valid sums.
//   hipcc -O2 -Iinclude examples/lro_rx.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/lro_rx && ./examples/lro_rx
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "rpkt_gpu.h"

#define HIP_OK(call)                                              \
    do {                                                          \
        if ((call) != hipSuccess) {                               \
            fprintf(stderr, "%s failed\n", #call);                \
            return 2;                                             \
        }                                                         \
    } while (0)

template <typename T>
static T* dev_alloc(size_t count) {
    void* p = nullptr;
    return hipMalloc(&p, count * sizeof(T) + 16) == hipSuccess ? static_cast<T*>(p) : nullptr;
}

int main() {
    const uint32_t S = 3, hdr = 14 + 20 + 20, payload = 8000, mss = 1448, n_buckets = 4096;
    const uint32_t stride = hdr + payload, per = (payload + mss - 1) / mss, n_seg = S * per;
    const uint32_t F = RPKT_F_IP_SUM | RPKT_F_L4_SUM;

    // the streams: one super-frame each, payload bytes that tell the streams apart
    std::vector<uint8_t> host(S * stride + 16, 0);
    std::vector<rpkt_rec_t> build(S);
    for (uint32_t s = 0; s < S; s++) {
        for (uint32_t k = 0; k < payload; k++) host[s * stride + hdr + k] = (uint8_t)(k * 7 + s * 31 + (k >> 8));
        rpkt_rec_t& r = build[s];
        memset(&r, 0, sizeof(r));
        const uint8_t dmac[6] = {0xac, 0xdc, 0xca, 0x79, 0xe5, 0xc6};
        const uint8_t smac[6] = {0xac, 0xdc, 0xca, 0x79, 0xca, 0x86};
        memcpy(r.dst_addr, dmac, 6);
        memcpy(r.src_addr, smac, 6);
        r.ethertype = 0x0800;
        r.ip_vhl = 0x45;
        r.ip_ttl = 64;
        r.ip_protocol = 6;
        r.ip_ident = (uint16_t)(1000 * s + 65530);                // stream 0 wraps
        r.ip_src = (192u << 24) | (168u << 16) | (22u << 8) | 2u;
        r.ip_dst = (192u << 24) | (168u << 16) | (23u << 8) | 2u;
        r.src_port = (uint16_t)(40000 + 11 * s);
        r.dst_port = 9000;
        r.tcp_seq = 0xfffff000u + 0x01000000u * s;                // stream 0 wraps
        r.tcp_ack = 0x00c0ffeeu + s;
        r.l4_word6 = 0x5000 | 0x10 | 0x08;                        // header_len 20, ACK, PSH
        r.tcp_window = (uint16_t)(512 + s);
    }

    uint8_t* frames = dev_alloc<uint8_t>(host.size());
    uint8_t* wire = dev_alloc<uint8_t>(n_seg * (hdr + mss));
    uint8_t* rx = dev_alloc<uint8_t>(n_seg * (hdr + mss));
    uint8_t* merged = dev_alloc<uint8_t>(n_seg * (hdr + mss));
    rpkt_rec_t* recs = dev_alloc<rpkt_rec_t>(n_seg);
    rpkt_rec_t* rec_build = dev_alloc<rpkt_rec_t>(S);
    uint32_t* offs = dev_alloc<uint32_t>(n_seg + 1);
    uint32_t* first = dev_alloc<uint32_t>(n_seg + 1);
    uint32_t* order = dev_alloc<uint32_t>(n_seg);
    uint16_t* gso = dev_alloc<uint16_t>(n_seg);
    uint64_t* totals = dev_alloc<uint64_t>(2);
    rpkt_flow_ev_t* ev = dev_alloc<rpkt_flow_ev_t>(n_seg);
    const size_t ws_bytes = std::max(rpkt_gpu_segment_workspace_bytes(S), rpkt_gpu_coalesce_workspace_bytes(n_seg));
    uint8_t* ws = dev_alloc<uint8_t>(ws_bytes);
    if (!frames || !wire || !rx || !merged || !recs || !rec_build || !offs || !first || !order || !gso ||
        !totals || !ev || !ws) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(rec_build, build.data(), S * sizeof(rpkt_rec_t), hipMemcpyHostToDevice));

    // the sender: build, parse, segment as the port's TSO would
    const rpkt_batch_t tx = {frames, host.size(), nullptr, stride, 0, S, 0};
    int rc = rpkt_gpu_build_batch(&tx, rec_build, RPKT_BUILD_IP_CSUM | RPKT_BUILD_L4_CSUM, nullptr, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_parse_batch(&tx, F, recs, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_segment_batch(&tx, recs, mss, 0, wire, n_seg * (hdr + mss), offs, n_seg, first,
                                    totals, ws, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "tx failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }
    uint64_t tot[2];
    std::vector<uint32_t> woffs(n_seg + 1);
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(woffs.data(), offs, (n_seg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (tot[0] != n_seg) {
        fprintf(stderr, "%llu segments, want %u\n", (unsigned long long)tot[0], n_seg);
        return 1;
    }

    // the wire: segment k of every stream in turn (device copies; the offsets on the host)
    std::vector<uint32_t> roffs(n_seg + 1, 0);
    for (uint32_t k = 0, at = 0; k < per; k++)
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t j = s * per + k, len = woffs[j + 1] - woffs[j];
            HIP_OK(hipMemcpy(rx + at, wire + woffs[j], len, hipMemcpyDeviceToDevice));
            at += len;
            roffs[k * S + s + 1] = at;
        }
    HIP_OK(hipMemcpy(offs, roffs.data(), (n_seg + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));

    // the receiver: parse with flow events, order by bucket (stable), coalesce, parse again
    const rpkt_batch_t rb = {rx, tot[1], offs, 0, 0, n_seg, 0};
    rc = rpkt_gpu_parse_batch(&rb, F | RPKT_F_FLOW_EV, recs, ev, n_buckets, nullptr);
    std::vector<rpkt_flow_ev_t> hev(n_seg);
    if (rc == RPKT_OK) HIP_OK(hipMemcpy(hev.data(), ev, n_seg * sizeof(rpkt_flow_ev_t), hipMemcpyDeviceToHost));
    std::vector<uint32_t> ord(n_seg);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        return ((hev[a] >> 32) & 0xffff) < ((hev[b] >> 32) & 0xffff);
    });
    HIP_OK(hipMemcpy(order, ord.data(), n_seg * sizeof(uint32_t), hipMemcpyHostToDevice));
    uint32_t* moffs = dev_alloc<uint32_t>(n_seg + 1);
    rpkt_rec_t* mrecs = dev_alloc<rpkt_rec_t>(n_seg);
    if (!moffs || !mrecs) return 2;
    if (rc == RPKT_OK)
        rc = rpkt_gpu_coalesce_batch(&rb, recs, order, 65535, 0, merged, n_seg * (hdr + mss), moffs, n_seg,
                                     first, gso, totals, ws, nullptr);
    const rpkt_batch_t mb = {merged, n_seg * (hdr + mss), moffs, 0, 0, n_seg, 0};
    if (rc == RPKT_OK) rc = rpkt_gpu_parse_batch(&mb, F, mrecs, nullptr, 0, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "rx failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }

    std::vector<rpkt_rec_t> out(n_seg);
    std::vector<uint32_t> ooffs(n_seg + 1), sfirst(n_seg + 1);
    std::vector<uint16_t> hgso(n_seg);
    std::vector<uint8_t> bytes(n_seg * (hdr + mss));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.data(), mrecs, n_seg * sizeof(rpkt_rec_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ooffs.data(), moffs, (n_seg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(sfirst.data(), first, (n_seg + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hgso.data(), gso, n_seg * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bytes.data(), merged, bytes.size(), hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    printf("rx : %u segments of %u streams, interleaved; coalesced into %llu frames, %llu bytes\n",
           n_seg, S, (unsigned long long)tot[0], (unsigned long long)tot[1]);
    bool ok = tot[0] == S && tot[1] == (uint64_t)S * (hdr + payload);
    uint32_t seen = 0;
    for (uint32_t j = 0; j < tot[0] && j < n_seg; j++) {
        const rpkt_rec_t& r = out[j];
        // lro_rx.rs:81-99
        printf("tcp packet: src port %u, dst port %u, seq_num %u, ack_num %u, ack %d, psh %d, "
               "window_size %u, payload_len %u, checksum 0x%04x (ip_sum=0x%04x l4_sum=0x%04x; %u "
               "segments of %u)\n", r.src_port, r.dst_port, r.tcp_seq, r.tcp_ack,
               (r.l4_word6 & 0x10) != 0, (r.l4_word6 & 0x08) != 0, r.tcp_window, r.payload_len,
               r.l4_checksum, r.ip_sum, r.l4_sum, sfirst[j + 1] - sfirst[j], hgso[j]);
        const uint32_t s = (uint32_t)(r.src_port - 40000) / 11;
        if (s >= S || r.src_port != build[s].src_port) {
            ok = false;
            continue;
        }
        seen |= 1u << s;
        ok = ok && r.status == RPKT_S_OK && r.ip_sum == 0xffff && r.l4_sum == 0xffff &&
             r.payload_len == payload && r.frame_len == hdr + payload && r.tcp_seq == build[s].tcp_seq &&
             r.tcp_ack == build[s].tcp_ack && r.tcp_window == build[s].tcp_window &&
             r.ip_ident == build[s].ip_ident && (r.l4_word6 & 0xff) == 0x18 && hgso[j] == mss &&
             sfirst[j + 1] - sfirst[j] == per &&
             memcmp(bytes.data() + ooffs[j] + hdr, host.data() + s * stride + hdr, payload) == 0;
    }
    ok = ok && seen == (1u << S) - 1;
    printf("%s\n", ok ? "ok: every stream came back whole, sums valid" : "MISMATCH");
    (void)hipFree(frames); (void)hipFree(wire); (void)hipFree(rx); (void)hipFree(merged);
    (void)hipFree(recs); (void)hipFree(rec_build); (void)hipFree(offs); (void)hipFree(first);
    (void)hipFree(order); (void)hipFree(gso); (void)hipFree(totals); (void)hipFree(ev); (void)hipFree(ws);
    (void)hipFree(moffs); (void)hipFree(mrecs);
    return ok ? 0 : 1;
}
