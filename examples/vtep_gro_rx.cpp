// vtep_gro_rx.cpp — the receive twin of vtep_tx.cpp, through the C ABI only (include/rpkt_gpu.h).
// The sender of vtep_tx.cpp builds four VXLAN frames around 32 KB inner TCP payloads and cuts
// them at mss 1448 into 92 wire frames; here the wire interleaves the four streams and the
// receiving VTEP brings every application write back in one frame without leaving the device:
// rpkt_gpu_parse_tunnel_batch with flow events (keyed by the INNER flow), the burst ordered by
// flow bucket, rpkt_gpu_coalesce_tunnel_batch.  The four outputs are compared byte for byte
// with the four frames that were sent: coalesce(segment(F)) == F, outer headers included.
//   hipcc -O2 -Iinclude examples/vtep_gro_rx.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/vtep_gro_rx && ./examples/vtep_gro_rx
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

template <class T>
static bool dev_alloc(T** p, size_t bytes) {
    return hipMalloc((void**)p, bytes ? bytes : 16) == hipSuccess;
}

int main() {
    // outer Ether 14 + IPv4 20 + UDP 8 + VXLAN 8 = 50, inner Ether 14 + IPv4 20 + TCP 20 = 54
    const uint32_t n = 4, ohdr = 50, ihdr = 54, payload = 32768, mss = 1448, n_buckets = 4096;
    const uint32_t flen = ohdr + ihdr + payload, lead = 14;       // lead + ohdr = 64
    const uint32_t per = (payload + mss - 1) / mss;               // 23 segments a frame
    const uint32_t n_seg = n * per;                               // 92
    const uint64_t wire_bytes = (uint64_t)n * ((uint64_t)per * (ohdr + ihdr) + payload);
    const uint32_t sums = RPKT_F_IP_SUM | RPKT_F_L4_SUM, fill = RPKT_BUILD_IP_CSUM | RPKT_BUILD_L4_CSUM;

    // the four frames of vtep_tx.cpp
    std::vector<uint8_t> host(lead + (size_t)n * flen + 16, 0);
    std::vector<uint32_t> off_outer(n + 1);
    std::vector<rpkt_rec_t> r_inner(n), r_outer(n);
    std::vector<rpkt_tun_t> t_build(n);
    memset(r_inner.data(), 0, n * sizeof(rpkt_rec_t));
    memset(r_outer.data(), 0, n * sizeof(rpkt_rec_t));
    memset(t_build.data(), 0, n * sizeof(rpkt_tun_t));
    for (uint32_t i = 0; i < n; i++) {
        off_outer[i] = lead + i * flen;
        uint8_t* pay = host.data() + off_outer[i] + ohdr + ihdr;
        for (uint32_t k = 0; k < payload; k++) pay[k] = (uint8_t)(k * 7 + (k >> 8) + i);
        rpkt_rec_t& a = r_inner[i];
        const uint8_t m1[6] = {0x02, 0, 0, 0, 1, (uint8_t)i}, m2[6] = {0x02, 0, 0, 0, 2, (uint8_t)i};
        memcpy(a.dst_addr, m1, 6);
        memcpy(a.src_addr, m2, 6);
        a.ethertype = 0x0800;
        a.ip_vhl = 0x45;
        a.ip_ttl = 64;
        a.ip_protocol = 6;
        a.ip_ident = (uint16_t)(0xfff0 + 8 * i);                  // wraps inside frames 0 and 1
        a.ip_src = (192u << 24) | (168u << 16) | (i << 8) | 1u;
        a.ip_dst = (192u << 24) | (168u << 16) | (i << 8) | 2u;
        a.src_port = (uint16_t)(40000 + i);
        a.dst_port = 443;
        a.tcp_seq = 0xffff0000u + i;                              // wraps inside the frame
        a.tcp_ack = 0x01020304u;
        a.l4_word6 = 0x5000 | 0x10 | 0x08;                        // header_len 20, ACK, PSH
        a.tcp_window = 512;
        rpkt_rec_t& o = r_outer[i];
        const uint8_t v1[6] = {0x02, 0, 0, 0, 9, 1}, v2[6] = {0x02, 0, 0, 0, 9, 2};
        memcpy(o.dst_addr, v1, 6);
        memcpy(o.src_addr, v2, 6);
        o.ethertype = 0x0800;
        o.ip_vhl = 0x45;
        o.ip_ttl = 64;
        o.ip_protocol = 17;
        o.ip_ident = (uint16_t)(100 * i);
        o.ip_src = (10u << 24) | 1u;
        o.ip_dst = (10u << 24) | 2u;
        o.src_port = (uint16_t)(49152 + i);
        o.dst_port = 4789;
        t_build[i].kind = RPKT_TUN_VXLAN;
        t_build[i].hdr0 = 0x08;                                   // vni_present
        t_build[i].id = 5000 + i;
    }
    off_outer[n] = lead + n * flen;

    uint8_t *frames = nullptr, *wire = nullptr, *rx = nullptr, *merged = nullptr, *built = nullptr;
    rpkt_rec_t *d_rin = nullptr, *d_rout = nullptr, *outer = nullptr, *inner = nullptr;
    rpkt_tun_t *d_tb = nullptr, *tun = nullptr;
    uint32_t *d_oo = nullptr, *offs = nullptr, *moffs = nullptr, *first = nullptr, *order = nullptr;
    uint16_t* gso = nullptr;
    uint64_t* totals = nullptr;
    rpkt_flow_ev_t* ev = nullptr;
    void *ws_seg = nullptr, *ws_co = nullptr;
    const size_t rb = sizeof(rpkt_rec_t), tb = sizeof(rpkt_tun_t);
    if (!(dev_alloc(&frames, host.size()) && dev_alloc(&wire, wire_bytes + 64) &&
          dev_alloc(&rx, wire_bytes + 64) && dev_alloc(&merged, wire_bytes + 64) &&
          dev_alloc(&built, 2 * n) && dev_alloc(&d_rin, n * rb) && dev_alloc(&d_rout, n * rb) &&
          dev_alloc(&outer, n_seg * rb) && dev_alloc(&inner, n_seg * rb) && dev_alloc(&d_tb, n * tb) &&
          dev_alloc(&tun, n_seg * tb) && dev_alloc(&d_oo, (n + 1) * 4) &&
          dev_alloc(&offs, (n_seg + 1) * 4) && dev_alloc(&moffs, (n_seg + 1) * 4) &&
          dev_alloc(&first, (n_seg + 1) * 4) && dev_alloc(&order, n_seg * 4) &&
          dev_alloc(&gso, n_seg * 2) && dev_alloc(&totals, 16) &&
          dev_alloc(&ev, n_seg * sizeof(rpkt_flow_ev_t)) &&
          dev_alloc(&ws_seg, rpkt_gpu_segment_tunnel_workspace_bytes(n)) &&
          dev_alloc(&ws_co, rpkt_gpu_coalesce_tunnel_workspace_bytes(n_seg)))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rin, r_inner.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rout, r_outer.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tb, t_build.data(), n * tb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_oo, off_outer.data(), (n + 1) * 4, hipMemcpyHostToDevice));

    // the sender: build inside-out, parse, cut at mss
    const rpkt_batch_t bi = {frames + lead + ohdr, host.size() - lead - ohdr, nullptr, flen,
                             ihdr + payload, n, 0};
    const rpkt_batch_t bo = {frames, host.size(), d_oo, 0, 0, n, 0};
    int rc = rpkt_gpu_build_batch(&bi, d_rin, fill, built, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_build_tunnel_batch(&bo, d_rout, d_tb, fill, built + n, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_parse_tunnel_batch(&bo, sums, outer, tun, inner, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_segment_tunnel_batch(&bo, outer, tun, inner, mss, 0, wire, wire_bytes + 64, offs,
                                           n_seg, first, totals, ws_seg, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "tx failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }
    uint64_t tot[2];
    std::vector<uint32_t> woffs(n_seg + 1);
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(woffs.data(), offs, (n_seg + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(host.data(), frames, host.size(), hipMemcpyDeviceToHost));   // the sent frames
    if (tot[0] != n_seg || tot[1] != wire_bytes) {
        fprintf(stderr, "%llu segments, want %u\n", (unsigned long long)tot[0], n_seg);
        return 1;
    }
    printf("%s\n", rpkt_gpu_build_info());
    printf("wire: %llu frames, %llu bytes\n", (unsigned long long)tot[0], (unsigned long long)tot[1]);

    // the wire: segment k of every stream in turn (device copies; the offsets on the host)
    std::vector<uint32_t> roffs(n_seg + 1, 0);
    for (uint32_t k = 0, at = 0; k < per; k++)
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t j = s * per + k, len = woffs[j + 1] - woffs[j];
            HIP_OK(hipMemcpy(rx + at, wire + woffs[j], len, hipMemcpyDeviceToDevice));
            at += len;
            roffs[k * n + s + 1] = at;
        }
    HIP_OK(hipMemcpy(offs, roffs.data(), (n_seg + 1) * 4, hipMemcpyHostToDevice));

    // the receiver: tunnel parse with flow events, order by bucket (stable), coalesce
    const rpkt_batch_t rxb = {rx, wire_bytes, offs, 0, 0, n_seg, 0};
    rc = rpkt_gpu_parse_tunnel_batch(&rxb, sums | RPKT_F_FLOW_EV, outer, tun, inner, ev, n_buckets,
                                     nullptr);
    std::vector<rpkt_flow_ev_t> hev(n_seg);
    if (rc == RPKT_OK) HIP_OK(hipMemcpy(hev.data(), ev, n_seg * sizeof(rpkt_flow_ev_t), hipMemcpyDeviceToHost));
    std::vector<uint32_t> ord(n_seg);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        return ((hev[a] >> 32) & 0xffff) < ((hev[b] >> 32) & 0xffff);
    });
    HIP_OK(hipMemcpy(order, ord.data(), n_seg * 4, hipMemcpyHostToDevice));
    if (rc == RPKT_OK)
        rc = rpkt_gpu_coalesce_tunnel_batch(&rxb, outer, tun, inner, order, 65535, 0, merged,
                                            wire_bytes + 64, moffs, n_seg, first, gso, totals, ws_co,
                                            nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "rx failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }

    std::vector<uint32_t> mo(n_seg + 1), src(n_seg + 1);
    std::vector<uint16_t> hgso(n_seg);
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(mo.data(), moffs, (n_seg + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(src.data(), first, (n_seg + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hgso.data(), gso, n_seg * 2, hipMemcpyDeviceToHost));
    printf("out: %llu frames, %llu bytes\n", (unsigned long long)tot[0], (unsigned long long)tot[1]);
    bool ok = tot[0] == n && tot[1] == (uint64_t)n * flen;
    std::vector<uint8_t> got(ok ? tot[1] : 0);
    if (ok) HIP_OK(hipMemcpy(got.data(), merged, tot[1], hipMemcpyDeviceToHost));
    uint32_t seen = 0;
    for (uint32_t j = 0; ok && j < n; j++) {
        const uint32_t len = mo[j + 1] - mo[j];
        int which = -1;
        for (uint32_t i = 0; i < n && len == flen; i++)
            if (memcmp(got.data() + mo[j], host.data() + off_outer[i], flen) == 0) which = (int)i;
        printf("out %u: %u bytes from positions [%u, %u), gso_size %u: %s\n", j, len, src[j], src[j + 1],
               hgso[j], which >= 0 ? "a sent frame" : "no sent frame");
        ok = ok && which >= 0 && src[j + 1] - src[j] == per && hgso[j] == mss;
        if (which >= 0) seen |= 1u << which;
    }
    ok = ok && seen == (1u << n) - 1u;
    printf("%s\n", ok ? "ok: 92 wire frames came back as 4, equal to the sent frames" : "MISMATCH");
    (void)hipFree(frames); (void)hipFree(wire); (void)hipFree(rx); (void)hipFree(merged);
    (void)hipFree(built); (void)hipFree(d_rin); (void)hipFree(d_rout); (void)hipFree(outer);
    (void)hipFree(inner); (void)hipFree(d_tb); (void)hipFree(tun); (void)hipFree(d_oo);
    (void)hipFree(offs); (void)hipFree(moffs); (void)hipFree(first); (void)hipFree(order);
    (void)hipFree(gso); (void)hipFree(totals); (void)hipFree(ev); (void)hipFree(ws_seg);
    (void)hipFree(ws_co);
    return ok ? 0 : 1;
}
