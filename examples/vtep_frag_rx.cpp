// vtep_frag_rx.cpp — the receive side of vtep_frag_tx.cpp, through the C ABI only
// (include/rpkt_gpu.h).  A peer VTEP put 50 bytes of Ether/IPv4/UDP/VXLAN around MTU-sized
// tenant frames and fragmented the over-MTU outer packets at 1500: two fragments a frame, and
// here they arrive in reverse order, so the last fragment of the last frame comes first.  The
// parser alone cannot get at the inner frames: the first fragment's UDP length does not fit and
// the second has no UDP header at all.  rpkt_gpu_parse_batch -> rpkt_gpu_reassemble_keys -> a
// stable sort of the keys (the caller's: std::stable_sort here) -> rpkt_gpu_reassemble_batch
// brings every outer packet back, and rpkt_gpu_parse_tunnel_batch of the output decodes the
// tenant's frames, which are checked field by field against what was built.
//   hipcc -O2 -Iinclude examples/vtep_frag_rx.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/vtep_frag_rx && ./examples/vtep_frag_rx
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

int main() {
    // outer Ether 14 + IPv4 20 + UDP 8 + VXLAN 8 = 50, inner Ether 14 + IPv4 20 + TCP 20 = 54
    const uint32_t n = 6, ohdr = 50, ihdr = 54, payload = 1500 - 40, mtu = 1500;
    const uint32_t flen = ohdr + ihdr + payload;                  // 1564: an IP packet of 1550
    const uint32_t lead = 14;                                     // lead + ohdr = 64
    const uint32_t P = flen - 34, c = (mtu - 20) & ~7u, per = (P + c - 1) / c;   // 1530, 1480, 2
    const uint32_t nf = n * per;                                  // fragments
    const uint64_t fbytes = (uint64_t)n * (per * 34 + P), fbuf = fbytes + 64;
    const uint32_t sums = RPKT_F_IP_SUM | RPKT_F_L4_SUM, fill = RPKT_BUILD_IP_CSUM | RPKT_BUILD_L4_CSUM;

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
        // the tenant's frame: Ether / IPv4 / TCP, an IP packet of exactly the MTU
        rpkt_rec_t& a = r_inner[i];
        const uint8_t m1[6] = {0x02, 0, 0, 0, 1, (uint8_t)i}, m2[6] = {0x02, 0, 0, 0, 2, (uint8_t)i};
        memcpy(a.dst_addr, m1, 6);
        memcpy(a.src_addr, m2, 6);
        a.ethertype = 0x0800;
        a.ip_vhl = 0x45;
        a.ip_ttl = 64;
        a.ip_protocol = 6;
        a.ip_ident = (uint16_t)(7 + i);
        a.ip_frag = 0x4000;                                       // DF: the tenant's business
        a.ip_src = (192u << 24) | (168u << 16) | (i << 8) | 1u;
        a.ip_dst = (192u << 24) | (168u << 16) | (i << 8) | 2u;
        a.src_port = (uint16_t)(40000 + i);
        a.dst_port = 443;
        a.tcp_seq = 1000u * i;
        a.l4_word6 = 0x5000 | 0x10;                               // header_len 20, ACK
        a.tcp_window = 512;
        // the underlay: Ether / IPv4 (DF clear) / UDP 4789 / VXLAN; one ident per packet
        rpkt_rec_t& o = r_outer[i];
        const uint8_t v1[6] = {0x02, 0, 0, 0, 9, 1}, v2[6] = {0x02, 0, 0, 0, 9, 2};
        memcpy(o.dst_addr, v1, 6);
        memcpy(o.src_addr, v2, 6);
        o.ethertype = 0x0800;
        o.ip_vhl = 0x45;
        o.ip_ttl = 64;
        o.ip_protocol = 17;
        o.ip_ident = (uint16_t)(0x4000 + i);
        o.ip_src = (10u << 24) | 1u;
        o.ip_dst = (10u << 24) | 2u;
        o.src_port = (uint16_t)(49152 + i);
        o.dst_port = 4789;
        t_build[i].kind = RPKT_TUN_VXLAN;
        t_build[i].hdr0 = 0x08;                                   // vni_present
        t_build[i].id = 5000 + i;
    }
    off_outer[n] = lead + n * flen;

    uint8_t *frames = nullptr, *frags = nullptr, *rx = nullptr, *out = nullptr, *built = nullptr;
    rpkt_rec_t *d_rin = nullptr, *d_rout = nullptr, *recs = nullptr, *f_recs = nullptr;
    rpkt_rec_t *o_outer = nullptr, *o_inner = nullptr;
    rpkt_tun_t *d_tb = nullptr, *o_tun = nullptr;
    uint32_t *d_oo = nullptr, *frag_offsets = nullptr, *frag_first = nullptr, *rx_offsets = nullptr;
    uint32_t *order = nullptr, *out_offsets = nullptr, *src_first = nullptr;
    uint64_t *totals = nullptr, *keys = nullptr;
    void *ws_frag = nullptr, *ws = nullptr;
    const size_t rb = sizeof(rpkt_rec_t), tb = sizeof(rpkt_tun_t);
    if (!(dev_alloc(&frames, host.size()) && dev_alloc(&frags, fbuf) && dev_alloc(&rx, fbuf) &&
          dev_alloc(&out, fbuf) && dev_alloc(&built, 2 * n) && dev_alloc(&d_rin, n * rb) &&
          dev_alloc(&d_rout, n * rb) && dev_alloc(&recs, n * rb) && dev_alloc(&f_recs, nf * rb) &&
          dev_alloc(&o_outer, nf * rb) && dev_alloc(&o_inner, nf * rb) && dev_alloc(&d_tb, n * tb) &&
          dev_alloc(&o_tun, nf * tb) && dev_alloc(&d_oo, (n + 1) * 4) &&
          dev_alloc(&frag_offsets, (nf + 1) * 4) && dev_alloc(&frag_first, (n + 1) * 4) &&
          dev_alloc(&rx_offsets, (nf + 1) * 4) && dev_alloc(&order, nf * 4) &&
          dev_alloc(&out_offsets, (nf + 1) * 4) && dev_alloc(&src_first, (nf + 1) * 4) &&
          dev_alloc(&totals, 16) && dev_alloc(&keys, nf * 8) &&
          dev_alloc(&ws_frag, rpkt_gpu_fragment_workspace_bytes(n)) &&
          dev_alloc(&ws, rpkt_gpu_reassemble_workspace_bytes(nf)))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rin, r_inner.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rout, r_outer.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tb, t_build.data(), n * tb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_oo, off_outer.data(), (n + 1) * 4, hipMemcpyHostToDevice));

    // the peer: build inside-out, parse, fragment the outer packets at the underlay's MTU
    const rpkt_batch_t bi = {frames + lead + ohdr, host.size() - lead - ohdr, nullptr, flen,
                             ihdr + payload, n, 0};
    const rpkt_batch_t bo = {frames, host.size(), d_oo, 0, 0, n, 0};
    RPKT_OK_OR_FAIL(rpkt_gpu_build_batch(&bi, d_rin, fill, built, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_build_tunnel_batch(&bo, d_rout, d_tb, fill, built + n, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_parse_batch(&bo, sums, recs, nullptr, 0, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_fragment_batch(&bo, recs, mtu, 0, 0, frags, fbuf, frag_offsets, nf,
                                            frag_first, totals, ws_frag, nullptr));
    HIP_OK(hipDeviceSynchronize());
    uint64_t tot[2];
    std::vector<uint32_t> foffs(nf + 1), roffs(nf + 1);
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(foffs.data(), frag_offsets, (nf + 1) * 4, hipMemcpyDeviceToHost));
    if (tot[0] != nf || tot[1] != fbytes) {
        fprintf(stderr, "fragmentation gave %llu frames, %llu bytes\n", (unsigned long long)tot[0],
                (unsigned long long)tot[1]);
        return 1;
    }

    // the wire: the fragments arrive in reverse order (device-to-device copies)
    roffs[0] = 0;
    for (uint32_t k = 0; k < nf; k++) {
        const uint32_t j = nf - 1 - k, len = foffs[j + 1] - foffs[j];
        HIP_OK(hipMemcpy(rx + roffs[k], frags + foffs[j], len, hipMemcpyDeviceToDevice));
        roffs[k + 1] = roffs[k] + len;
    }
    HIP_OK(hipMemcpy(rx_offsets, roffs.data(), (nf + 1) * 4, hipMemcpyHostToDevice));

    // this VTEP: parse, keys, the caller's sort, reassemble, decode the tunnels
    const rpkt_batch_t rxb = {rx, fbuf, rx_offsets, 0, 0, nf, 0};
    const rpkt_batch_t ob = {out, fbuf, out_offsets, 0, 0, nf, 0};
    RPKT_OK_OR_FAIL(rpkt_gpu_parse_batch(&rxb, sums, f_recs, nullptr, 0, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_reassemble_keys(&rxb, f_recs, 0, keys, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint64_t> h_keys(nf);
    std::vector<uint32_t> h_order(nf);
    HIP_OK(hipMemcpy(h_keys.data(), keys, nf * 8, hipMemcpyDeviceToHost));
    std::iota(h_order.begin(), h_order.end(), 0u);
    std::stable_sort(h_order.begin(), h_order.end(),
                     [&](uint32_t a, uint32_t b) { return h_keys[a] < h_keys[b]; });
    HIP_OK(hipMemcpy(order, h_order.data(), nf * 4, hipMemcpyHostToDevice));
    RPKT_OK_OR_FAIL(rpkt_gpu_reassemble_batch(&rxb, f_recs, order, 0, out, fbuf, out_offsets, nf,
                                              src_first, totals, ws, nullptr));
    RPKT_OK_OR_FAIL(rpkt_gpu_parse_tunnel_batch(&ob, sums, o_outer, o_tun, o_inner, nullptr, 0, nullptr));
    HIP_OK(hipDeviceSynchronize());

    std::vector<uint8_t> h_frames(host.size()), h_out(fbuf);
    std::vector<rpkt_rec_t> h_frecs(nf), h_outer(nf), h_inner(nf);
    std::vector<rpkt_tun_t> h_tun(nf);
    std::vector<uint32_t> first(nf + 1), offs(nf + 1);
    HIP_OK(hipMemcpy(h_frames.data(), frames, host.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_out.data(), out, fbuf, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_frecs.data(), f_recs, nf * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_outer.data(), o_outer, nf * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_inner.data(), o_inner, nf * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_tun.data(), o_tun, nf * tb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first.data(), src_first, (nf + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs.data(), out_offsets, (nf + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    // what the parser alone makes of the fragments: no inner frame to be had
    uint32_t undecodable = 0;
    for (uint32_t k = 0; k < nf; k++)
        if (h_frecs[k].status != RPKT_S_OK || (h_frecs[k].ip_frag & 0x3fff) != 0) undecodable++;
    printf("rx: %u fragments in reverse order, %u of them no whole datagram to the parser\n", nf,
           undecodable);
    bool ok = undecodable == nf && tot[0] == n && tot[1] == (uint64_t)n * flen && offs[0] == 0;
    uint32_t seen = 0, bad = 0;
    for (uint32_t j = 0; j < n && ok; j++) {
        const rpkt_rec_t &O = h_outer[j], &I = h_inner[j];
        const rpkt_tun_t& T = h_tun[j];
        const uint32_t i = T.id - 5000;                           // which frame this is: its VNI
        printf("out %u: positions [%u, %u) len=%u outer %s frag=0x%04x sums 0x%04x 0x%04x vni=%u inner %s "
               "seq=%u payload=%u sums 0x%04x 0x%04x\n", j, first[j], first[j + 1], O.frame_len,
               rpkt_gpu_status_name(O.status), O.ip_frag, O.ip_sum, O.l4_sum, T.id,
               rpkt_gpu_status_name(I.status), I.tcp_seq, I.payload_len, I.ip_sum, I.l4_sum);
        if (i >= n) {
            bad++;
            continue;
        }
        seen |= 1u << i;
        const rpkt_rec_t& a = r_inner[i];
        const bool same =
            first[j + 1] - first[j] == per && offs[j + 1] - offs[j] == flen && O.status == RPKT_S_OK &&
            O.ip_frag == 0 && O.ip_packet_len == flen - 14 && O.ip_sum == 0xffff && O.l4_sum == 0xffff &&
            O.ip_ident == r_outer[i].ip_ident && O.src_port == r_outer[i].src_port &&
            T.kind == RPKT_TUN_VXLAN && T.status == RPKT_T_OK && T.inner_off == ohdr &&
            I.status == RPKT_S_OK && memcmp(I.dst_addr, a.dst_addr, 6) == 0 &&
            memcmp(I.src_addr, a.src_addr, 6) == 0 && I.ip_ident == a.ip_ident && I.ip_frag == a.ip_frag &&
            I.ip_src == a.ip_src && I.ip_dst == a.ip_dst && I.src_port == a.src_port &&
            I.dst_port == a.dst_port && I.tcp_seq == a.tcp_seq && I.tcp_window == a.tcp_window &&
            I.ip_packet_len == mtu && I.payload_off == ohdr + ihdr && I.payload_len == payload &&
            I.ip_sum == 0xffff && I.l4_sum == 0xffff &&
            memcmp(h_out.data() + offs[j], h_frames.data() + off_outer[i], flen) == 0;
        if (!same) bad++;
    }
    for (uint32_t j = n; j < nf && ok; j++)                       // the spare slots: empty frames
        ok = ok && h_outer[j].frame_len == 0 && offs[j + 1] == tot[1] && first[j + 1] == nf;
    ok = ok && bad == 0 && seen == (1u << n) - 1u;
    if (ok) printf("ok: %u frames reassembled\n", n);
    else printf("MISMATCH (%u outputs differ)\n", bad);
    (void)hipFree(frames); (void)hipFree(frags); (void)hipFree(rx); (void)hipFree(out);
    (void)hipFree(built); (void)hipFree(d_rin); (void)hipFree(d_rout); (void)hipFree(recs);
    (void)hipFree(f_recs); (void)hipFree(o_outer); (void)hipFree(o_inner); (void)hipFree(d_tb);
    (void)hipFree(o_tun); (void)hipFree(d_oo); (void)hipFree(frag_offsets); (void)hipFree(frag_first);
    (void)hipFree(rx_offsets); (void)hipFree(order); (void)hipFree(out_offsets);
    (void)hipFree(src_first); (void)hipFree(totals); (void)hipFree(keys); (void)hipFree(ws_frag);
    (void)hipFree(ws);
    return ok ? 0 : 1;
}
