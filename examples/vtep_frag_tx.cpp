// vtep_frag_tx.cpp — a VTEP whose encapsulation is over the MTU, through the C ABI only
// (include/rpkt_gpu.h).  The tenant's frames carry MTU-sized IP packets (1500 bytes);
// rpkt_gpu_build_tunnel_batch puts 50 bytes of Ether/IPv4/UDP/VXLAN around each, so the outer IP
// packet is 1550 bytes and does not fit the underlay's 1500.  rpkt_gpu_parse_batch ->
// rpkt_gpu_fragment_batch (mtu 1500) -> rpkt_gpu_parse_batch cuts the OUTER packet into two
// fragments (1480 and 50 bytes of IP payload) and reads them back: offsets, MF, a valid header
// sum on each, and the fragments' payloads together are the built packet's.  One stream, no
// host step between the calls.
//   hipcc -O2 -Iinclude examples/vtep_frag_tx.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/vtep_frag_tx && ./examples/vtep_frag_tx
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

template <class T>
static bool dev_alloc(T** p, size_t bytes) {
    return hipMalloc((void**)p, bytes ? bytes : 16) == hipSuccess;
}

int main() {
    // outer Ether 14 + IPv4 20 + UDP 8 + VXLAN 8 = 50, inner Ether 14 + IPv4 20 + TCP 20 = 54
    const uint32_t n = 4, ohdr = 50, ihdr = 54, payload = 1500 - 40, mtu = 1500;
    const uint32_t flen = ohdr + ihdr + payload;                  // 1564: an IP packet of 1550
    const uint32_t lead = 14;                                     // lead + ohdr = 64
    const uint32_t P = flen - 34, c = (mtu - 20) & ~7u, per = (P + c - 1) / c;   // 1530, 1480, 2
    const uint32_t n_out = n * per, out_cap = n_out + 3;
    const uint64_t need = (uint64_t)n * (per * 34 + P);
    const uint64_t out_bytes = need + 64;
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
        // the underlay: Ether / IPv4 (DF clear) / UDP 4789 / VXLAN
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

    uint8_t *frames = nullptr, *out = nullptr, *built = nullptr;
    rpkt_rec_t *d_rin = nullptr, *d_rout = nullptr, *recs = nullptr, *o_recs = nullptr;
    rpkt_tun_t* d_tb = nullptr;
    uint32_t *d_oo = nullptr, *out_offsets = nullptr, *frag_first = nullptr;
    uint64_t* totals = nullptr;
    void* ws = nullptr;
    const size_t rb = sizeof(rpkt_rec_t), tb = sizeof(rpkt_tun_t);
    if (!(dev_alloc(&frames, host.size()) && dev_alloc(&out, out_bytes) && dev_alloc(&built, 2 * n) &&
          dev_alloc(&d_rin, n * rb) && dev_alloc(&d_rout, n * rb) && dev_alloc(&recs, n * rb) &&
          dev_alloc(&o_recs, out_cap * rb) && dev_alloc(&d_tb, n * tb) &&
          dev_alloc(&d_oo, (n + 1) * 4) && dev_alloc(&out_offsets, (out_cap + 1) * 4) &&
          dev_alloc(&frag_first, (n + 1) * 4) && dev_alloc(&totals, 16) &&
          dev_alloc(&ws, rpkt_gpu_fragment_workspace_bytes(n)))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rin, r_inner.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rout, r_outer.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tb, t_build.data(), n * tb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_oo, off_outer.data(), (n + 1) * 4, hipMemcpyHostToDevice));

    // inside-out: the inner frames, then the tunnel around them; parse, fragment, parse the output
    const rpkt_batch_t bi = {frames + lead + ohdr, host.size() - lead - ohdr, nullptr, flen,
                             ihdr + payload, n, 0};
    const rpkt_batch_t bo = {frames, host.size(), d_oo, 0, 0, n, 0};
    const rpkt_batch_t ob = {out, out_bytes, out_offsets, 0, 0, out_cap, 0};
    int rc = rpkt_gpu_build_batch(&bi, d_rin, fill, built, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_build_tunnel_batch(&bo, d_rout, d_tb, fill, built + n, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_parse_batch(&bo, sums, recs, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_fragment_batch(&bo, recs, mtu, 0, 0, out, out_bytes, out_offsets, out_cap,
                                     frag_first, totals, ws, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_parse_batch(&ob, sums, o_recs, nullptr, 0, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }

    std::vector<uint8_t> h_built(2 * n), h_frames(host.size()), h_out(out_bytes);
    std::vector<rpkt_rec_t> h_recs(n), f_recs(out_cap);
    std::vector<uint32_t> first(n + 1), offs(out_cap + 1);
    uint64_t tot[2];
    HIP_OK(hipMemcpy(h_built.data(), built, 2 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_frames.data(), frames, host.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_out.data(), out, out_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_recs.data(), recs, n * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(f_recs.data(), o_recs, out_cap * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first.data(), frag_first, (n + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs.data(), out_offsets, (out_cap + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    bool ok = tot[0] == n_out && tot[1] == need && offs[0] == 0 && first[n] == n_out;
    uint32_t bad_sums = 0, bad_fields = 0, bad_bytes = 0;
    for (uint32_t i = 0; i < n && ok; i++) {
        const rpkt_rec_t& O = h_recs[i];
        printf("in  %u: %s len=%u ip packet=%u frag=0x%04x sums 0x%04x 0x%04x -> outputs [%u, %u)\n", i,
               rpkt_gpu_status_name(O.status), O.frame_len, O.ip_packet_len, O.ip_frag, O.ip_sum,
               O.l4_sum, first[i], first[i + 1]);
        ok = ok && h_built[i] == 1 && h_built[n + i] == 1 && O.status == RPKT_S_OK &&
             O.frame_len == flen && O.ip_packet_len == flen - 14 && O.ip_frag == 0 &&
             O.ip_sum == 0xffff && O.l4_sum == 0xffff && first[i] == i * per &&
             first[i + 1] == (i + 1) * per;
        const uint8_t* src = h_frames.data() + off_outer[i];
        for (uint32_t k = 0; k < per; k++) {
            const uint32_t j = i * per + k, p = k + 1 < per ? c : P - (per - 1) * c;
            const rpkt_rec_t& F = f_recs[j];
            const uint8_t* o = h_out.data() + offs[j];
            printf("out %u: len=%u ip packet=%u frag=0x%04x ident=0x%04x ip_sum=0x%04x\n", j,
                   F.frame_len, F.ip_packet_len, F.ip_frag, F.ip_ident, F.ip_sum);
            if (F.ip_sum != 0xffff) bad_sums++;
            // offset k * c / 8, MF on every fragment but the last, everything else the packet's
            if (!(offs[j + 1] - offs[j] == 34 + p && F.frame_len == 34 + p && F.ip_packet_len == 20 + p &&
                  F.ip_frag == ((k * c / 8) | (k + 1 < per ? 0x2000u : 0u)) &&
                  F.ip_ident == r_outer[i].ip_ident && F.ip_protocol == 17 && F.ip_ttl == 64 &&
                  F.ip_src == r_outer[i].ip_src && F.ip_dst == r_outer[i].ip_dst && F.l3_off == 14))
                bad_fields++;
            // the Ethernet header, and this fragment's slice of the built packet's IP payload
            if (memcmp(o, src, 14) != 0 || memcmp(o + 34, src + 34 + k * c, p) != 0) bad_bytes++;
        }
    }
    for (uint32_t j = n_out; j < out_cap; j++)                    // the spare slots: empty frames
        ok = ok && f_recs[j].frame_len == 0 && offs[j + 1] == tot[1];
    printf("out: %llu frames, %llu bytes; fragments with a header sum that does not verify: %u, "
           "with a wrong field: %u, with wrong bytes: %u\n", (unsigned long long)tot[0],
           (unsigned long long)tot[1], bad_sums, bad_fields, bad_bytes);
    ok = ok && bad_sums == 0 && bad_fields == 0 && bad_bytes == 0;
    printf("%s\n", ok ? "ok: 2 fragments a frame, header sums valid, payloads reassemble" : "MISMATCH");
    (void)hipFree(frames); (void)hipFree(out); (void)hipFree(built); (void)hipFree(d_rin);
    (void)hipFree(d_rout); (void)hipFree(recs); (void)hipFree(o_recs); (void)hipFree(d_tb);
    (void)hipFree(d_oo); (void)hipFree(out_offsets); (void)hipFree(frag_first);
    (void)hipFree(totals); (void)hipFree(ws);
    return ok ? 0 : 1;
}
