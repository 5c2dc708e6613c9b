// vtep_prefrag_tx.cpp — a tunnel ingress that fragments BEFORE it encapsulates (RFC 4459 section
// 3.2), through the C ABI only (include/rpkt_gpu.h).  The tenants' frames carry MTU-sized IPv4 /
// UDP packets (1500 bytes, DF clear); half of them sit behind VXLAN (50 bytes from the outer IP
// header to the inner one), half behind GTP-U (36 bytes), so every outer packet is over the
// underlay's 1500.  rpkt_gpu_parse_tunnel_batch -> rpkt_gpu_fragment_tunnel_batch (mtu 1500) ->
// rpkt_gpu_parse_tunnel_batch cuts the INNER packet in two and reads the outputs back: each is a
// complete tunnel packet of at most 1500 bytes with its own outer UDP header and valid outer
// sums, the tunnel decodes, and the inner fragments' offsets, MF and payloads are the inner
// packet's in order.  The egress decapsulates each on its own; the destination host
// reassembles.  One stream, no host step between the calls.
//   hipcc -O2 -Iinclude examples/vtep_prefrag_tx.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/vtep_prefrag_tx && ./examples/vtep_prefrag_tx
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

static void be16(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}

// RFC 1071 over [p, p + n) added to `acc`
static uint32_t sum16(const uint8_t* p, size_t n, uint32_t acc = 0) {
    for (size_t k = 0; k + 1 < n; k += 2) acc += (uint32_t)p[k] << 8 | p[k + 1];
    if (n & 1) acc += (uint32_t)p[n - 1] << 8;
    while (acc >> 16) acc = (acc & 0xffff) + (acc >> 16);
    return acc;
}

// an IPv4 header (20 bytes) at h for a packet of `len` bytes, its checksum filled
static void ip4_header(uint8_t* h, uint32_t len, uint32_t ident, uint8_t proto, uint32_t src, uint32_t dst) {
    memset(h, 0, 20);
    h[0] = 0x45;
    be16(h + 2, len);
    be16(h + 4, ident);
    h[8] = 64;
    h[9] = proto;
    be16(h + 12, src >> 16); be16(h + 14, src);
    be16(h + 16, dst >> 16); be16(h + 18, dst);
    be16(h + 10, ~sum16(h, 20) & 0xffff);
}

// a UDP header at u over `len` bytes (header and payload, the payload in place), checksum filled
static void udp_header(uint8_t* u, uint32_t len, uint32_t sport, uint32_t dport, const uint8_t* ip) {
    be16(u, sport);
    be16(u + 2, dport);
    be16(u + 4, len);
    be16(u + 6, 0);
    uint32_t acc = sum16(ip + 12, 8, 17 + len);
    const uint32_t ck = ~sum16(u, len, acc) & 0xffff;
    be16(u + 6, ck ? ck : 0xffff);
}

int main() {
    const uint32_t n = 8, mtu = 1500, ipl = 1500, P = ipl - 20;   // the inner IP packet and its payload
    const uint32_t over_of[2] = {50, 36};                         // VXLAN, GTP-U: outer l3 to inner l3
    const uint32_t il3_of[2] = {14 + 50, 14 + 36};
    uint32_t n_out = 0, off = 7;                                  // an odd lead
    uint64_t need = 0;
    std::vector<uint32_t> offsets(n + 1);
    for (uint32_t i = 0; i < n; i++) {
        offsets[i] = off;
        off += il3_of[i & 1] + ipl;
        const uint32_t c = (mtu - over_of[i & 1] - 20) & ~7u, per = (P + c - 1) / c;
        n_out += per;
        need += (uint64_t)per * (il3_of[i & 1] + 20) + P;
    }
    offsets[n] = off;
    const uint32_t out_cap = n_out + 3;
    const uint64_t out_bytes = need + 64;
    std::vector<uint8_t> host(off + 16, 0);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t* f = host.data() + offsets[i];
        const bool gtp = i & 1;
        const uint32_t il3 = il3_of[i & 1], flen = il3 + ipl;
        // the tenant's packet: IPv4 (DF clear) / UDP / payload
        uint8_t* ip = f + il3;
        for (uint32_t k = 28; k < ipl; k++) ip[k] = (uint8_t)(k * 7 + (k >> 8) + i);
        ip4_header(ip, ipl, 0x100 + i, 17, (192u << 24) | (168u << 16) | (i << 8) | 1u,
                   (192u << 24) | (168u << 16) | (i << 8) | 2u);
        udp_header(ip + 20, P, 40000 + i, 53, ip);
        // the underlay: Ether / IPv4 / UDP / VXLAN / Ether, or Ether / IPv4 / UDP / GTP-U
        const uint8_t mac[12] = {0x02, 0, 0, 0, 9, 1, 0x02, 0, 0, 0, 9, 2};
        memcpy(f, mac, 12);
        be16(f + 12, 0x0800);
        uint8_t* t = f + 42;
        if (!gtp) {
            t[0] = 0x08;                                          // VXLAN: I flag, VNI
            t[4] = 0; t[5] = 0x13; t[6] = (uint8_t)(0x88 + i);
            const uint8_t m2[12] = {0x02, 0, 0, 0, 1, (uint8_t)i, 0x02, 0, 0, 0, 2, (uint8_t)i};
            memcpy(t + 8, m2, 12);
            be16(t + 20, 0x0800);
        } else {
            t[0] = 0x30;                                          // GTPv1, G-PDU
            t[1] = 255;
            be16(t + 2, ipl);
            t[4] = 0xde; t[5] = 0xad; t[6] = 0xbe; t[7] = (uint8_t)i;
        }
        ip4_header(f + 14, flen - 14, 0x4000 + i, 17, (10u << 24) | 1u, (10u << 24) | 2u);
        udp_header(f + 34, flen - 34, 49152 + i, gtp ? 2152 : 4789, f + 14);
    }

    uint8_t *frames = nullptr, *out = nullptr;
    rpkt_rec_t *outer = nullptr, *inner = nullptr, *o_outer = nullptr, *o_inner = nullptr;
    rpkt_tun_t *tun = nullptr, *o_tun = nullptr;
    uint32_t *d_off = nullptr, *out_offsets = nullptr, *frag_first = nullptr;
    uint64_t* totals = nullptr;
    void* ws = nullptr;
    const size_t rb = sizeof(rpkt_rec_t), tb = sizeof(rpkt_tun_t);
    if (!(dev_alloc(&frames, host.size()) && dev_alloc(&out, out_bytes) && dev_alloc(&outer, n * rb) &&
          dev_alloc(&inner, n * rb) && dev_alloc(&tun, n * tb) && dev_alloc(&o_outer, out_cap * rb) &&
          dev_alloc(&o_inner, out_cap * rb) && dev_alloc(&o_tun, out_cap * tb) &&
          dev_alloc(&d_off, (n + 1) * 4) && dev_alloc(&out_offsets, (out_cap + 1) * 4) &&
          dev_alloc(&frag_first, (n + 1) * 4) && dev_alloc(&totals, 16) &&
          dev_alloc(&ws, rpkt_gpu_fragment_tunnel_workspace_bytes(n)))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_off, offsets.data(), (n + 1) * 4, hipMemcpyHostToDevice));

    const uint32_t sums = RPKT_F_IP_SUM | RPKT_F_L4_SUM;
    const rpkt_batch_t b = {frames, host.size(), d_off, 0, 0, n, 0};
    const rpkt_batch_t ob = {out, out_bytes, out_offsets, 0, 0, out_cap, 0};
    int rc = rpkt_gpu_parse_tunnel_batch(&b, sums, outer, tun, inner, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_fragment_tunnel_batch(&b, outer, tun, inner, mtu, 0, 0, out, out_bytes,
                                            out_offsets, out_cap, frag_first, totals, ws, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_parse_tunnel_batch(&ob, sums, o_outer, o_tun, o_inner, nullptr, 0, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }

    std::vector<uint8_t> h_out(out_bytes);
    std::vector<rpkt_rec_t> O(n), I(n), FO(out_cap), FI(out_cap);
    std::vector<rpkt_tun_t> T(n), FT(out_cap);
    std::vector<uint32_t> first(n + 1), offs(out_cap + 1);
    uint64_t tot[2];
    HIP_OK(hipMemcpy(h_out.data(), out, out_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(O.data(), outer, n * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(I.data(), inner, n * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(T.data(), tun, n * tb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(FO.data(), o_outer, out_cap * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(FI.data(), o_inner, out_cap * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(FT.data(), o_tun, out_cap * tb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first.data(), frag_first, (n + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs.data(), out_offsets, (out_cap + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    bool ok = tot[0] == n_out && tot[1] == need && offs[0] == 0 && first[n] == n_out && n_out == 2 * n;
    uint32_t too_long = 0, bad_tunnel = 0, bad_sums = 0, bad_inner = 0, bad_bytes = 0;
    for (uint32_t i = 0; i < n && ok; i++) {
        const uint32_t il3 = il3_of[i & 1], c = (mtu - over_of[i & 1] - 20) & ~7u;
        printf("in  %u: %s outer packet=%u tunnel kind %u status %u inner %s packet=%u -> outputs [%u, %u)\n",
               i, rpkt_gpu_status_name(O[i].status), O[i].ip_packet_len, T[i].kind, T[i].status,
               rpkt_gpu_status_name(I[i].status), I[i].ip_packet_len, first[i], first[i + 1]);
        ok = ok && O[i].status == RPKT_S_OK && O[i].ip_packet_len > mtu && T[i].status == RPKT_T_OK &&
             T[i].kind == ((i & 1) ? RPKT_TUN_GTPU : RPKT_TUN_VXLAN) && I[i].status == RPKT_S_OK &&
             I[i].l4_sum == 0xffff && I[i].l3_off == il3 && first[i] == 2 * i && first[i + 1] == 2 * i + 2;
        const uint8_t* src = host.data() + offsets[i];
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t j = 2 * i + k, p = k == 0 ? c : P - c, len = offs[j + 1] - offs[j];
            const uint8_t* o = h_out.data() + offs[j];
            printf("out %u: len=%u outer packet=%u ident=0x%04x sums 0x%04x 0x%04x tunnel status %u "
                   "inner packet=%u frag=0x%04x ip_sum=0x%04x\n", j, len, FO[j].ip_packet_len,
                   FO[j].ip_ident, FO[j].ip_sum, FO[j].l4_sum, FT[j].status, FI[j].ip_packet_len,
                   FI[j].ip_frag, FI[j].ip_sum);
            if (len != il3 + 20 + p || FO[j].ip_packet_len != len - 14 || len - 14 > mtu) too_long++;
            if (FT[j].status != RPKT_T_OK || FT[j].kind != T[i].kind || FT[j].id != T[i].id ||
                FT[j].inner_off != T[i].inner_off)
                bad_tunnel++;
            if (FO[j].status != RPKT_S_OK || FO[j].ip_sum != 0xffff || FO[j].l4_sum != 0xffff ||
                FO[j].ip_ident != (uint16_t)(0x4000 + i + k) || FO[j].src_port != O[i].src_port)
                bad_sums++;
            // offset k * c / 8, MF on the first, everything else the inner packet's
            if (!(FI[j].ip_packet_len == 20 + p && FI[j].ip_frag == ((k * c / 8) | (k == 0 ? 0x2000u : 0u)) &&
                  FI[j].ip_ident == I[i].ip_ident && FI[j].ip_sum == 0xffff && FI[j].ip_protocol == 17 &&
                  FI[j].ip_src == I[i].ip_src && FI[j].ip_dst == I[i].ip_dst && FI[j].l3_off == il3))
                bad_inner++;
            // the bytes between the outer UDP header and the inner IP header, and the slice
            if (memcmp(o, src, 14) != 0 || memcmp(o + 42, src + 42, 2) != 0 ||
                memcmp(o + 46, src + 46, il3 - 46) != 0 ||
                memcmp(o + il3 + 20, src + il3 + 20 + k * c, p) != 0)
                bad_bytes++;
        }
    }
    for (uint32_t j = n_out; j < out_cap; j++)                    // the spare slots: empty frames
        ok = ok && FO[j].frame_len == 0 && offs[j + 1] == tot[1];
    printf("out: %llu frames, %llu bytes; outer packets over the mtu or of a wrong length: %u, tunnels "
           "that do not decode: %u, outer headers with a wrong sum or field: %u, inner fragments with a "
           "wrong field: %u, with wrong bytes: %u\n", (unsigned long long)tot[0],
           (unsigned long long)tot[1], too_long, bad_tunnel, bad_sums, bad_inner, bad_bytes);
    ok = ok && !too_long && !bad_tunnel && !bad_sums && !bad_inner && !bad_bytes;
    printf("%s\n", ok ? "ok: 2 tunnel packets a frame, every outer packet <= 1500 with valid sums, "
                        "inner fragments in order" : "MISMATCH");
    (void)hipFree(frames); (void)hipFree(out); (void)hipFree(outer); (void)hipFree(inner);
    (void)hipFree(tun); (void)hipFree(o_outer); (void)hipFree(o_inner); (void)hipFree(o_tun);
    (void)hipFree(d_off); (void)hipFree(out_offsets); (void)hipFree(frag_first);
    (void)hipFree(totals); (void)hipFree(ws);
    return ok ? 0 : 1;
}
