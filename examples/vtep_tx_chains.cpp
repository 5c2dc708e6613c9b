// vtep_tx_chains.cpp — vtep_tx.cpp's four VXLAN frames as the mbuf chains a DPDK port would be
// handed, through the C ABI only (include/rpkt_gpu.h).  A 32 KB application write never fits one
// data room: Mbuf::from_slice splits it over sixteen 2048-byte rooms and extend_front puts the
// 104 header bytes (outer Ether/IPv4/UDP/VXLAN 50, inner Ether/IPv4/TCP 54) into the first
// mbuf's 128-byte headroom, as tso_tx_chains.cpp lays its chain out (2048-B rooms in 2176-B
// slots).  The frames are built on the device as in vtep_tx.cpp and copied, device to device,
// into such slots; then rpkt_gpu_parse_tunnel_chains -> rpkt_gpu_segment_tunnel_chains ->
// rpkt_gpu_parse_tunnel_batch cuts the inner TCP at mss 1448 straight from the chains -- no
// gather into a flat batch -- and the parse of the flat output plays the receiving VTEP's RX
// checksum offloads, outer and inner.
//   hipcc -O2 -Iinclude examples/vtep_tx_chains.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/vtep_tx_chains && ./examples/vtep_tx_chains
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
    const uint32_t n = 4, ohdr = 50, ihdr = 54, hdr = ohdr + ihdr, payload = 32768, mss = 1448;
    const uint32_t flen = hdr + payload, lead = 14;               // lead + ohdr = 64
    const uint32_t per = (payload + mss - 1) / mss;               // 23 segments a frame
    const uint32_t n_out = n * per, out_cap = n_out + 4;
    const uint64_t need = (uint64_t)n * ((uint64_t)per * hdr + payload);
    const uint64_t out_bytes = need + 64;
    const uint32_t sums = RPKT_F_IP_SUM | RPKT_F_L4_SUM, fill = RPKT_BUILD_IP_CSUM | RPKT_BUILD_L4_CSUM;
    const uint32_t head_room = 128, data_room = 2048, slot = head_room + data_room;
    const uint32_t rooms = payload / data_room, n_segs = n * rooms;   // 16 mbufs a chain

    std::vector<uint8_t> host(lead + (size_t)n * flen + 16, 0);
    std::vector<uint32_t> off_outer(n + 1);
    std::vector<rpkt_rec_t> r_inner(n), r_outer(n);
    std::vector<rpkt_tun_t> t_build(n);
    memset(r_inner.data(), 0, n * sizeof(rpkt_rec_t));
    memset(r_outer.data(), 0, n * sizeof(rpkt_rec_t));
    memset(t_build.data(), 0, n * sizeof(rpkt_tun_t));
    for (uint32_t i = 0; i < n; i++) {
        off_outer[i] = lead + i * flen;
        uint8_t* pay = host.data() + off_outer[i] + hdr;
        for (uint32_t k = 0; k < payload; k++) pay[k] = (uint8_t)(k * 7 + (k >> 8) + i);
        rpkt_rec_t& a = r_inner[i];                               // the tenant's Ether / IPv4 / TCP
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
        rpkt_rec_t& o = r_outer[i];                               // Ether / IPv4 / UDP 4789 / VXLAN
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
    // chain i: mbuf 0 holds the headers in its headroom and the first room of payload, mbufs
    // 1..15 one room each; the pool hands its slots out from the top
    std::vector<uint32_t> segs_host(2 * n_segs), first_host(n + 1);
    for (uint32_t i = 0; i < n; i++) {
        first_host[i] = i * rooms;
        for (uint32_t r = 0; r < rooms; r++) {
            const uint32_t s = i * rooms + r, at = (n_segs - 1 - s) * slot;
            segs_host[2 * s] = at + head_room - (r == 0 ? hdr : 0);
            segs_host[2 * s + 1] = data_room + (r == 0 ? hdr : 0);
        }
    }
    first_host[n] = n_segs;
    const size_t arena_bytes = (size_t)n_segs * slot;

    uint8_t *frames = nullptr, *arena = nullptr, *out = nullptr, *built = nullptr;
    rpkt_rec_t *d_rin = nullptr, *d_rout = nullptr, *outer = nullptr, *inner = nullptr;
    rpkt_rec_t *o_outer = nullptr, *o_inner = nullptr;
    rpkt_tun_t *d_tb = nullptr, *tun = nullptr, *o_tun = nullptr;
    uint32_t *d_oo = nullptr, *segs = nullptr, *chain_first = nullptr, *out_offsets = nullptr;
    uint32_t* seg_first = nullptr;
    uint64_t* totals = nullptr;
    void* ws = nullptr;
    const size_t rb = sizeof(rpkt_rec_t), tb = sizeof(rpkt_tun_t);
    if (!(dev_alloc(&frames, host.size()) && dev_alloc(&arena, arena_bytes) &&
          dev_alloc(&out, out_bytes) && dev_alloc(&built, 2 * n) && dev_alloc(&d_rin, n * rb) &&
          dev_alloc(&d_rout, n * rb) && dev_alloc(&outer, n * rb) && dev_alloc(&inner, n * rb) &&
          dev_alloc(&o_outer, out_cap * rb) && dev_alloc(&o_inner, out_cap * rb) &&
          dev_alloc(&d_tb, n * tb) && dev_alloc(&tun, n * tb) && dev_alloc(&o_tun, out_cap * tb) &&
          dev_alloc(&d_oo, (n + 1) * 4) && dev_alloc(&segs, 2 * n_segs * 4) &&
          dev_alloc(&chain_first, (n + 1) * 4) && dev_alloc(&out_offsets, (out_cap + 1) * 4) &&
          dev_alloc(&seg_first, (n + 1) * 4) && dev_alloc(&totals, 16) &&
          dev_alloc(&ws, rpkt_gpu_segment_tunnel_chains_workspace_bytes(n)))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 2;
    }
    HIP_OK(hipMemcpy(frames, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(arena, 0x11, arena_bytes));
    HIP_OK(hipMemcpy(d_rin, r_inner.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rout, r_outer.data(), n * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tb, t_build.data(), n * tb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_oo, off_outer.data(), (n + 1) * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(segs, segs_host.data(), 2 * n_segs * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(chain_first, first_host.data(), (n + 1) * 4, hipMemcpyHostToDevice));

    // inside-out as in vtep_tx.cpp: the inner frames, then the tunnel around them
    const rpkt_batch_t bi = {frames + lead + ohdr, host.size() - lead - ohdr, nullptr, flen,
                             ihdr + payload, n, 0};
    const rpkt_batch_t bo = {frames, host.size(), d_oo, 0, 0, n, 0};
    int rc = rpkt_gpu_build_batch(&bi, d_rin, fill, built, nullptr);
    if (rc == RPKT_OK) rc = rpkt_gpu_build_tunnel_batch(&bo, d_rout, d_tb, fill, built + n, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "build failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }
    // each frame into its chain's mbufs
    for (uint32_t i = 0; i < n; i++) {
        uint32_t at = off_outer[i];
        for (uint32_t r = 0; r < rooms; r++) {
            const uint32_t s = i * rooms + r;
            HIP_OK(hipMemcpy(arena + segs_host[2 * s], frames + at, segs_host[2 * s + 1],
                             hipMemcpyDeviceToDevice));
            at += segs_host[2 * s + 1];
        }
    }

    // parse the chains, cut them, parse the flat output: one stream, no host step
    const rpkt_chains_t c = {arena, arena_bytes, segs, chain_first, n_segs, n};
    const rpkt_batch_t ob = {out, out_bytes, out_offsets, 0, 0, out_cap, 0};
    rc = rpkt_gpu_parse_tunnel_chains(&c, sums, outer, tun, inner, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_segment_tunnel_chains(&c, outer, tun, inner, mss, 0, out, out_bytes,
                                            out_offsets, out_cap, seg_first, totals, ws, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_parse_tunnel_batch(&ob, sums, o_outer, o_tun, o_inner, nullptr, 0, nullptr);
    if (rc != RPKT_OK || hipDeviceSynchronize() != hipSuccess) {
        fprintf(stderr, "failed rc=%d hip=%d\n", rc, rpkt_gpu_last_hip_error());
        return 1;
    }

    std::vector<uint8_t> h_built(2 * n), wire(out_bytes);
    std::vector<rpkt_rec_t> h_outer(n), h_inner(n), s_outer(out_cap), s_inner(out_cap);
    std::vector<rpkt_tun_t> h_tun(n), s_tun(out_cap);
    std::vector<uint32_t> first(n + 1), offs(out_cap + 1);
    uint64_t tot[2];
    HIP_OK(hipMemcpy(h_built.data(), built, 2 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_outer.data(), outer, n * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_inner.data(), inner, n * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_tun.data(), tun, n * tb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(s_outer.data(), o_outer, out_cap * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(s_inner.data(), o_inner, out_cap * rb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(s_tun.data(), o_tun, out_cap * tb, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first.data(), seg_first, (n + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs.data(), out_offsets, (out_cap + 1) * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(wire.data(), out, out_bytes, hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    bool ok = tot[0] == n_out && tot[1] == need && offs[0] == 0 && first[n] == n_out;
    uint32_t bad_sums = 0, bad_fields = 0, bad_bytes = 0;
    for (uint32_t i = 0; i < n; i++) {
        const rpkt_rec_t &O = h_outer[i], &I = h_inner[i];
        const rpkt_tun_t& T = h_tun[i];
        printf("in  %u: %s / %s vni=%u / %s pkt_len=%u in %u mbufs, inner payload=%u sums outer "
               "0x%04x 0x%04x inner 0x%04x 0x%04x -> outputs [%u, %u)\n", i,
               rpkt_gpu_status_name(O.status),
               T.kind == RPKT_TUN_VXLAN && T.status == RPKT_T_OK ? "VXLAN" : "?", T.id,
               rpkt_gpu_status_name(I.status), O.frame_len, rooms, I.payload_len, O.ip_sum, O.l4_sum,
               I.ip_sum, I.l4_sum, first[i], first[i + 1]);
        ok = ok && h_built[i] == 1 && h_built[n + i] == 1 && O.status == RPKT_S_OK &&
             T.kind == RPKT_TUN_VXLAN && T.status == RPKT_T_OK && I.status == RPKT_S_OK &&
             O.frame_len == flen && I.payload_len == payload && O.ip_sum == 0xffff &&
             O.l4_sum == 0xffff && I.ip_sum == 0xffff && I.l4_sum == 0xffff &&
             first[i] == i * per && first[i + 1] == (i + 1) * per;
        for (uint32_t k = 0; k < per; k++) {
            const uint32_t j = i * per + k, p = k + 1 < per ? mss : payload - (per - 1) * mss;
            const rpkt_rec_t &so = s_outer[j], &si = s_inner[j];
            const rpkt_tun_t& st = s_tun[j];
            if (!(so.ip_sum == 0xffff && so.l4_sum == 0xffff && si.ip_sum == 0xffff && si.l4_sum == 0xffff))
                bad_sums++;
            if (!(so.status == RPKT_S_OK && st.kind == RPKT_TUN_VXLAN && st.status == RPKT_T_OK &&
                  st.id == 5000 + i && si.status == RPKT_S_OK && si.payload_len == p &&
                  so.frame_len == hdr + p && offs[j + 1] - offs[j] == hdr + p &&
                  so.ip_packet_len == so.frame_len - 14 && so.l4_word6 == so.frame_len - 34 &&
                  so.ip_ident == (uint16_t)(r_outer[i].ip_ident + k) &&
                  si.ip_ident == (uint16_t)(r_inner[i].ip_ident + k) &&
                  si.tcp_seq == r_inner[i].tcp_seq + k * mss &&
                  ((si.l4_word6 & 0x08) != 0) == (k + 1 == per) && (si.l4_word6 & 0x10) != 0 &&
                  so.src_port == r_outer[i].src_port && si.src_port == r_inner[i].src_port)) {
                bad_fields++;
                continue;
            }
            // most wire frames carry payload from two mbufs
            const uint8_t* want = host.data() + off_outer[i] + hdr + k * mss;
            if (memcmp(wire.data() + offs[j] + hdr, want, p) != 0) bad_bytes++;
        }
    }
    for (uint32_t j = n_out; j < out_cap; j++)                    // the spare slots: empty frames
        ok = ok && s_outer[j].frame_len == 0 && offs[j + 1] == tot[1];
    printf("out: %llu frames, %llu bytes; segments with a sum that does not verify: %u, with a "
           "wrong field: %u, with wrong payload bytes: %u\n", (unsigned long long)tot[0],
           (unsigned long long)tot[1], bad_sums, bad_fields, bad_bytes);
    ok = ok && bad_sums == 0 && bad_fields == 0 && bad_bytes == 0;
    printf("%s\n", ok ? "ok: 92 segments of 4 VXLAN chains of 16 mbufs, all four sums valid"
                      : "MISMATCH");
    (void)hipFree(frames); (void)hipFree(arena); (void)hipFree(out); (void)hipFree(built);
    (void)hipFree(d_rin); (void)hipFree(d_rout); (void)hipFree(outer); (void)hipFree(inner);
    (void)hipFree(o_outer); (void)hipFree(o_inner); (void)hipFree(d_tb); (void)hipFree(tun);
    (void)hipFree(o_tun); (void)hipFree(d_oo); (void)hipFree(segs); (void)hipFree(chain_first);
    (void)hipFree(out_offsets); (void)hipFree(seg_first); (void)hipFree(totals); (void)hipFree(ws);
    return ok ? 0 : 1;
}
