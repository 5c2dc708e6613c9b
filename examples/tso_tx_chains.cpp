// tso_tx_chains.cpp — the super-frame of rpkt-dpdk/examples/tso_tx.rs as the mbuf chain the
// reference really hands to the port, through the C ABI only (include/rpkt_gpu.h).
// build_tcp_packet (tso_tx.rs:47-78) calls Mbuf::from_slice on the 4000-byte payload and
// then extend_front(54) for the headers.  Checked against rpkt-dpdk/src/mbuf.rs: a fresh mbuf
// has data_off = head_room (128) in a buffer of data_room + head_room (2048 + 128 = 2176)
// bytes (:549-552), capacity() is buf_len - data_off = 2048 (:29-31), from_slice puts the
// first `cap` bytes into the first mbuf and the rest into further ones (:301-312, 261-296),
// and extend_front moves data_off down (:103).  So segment 0 is 54 header bytes in the
// headroom plus 2048 payload bytes, at byte 128 - 54 = 74 of its slot, and segment 1 the
// remaining 1952 bytes at byte 128 of its own slot.  The port has the multi-segment offload
// and cuts that chain; here the chain stays in HBM: rpkt_gpu_parse_chains locates the
// headers, rpkt_gpu_segment_chains cuts the chain at mss 1024 into flat wire frames, and a
// parse of the output with both sums plays the receiving port's RX checksum offload.
//   hipcc -O2 -Iinclude examples/tso_tx_chains.cpp -Lrpkt_amd/_build -lrpkt_gpu \
//         -Wl,-rpath,$PWD/rpkt_amd/_build -o examples/tso_tx_chains && ./examples/tso_tx_chains
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

static void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }
static void put32(uint8_t* p, uint32_t v) { put16(p, v >> 16); put16(p + 2, v & 0xffff); }

int main() {
    const uint32_t hdr = 14 + 20 + 20, payload = 4000, mss = 1024, out_cap = 8;
    const uint32_t head_room = 128, data_room = 2048, slot = head_room + data_room;
    const uint64_t out_bytes = 8192;
    const uint32_t seq0 = 0x8e501902u;

    // two mempool slots; the chain takes the second one first, as a pool hands them out
    std::vector<uint8_t> arena(2 * slot + 16, 0x11);
    const uint32_t seg0 = 1 * slot + head_room - hdr, len0 = hdr + data_room;
    const uint32_t seg1 = 0 * slot + head_room, len1 = payload - data_room;
    memset(arena.data() + seg0 + hdr, 0xae, data_room);           // PAYLOAD_BYTE x PAYLOAD_LEN
    memset(arena.data() + seg1, 0xae, len1);
    // the header values of tso_tx.rs:36-75; the checksums are left to the offload (zero)
    uint8_t* h = arena.data() + seg0;
    memset(h, 0, hdr);
    const uint8_t dmac[6] = {0xac, 0xdc, 0xca, 0x79, 0xe5, 0xc6};
    const uint8_t smac[6] = {0xac, 0xdc, 0xca, 0x79, 0xca, 0x86};
    memcpy(h, dmac, 6);
    memcpy(h + 6, smac, 6);
    put16(h + 12, 0x0800);
    uint8_t* ip = h + 14;
    ip[0] = 0x45;
    put16(ip + 2, 20 + 20 + payload);
    ip[8] = 128;
    ip[9] = 6;
    const uint8_t sip[4] = {172, 0, 10, 17}, dip[4] = {192, 168, 23, 2};
    memcpy(ip + 12, sip, 4);
    memcpy(ip + 16, dip, 4);
    uint8_t* tcp = ip + 20;
    put16(tcp, 60376);
    put16(tcp + 2, 161);
    put32(tcp + 4, seq0);
    put32(tcp + 8, 0xc7529d89u);
    tcp[12] = 0x50;
    tcp[13] = 0x10 | 0x08;                                        // ACK, PSH
    put16(tcp + 14, 46);
    const uint32_t segs_host[4] = {seg0, len0, seg1, len1};
    const uint32_t first_host[2] = {0, 2};

    uint8_t *buf = nullptr, *out = nullptr;
    uint32_t *segs = nullptr, *chain_first = nullptr, *out_offsets = nullptr, *seg_first = nullptr;
    rpkt_rec_t *recs = nullptr, *out_recs = nullptr;
    uint64_t* totals = nullptr;
    void* ws = nullptr;
    HIP_OK(hipMalloc(&buf, arena.size()));
    HIP_OK(hipMalloc(&out, out_bytes));
    HIP_OK(hipMalloc(&segs, sizeof(segs_host)));
    HIP_OK(hipMalloc(&chain_first, sizeof(first_host)));
    HIP_OK(hipMalloc(&recs, sizeof(rpkt_rec_t)));
    HIP_OK(hipMalloc(&out_recs, out_cap * sizeof(rpkt_rec_t)));
    HIP_OK(hipMalloc(&out_offsets, (out_cap + 1) * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&seg_first, 2 * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&totals, 2 * sizeof(uint64_t)));
    HIP_OK(hipMalloc(&ws, rpkt_gpu_segment_chains_workspace_bytes(1) + 16));
    HIP_OK(hipMemcpy(buf, arena.data(), arena.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(segs, segs_host, sizeof(segs_host), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(chain_first, first_host, sizeof(first_host), hipMemcpyHostToDevice));

    // parse the chain, segment it, parse the flat output: one stream, no host step
    const rpkt_chains_t c = {buf, arena.size(), segs, chain_first, 2, 1};
    int rc = rpkt_gpu_parse_chains(&c, 0, recs, nullptr, 0, nullptr);
    if (rc == RPKT_OK)
        rc = rpkt_gpu_segment_chains(&c, recs, mss, 0, out, out_bytes, out_offsets, out_cap,
                                     seg_first, totals, ws, nullptr);
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
    std::vector<uint8_t> wire(out_bytes);
    HIP_OK(hipMemcpy(&in, recs, sizeof(in), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(seg, out_recs, sizeof(seg), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tot, totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(first, seg_first, sizeof(first), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(offs, out_offsets, sizeof(offs), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(wire.data(), out, out_bytes, hipMemcpyDeviceToHost));

    printf("%s\n", rpkt_gpu_build_info());
    printf("in : %s pkt_len=%u in segments of %u + %u, payload=%u seq=0x%08x flags=0x%02x\n",
           rpkt_gpu_status_name(in.status), in.frame_len, len0, len1, in.payload_len, in.tcp_seq,
           in.l4_word6 & 0xff);
    printf("out: %llu frames, %llu bytes; chain 0 -> outputs [%u, %u)\n",
           (unsigned long long)tot[0], (unsigned long long)tot[1], first[0], first[1]);
    const uint32_t want[4] = {1024, 1024, 1024, 928};
    bool ok = in.status == RPKT_S_OK && in.frame_len == hdr + payload && in.payload_len == payload &&
              tot[0] == 4 && tot[1] == payload + 4 * hdr && first[0] == 0 && first[1] == 4 &&
              offs[0] == 0;
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
             s.frame_len == hdr + want[k] && s.tcp_seq == seq0 + k * mss && s.ip_ident == k &&
             ((s.l4_word6 & 0x08) != 0) == (k == 3) && (s.l4_word6 & 0x10) != 0 &&
             s.ip_sum == 0xffff && s.l4_sum == 0xffff && s.src_port == 60376 && s.dst_port == 161;
        // the third wire frame's payload crosses from segment 0 into segment 1
        for (uint32_t x = offs[k] + hdr; ok && x < offs[k + 1]; x++) ok = wire[x] == 0xae;
    }
    printf("%s\n", ok ? "ok: 4 segments from a 2-segment chain, sums valid" : "MISMATCH");
    (void)hipFree(buf); (void)hipFree(out); (void)hipFree(segs); (void)hipFree(chain_first);
    (void)hipFree(recs); (void)hipFree(out_recs); (void)hipFree(out_offsets); (void)hipFree(seg_first);
    (void)hipFree(totals); (void)hipFree(ws);
    return ok ? 0 : 1;
}
