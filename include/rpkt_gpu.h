/*
 * rpkt_gpu.h — C ABI of the MI355X packet-batch parse + checksum engine.
 *
 * This is the drop-in boundary for rpkt's Ether -> (802.1Q/802.1ad)* -> IPv4 ->
 * {TCP, UDP} decode-and-verify path.  rpkt itself has no FFI for this path: its
 * "operator API" is the generic header views over `T: Buf`
 *   EtherFrame::parse      rpkt/src/ether/generated.rs:34-41
 *   VlanFrame::parse       rpkt/src/vlan/generated.rs:32-39
 *   Ipv4::parse            rpkt/src/ipv4/generated.rs:35-51
 *   Udp::parse             rpkt/src/udp/generated.rs:31-42
 *   Tcp::parse             rpkt/src/tcp/generated.rs:34-45
 *   checksum::from_slice   rpkt/src/checksum.rs:33-62
 *   checksum::combine      rpkt/src/checksum.rs:68-74
 * which a caller drives one frame at a time (benches/rpkt/rpkt_parse.rs:62-80,
 * rpkt-dpdk/examples/loopback_rx.rs:96-121).  The entry points below replace that
 * per-frame loop with one call over a device-resident batch of frames, and return
 * one fixed-size record per frame holding every getter value the chain above
 * exposes, the parse outcome and the raw RFC 1071 sums.
 *
 * Conventions (no HIP/torch types cross this header):
 *   - every pointer named *_dev is device memory owned by the caller;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - calls are asynchronous on `stream` and never allocate or synchronise;
 *   - API-level failures are negative return codes; per-frame parse failures are
 *     never errors, they are reported in rpkt_rec_t.status.
 */
#ifndef RPKT_GPU_H
#define RPKT_GPU_H

#include <stddef.h>

#include "rpkt_protocols.h"
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPKT_ABI_VERSION 1u

/* ---- per-frame status: which rpkt `parse` would return Err (first one) ----
 * The chain is EtherFrame::parse -> while ethertype in {VLAN, QINQ}:
 * VlanFrame::parse -> (ethertype == IPV4) -> Ipv4::parse -> protocol dispatch ->
 * Udp::parse | Tcp::parse.  At most RPKT_MAX_VLAN tags are walked; a further
 * tag leaves the dispatch ethertype at 0x8100/0x88a8 -> RPKT_S_NOT_IPV4. */
enum rpkt_status {
    RPKT_S_OK = 0,              /* Udp::parse or Tcp::parse returned Ok           */
    RPKT_S_ETH_SHORT = 1,       /* chunk_len < 14     ether/generated.rs:36        */
    RPKT_S_VLAN_SHORT = 2,      /* chunk_len < 4      vlan/generated.rs:34         */
    RPKT_S_NOT_IPV4 = 3,        /* ethertype != 0x0800 (caller check, rpkt_parse.rs:66) */
    RPKT_S_IP_SHORT = 4,        /* chunk_len < 20     ipv4/generated.rs:37         */
    RPKT_S_IP_BAD_IHL = 5,      /* header_len < 20    ipv4/generated.rs:43         */
    RPKT_S_IP_IHL_GT_LEN = 6,   /* header_len > chunk_len   ipv4/generated.rs:44   */
    RPKT_S_IP_TOT_LT_IHL = 7,   /* packet_len < header_len  ipv4/generated.rs:45   */
    RPKT_S_IP_TOT_GT_LEN = 8,   /* packet_len > remaining   ipv4/generated.rs:46   */
    RPKT_S_L4_OTHER = 9,        /* IPv4 ok, protocol not TCP(6)/UDP(17)            */
    RPKT_S_UDP_SHORT = 10,      /* chunk_len < 8      udp/generated.rs:33          */
    RPKT_S_UDP_BAD_LEN = 11,    /* len < 8 || len > remaining  udp/generated.rs:38 */
    RPKT_S_TCP_SHORT = 12,      /* chunk_len < 20     tcp/generated.rs:36          */
    RPKT_S_TCP_BAD_DOFF = 13,   /* hlen < 20 || hlen > chunk_len  tcp/generated.rs:41 */
    /* IPv6 (RPKT_F_IPV6 only): ethertype 0x86DD -> Ipv6::parse -> extension headers */
    RPKT_S_IP6_SHORT = 14,      /* chunk_len < 40     ipv6/generated.rs:42         */
    RPKT_S_IP6_BAD_LEN = 15,    /* payload_len + 40 > remaining  ipv6/generated.rs:47 */
    RPKT_S_IP6_EXT_SHORT = 16,  /* extension header: chunk_len < its fixed size
                                   (2 HopByHop/DestOptions, 8 Routing/Fragment, 12 AH;
                                   ipv6/generated.rs:243,386,530,698,852)          */
    RPKT_S_IP6_EXT_BAD_LEN = 17,/* extension header: header_len < min or > chunk_len
                                   (ipv6/generated.rs:248,391,535,857)             */
    RPKT_S_IP6_FRAGMENT = 18,   /* a Fragment header with offset != 0 or M set: the
                                   upper-layer header needs reassembly, not parsed */
    RPKT_S_ICMP_EMPTY = 19,     /* IPv4 parsed, protocol 1 (ICMP), empty payload: the
                                   reference's calculate_icmp_checksum panics on it
                                   (icmp_data.len() - 1 underflows,
                                   icmpv4/generated.rs:2684); otherwise as L4_OTHER */
    RPKT_S_NO_INNER = 20        /* rpkt_gpu_parse_tunnel_batch's inner record of a frame
                                   whose tunnel was not decoded (rpkt_tun_t.status != OK):
                                   every other field 0 */
};

#define RPKT_MAX_VLAN 2
/* Extension headers walked after the IPv6 header: HopByHop (0), Routing (43),
 * Fragment (44), DestOptions (60), AH (51).  A chain longer than this leaves the next
 * header at an extension type -> RPKT_S_L4_OTHER (as a third VLAN tag -> NOT_IPV4). */
#define RPKT_MAX_IP6_EXT 8

/* ---- API return codes ----
 * Every entry checks its arguments before it launches anything and returns the status of
 * the first check that fails.  The order (one set of checks, rpkt_amd/csrc/rpkt_args.h;
 * pinned case by case by tests/test_abi_status_matrix.py):
 *   batch entries (parse, compact, options, build, forward, layers): a NULL descriptor or
 *     required output (E_INVAL); unknown flags (E_INVAL); n == 0 (RPKT_OK, nothing else is
 *     looked at); NULL frames_dev (E_INVAL; forward: or n_forbid without forbid_dev);
 *     frames_bytes (E_TOO_LARGE); no layout -- offsets_dev NULL and stride 0 (E_INVAL);
 *     alignment (E_ALIGN); with RPKT_F_FLOW_EV a NULL flow_ev_dev or n_buckets outside
 *     1..RPKT_FLOW_MAX_BUCKETS (E_INVAL), then flow_ev_dev's alignment (E_ALIGN);
 *   chain entries: the same with, in the batch's place, NULL chain_first_dev / buf_dev /
 *     segs_dev (E_INVAL), then buf_bytes and n_segs (E_TOO_LARGE); segs_dev's alignment goes
 *     with the other alignments;
 *   tunnel entries (batch, chains, next, ring): only the descriptor is tested before the
 *     flags and n == 0, the record pointers after it with frames_dev;
 *   ring entries: NULL slots with n_slots > 0, the flags, then each non-empty slot in
 *     order with its batch entry's checks, all before the first launch;
 *   rpkt_gpu_segment_batch: the batch entries' order with its own arguments in their places:
 *     a NULL batch, recs_dev, output (out_frames_dev, out_offsets_dev, seg_first_dev,
 *     totals_dev) or workspace_dev (E_INVAL); flags other than 0 or RPKT_SEGMENT_UDP, then mss
 *     outside 1..65535 (E_INVAL); n == 0 (RPKT_OK); NULL frames_dev (E_INVAL); frames_bytes, then out_bytes at
 *     the same limit (E_TOO_LARGE); no layout (E_INVAL); out_cap == 0 (E_INVAL); alignment
 *     (E_ALIGN): recs_dev, out_frames_dev, workspace_dev 16 B, totals_dev 8 B;
 *   rpkt_gpu_segment_chains: rpkt_gpu_segment_batch's order with the chain entries' checks in
 *     the batch's place: a NULL chains, recs_dev, output or workspace_dev (E_INVAL); flags other
 *     than 0 or RPKT_SEGMENT_UDP, then mss outside 1..65535 (E_INVAL); n_chains == 0 (RPKT_OK); NULL
 *     chain_first_dev, or with n_segs > 0 NULL buf_dev / segs_dev (E_INVAL); buf_bytes and
 *     n_segs (E_TOO_LARGE); out_bytes (E_TOO_LARGE); out_cap == 0 (E_INVAL); alignment
 *     (E_ALIGN): segs_dev and totals_dev 8 B, recs_dev, out_frames_dev, workspace_dev 16 B;
 *   rpkt_gpu_segment_tunnel_batch: rpkt_gpu_segment_batch's order with outer_dev, tun_dev and
 *     inner_dev in recs_dev's places: each required (E_INVAL) and 16-byte aligned (E_ALIGN);
 *   rpkt_gpu_segment_tunnel_chains: rpkt_gpu_segment_chains' order with the same three in
 *     recs_dev's places;
 *   rpkt_gpu_fragment_batch: rpkt_gpu_segment_batch's order with frag_first_dev in
 *     seg_first_dev's place, flags other than 0 or RPKT_FRAGMENT_IGNORE_DF, then mtu outside
 *     1..65535 in mss's place;
 *   rpkt_gpu_fragment_chains: rpkt_gpu_segment_chains' order with frag_first_dev in
 *     seg_first_dev's place, flags other than 0 or RPKT_FRAGMENT_IGNORE_DF, then mtu outside
 *     1..65535 in mss's place;
 *   rpkt_gpu_fragment_tunnel_batch: rpkt_gpu_segment_tunnel_batch's order with frag_first_dev
 *     in seg_first_dev's place, flags with a bit other than RPKT_FRAGMENT_IGNORE_DF and
 *     RPKT_FRAGMENT_TUNNEL_OUTER, then mtu outside 1..65535 in mss's place;
 *   rpkt_gpu_coalesce_batch: rpkt_gpu_segment_batch's order with src_first_dev in
 *     seg_first_dev's place (order_dev and out_mss_dev may be NULL), flags with a bit other
 *     than RPKT_COALESCE_TRUST_SUMS and RPKT_COALESCE_UDP, then max_payload outside 1..65535 in
 *     mss's place;
 *   rpkt_gpu_coalesce_tunnel_batch: rpkt_gpu_coalesce_batch's order with outer_dev, tun_dev and
 *     inner_dev in recs_dev's places: each required (E_INVAL) and 16-byte aligned (E_ALIGN);
 *   rpkt_gpu_reassemble_batch: rpkt_gpu_coalesce_batch's order without a max_payload (order_dev
 *     may be NULL), flags other than 0 or RPKT_REASSEMBLE_TRUST_SUMS;
 *   rpkt_gpu_reassemble_keys: the batch entries' order: a NULL batch, recs_dev or keys_dev
 *     (E_INVAL); flags other than 0 or RPKT_REASSEMBLE_TRUST_SUMS (E_INVAL); n == 0 (RPKT_OK);
 *     NULL frames_dev (E_INVAL); frames_bytes (E_TOO_LARGE); no layout (E_INVAL); alignment
 *     (E_ALIGN): recs_dev 16 B, keys_dev 8 B.
 * Where an entry leaves that order (kept as it is, callers may rely on it):
 *   rpkt_gpu_parse_tunnel_batch and each slot of rpkt_gpu_parse_tunnel_ring test the flow
 *     events first, before n == 0: an empty batch with RPKT_F_FLOW_EV and no event buffer is
 *     E_INVAL there (an empty slot of a ring is skipped before it) and RPKT_OK from
 *     rpkt_gpu_parse_batch;
 *   rpkt_gpu_parse_tunnel_next tests the layout, then that no output aliases its input,
 *     before frames_bytes;
 *   rpkt_gpu_fields_batch tests n_req and every request before n == 0;
 *   rpkt_gpu_parse_options_batch[_compact] tests opts_dev's alignment last, after the flow
 *     events;
 *   rpkt_gpu_parse_ring[_compact] tests n_buckets (RPKT_F_FLOW_EV) first in each non-empty
 *     slot, before the slot's pointers, and the slot's flow_ev_dev last. */
enum rpkt_err {
    RPKT_OK = 0,
    RPKT_E_INVAL = -1,       /* NULL pointer / zero stride / bad flags            */
    RPKT_E_HIP = -2,         /* a HIP runtime call failed (see rpkt_gpu_last_hip_error) */
    RPKT_E_TOO_LARGE = -3,   /* frames_bytes >= 4 GiB: split the batch             */
    RPKT_E_ALIGN = -4,       /* out/flow buffer not 16-byte aligned               */
    RPKT_E_COLL = -5         /* an RCCL call failed (see rpkt_gpu_last_coll_error) */
};

/* ---- flags for rpkt_gpu_parse_batch ---- */
enum rpkt_flags {
    RPKT_F_IP_SUM = 1u,      /* compute ip_sum = from_slice(ipv4 header[0..ihl4])  */
    RPKT_F_L4_SUM = 2u,      /* compute l4_sum = combine(pseudo, from_slice(l4))    */
    RPKT_F_FLOW_EV = 4u,     /* also write one rpkt_flow_ev_t per frame             */
    RPKT_F_IPV6 = 8u         /* also decode and verify IPv6 (ethertype 0x86DD); without
                                it such frames stop at RPKT_S_NOT_IPV4 as before      */
};

/* Record layout: 80 bytes, 16-byte aligned, little-endian host order.
 * Field  <-> rpkt getter (all getters of the path are recoverable exactly):
 *   ethertype          EtherFrame::ethertype          ether/generated.rs:55-59
 *   dst_addr/src_addr  EtherFrame::{dst,src}_addr     ether/generated.rs:47-54
 *   vlan_tci[i]        be16[0..2] of tag i: priority = tci>>13, dei = tci&0x1000,
 *                      vlan_id = tci&0xfff            vlan/generated.rs:45-56
 *   vlan_ethertype[i]  VlanFrame::ethertype           vlan/generated.rs:57-61
 *   ip_vhl             byte 0: version = >>4, header_len = (&0xf)*4
 *   ip_tos             byte 1: dscp = >>2, ecn = &3
 *   ip_frag            be16[6..8]: flag_reserved = >>15, dont_frag = &0x4000,
 *                      more_frag = &0x2000, frag_offset = &0x1fff
 *                      (Ipv4 getters ipv4/generated.rs:61-112, 269-288)
 *   l4_word6           TCP: be16[12..14] (header_len = (>>12)*4, reserved =
 *                      (>>8)&0xf, flags = &0xff); UDP: packet_len be16[4..6]
 *   l4_checksum        TCP be16[16..18] / UDP be16[6..8]
 *   tcp_*              Tcp getters tcp/generated.rs:55-122
 *   l3_off             frame offset of the IPv4 header (EtherFrame/VlanFrame::payload)
 *   l4_off             frame offset of Ipv4::payload() (trimmed to packet_len)
 *   payload_off/_len   Udp::payload() / Tcp::payload() when status == OK,
 *                      otherwise Ipv4::payload() when IPv4 parsed
 *   ip_sum             checksum::from_slice(ipv4[0..header_len]); 0xffff <=> valid
 *   l4_sum             checksum::combine(&[pseudo(src,dst,proto,l4_len),
 *                      from_slice(l4[0..l4_len])]); 0xffff <=> valid
 *                      Status L4_OTHER (RPKT_F_L4_SUM), no pseudo header:
 *                      - IPv4 protocol 1 (ICMP): from_slice over the whole IPv4 payload
 *                        [l4_off, l3_off + packet_len); the reference's
 *                        calculate_icmp_checksum (icmpv4/generated.rs:2678-2701) over the
 *                        same bytes is !l4_sum, so 0xffff <=> it returns 0 (a valid
 *                        message, icmpv4_test.rs:82-96); an empty payload is
 *                        RPKT_S_ICMP_EMPTY, not summed;
 *                      - protocol / next header 47 (GRE) with the checksum-present bit
 *                        (byte 0 & 0x80, gre/generated.rs:55) and >= 4 payload bytes:
 *                        from_slice over the GRE header and its payload (RFC 2784 section
 *                        2.5; Gre::checksum, gre/generated.rs:239): 0xffff <=> valid.
 *                      (These are the sums of the outer layer only: a frame whose l4_sum
 *                      is one of them keeps status L4_OTHER, so the compact verdict bit 1
 *                      and the flow event's bit 49 do not cover them.)
 * Fields of layers that were not reached are zero.  Sums not requested by the
 * flags, or whose layer did not parse, are zero.
 *
 * IPv6 frames (RPKT_F_IPV6, dispatch ethertype 0x86DD: `ethertype`, or
 * vlan_ethertype[n_vlan-1] when tagged) use bytes 24..43 as the IPv6 block below
 * instead of the IPv4 fields; everything else keeps its meaning.  Chain:
 * Ipv6::parse (ipv6/generated.rs:40-51) -> Ipv6::payload (trim to payload_len,
 * advance 40, :83-92) -> up to RPKT_MAX_IP6_EXT extension headers, each its parse and
 * payload() (DestOptions :241-279, HopByHopOption :384-421, RoutingHeader :528-577,
 * FragmentHeader :696-739, AuthenticationHeader :850-899) -> Udp|Tcp::parse.
 *   24 u32 ip6_vtcfl     be32 of bytes 0..3: version = >>28, traffic_class =
 *                        (>>20)&0xff, flow_label = &0xfffff     (:57-67)
 *   28 u16 ip6_payload_len                                      (:77-79)
 *   30 u8  ip6_next_header   the IPv6 header's next_header       (:69-71)
 *   31 u8  ip6_hop_limit                                         (:73-75)
 *   32 u8  ip6_n_ext     extension headers walked
 *   33 u8  ip_protocol   the upper-layer protocol: the next_header where the walk
 *                        stopped (the extension type that failed for IP6_EXT_*,
 *                        the Fragment header's next_header for IP6_FRAGMENT)
 *   34 u16 ip6_pdst_off  frame offset of the 16-B address the L4 pseudo header uses
 *                        as destination: dst_addr (l3 + 24), or, after a Routing
 *                        header with segments_left > 0 (RFC 8200 section 8.1), its
 *                        final address -- the last of the list for types 0 and 2, the
 *                        first (Segment List[0]) for type 4; other types keep dst_addr
 *   36 u32 ip6_src_fold  src_addr as four be32 words XORed (the flow key)
 *   40 u32 ip6_dst_fold  dst_addr likewise (src_addr/dst_addr themselves: frame bytes
 *                        l3_off + 8 and l3_off + 24, or rpkt_gpu_fields_batch)
 * l4_off = the cursor after the extension headers (the header where the walk stopped);
 * payload_off/_len = Udp/Tcp::payload() when status == OK, otherwise [l4_off, end of
 * the trimmed IPv6 payload).  ip_sum = 0 (IPv6 has no header checksum).  l4_sum =
 * combine(&[pseudo_v6(src, pdst, u32 l4_len, next header), from_slice(l4)]); a UDP
 * checksum of 0 is NOT "not computed" over IPv6 (RFC 8200 section 8.1). */
typedef struct rpkt_rec {
    uint8_t  status;            /*  0 enum rpkt_status                          */
    uint8_t  n_vlan;            /*  1 tags walked, 0..RPKT_MAX_VLAN             */
    uint16_t ethertype;         /*  2                                           */
    uint8_t  dst_addr[6];       /*  4                                           */
    uint8_t  src_addr[6];       /* 10                                           */
    uint16_t vlan_tci[2];       /* 16                                           */
    uint16_t vlan_ethertype[2]; /* 20                                           */
    uint8_t  ip_vhl;            /* 24                                           */
    uint8_t  ip_tos;            /* 25                                           */
    uint16_t ip_packet_len;     /* 26                                           */
    uint16_t ip_ident;          /* 28                                           */
    uint16_t ip_frag;           /* 30                                           */
    uint8_t  ip_ttl;            /* 32                                           */
    uint8_t  ip_protocol;       /* 33                                           */
    uint16_t ip_checksum;       /* 34                                           */
    uint32_t ip_src;            /* 36 a.b.c.d -> (a<<24)|(b<<16)|(c<<8)|d        */
    uint32_t ip_dst;            /* 40                                           */
    uint16_t src_port;          /* 44                                           */
    uint16_t dst_port;          /* 46                                           */
    uint32_t tcp_seq;           /* 48                                           */
    uint32_t tcp_ack;           /* 52                                           */
    uint16_t l4_word6;          /* 56                                           */
    uint16_t tcp_window;        /* 58                                           */
    uint16_t l4_checksum;       /* 60                                           */
    uint16_t tcp_urgent;        /* 62                                           */
    uint16_t l3_off;            /* 64                                           */
    uint16_t l4_off;            /* 66                                           */
    uint16_t payload_off;       /* 68                                           */
    uint16_t payload_len;       /* 70                                           */
    uint16_t ip_sum;            /* 72                                           */
    uint16_t l4_sum;            /* 74                                           */
    uint32_t frame_len;         /* 76 Cursor::remaining() of the whole frame    */
} rpkt_rec_t;

#define RPKT_REC_BYTES 80u

/* Per-frame flow event (RPKT_F_FLOW_EV), 8 bytes:
 *   bits  0..31  frame_len
 *   bits 32..47  flow bucket = rpkt_flow_hash(5-tuple) % n_buckets (status OK),
 *                n_buckets for frames that did not parse to L4
 *   bit  48      ip header sum != 0xffff (IPv4 header parsed; never for IPv6)
 *   bit  49      l4 sum != 0xffff (an IPv4 UDP checksum field of 0 counts as valid)
 * IPv6 frames hash ip6_src_fold / ip6_dst_fold in place of the IPv4 addresses.
 * Counters (rpkt_gpu_flow_count) are u64[(n_buckets + 1) * 4]:
 *   row b = {pkts, bytes, ip_bad, l4_bad}; row n_buckets = unparsed frames. */
typedef uint64_t rpkt_flow_ev_t;
#define RPKT_FLOW_MAX_BUCKETS 65535u

/* Frame batch descriptor.  Frame i is [off_i, off_i + len_i) of `frames_dev`:
 *   packed  (offsets_dev != NULL): off_i = offsets[i], len_i = offsets[i+1] - offsets[i]
 *                                  (n + 1 entries, non-decreasing);
 *   strided (offsets_dev == NULL): off_i = i * stride, len_i = frame_len (0 -> stride).
 * Loads are bounds-checked in hardware against frames_bytes, so a malformed
 * descriptor yields wrong records, never a fault.  frames_bytes < 4 GiB. */
typedef struct rpkt_batch {
    const uint8_t*  frames_dev;
    uint64_t        frames_bytes;
    const uint32_t* offsets_dev;
    uint32_t        stride;
    uint32_t        frame_len;
    uint32_t        n;
    uint32_t        reserved;
} rpkt_batch_t;

/* ABI version and build information (host-only, no device calls). */
uint32_t rpkt_gpu_abi_version(void);
const char* rpkt_gpu_build_info(void);
const char* rpkt_gpu_status_name(int status);
/* Last HIP error code seen by this thread (hipError_t as int), 0 if none. */
int rpkt_gpu_last_hip_error(void);
/* Human-readable runtime/device description into buf (diagnostics). */
int rpkt_gpu_device_info(char* buf, size_t len);

/* Parse + verify a batch.  Replaces, per frame i, the reference sequence
 *   EtherFrame::parse -> [VlanFrame::parse]* -> Ipv4::parse -> Udp|Tcp::parse
 * plus the checksum composition selected by `flags`, writing recs_dev[i]
 * (n * 80 bytes, 16-byte aligned).  flow_ev_dev (n * 8 bytes) is written when
 * RPKT_F_FLOW_EV is set, using n_buckets (1..RPKT_FLOW_MAX_BUCKETS). */
int rpkt_gpu_parse_batch(const rpkt_batch_t* batch, uint32_t flags,
                         rpkt_rec_t* recs_dev, rpkt_flow_ev_t* flow_ev_dev,
                         uint32_t n_buckets, void* stream);

/* Compact record: 16 bytes, the projection of rpkt_rec_t a caller needs to locate the
 * layers and read the verdicts, for receive loops that read getters from the frame
 * itself (rpkt's views hold only the buffer and read fields lazily,
 * ipv4/generated.rs:17-20).  Fields equal the rpkt_rec_t fields of the same name;
 * verdict bit 0 = RPKT_F_IP_SUM requested and ip_sum == 0xffff (IPv6: requested and
 * the IPv6 header parsed -- it carries no checksum), bit 1 = RPKT_F_L4_SUM requested,
 * status OK and (l4_sum == 0xffff or, IPv4 only, a UDP checksum field of 0: "not
 * computed"), bit 2 = the frame was dispatched to Ipv6::parse (RPKT_F_IPV6). */
typedef struct rpkt_rec16 {
    uint8_t  status;            /*  0 enum rpkt_status                          */
    uint8_t  n_vlan;            /*  1                                           */
    uint8_t  ip_protocol;       /*  2                                           */
    uint8_t  verdict;           /*  3 bit 0 IPv4 header sum ok, bit 1 L4 sum ok */
    uint16_t l3_off;            /*  4                                           */
    uint16_t l4_off;            /*  6                                           */
    uint16_t payload_off;       /*  8                                           */
    uint16_t payload_len;       /* 10                                           */
    uint16_t ip_sum;            /* 12                                           */
    uint16_t l4_sum;            /* 14                                           */
} rpkt_rec16_t;

#define RPKT_REC16_BYTES 16u

/* rpkt_gpu_parse_batch writing rpkt_rec16_t records (recs_dev n * 16 B, 16-byte
 * aligned): the same parse, sums and flow events, one fifth of the record bytes. */
int rpkt_gpu_parse_batch_compact(const rpkt_batch_t* batch, uint32_t flags,
                                 rpkt_rec16_t* recs_dev, rpkt_flow_ev_t* flow_ev_dev,
                                 uint32_t n_buckets, void* stream);

/* A receive ring's slots (a NIC ring's bursts, rpkt-dpdk/examples/loopback_rx.rs:96-121)
 * parsed in one launch per RPKT_RING_MAX_SLOTS slots: results equal one
 * rpkt_gpu_parse_batch call per slot (records into each slot's recs_dev, flow events into
 * its flow_ev_dev when RPKT_F_FLOW_EV is set), but small batches no longer pay a
 * dependent kernel launch each.  Slots with n == 0 are skipped; every slot is checked
 * before anything is launched.  Layouts may differ from slot to slot.  recs_dev points to
 * rpkt_rec_t records for rpkt_gpu_parse_ring and to rpkt_rec16_t records for
 * rpkt_gpu_parse_ring_compact (equal to rpkt_gpu_parse_batch_compact per slot). */
typedef struct rpkt_ring_slot {
    rpkt_batch_t    batch;
    void*           recs_dev;
    rpkt_flow_ev_t* flow_ev_dev;
} rpkt_ring_slot_t;
#define RPKT_RING_MAX_SLOTS 32u
int rpkt_gpu_parse_ring(const rpkt_ring_slot_t* slots, uint32_t n_slots, uint32_t flags,
                        uint32_t n_buckets, void* stream);
int rpkt_gpu_parse_ring_compact(const rpkt_ring_slot_t* slots, uint32_t n_slots, uint32_t flags,
                                uint32_t n_buckets, void* stream);

/* Accumulate flow events into counters_dev (u64[(n_buckets+1)*4], caller
 * zeroes it once; calls add).  workspace_dev must hold
 * rpkt_gpu_flow_workspace_bytes(n, n_buckets) bytes.  Calls that add into the
 * same counters (or share a workspace) must be ordered, e.g. on one stream: up
 * to 8192 buckets each bucket is added by one thread without atomics, so the
 * counters are bitwise reproducible. */
size_t rpkt_gpu_flow_workspace_bytes(uint32_t n, uint32_t n_buckets);
int rpkt_gpu_flow_count(const rpkt_flow_ev_t* flow_ev_dev, uint32_t n,
                        uint32_t n_buckets, uint64_t* counters_dev,
                        void* workspace_dev, void* stream);

/* Sum the flow counters of every rank (the path's only collective):
 * one RCCL ncclAllReduce (root == -1) or ncclReduce to rank `root` of
 * u64[(n_buckets+1)*4] in place, ncclUint64 / ncclSum, on `nccl_comm` (an
 * ncclComm_t passed as void*) and `stream`.  Asynchronous like every call here.
 * Replaces the per-queue counters a DPDK receive thread keeps and the final sum
 * over threads (rpkt-dpdk/examples/loopback_tx.rs:176-181, rss_rx.rs:54-113).
 * counters_dev 8-byte aligned.  RPKT_E_COLL: rpkt_gpu_last_coll_error() holds the
 * ncclResult_t. */
int rpkt_gpu_flow_reduce(uint64_t* counters_dev, uint32_t n_buckets, int root, void* nccl_comm,
                         void* stream);
/* Last ncclResult_t seen by this thread (0 if none); RCCL version (ncclGetVersion). */
int rpkt_gpu_last_coll_error(void);
int rpkt_gpu_coll_version(void);

/* A communicator the library makes itself, so a host need not take one from another
 * runtime (torch's ProcessGroupNCCL) for rpkt_gpu_flow_reduce: rank 0 calls
 * rpkt_gpu_coll_unique_id (ncclGetUniqueId) and hands the RPKT_COLL_ID_BYTES bytes to
 * every rank by any channel (the reference's receive threads share memory; ranks of
 * one host here use the torch group, an MPI broadcast or a file), then every rank
 * calls rpkt_gpu_comm_init (ncclCommInitRank on its current HIP device; collective:
 * it returns when all `world` ranks have joined) and, when done,
 * rpkt_gpu_comm_destroy.  *comm_out is an ncclComm_t as void*. */
#define RPKT_COLL_ID_BYTES 128
int rpkt_gpu_coll_unique_id(uint8_t* id_out);
int rpkt_gpu_comm_init(void** comm_out, int world, const uint8_t* id, int rank);
int rpkt_gpu_comm_destroy(void* comm);
/* rpkt_gpu_comm_init with a deadline (timeout_ms <= 0: blocking, as rpkt_gpu_comm_init):
 * a non-blocking ncclCommInitRankConfig polled with ncclCommGetAsyncError.  When not
 * every rank joins within timeout_ms (a peer failed before its init) or the init fails,
 * the half-made communicator is aborted and RPKT_E_COLL returned
 * (rpkt_gpu_last_coll_error() = 7, ncclInProgress, on a timeout), so no rank is left
 * blocked and the group can agree on a fallback.  rpkt_gpu_comm_abort (ncclCommAbort)
 * releases a communicator without waiting for its peers. */
int rpkt_gpu_comm_init_timeout(void** comm_out, int world, const uint8_t* id, int rank,
                               int timeout_ms);
int rpkt_gpu_comm_abort(void* comm);

/* Batched checksum::from_slice over byte ranges of a device buffer:
 * out_dev[i] = from_slice(buf[start_i .. start_i + len_i]) for
 * ranges_dev[i] = {start_i, len_i}.  Drop-in for rpkt/src/checksum.rs:33-62. */
int rpkt_gpu_checksum_ranges(const uint8_t* buf_dev, uint64_t buf_bytes,
                             const uint32_t* ranges_dev, uint32_t n,
                             uint16_t* out_dev, void* stream);

/* Batched checksum::from_buf over multi-segment buffers (mbuf chains, rpkt-dpdk's
 * Pbuf): chain p is segments chain_first_dev[p] .. chain_first_dev[p+1]-1 (n_chains+1
 * entries), segment i = buf[segs_dev[2i] .. segs_dev[2i] + segs_dev[2i+1]).
 * out_dev[p] = from_buf over the chain's bytes in order, pairing a segment's odd tail
 * byte with the next segment's first byte.  Drop-in for rpkt/src/checksum.rs:8-27
 * (with from_slice_with_tail_byte :77-111).  workspace_dev holds
 * rpkt_gpu_checksum_chains_workspace_bytes(n_segs) bytes. */
size_t rpkt_gpu_checksum_chains_workspace_bytes(uint32_t n_segs);
int rpkt_gpu_checksum_chains(const uint8_t* buf_dev, uint64_t buf_bytes, const uint32_t* segs_dev,
                             uint32_t n_segs, const uint32_t* chain_first_dev, uint32_t n_chains,
                             uint16_t* out_dev, void* workspace_dev, void* stream);

/* Mbuf-chain batch (rpkt-dpdk's Mbuf segments read through a Pbuf,
 * rpkt-dpdk/src/pbuf.rs).  Segment k = buf_dev[segs_dev[2k] .. segs_dev[2k] +
 * segs_dev[2k+1]) (data offset, data_len; clamped to buf_bytes like frames; segs_dev
 * 8-byte aligned).  Chain p = segments [a, b) with a = min(chain_first_dev[p], n_segs),
 * b = min(max(chain_first_dev[p+1], a), n_segs) (n_chains + 1 entries); its pkt_len is
 * the sum of its segments' lengths.  buf_bytes < 4 GiB, n_segs < 2^31. */
typedef struct rpkt_chains {
    const uint8_t*  buf_dev;
    uint64_t        buf_bytes;
    const uint32_t* segs_dev;
    const uint32_t* chain_first_dev;
    uint32_t        n_segs;
    uint32_t        n_chains;
} rpkt_chains_t;

/* Parse + verify mbuf chains: rpkt_gpu_parse_batch's chain and record per chain, with
 * each view's tests taken as they are over a Pbuf: header sizes against chunk() (the
 * rest of the segment holding the header's first byte; Pbuf::new starts at segment 0
 * even when it is empty), totals against remaining(), the packet end cut by the
 * IPv4/IPv6/UDP trim_off.  With RPKT_F_IPV6 the IPv6 chain too: the 40-byte header and
 * each extension header tested against its own chunk.  Record offsets are logical
 * positions in the chain's bytes,
 * frame_len = pkt_len, l4_sum = from_buf over the segments (rpkt/src/checksum.rs:8-27).
 * The caller's segments are never modified (the reference's trim_off truncates the
 * mbuf chain, mbuf.rs:346-382).  recs_dev n_chains * 80 B, 16-byte aligned. */
int rpkt_gpu_parse_chains(const rpkt_chains_t* chains, uint32_t flags, rpkt_rec_t* recs_dev,
                          rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream);

/* ---- Tunnels: the inner frame of VXLAN, GTP-U and GRE ------------------------- */

/* rpkt_gpu_parse_tunnel_batch decodes one tunnel level after the outer parse, as the
 * reference's receive loops chain the views (the dispatch is the caller's in rpkt):
 *   VXLAN   Udp::payload -> Vxlan::parse (vxlan/generated.rs:32-39) -> payload() (advance 8)
 *           -> EtherFrame::parse ... (rpkt/tests/vlan_mpls_tests.rs:224-251);
 *   GTP-U   Udp::payload -> Gtpv1::parse (gtpv1/generated.rs:33-49) -> payload() (trim to
 *           packet_len, advance header_len, :98-108) -> the extension headers named by
 *           next_extention_header (ExtPduNumber, ExtUdpPort, ExtLongPduNumber,
 *           ExtServiceClassIndicator, ExtContainer, NrUp / PduSessionUp::group_parse, each
 *           its parse and payload()) -> Ipv4|Ipv6::parse (gtpv1_test.rs:199-231, 284-320,
 *           468-505);
 *   GRE     Ipv4|Ipv6::payload -> GreGroup::group_parse (gre/generated.rs:800-820) ->
 *           Gre::payload() (advance header_len) -> Ipv4|Ipv6|EtherFrame::parse
 *           (gre_test.rs:20-99).
 * Dispatch: an outer frame that parsed OK as UDP with destination port 4789 (VXLAN) or
 * 2152 (GTP-U), else with that source port; or an outer IPv4 (first fragment) / IPv6
 * frame whose upper-layer protocol is 47 (status L4_OTHER).  GTP-U carries an inner
 * packet only as a GTPv1 (version 1) G-PDU (message type 255), by the version nibble of
 * its first byte (4 / 6).  GRE's protocol type selects 0x0800 IPv4, 0x86DD IPv6,
 * 0x6558 Ethernet (transparent bridging).  IPv6 inner packets need RPKT_F_IPV6. */
enum rpkt_tun_kind {
    RPKT_TUN_NONE = 0,
    RPKT_TUN_VXLAN = 1,
    RPKT_TUN_GTPU = 2,
    RPKT_TUN_GRE = 3
};
enum rpkt_tun_status {
    RPKT_T_OK = 0,            /* tunnel decoded: the inner record holds the inner frame     */
    RPKT_T_NONE = 1,          /* no tunnel dispatch on this frame (kind NONE)               */
    RPKT_T_BAD = 2,           /* Vxlan::parse / Gtpv1::parse / GreGroup::group_parse Err     */
    RPKT_T_NOT_TPDU = 3,      /* GTP: not a GTPv1 G-PDU (version != 1 or message != 255)    */
    RPKT_T_EXT_BAD = 4,       /* GTP: an extension header's parse Err, an unknown next
                                 extension type, or more than RPKT_MAX_GTP_EXT of them      */
    RPKT_T_INNER_UNKNOWN = 5  /* the inner protocol is none of Ether / IPv4 / IPv6 (an
                                 IPv6 one without RPKT_F_IPV6, an empty T-PDU, GRE for
                                 PPTP's PPP payload): inner_type says what it is, or 0     */
};
#define RPKT_MAX_GTP_EXT 8

/* One frame's tunnel, 16 bytes. */
typedef struct rpkt_tun {
    uint8_t  kind;       /*  0 enum rpkt_tun_kind                                     */
    uint8_t  status;     /*  1 enum rpkt_tun_status                                   */
    uint16_t tun_off;    /*  2 frame offset of the VXLAN / GTPv1 / GRE header           */
    uint16_t inner_off;  /*  4 frame offset of the inner frame: the tunnel's payload()  */
    uint16_t inner_type; /*  6 0x6558 (an Ethernet frame), 0x0800, 0x86DD; GRE: its
                             protocol_type (0x880B for PPTP); GTP: 0 when the T-PDU's
                             version nibble is not 4 / 6                                 */
    uint32_t id;         /*  8 Vxlan::vni, Gtpv1::teid, Gre::key (0 without the K bit)  */
    uint8_t  hdr0;       /* 12 header byte 0: VXLAN flags (gbp_extention, vni_present),
                             GTPv1 version / protocol_type / E / S / PN, GRE C / R / K / S
                             / recursion_control                                         */
    uint8_t  hdr1;       /* 13 header byte 1: VXLAN dont_learn / policy_applied, GTPv1
                             message_type, GRE flags / version                           */
    uint16_t aux;        /* 14 Vxlan::group_id; Gtpv1::sequence (a 12-B header, else 0);
                             Gre::checksum (C or R bit, else 0)                          */
} rpkt_tun_t;

#define RPKT_TUN_BYTES 16u

/* Parse + verify a batch and decode one tunnel level per frame:
 *   outer_dev[i]  the record rpkt_gpu_parse_batch writes for frame i with the same flags;
 *   tun_dev[i]    its tunnel (kind NONE / status NONE when there is none);
 *   inner_dev[i]  the record of the inner frame [inner_off, the tunnel payload's end):
 *                 rpkt_gpu_parse_batch's record of those bytes (an inner IPv4 / IPv6
 *                 packet is parsed from its IP header: ethertype = inner_type, n_vlan 0,
 *                 MACs 0), with l3_off / l4_off / payload_off / ip6_pdst_off as offsets in
 *                 the OUTER frame (rpkt's Cursor::cursor() of the inner views) and
 *                 frame_len = the inner frame's length; status RPKT_S_NO_INNER (all else
 *                 0) when tun_dev[i].status != RPKT_T_OK.
 * flags: RPKT_F_IP_SUM, RPKT_F_L4_SUM, RPKT_F_IPV6, applied to both levels, and
 * RPKT_F_FLOW_EV: flow_ev_dev[i] (n * 8 B, 8-byte aligned; n_buckets 1..
 * RPKT_FLOW_MAX_BUCKETS) is the flow event of the INNER record when the tunnel decoded
 * (tun_dev[i].status == RPKT_T_OK: the inner 5-tuple, the inner frame's length, the inner
 * sums' bad bits -- per-subscriber / per-tenant accounting of the overlay through
 * rpkt_gpu_flow_count and rpkt_gpu_flow_reduce), else of the outer record, exactly as
 * rpkt_gpu_parse_batch forms it from a record.  Each byte is read from HBM about once:
 * the outer L4 sum (UDP, or GRE with its checksum) reuses the inner L4 sum's stream over
 * the bytes the two share.  outer_dev / inner_dev n * 80 B, tun_dev n * 16 B, all
 * 16-byte aligned. */
int rpkt_gpu_parse_tunnel_batch(const rpkt_batch_t* batch, uint32_t flags, rpkt_rec_t* outer_dev,
                                rpkt_tun_t* tun_dev, rpkt_rec_t* inner_dev,
                                rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream);

/* A receive ring of tunnelled bursts (a VTEP's / UPF's rx queue: the loopback_rx.rs:96-121
 * loop with the tunnel views of vlan_mpls_tests.rs:237-251 / gtpv1_test.rs:199-231 on
 * each frame) in one launch per RPKT_RING_MAX_SLOTS slots: results equal one
 * rpkt_gpu_parse_tunnel_batch call per slot, into that slot's outer_dev / tun_dev /
 * inner_dev (and flow_ev_dev when RPKT_F_FLOW_EV is set).  Slots with n == 0 are skipped;
 * every slot is checked before anything is launched; layouts may differ from slot to
 * slot. */
typedef struct rpkt_tun_ring_slot {
    rpkt_batch_t    batch;
    rpkt_rec_t*     outer_dev;
    rpkt_tun_t*     tun_dev;
    rpkt_rec_t*     inner_dev;
    rpkt_flow_ev_t* flow_ev_dev;
} rpkt_tun_ring_slot_t;
int rpkt_gpu_parse_tunnel_ring(const rpkt_tun_ring_slot_t* slots, uint32_t n_slots,
                               uint32_t flags, uint32_t n_buckets, void* stream);

/* Tunnels over mbuf chains: rpkt_gpu_parse_tunnel_batch's three records per chain, with
 * every view's tests taken as they are over a Pbuf (rpkt-dpdk/src/pbuf.rs:49-104; the same
 * Vxlan::parse(udp.payload()) chain of rpkt/tests/vlan_mpls_tests.rs:237-251 runs
 * unchanged over one) -- jumbo overlay traffic in 2048-B mbuf data rooms without
 * flattening it on the host first:
 *   outer_dev[p]  byte for byte the record rpkt_gpu_parse_chains writes for chain p with
 *                 the same flags;
 *   tun_dev[p]    the tunnel of the Pbuf the outer view's payload() returned, dispatched as
 *                 rpkt_gpu_parse_tunnel_batch dispatches.  Header sizes are tested against
 *                 chunk() (the rest of the segment holding the header's first byte, cut at
 *                 the current packet end, empty segments skipped as advance_common walks
 *                 them), total lengths against remaining(): Vxlan::parse chunk >= 8
 *                 (vxlan/generated.rs:32-39); Gtpv1::parse chunk >= 8 and header_len <=
 *                 chunk, packet_len <= remaining (gtpv1/generated.rs:33-49); each GTP-U
 *                 extension header against its own chunk (:336-341, :461-466, :587-592,
 *                 :747-752, :880-892, the NrUp / PduSessionUp group parses); Gre::parse
 *                 header_len in [4, chunk]; GreForPPTP::parse chunk >= 8 and header_len <=
 *                 chunk, payload_len + header_len <= remaining (gre/generated.rs:371-386).
 *                 A tunnel or extension header that straddles a segment boundary is
 *                 therefore RPKT_T_BAD / RPKT_T_EXT_BAD, as the reference returns Err: it
 *                 is not reassembled.  tun_off / inner_off are logical positions in the
 *                 chain's bytes;
 *   inner_dev[p]  the record of the sub-chain [inner_off, the tunnel payload's end) under
 *                 the same Pbuf rules (an inner IPv4 / IPv6 packet parsed from its IP
 *                 header: ethertype = inner_type, n_vlan 0, MACs 0), l3_off / l4_off /
 *                 payload_off / ip6_pdst_off logical positions in the OUTER chain,
 *                 frame_len = the inner frame's length, l4_sum = from_buf over the
 *                 segments with the odd-byte pairing of rpkt/src/checksum.rs:77-111;
 *                 status RPKT_S_NO_INNER (all else 0) when tun_dev[p].status != RPKT_T_OK.
 * flags and flow_ev_dev / n_buckets as rpkt_gpu_parse_tunnel_batch (the event is the inner
 * record's when the tunnel decoded, else the outer's); chains as rpkt_gpu_parse_chains.
 * Record offsets are 16-bit: a chain longer than 65,535 B has them truncated, as
 * rpkt_gpu_parse_chains truncates them, and the tunnel is then looked for at the truncated
 * position.  outer_dev / inner_dev n_chains * 80 B, tun_dev n_chains * 16 B, all 16-byte
 * aligned. */
int rpkt_gpu_parse_tunnel_chains(const rpkt_chains_t* chains, uint32_t flags,
                                 rpkt_rec_t* outer_dev, rpkt_tun_t* tun_dev, rpkt_rec_t* inner_dev,
                                 rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream);

/* Nested tunnels: the next tunnel level of a batch, from the records of the level before
 * (a UPF's GTP-U over a VXLAN underlay, VXLAN over GRE, GRE inside GTP-U).  The reference
 * has no depth limit: a receive loop keeps chaining the views, Vxlan::parse(udp.payload())
 * -> EtherFrame::parse -> ... -> Gtpv1::parse(udp.payload()) -> Ipv4::parse, because every
 * view takes any Buf.  Here each level is one call, and the call can be applied to its own
 * output for a third level and beyond.
 *   tun_dev / inner_dev   what rpkt_gpu_parse_tunnel_batch wrote for this SAME batch (level
 *                 1), or what an earlier call of this entry wrote for it (level k);
 *   tun_next_dev[i] / inner_next_dev[i]   level k + 1, in the same formats.  Where
 *                 tun_dev[i].status != RPKT_T_OK: kind NONE / status RPKT_T_NONE (all else
 *                 0) and status RPKT_S_NO_INNER (all else 0).  Otherwise the level-k inner
 *                 frame is bytes [inner_off, inner_off + inner_dev[i].frame_len) of frame i
 *                 and inner_dev[i] plays the outer record's part: the tunnel is dispatched
 *                 from it and decoded exactly as rpkt_gpu_parse_tunnel_batch dispatches and
 *                 decodes from its outer record (the same rpkt_tun_status values), and the
 *                 next inner frame is parsed and verified as that entry's inner frame is
 *                 (an inner IP packet from its IP header: ethertype = inner_type, n_vlan 0,
 *                 MACs 0; frame_len = the innermost frame's length).
 * Every offset written -- tun_off, inner_off, the record's l3_off / l4_off / payload_off /
 * ip6_pdst_off -- is a position in the OUTERMOST frame, as the level-1 offsets are.  The
 * sums of the levels before are in their records; this pass computes the innermost
 * record's sums only.
 * flags: RPKT_F_IP_SUM, RPKT_F_L4_SUM, RPKT_F_IPV6 (any other bit: RPKT_E_INVAL) and
 * RPKT_F_FLOW_EV: flow_ev_dev[i] (n * 8 B, 8-byte aligned; n_buckets 1..
 * RPKT_FLOW_MAX_BUCKETS) is written ONLY where tun_next_dev[i].status == RPKT_T_OK, with
 * the event of inner_next_dev[i] as rpkt_gpu_parse_tunnel_batch forms an inner record's;
 * the other entries are left as they are, so passing the level-1 call's event buffer moves
 * the accounting to the innermost flow and changes nothing else.
 * Flat batches (packed or strided); n == 0 returns RPKT_OK.  tun_next_dev == tun_dev or
 * inner_next_dev == inner_dev is RPKT_E_INVAL; tun_dev / inner_dev are not written.
 * The records must come from a call on the same batch.  With other records the outputs are
 * unspecified, but every frame byte is still read through the bounds-checked buffer
 * resource, with [inner_off, + frame_len) clamped to frame i's span: wrong records, never a
 * fault.  Frames longer than 65,535 B have truncated offsets, as everywhere else.
 * inner_dev / inner_next_dev n * 80 B, tun_dev / tun_next_dev n * 16 B, all 16-byte
 * aligned. */
int rpkt_gpu_parse_tunnel_next(const rpkt_batch_t* batch, uint32_t flags,
                               const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                               rpkt_tun_t* tun_next_dev, rpkt_rec_t* inner_next_dev,
                               rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream);

/* ---- TX side ---------------------------------------------------------------- */

/* Build flags: fill a checksum the way the NIC TX offload requested by the
 * reference computes it (rpkt-dpdk/examples/loopback_rx.rs:133): field zeroed, the
 * complement of the RFC 1071 sum; a UDP result of 0 is sent as 0xffff.  Without the
 * flag the checksum field is the record's (a set_checksum setter value). */
#define RPKT_BUILD_IP_CSUM 1u
#define RPKT_BUILD_L4_CSUM 2u

/* Batched header build (benches/rpkt/rpkt_build.rs:9-28): for each frame i of
 * `batch` (payload already in place), write the headers the record recs_dev[i] asks
 * for, as Udp|Tcp::prepend_header + setters, Ipv4::prepend_header + setters,
 * VlanFrame::prepend_header + setters (n_vlan tags), EtherFrame::prepend_header +
 * setters would: l3 = 14 + 4 n_vlan, l4 = l3 + IHL*4, UDP (protocol 17, 8 B) or TCP
 * (6, the 20 fixed bytes; doff from l4_word6) or no L4 header.  Length fields are
 * set from the frame span (prepend_header's remaining()): IPv4 packet_len =
 * len - l3, UDP length = len - l4.  Option bytes are left as the buffer holds them.
 * A frame too short for its headers (where prepend_header asserts) is left
 * untouched; built_dev[i] (optional, n bytes) = 1 if written, else 0.  Records use
 * the rpkt_rec_t getter layout, so building from parse records reproduces frames.
 * frames_dev and recs_dev 16-byte aligned. */
int rpkt_gpu_build_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev, uint32_t flags,
                         uint8_t* built_dev, void* stream);

/* Encapsulation build: rpkt_gpu_build_batch plus, for each frame whose tun_dev[i].kind is
 * not RPKT_TUN_NONE, the tunnel header written first, inside-out as the reference builds
 * these frames (the inner frame, and a GTP-U frame's extension headers, are payload already
 * in place):
 *   VXLAN  Vxlan::prepend_header + set_gbp_extention / set_vni_present / set_dont_learn /
 *          set_policy_applied (hdr0, hdr1) + set_group_id (aux) + set_vni (id), at the
 *          outer UDP payload (l4 + 8; the record's protocol must be 17), byte 7 0
 *          (vxlan/generated.rs:99-150; vlan_mpls_tests.rs:254-300);
 *   GTP-U  Gtpv1::prepend_header(header of hdr0, hdr1) (length = remaining - 8) + set_teid
 *          (id), and for a 12-B header (any of E/S/PN in hdr0) set_sequence (aux); bytes
 *          10-11 (npdu, next_extention_header) are left as the buffer holds them, as the
 *          extension headers after them (gtpv1/generated.rs:110-170, 254-310;
 *          gtpv1_test.rs:236-282);
 *   GRE    Gre::prepend_header(hdr0, hdr1) + set_protocol_type (inner_type), with a
 *          checksum word (C or R) = aux, or with RPKT_BUILD_L4_CSUM and the C bit the RFC
 *          2784 checksum over the GRE header and payload; a key word (K) = id; offset and
 *          sequence words left as the buffer holds them; at l4 (protocol 47)
 *          (gre/generated.rs:95-267; gre_test.rs:213-278).
 * The outer UDP checksum fill then covers the tunnel header.  status, tun_off and inner_off
 * are not read.  A frame whose tunnel header does not end within the frame and within
 * its first RPKT_TUN_BUILD_MAX_END bytes (the header window at any 16-B phase: every IPv4
 * outer frame and IPv6 ones with short extension chains), or does not match the record's
 * protocol, is left untouched (built 0).  tun_dev n * 16 B, 16-byte aligned. */
#define RPKT_TUN_BUILD_MAX_END 113u
int rpkt_gpu_build_tunnel_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev,
                                const rpkt_tun_t* tun_dev, uint32_t flags, uint8_t* built_dev,
                                void* stream);

/* Firewall forward (rpkt-dpdk/examples/loopback_rx.rs:96-140), one fused pass per
 * frame: the parse chain of rpkt_gpu_parse_batch with both sums, then frame i is
 * forwarded when it is an untagged IPv4/UDP frame that parsed OK with a valid IPv4
 * sum and a valid UDP sum (or UDP checksum 0) -- the RX offload verdicts of the
 * reference -- and its source address is not in forbid_dev (n_forbid u32
 * addresses, sorted ascending).  A forwarded frame is rewritten in place: ports and
 * addresses swapped, TTL - 1 (wrapping), dst/src MAC = dmac/smac, IPv4 and UDP
 * checksums recomputed (the reference's TX offload).  keep_dev[i] = 1 if forwarded;
 * other frames are not written.  frames_dev 16-byte aligned.
 * With fwd->flags = RPKT_F_IPV6 the parse also decodes IPv6 and an untagged IPv6/UDP
 * frame is forwarded the same way: parsed OK with a valid L4 sum (a zero UDP checksum is
 * invalid over IPv6), never matched against the (IPv4) forbidden list; addresses (16 B)
 * and ports swapped, hop_limit - 1 (wrapping), MACs set, the UDP checksum updated over
 * the IPv6 pseudo header (its destination stays a routing header's final address).
 * IPv6 records are built by rpkt_gpu_build_batch as Ipv6::prepend_header + setters
 * (ipv6/generated.rs:94-135): bytes 0..7 of the header from the record (ip6_vtcfl,
 * payload_len = remaining, next_header, hop_limit), the addresses and the extension
 * headers up to l4_off left as the buffer holds them (the record keeps the addresses
 * folded), the L4 checksum over the IPv6 pseudo header (src, the address at
 * ip6_pdst_off -- dst_addr when that offset does not lie in [l3 + 24, l4_off - 16] --,
 * u32 length, next header), a UDP result of 0 sent as 0xffff. */
typedef struct rpkt_fwd {
    uint8_t         dmac[6];
    uint8_t         smac[6];
    const uint32_t* forbid_dev;
    uint32_t        n_forbid;
    uint32_t        flags;      /* 0, or RPKT_F_IPV6 (was `reserved`, always 0) */
} rpkt_fwd_t;
int rpkt_gpu_forward_batch(const rpkt_batch_t* batch, const rpkt_fwd_t* fwd, uint8_t* keep_dev,
                           void* stream);

/* ---- TCP and UDP segmentation (TSO, UDP GSO) ------------------------------------ */

/* The third TX offload of the reference's examples: rpkt-dpdk/examples/tso_tx.rs:128-134
 * sets TCP_SEG (1 << 50) next to the IP_CKSUM / TCP_CKSUM bits, l2_len / l3_len / l4_len and
 * set_tso_segsz(1024), and the port cuts the 4000-byte frame into MSS-sized TCP segments
 * with fixed-up headers and fresh checksums.  rpkt_gpu_segment_batch does that cut on the
 * device, for frames that stay in HBM, under the Linux tcp_gso_segment / DPDK rte_gso TCP
 * rules.  The output is the complete transmit batch, in input order: every input frame
 * yields one output frame or more.
 *
 * recs_dev: the rpkt_rec_t records of a parse of this same batch (RPKT_F_IPV6 for IPv6
 * frames; the sum flags do not matter).  As for rpkt_gpu_options_batch the records only
 * locate things -- status, the dispatch ethertype, ip_protocol, ip_frag, l3_off, l4_off,
 * payload_off, payload_len, ip6_pdst_off -- and every header byte is taken from the frame.
 * mss: 1..65535.  flags: 0, or RPKT_SEGMENT_UDP to segment UDP datagrams too (below).
 *
 * Frame i is segmented iff status == RPKT_S_OK, ip_protocol == 6, for IPv4
 * (ip_frag & 0x3fff) == 0 (not a fragment) and payload_len > mss; it yields
 * n_i = ceil(payload_len / mss) frames.  Every other frame (UDP, unparsed, short TCP,
 * fragments) passes through as one frame, a byte copy of [0, frame_len).
 * Segment k of a segmented frame, with p_k = mss but p_last = payload_len - (n_i - 1) * mss:
 *   bytes   [0, payload_off) of the frame (Ethernet, tags, the IP header with its options or
 *           extension headers, the TCP header with its options: any length), then payload
 *           bytes [payload_off + k * mss, + p_k); bytes after the IP packet's end (Ethernet
 *           padding) are not carried;
 *   IPv4    packet_len = (payload_off - l3_off) + p_k; ident = (ident + k) & 0xffff; the
 *           header checksum filled as RPKT_BUILD_IP_CSUM fills it;
 *   IPv6    payload_len = (payload_off - l3_off - 40) + p_k; extension headers untouched;
 *   TCP     seq = seq + k * mss (mod 2^32); FIN (0x01) and PSH (0x08) cleared on every
 *           segment but the last, CWR (0x80) on every segment but the first; everything
 *           else, options included, copied; the checksum filled as RPKT_BUILD_L4_CSUM fills
 *           a TCP one, over the pseudo header (for IPv6 its destination is the address at
 *           ip6_pdst_off under rpkt_gpu_build_batch's rule), the header and the segment's
 *           payload; a result of 0 stays 0.
 *
 * With RPKT_SEGMENT_UDP, TCP frames are handled as above and UDP datagrams are cut under the
 * Linux __udp_gso_segment rules (the UDP_SEGMENT socket option, DPDK's rte_gso UDP path): a
 * frame is also segmented iff status == RPKT_S_OK, ip_protocol == 17, for IPv4
 * (ip_frag & 0x3fff) == 0, payload_off - l4_off == 8 and payload_len > mss; it yields
 * n_i = ceil(payload_len / mss) frames.  Segment k: the bytes, the IPv4 packet_len, ident + k
 * and checksum, and the IPv6 payload_len exactly as for TCP;
 *   UDP     length (bytes l4+4..5) = 8 + p_k; ports copied; the checksum (bytes l4+6..7)
 *           filled as RPKT_BUILD_L4_CSUM fills a UDP one, over the pseudo header (protocol 17,
 *           the UDP length; the IPv6 destination as for TCP), the 8-byte header and the
 *           segment's payload; a result of 0 is written as 0xffff.  It is always filled, also
 *           when the input's checksum field is 0: "no checksum" is not a property a cut can
 *           carry (Linux refuses UDP_SEGMENT without a checksum).
 * Without the flag a UDP frame passes through, as every output is then what it was before
 * the flag existed.  One mss serves the call, TCP and UDP alike.
 *
 * Outputs:
 *   seg_first_dev  n + 1 entries: the outputs of frame i are [seg_first[i], seg_first[i+1]);
 *   totals_dev     u64[2], 8-byte aligned: {n_out, out_bytes_needed}, whatever the capacities;
 *   out_frames_dev (16-byte aligned, out_bytes bytes) and out_offsets_dev (out_cap + 1
 *                  entries): a packed rpkt_batch_t.  When n_out <= out_cap and
 *                  out_bytes_needed <= out_bytes, entries 0..n_out are the true offsets
 *                  (frames back to back from 0, no padding) and entries n_out+1..out_cap
 *                  equal out_bytes_needed: a parse over all out_cap slots needs no host round
 *                  trip, the spare slots are empty frames.  Otherwise (overflow) seg_first_dev
 *                  and totals_dev are still exact and the rest is unspecified; nothing is ever
 *                  written outside [out_frames_dev, + out_bytes) and out_offsets_dev[0..out_cap].
 * Bounds for sizing: n_out <= n + floor(frames_bytes / mss); out_bytes_needed <= frames_bytes
 * + (n_out - n) * H, H the longest header (payload_off) of the batch.  (n_out > 2^32 - 1
 * does not fit seg_first_dev; out_cap cannot hold it either.)
 * workspace_dev: rpkt_gpu_segment_workspace_bytes(n) bytes, 16-byte aligned; calls that
 * share one must be ordered (one stream).  The call is plan, prefix sums and write on
 * `stream` with no host step, so it can be captured in a graph with the parse that follows.
 * The records must come from a parse of the same batch.  With other records the outputs are
 * unspecified, but every frame byte is read through the bounds-checked buffer resource with
 * [payload_off, + payload_len) clamped to the frame's span, and a record whose offsets do not
 * nest as a parse leaves them (l3_off + 20 (IPv6: 40) <= l4_off, l4_off + 20 <= payload_off
 * <= frame_len, header lengths within 60; UDP: l4_off + 8 == payload_off) passes through:
 * wrong frames, never a fault.
 * A tunnelled frame is to this entry what its outer record says: it passes through, and with
 * RPKT_SEGMENT_UDP the OUTER datagram of a VXLAN / GTP-U frame would be cut, which destroys the
 * tunnel; rpkt_gpu_segment_tunnel_batch (below) cuts the inner TCP or UDP instead.
 * Not covered: a segment size per flow.  (IPv4 UDP fragmentation, UFO, is
 * rpkt_gpu_fragment_batch below: another contract, one datagram in many IP fragments.) */
#define RPKT_SEGMENT_UDP  16u   /* also segment UDP datagrams (flags of both segment entries) */

size_t rpkt_gpu_segment_workspace_bytes(uint32_t n);
int rpkt_gpu_segment_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev, uint32_t mss,
                           uint32_t flags, uint8_t* out_frames_dev, uint64_t out_bytes,
                           uint32_t* out_offsets_dev, uint32_t out_cap, uint32_t* seg_first_dev,
                           uint64_t* totals_dev, void* workspace_dev, void* stream);

/* The same over mbuf chains.  The super-frame tso_tx.rs hands to the port is a chain
 * (Mbuf::from_slice splits 4000 bytes over 2048-byte data rooms, mbuf.rs:261-312; the port
 * has the multi-segment offload, tx_offloads bit 15), and so is every jumboframe_tx.rs frame:
 * anything larger than one data room.  rpkt_gpu_segment_chains reads the chains in place --
 * no gather into a flat batch first -- and writes wire frames, which are linear by nature.
 *
 * Let F_p be chain p's bytes in order under rpkt_chains_t's clamps (a = min(chain_first[p],
 * n_segs), b = min(max(chain_first[p+1], a), n_segs), each segment clamped to buf_bytes, empty
 * segments contributing nothing).  Every output -- out_frames_dev, out_offsets_dev,
 * seg_first_dev, totals_dev -- is byte for byte what rpkt_gpu_segment_batch writes for the
 * packed batch F_0 .. F_{n_chains-1} with the same recs_dev, mss, out_cap and out_bytes: the
 * overflow contract, the spare offset slots, nothing written outside the buffers, and the
 * pass-through of every chain that is not segmented as a copy of [0, pkt_len).
 *   Records   recs_dev are normally rpkt_gpu_parse_chains' records of these chains: their
 *             offsets are logical positions in F_p already.  A header that straddles a
 *             segment boundary is a parse error there, so such a chain passes through.  The
 *             entry itself puts no condition on where segments are cut: with records that say
 *             "segment this" (a parse of the flattened bytes), the header [0, payload_off) and
 *             the payload are gathered across any cuts.
 *   Nesting   pkt_len, the sum of the clamped segment lengths, takes frame_len's place in
 *             the nesting test and in the payload_len clamp.
 *   Overlap   segments may overlap or be shared between chains: the arena is only read.
 *   Huge      pkt_len is summed in 64 bits for totals_dev; a chain of 4 GiB or more cannot
 *             fit out_bytes, so the call ends as an overflow.
 *   Faults    every arena load goes through the buffer resource over [buf_dev, + buf_bytes)
 *             and every store through one over the output: wrong records give wrong frames,
 *             never a fault.
 *   Limits    no cap on the segments of a chain (many tiny segments are slow, not wrong).
 * flags: 0 or RPKT_SEGMENT_UDP, as for rpkt_gpu_segment_batch: a UDP header gathered across
 * segment cuts is cut like a TCP one.  workspace_dev:
 * rpkt_gpu_segment_chains_workspace_bytes(n_chains) bytes, 16-byte aligned; calls that share
 * one must be ordered.  No host step: rpkt_gpu_parse_chains -> rpkt_gpu_segment_chains ->
 * rpkt_gpu_parse_batch over out_cap slots captures as one graph.
 * Bounds for sizing: rpkt_gpu_segment_batch's with the sum of the chains' pkt_len in
 * frames_bytes' place; that sum is at most buf_bytes when segments do not overlap.
 * A tunnelled chain is to this entry what its outer record says, as a tunnelled frame is to
 * rpkt_gpu_segment_batch; rpkt_gpu_segment_tunnel_chains (below) cuts the inner TCP or UDP.
 * Not covered: coalescing over chains. */
size_t rpkt_gpu_segment_chains_workspace_bytes(uint32_t n_chains);
int rpkt_gpu_segment_chains(const rpkt_chains_t* chains, const rpkt_rec_t* recs_dev, uint32_t mss,
                            uint32_t flags, uint8_t* out_frames_dev, uint64_t out_bytes,
                            uint32_t* out_offsets_dev, uint32_t out_cap, uint32_t* seg_first_dev,
                            uint64_t* totals_dev, void* workspace_dev, void* stream);

/* Segmentation of the inner TCP / UDP of tunnels: what a VTEP or UPF needs to send a large
 * application write through VXLAN, GTP-U or GRE without leaving the device.  Every NIC the
 * reference targets pairs TSO with the tunnel offloads (rpkt-dpdk/src/conf.rs:80 lists
 * DEV_TX_OFFLOAD_OUTER_IPV4_CKSUM next to TCP_TSO); Linux does this cut in
 * skb_udp_tunnel_segment and gre_gso_segment.
 *
 * outer_dev, tun_dev, inner_dev: the three outputs of rpkt_gpu_parse_tunnel_batch on this same
 * batch (level 1; RPKT_F_IPV6 for IPv6 at either level; the sum flags do not matter).  As for
 * rpkt_gpu_segment_batch the records only locate things and every header byte is taken from the
 * frame.  mss: 1..65535.  flags: 0 or RPKT_SEGMENT_UDP.  Below O, T, I are frame i's outer,
 * tunnel and inner record; ipo = I.payload_off, ipl = I.payload_len clamped to the frame, toff =
 * T.tun_off, ioff = T.inner_off.
 *   No tunnel   T.kind == RPKT_TUN_NONE: the frame is handled exactly as
 *               rpkt_gpu_segment_batch handles it with record O and the same mss and flags, so a
 *               mixed transmit batch needs this one call only.
 *   Undecoded   T.kind != NONE and T.status != RPKT_T_OK: the frame passes through, a byte copy
 *               of [0, frame_len).  Its outer UDP is never cut, with or without the flag.
 *   Decoded     the frame is segmented iff all of these hold; anything else passes through:
 *               - I: status == RPKT_S_OK; ip_protocol 6, or with RPKT_SEGMENT_UDP 17 with
 *                 payload_off - l4_off == 8; for IPv4 (ip_frag & 0x3fff) == 0; ipl > mss; its
 *                 offsets, all positions in the outer frame, nest as rpkt_gpu_segment_batch
 *                 requires;
 *               - O: IPv4 or IPv6 by its dispatch ethertype; for IPv4 (ip_frag & 0x3fff) == 0;
 *                 O.l3_off + 20 (IPv6: + 40) <= O.l4_off, an IPv4 header within 60 bytes;
 *                 VXLAN / GTP-U: O.status == RPKT_S_OK, ip_protocol 17, O.l4_off + 8 <= toff;
 *                 GRE: ip_protocol 47, O.l4_off == toff;
 *               - toff + 8 (GRE: + 4, with the C bit + 8) <= ioff <= I.l3_off;
 *               - GRE: the S (sequence) and R bits of the frame's byte toff are clear: Linux
 *                 disables GSO on a GRE device with sequence numbers, a cut cannot invent them.
 * A segmented frame yields n_i = ceil(ipl / mss) frames.  Segment k, with p_k as above and
 * tot = ipo + p_k:
 *   bytes       [0, ipo) of the frame, then payload bytes [ipo + k * mss, + p_k); nothing after
 *               the inner IP packet's end is carried (inner and outer Ethernet padding);
 *   inner       the inner IP and L4 headers exactly as rpkt_gpu_segment_batch writes them for
 *               the inner frame on its own: IPv4 packet_len / ident + k / checksum or IPv6
 *               payload_len; TCP seq / FIN, PSH, CWR / checksum, or UDP length / checksum;
 *   GTP-U       length (bytes toff+2..3) = tot - toff - 8; sequence, N-PDU and extension
 *               headers copied;
 *   GRE         with the C bit the checksum word (bytes toff+4..5) is the RFC 2784 checksum
 *               over [toff, tot) of the output, as rpkt_gpu_build_tunnel_batch fills it (a
 *               result of 0 stays 0); without C nothing changes in the GRE header;
 *   outer UDP   length = tot - O.l4_off.  A checksum field of 0 in the input stays 0 in every
 *               output, over IPv4 and IPv6 alike (Linux keeps a tunnel's "no checksum"; RFC
 *               6935 / 6936).  Otherwise it is filled over the outer pseudo header (the IPv6
 *               destination under rpkt_gpu_build_batch's ip6_pdst_off rule) and
 *               [O.l4_off, tot) of the output, a result of 0 written as 0xffff;
 *   outer IPv4  packet_len = tot - O.l3_off; ident = (ident + k) & 0xffff; the header checksum
 *               refilled;
 *   outer IPv6  payload_len = tot - O.l3_off - 40; extension headers untouched.
 * Length fields are taken mod 2^16.
 * Outputs, overflow, the spare offset slots, the packed layout, "nothing written outside the
 * buffers" and plan -> prefix sums -> write on `stream` with no host step are
 * rpkt_gpu_segment_batch's contract word for word: rpkt_gpu_parse_tunnel_batch ->
 * rpkt_gpu_segment_tunnel_batch -> rpkt_gpu_parse_tunnel_batch over out_cap slots captures as
 * one graph.  Bounds for sizing: that entry's, with H the longest INNER payload_off of the
 * batch.  workspace_dev: rpkt_gpu_segment_tunnel_workspace_bytes(n) bytes, 16-byte aligned.
 * Argument checks: rpkt_gpu_segment_batch's in its order, with tun_dev and inner_dev required
 * and 16-byte aligned along with outer_dev.
 * The records must come from a parse of the same batch.  With other records the outputs are
 * unspecified, but every load goes through the frames buffer resource and every store through
 * the output's, and offsets that do not nest as above make the frame pass through: wrong
 * frames, never a fault.
 * The inverse is rpkt_gpu_coalesce_tunnel_batch (below).
 * Over mbuf chains: rpkt_gpu_segment_tunnel_chains (below).
 * Not covered: nested
 * tunnels (only the level-1 records are accepted: the inner frame of a second tunnel level is
 * payload here), a segment size per flow, GRE sequence numbers, turning a zero outer UDP
 * checksum into a filled one. */
size_t rpkt_gpu_segment_tunnel_workspace_bytes(uint32_t n);
int rpkt_gpu_segment_tunnel_batch(const rpkt_batch_t* batch, const rpkt_rec_t* outer_dev,
                                  const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                  uint32_t mss, uint32_t flags, uint8_t* out_frames_dev,
                                  uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                                  uint32_t* seg_first_dev, uint64_t* totals_dev, void* workspace_dev,
                                  void* stream);

/* The same over mbuf chains: the case a tunnel endpoint meets, since a super-frame is larger
 * than one data room and so a chain.  The chains are read in place, the output is linear.
 *
 * Let F_p be chain p's bytes in order under rpkt_chains_t's clamps, as rpkt_gpu_segment_chains
 * defines them.  Every output -- out_frames_dev, out_offsets_dev, seg_first_dev, totals_dev --
 * is byte for byte what rpkt_gpu_segment_tunnel_batch writes for the packed batch
 * F_0 .. F_{n_chains-1} with the same outer_dev, tun_dev, inner_dev, mss, flags, out_cap and
 * out_bytes: its three rules (no tunnel, undecoded, decoded), every header fix-up, the overflow
 * contract, the spare offset slots, and nothing written outside the buffers.
 *   Records   normally the three outputs of rpkt_gpu_parse_tunnel_chains on these chains: their
 *             offsets are logical positions in F_p already.  An outer, tunnel or inner header
 *             that straddles a segment end is a parse error or RPKT_T_BAD there, so such a chain
 *             passes through.  The entry itself puts no condition on where segments are cut:
 *             with records that say "cut" (a tunnel parse of the flattened bytes), the header
 *             [0, I.payload_off) and the payload are gathered across any cuts.
 *   Nesting   pkt_len takes frame_len's place in the nesting tests and in the payload_len clamp.
 * Overlap, Huge, Faults and Limits are rpkt_gpu_segment_chains' word for word.  flags: 0 or
 * RPKT_SEGMENT_UDP.  workspace_dev: rpkt_gpu_segment_tunnel_chains_workspace_bytes(n_chains)
 * bytes, 16-byte aligned; calls that share one must be ordered.  No host step:
 * rpkt_gpu_parse_tunnel_chains -> rpkt_gpu_segment_tunnel_chains -> rpkt_gpu_parse_tunnel_batch
 * over out_cap slots captures as one graph.
 * Bounds for sizing: rpkt_gpu_segment_tunnel_batch's with the sum of the chains' pkt_len in
 * frames_bytes' place.  Argument checks: rpkt_gpu_segment_chains' in its order, with tun_dev and
 * inner_dev required and 16-byte aligned along with outer_dev.
 * Not covered: what rpkt_gpu_segment_tunnel_batch does not cover; coalescing over chains. */
size_t rpkt_gpu_segment_tunnel_chains_workspace_bytes(uint32_t n_chains);
int rpkt_gpu_segment_tunnel_chains(const rpkt_chains_t* chains, const rpkt_rec_t* outer_dev,
                                   const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                   uint32_t mss, uint32_t flags, uint8_t* out_frames_dev,
                                   uint64_t out_bytes, uint32_t* out_offsets_dev, uint32_t out_cap,
                                   uint32_t* seg_first_dev, uint64_t* totals_dev,
                                   void* workspace_dev, void* stream);

/* ---- IPv4 / IPv6 fragmentation ---------------------------------------------------- */

/* What makes a frame fit a link: rpkt_gpu_build_tunnel_batch puts 50 bytes or more of outer
 * headers around a frame that was MTU-sized already, and a UDP datagram without UDP_SEGMENT, an
 * ICMP message or any other IP packet larger than the MTU has no other way onto the wire
 * (RPKT_SEGMENT_UDP re-frames a datagram into several datagrams, a different contract).
 * rpkt_gpu_fragment_batch cuts IP packets into fragments on the device: IPv4 under RFC 791
 * and the Linux ip_do_fragment slow path with ip_options_fragment, IPv6 under RFC 8200
 * section 4.5.  The fragments are what rpkt_gpu_parse_batch reads: ip_frag in the record,
 * RPKT_S_IP6_FRAGMENT, the Fragment header among the extension headers it walks.  The output
 * is the complete transmit batch, in input order: every input frame yields one output frame or
 * more, and a frame that is not cut passes through as a byte copy of [0, frame_len), exactly as
 * in rpkt_gpu_segment_batch.
 *
 * mtu: 1..65535, the L3 MTU: the largest IP packet, its IP header included; one serves the
 * call.  flags: 0 or RPKT_FRAGMENT_IGNORE_DF.  recs_dev: the records of a parse of this same
 * batch (RPKT_F_IPV6 for IPv6 frames to be cut; the sum flags do not matter).  They only locate
 * things -- status, the dispatch ethertype, l3_off, l4_off -- and every header byte is read
 * from the frame.  Below l3 = l3_off, l4 = l4_off.
 *
 * IPv4.  With ihl (the low nibble of byte l3, times 4) and L (be16 at l3 + 2) from the frame,
 * frame i is cut iff all of these hold:
 *   - the dispatch ethertype is 0x0800 and status is one under which the IPv4 header parsed:
 *     OK, L4_OTHER, UDP_SHORT, UDP_BAD_LEN, TCP_SHORT, TCP_BAD_DOFF, ICMP_EMPTY;
 *   - l4 == l3 + ihl, ihl in 20..60;
 *   - l3 + L <= frame_len;
 *   - L > mtu;
 *   - DF (0x4000 of the frag word, be16 at l3 + 6) is clear, or RPKT_FRAGMENT_IGNORE_DF is set;
 *   - c = (mtu - ihl) & ~7 is at least 8;
 *   - with P = L - ihl, n_i = ceil(P / c) and o the frame's own 13-bit offset,
 *     o + (n_i - 1) * c / 8 <= 0x1fff.
 * A frame that is itself a fragment is cut again like any other, as a router does.  Fragment k
 * carries p_k = c bytes, the last one p_last = P - (n_i - 1) * c:
 *   bytes      [0, l4) of the frame, then [l4 + k * c, + p_k); bytes after the IP packet's end
 *              (Ethernet padding) are not carried;
 *   packet_len ihl + p_k; ident, tos, ttl, protocol and the addresses are copied;
 *   frag word  (o + k * c / 8) | MF, MF (0x2000) on every fragment but the last, and on the last
 *              too when the input had MF; the reserved bit and DF are written as 0, as Linux
 *              rebuilds frag_off (a DF frame is only ever cut under RPKT_FRAGMENT_IGNORE_DF);
 *   options    fragment 0 keeps them all.  In fragments k > 0 they are rewritten exactly as
 *              ip_options_fragment does it: walk from byte 20; an EOL (type 0) ends the walk; a
 *              NOOP (type 1) advances by one byte; otherwise the option's length is its byte
 *              1, and a length below 2 or past the header's end ends the walk; an option whose
 *              type has bit 0x80 (copied) clear has all its bytes overwritten with 0x01.  ihl
 *              does not change;
 *   checksum   the header checksum filled as RPKT_BUILD_IP_CSUM fills it;
 *   L4 bytes   untouched: a filled UDP checksum stays what it was, over the whole datagram,
 *              which is UFO.
 *
 * IPv6.  Frame i is eligible iff the dispatch ethertype is 0x86DD (so the records were parsed
 * with RPKT_F_IPV6) and status is OK, L4_OTHER, UDP_SHORT, UDP_BAD_LEN, TCP_SHORT or
 * TCP_BAD_DOFF.  The extension headers are walked in the frame from x = l3 + 40 with the fixed
 * header's next_header, at most RPKT_MAX_IP6_EXT of them and while x < l4: types 0, 43 and 60
 * are 8 * (1 + byte x+1) long, type 51 is 4 * (2 + byte x+1); a type 44 anywhere makes the whole
 * frame pass through (it is a fragment or an atomic fragment already, and IPv6 is fragmented at
 * its source only); any other type ends the walk; a header that runs past l4 makes the frame pass
 * through.  U, the end of the per-fragment headers (RFC 8200: the headers every node on the
 * path looks at), is the end of the last Routing header met; without one the end of a
 * Hop-by-Hop header when that is the first header; otherwise l3 + 40.  With plen the fixed
 * header's payload_len (be16 at l3 + 4), E = l3 + 40 + plen and F = E - U, the frame is cut iff
 * l3 + 40 <= l4 <= E <= frame_len, 40 + plen > mtu, and c = (mtu - (U - l3) - 8) & ~7 is at
 * least 8.  It yields n_i = ceil(F / c) fragments; fragment k carries p_k = c bytes, the last
 * one the rest:
 *   bytes        [0, U) of the frame, an 8-byte Fragment header, then [U + k * c, + p_k);
 *   payload_len  (U - l3 - 40) + 8 + p_k;
 *   next header  the next-header byte of the last per-fragment header (byte l3 + 6 when there
 *                is none) becomes 44, and its old value the Fragment header's next_header;
 *   Fragment     byte 0 that next_header, byte 1 0, bytes 2..3 be16 (k * c) | (k < n_i - 1),
 *                bytes 4..7 be32 ip6_ident + i (mod 2^32; i the input frame's index).
 *
 * frag_first_dev, totals_dev, out_frames_dev, out_bytes, out_offsets_dev and out_cap are
 * rpkt_gpu_segment_batch's seg_first_dev, totals_dev (u64[2] = {n_out, out_bytes_needed}),
 * out_frames_dev, out_bytes, out_offsets_dev and out_cap word for word: the outputs of frame i
 * are [frag_first[i], frag_first[i+1]); the true offsets and the spare slots that equal
 * out_bytes_needed when the batch fits; on overflow frag_first_dev and totals_dev still exact
 * and the rest unspecified; nothing ever written outside [out_frames_dev, + out_bytes) and
 * out_offsets_dev[0..out_cap].
 * Bounds for sizing: every cut has c >= 8 and c >= cmin = (mtu - A - 8) & ~7, A the longest
 * per-fragment L3 header of the batch (ihl; U - l3), so n_out <= n + floor(frames_bytes /
 * max(8, cmin)); out_bytes_needed <= frames_bytes + (n_out - n) * H, H the longest l4_off
 * (IPv4) or U + 8 (IPv6) of the batch.
 * workspace_dev: rpkt_gpu_fragment_workspace_bytes(n) bytes, 16-byte aligned; calls that share
 * one must be ordered (one stream).  The call is plan, prefix sums and write on `stream` with
 * no host step: rpkt_gpu_parse_batch -> rpkt_gpu_fragment_batch -> rpkt_gpu_parse_batch over
 * out_cap slots captures as one graph.
 * The records must come from a parse of the same batch.  With other records the outputs are
 * unspecified, but every frame byte is read through the bounds-checked buffer resource and
 * every byte written through the one over the output, and a record whose offsets do not nest as
 * above makes the frame pass through: wrong frames, never a fault.
 * A tunnelled frame is to this entry what its outer record says: the OUTER IP packet is
 * fragmented, which is what a VTEP does with an encapsulation that is over the MTU.
 * Argument checks: rpkt_gpu_segment_batch's in its order (at enum rpkt_err).
 * Over mbuf chains: rpkt_gpu_fragment_chains, below.
 * Fragmenting the INNER packet of a tunnel instead: rpkt_gpu_fragment_tunnel_batch, below.
 * Not covered: an MTU per frame.  The receive-side inverse is rpkt_gpu_reassemble_batch,
 * below. */
#define RPKT_FRAGMENT_IGNORE_DF 1u   /* cut IPv4 packets that have DF set, too */

size_t rpkt_gpu_fragment_workspace_bytes(uint32_t n);
int rpkt_gpu_fragment_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev, uint32_t mtu,
                            uint32_t flags, uint32_t ip6_ident,
                            uint8_t* out_frames_dev, uint64_t out_bytes,
                            uint32_t* out_offsets_dev, uint32_t out_cap,
                            uint32_t* frag_first_dev, uint64_t* totals_dev,
                            void* workspace_dev, void* stream);

/* The same over mbuf chains.  A packet that needs fragmenting is larger than the MTU, and in a
 * DPDK port anything larger than one 2048-byte data room is a chain: every jumboframe_tx.rs
 * frame, a VTEP's encapsulated jumbo frame whose outer packet is over the MTU.
 * rpkt_gpu_fragment_chains reads the chains in place -- no gather into a flat batch first --
 * and writes wire frames, which are linear by nature.
 *
 * Let F_p be chain p's bytes in order under rpkt_chains_t's clamps (a = min(chain_first[p],
 * n_segs), b = min(max(chain_first[p+1], a), n_segs), each segment clamped to buf_bytes, empty
 * segments contributing nothing).  Every output -- out_frames_dev, out_offsets_dev,
 * frag_first_dev, totals_dev -- is byte for byte what rpkt_gpu_fragment_batch writes for the
 * packed batch F_0 .. F_{n_chains-1} with the same recs_dev, mtu, flags, ip6_ident, out_cap and
 * out_bytes: both rules (IPv4 with ip_options_fragment's NOOPs; IPv6 with the Fragment header
 * and identification ip6_ident + p), the pass-through of every chain that is not cut as a copy
 * of [0, pkt_len), the bytes after the IP packet's end dropped, the overflow contract, the
 * spare offset slots, nothing written outside the buffers.
 *   Records   recs_dev are normally rpkt_gpu_parse_chains' records of these chains
 *             (RPKT_F_IPV6 for IPv6): their offsets are logical positions in F_p already.  A
 *             header that straddles a segment boundary is a parse error there, so such a chain
 *             passes through.  The entry itself puts no condition on where segments are cut:
 *             with records that say "cut" (a parse of the flattened bytes), the IPv4 header
 *             with its options, the IPv6 extension-header walk up to l4_off, the copied header
 *             [0, l4_off) or [0, U) and the payload slices are gathered across any cuts.
 *   Nesting   pkt_len, the sum of the clamped segment lengths, takes frame_len's place in
 *             l3 + L <= frame_len and E <= frame_len.
 *   Overlap   segments may overlap or be shared between chains: the arena is only read.
 *   Huge      pkt_len is summed in 64 bits for totals_dev; a chain of 4 GiB or more cannot
 *             fit out_bytes, so the call ends as an overflow.
 *   Faults    every arena load goes through the buffer resource over [buf_dev, + buf_bytes)
 *             and every store through one over the output: wrong records give wrong frames,
 *             never a fault.
 *   Limits    no cap on the segments of a chain (many tiny segments are slow, not wrong).
 * flags: 0 or RPKT_FRAGMENT_IGNORE_DF.  workspace_dev:
 * rpkt_gpu_fragment_chains_workspace_bytes(n_chains) bytes (equal to
 * rpkt_gpu_fragment_workspace_bytes(n_chains)), 16-byte aligned; calls that share one must be
 * ordered.  No host step: rpkt_gpu_parse_chains -> rpkt_gpu_fragment_chains ->
 * rpkt_gpu_parse_batch over out_cap slots captures as one graph.
 * Bounds for sizing: rpkt_gpu_fragment_batch's with the sum of the chains' pkt_len in
 * frames_bytes' place; that sum is at most buf_bytes when segments do not overlap.
 * A tunnelled chain is to this entry what its outer record says: with the outer records of
 * rpkt_gpu_parse_tunnel_chains the OUTER IP packet is fragmented.
 * Argument checks: rpkt_gpu_segment_chains' in its order, with mtu in mss's place and
 * RPKT_FRAGMENT_IGNORE_DF the only flag (at enum rpkt_err).
 * Not covered: what rpkt_gpu_fragment_batch does not cover; reassembly or coalescing over
 * chains; a chain-shaped output. */
size_t rpkt_gpu_fragment_chains_workspace_bytes(uint32_t n_chains);
int rpkt_gpu_fragment_chains(const rpkt_chains_t* chains, const rpkt_rec_t* recs_dev, uint32_t mtu,
                             uint32_t flags, uint32_t ip6_ident,
                             uint8_t* out_frames_dev, uint64_t out_bytes,
                             uint32_t* out_offsets_dev, uint32_t out_cap,
                             uint32_t* frag_first_dev, uint64_t* totals_dev,
                             void* workspace_dev, void* stream);

/* Fragmenting the inner packet of a tunnel.  An encapsulation that is over the MTU can leave as
 * fragments of the OUTER packet (rpkt_gpu_fragment_batch with the outer records), which makes
 * the tunnel egress reassemble before it can decapsulate, leaves only the first fragment with
 * the outer UDP header (ECMP and RSS spread one datagram's fragments) and is dropped by many
 * middleboxes (RFC 4459 section 3.1, RFC 2003 section 5.1).  rpkt_gpu_fragment_tunnel_batch
 * fragments the inner IPv4 packet before the encapsulation instead (RFC 4459 section 3.2; the
 * "pre-fragmentation" of GRE / IPsec routers): every output is a complete tunnel packet with
 * its own outer headers that is decapsulated on its own, and the destination host reassembles.
 *
 * outer_dev, tun_dev, inner_dev: the three outputs of rpkt_gpu_parse_tunnel_batch on this
 * batch (level 1).  They only locate things; every header byte is read from the frame.  mtu,
 * 1..65535: the L3 MTU of the link the OUTER packet leaves on.  flags: any combination of
 * RPKT_FRAGMENT_IGNORE_DF and RPKT_FRAGMENT_TUNNEL_OUTER.  With O, T, I frame i's outer, tunnel
 * and inner record:
 *   1. No tunnel (T.kind == RPKT_TUN_NONE): the frame is handled exactly as
 *      rpkt_gpu_fragment_batch handles it with record O and the same mtu, IGNORE_DF and
 *      ip6_ident: its IPv4 and its IPv6 rule.  A mixed transmit batch needs one call.
 *   2. Inner cut.  Let over = I.l3_off - O.l3_off: everything the tunnel puts in front of the
 *      inner IP header, from the outer IP header through the inner Ethernet header and tags.
 *      The frame is inner-cut iff T.status == RPKT_T_OK; the carrier is one
 *      rpkt_gpu_segment_tunnel_batch accepts (outer IPv4 or IPv6 and not itself a fragment;
 *      VXLAN / GTP-U: O.status OK, protocol 17, l4 + 8 <= tun_off; GRE: protocol 47, l4 ==
 *      tun_off, S and R clear, room for the C word; tun_off + 8 (GRE: + 4, with C + 8) <=
 *      inner_off <= I.l3_off); I's dispatch ethertype is 0x0800 and I.status is one under which
 *      the IPv4 header parsed (rpkt_gpu_fragment_batch's list); mtu > over; and
 *      rpkt_gpu_fragment_batch's IPv4 rule says "cut" for the inner packet at mtu' = mtu -
 *      over with l3 = I.l3_off, l4 = I.l4_off and the outer frame's frame_len (l4 == l3 + ihl;
 *      l3 + L <= frame_len; L > mtu'; DF clear or IGNORE_DF; c = (mtu' - ihl) & ~7 >= 8; the
 *      13-bit offset does not overflow).  An inner packet that is already a fragment is cut
 *      again.  Fragment k, with p_k as in that rule and tot = I.l4_off + p_k:
 *        bytes        [0, I.l4_off) of the frame, then [I.l4_off + k * c, + p_k); nothing after
 *                     the inner IP packet's end is carried;
 *        inner IPv4   exactly what rpkt_gpu_fragment_batch writes for the inner packet on its
 *                     own: packet_len, the frag word (offset, MF; DF and reserved 0),
 *                     ip_options_fragment's NOOPs in fragments k > 0, the header checksum; the
 *                     inner L4 bytes are untouched;
 *        outer        exactly what rpkt_gpu_segment_tunnel_batch writes for an output of total
 *                     length tot: the GTP-U length, the GRE checksum with C (0 stays 0), the
 *                     outer UDP length and checksum (an input field of 0 stays 0; otherwise
 *                     filled over the pseudo header, ip6_pdst_off rule, 0 -> 0xffff), the outer
 *                     IPv4 packet_len, ident + k and checksum, or the outer IPv6 payload_len.
 *                     The outer DF is copied: every output fits the link.  Length fields are
 *                     taken mod 2^16.
 *      Every output's outer IP packet is therefore at most mtu bytes long.
 *   3. Everything else with a tunnel (kind != NONE: a tunnel that did not decode; inner IPv6,
 *      which a tunnel ingress never fragments, RFC 8200 section 5 and RFC 2473 section 7.1;
 *      inner DF without the flag; GRE with S or R; offsets that do not nest; an inner packet
 *      that fits).  Without RPKT_FRAGMENT_TUNNEL_OUTER the frame passes through as a byte copy
 *      of [0, frame_len): the caller owes an ICMP "fragmentation needed" / "packet too big".
 *      With the flag it is handled as in rule 1 with record O: the outer packet is fragmented
 *      if that rule cuts it.
 * ip6_ident + i is used by rules 1 and 3 only.
 * The outputs, frag_first_dev, totals_dev, the overflow behaviour, the spare offset slots and
 * "nothing written outside the buffers" are rpkt_gpu_fragment_batch's, word for word; every
 * load goes through the frames buffer resource and every store through the output's, so wrong
 * records give wrong frames, never a fault.  The call is plan, prefix sums and write on
 * `stream` with no host step: rpkt_gpu_parse_tunnel_batch -> rpkt_gpu_fragment_tunnel_batch ->
 * rpkt_gpu_parse_tunnel_batch over out_cap slots captures as one graph.
 * workspace_dev: rpkt_gpu_fragment_tunnel_workspace_bytes(n) bytes (a 64-byte plan a frame),
 * 16-byte aligned; calls that share one must be ordered.
 * Bounds for sizing: n_out <= n + floor(frames_bytes / max(8, cmin)), cmin = (mtu - A) & ~7, A
 * the longest per-fragment prefix from the outer L3 on: over + ihl for an inner cut,
 * rpkt_gpu_fragment_batch's A + 8 otherwise.  out_bytes_needed <= frames_bytes + (n_out - n) *
 * H, H the longest copied header: I.l4_off for an inner cut, rpkt_gpu_fragment_batch's H
 * otherwise.
 * Argument checks: rpkt_gpu_segment_tunnel_batch's in its order, with mtu in mss's place and
 * the two flags (at enum rpkt_err).
 * Not covered: mbuf chains; nested tunnels (only the level-1 records are accepted); an MTU per
 * frame; inner IPv6; GRE sequence numbers.  Reassembling the inner packet at the tunnel egress
 * is not built and not needed: the destination host reassembles. */
#define RPKT_FRAGMENT_TUNNEL_OUTER 2u  /* a tunnelled frame whose inner packet is not cut: cut its outer packet */

size_t rpkt_gpu_fragment_tunnel_workspace_bytes(uint32_t n);
int rpkt_gpu_fragment_tunnel_batch(const rpkt_batch_t* batch, const rpkt_rec_t* outer_dev,
                                   const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                   uint32_t mtu, uint32_t flags, uint32_t ip6_ident,
                                   uint8_t* out_frames_dev, uint64_t out_bytes,
                                   uint32_t* out_offsets_dev, uint32_t out_cap,
                                   uint32_t* frag_first_dev, uint64_t* totals_dev,
                                   void* workspace_dev, void* stream);

/* ---- IPv4 / IPv6 reassembly --------------------------------------------------------- */

/* The receive-side inverse of rpkt_gpu_fragment_batch.  Without it a fragmented datagram is lost
 * to the receive path: the parser reports an IPv6 fragment as RPKT_S_IP6_FRAGMENT with no upper
 * layer, parses a non-first IPv4 fragment as if its payload were an L4 header, and a VTEP whose
 * peer fragmented an over-MTU encapsulation cannot get at the inner frame.
 * rpkt_gpu_reassemble_batch merges consecutive positions that hold consecutive fragments of one
 * datagram into one frame on the device.  The output is the complete batch in position order:
 * every position ends up in exactly one output frame.  The rule is per position and local: no
 * table, no timers, one batch.  rpkt_gpu_reassemble_keys, below, gives the order that brings a
 * datagram's fragments to consecutive positions.
 *
 * recs_dev: the rpkt_rec_t records of a parse of this same batch (RPKT_F_IPV6 for IPv6 fragments;
 * RPKT_F_IP_SUM unless RPKT_REASSEMBLE_TRUST_SUMS).  They only locate things and give the
 * verdict -- status, the dispatch ethertype, l3_off, l4_off, ip_sum -- and every header byte is
 * read from the frame.  order_dev (optional, n entries): position i holds frame order[i] (NULL:
 * frame i).  An entry >= n makes its position an empty frame: never read, a zero-length output.
 * It need not be a permutation.  flags: 0 or RPKT_REASSEMBLE_TRUST_SUMS.  Below l3 = l3_off,
 * l4 = l4_off.
 *
 * A position is an eligible IPv4 FRAGMENT iff all of these hold, with ihl (the low nibble of
 * byte l3, times 4), L (be16 at l3 + 2) and the frag word fw (be16 at l3 + 6) from the frame:
 *   - the dispatch ethertype is 0x0800 and status is one under which the IPv4 header parsed:
 *     OK, L4_OTHER, UDP_SHORT, UDP_BAD_LEN, TCP_SHORT, TCP_BAD_DOFF, ICMP_EMPTY;
 *   - ihl in 20..60 and l4 == l3 + ihl;
 *   - l3 + L <= frame_len and P = L - ihl >= 1;
 *   - (fw & 0x3fff) != 0: MF set, or an offset;
 *   - with off = (fw & 0x1fff) * 8, ihl + off + P <= 65535, so no merge overflows packet_len;
 *   - without TRUST_SUMS, ip_sum == 0xffff.
 * A position is an eligible IPv6 FRAGMENT iff all of these hold, with x the start of its
 * Fragment header:
 *   - the dispatch ethertype is 0x86DD and status is RPKT_S_IP6_FRAGMENT;
 *   - x = l4 - 8 >= l3 + 40;
 *   - a walk in the frame from l3 + 40 with the fixed header's next_header, at most
 *     RPKT_MAX_IP6_EXT headers, meets only types 0, 43 and 60 (each 8 * (1 + byte 1) long) and 51
 *     (4 * (2 + byte 1) long) and arrives exactly at x with type 44;
 *   - with E = l3 + 40 + payload_len (be16 at l3 + 4), E <= frame_len and P = E - (x + 8) >= 1;
 *   - with off = be16 at x + 2 masked with 0xfff8 and M its bit 0, (x - l3 - 40) + 8 + off + P
 *     <= 65535, so no merge overflows payload_len.
 * An atomic fragment (offset 0, M clear) is parsed on by rpkt_gpu_parse_batch and is never
 * eligible.
 *
 * B(i), "position i continues position i - 1" (B(0) false), holds iff both are eligible and of
 * the same IP version with equal l3 and l4; position i - 1 has MF / M set and P_{i-1} % 8 == 0;
 * off_i == off_{i-1} + P_{i-1}; and
 *   IPv4: bytes [0, l3) are equal, and ident, protocol, source and destination.  TOS, TTL, the
 *         options, DF and the reserved bit are the head's and are not compared;
 *   IPv6: bytes [0, x + 8) are equal, ignoring l3+4..5 (payload_len) and x+2..3 (offset, M): so
 *         every extension header before the Fragment header, its next_header and the
 *         identification match.
 * A run of links is one group: there is no greedy cut, the 65535 conditions above already bound
 * every merge.  Overlapping, duplicated and out-of-order fragments do not link and pass through.
 *
 * Outputs, in position order, one per group:
 *   a group of one position   a byte copy of [0, frame_len), padding included;
 *   a merged IPv4 group       the head's bytes [0, l4), then every member's [l4, l4 + P) in order
 *                             (Ethernet padding is not carried); packet_len = ihl + the total;
 *                             the frag word the head's with MF replaced by the last member's; the
 *                             header checksum filled as RPKT_BUILD_IP_CSUM fills it;
 *   a merged IPv6 group that is not complete
 *                             the head's bytes [0, x + 8), then every member's [x + 8, + P);
 *                             payload_len = (x - l3 - 40) + 8 + the total; bytes 2..3 of the
 *                             Fragment header = the head's offset | the last member's M;
 *   a merged IPv6 group that is complete (the head's offset 0, the last member's M clear)
 *                             the Fragment header is removed: the head's bytes [0, x) with the
 *                             next-header byte of the last header before x (byte l3 + 6 when
 *                             there is none) set to the Fragment header's byte 0, then the
 *                             payloads; payload_len = (x - l3 - 40) + the total.
 * A complete IPv4 group needs no other treatment: its frag word comes out 0 but for the head's DF
 * and reserved bit.  A partial merge is a valid, larger fragment, so the entry composes: a second
 * call, or a later batch that carries the partial outputs along, finishes the merge; this is the
 * inverse of "a fragment is cut again like any other".
 * The inverse property: reassemble(fragment(F)) == F byte for byte, whatever the mtu and also for
 * frames that were fragments already, for every frame F whose IP packet ends at the frame's end
 * and whose IPv4 frag word has DF and the reserved bit clear; for the others it is F without its
 * padding and without those two bits, which rpkt_gpu_fragment_batch drops.
 *
 * src_first_dev (n + 1 entries: output j is made of positions [src_first[j], src_first[j+1]);
 * entries n_out+1..n equal n), totals_dev, out_frames_dev, out_bytes, out_offsets_dev and out_cap
 * are rpkt_gpu_coalesce_batch's word for word: totals {n_out, out_bytes_needed} and src_first
 * exact on overflow with the rest unspecified, spare offset slots equal out_bytes_needed, nothing
 * ever written outside [out_frames_dev, + out_bytes) and out_offsets_dev[0..out_cap].
 * Bounds for sizing: n_out <= n; out_bytes_needed <= the sum of the positions' frame lengths.
 * workspace_dev: rpkt_gpu_reassemble_workspace_bytes(n) bytes, 16-byte aligned; calls that share
 * one must be ordered.  The call is plan, prefix sums and write on `stream` with no host step:
 * parse -> keys -> (the caller's sort) -> reassemble -> parse captures as one graph.  Records from
 * another batch give wrong frames but never a fault: every load of frame bytes goes through the
 * frames buffer resource, every store through the one over the output, and offsets that do not
 * nest make a position ineligible.
 * Argument checks: rpkt_gpu_coalesce_batch's in its order, without a max_payload (at enum
 * rpkt_err).
 * Not covered: state across batches (timers, a fragment table: a caller carries partial outputs
 * into the next batch); overlap resolution; mbuf chains; the inner packet of a tunnel (to this
 * entry a tunnelled frame is what its outer record says: the OUTER fragments are merged, and
 * rpkt_gpu_parse_tunnel_batch of the output reaches the inner frame); an output cap below
 * 65,535. */
#define RPKT_REASSEMBLE_TRUST_SUMS 1u   /* do not require a valid IPv4 header sum */

size_t rpkt_gpu_reassemble_workspace_bytes(uint32_t n);
int rpkt_gpu_reassemble_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev,
                              const uint32_t* order_dev,      /* optional, n entries */
                              uint32_t flags,
                              uint8_t* out_frames_dev, uint64_t out_bytes,
                              uint32_t* out_offsets_dev, uint32_t out_cap,
                              uint32_t* src_first_dev,        /* n + 1 entries */
                              uint64_t* totals_dev, void* workspace_dev, void* stream);

/* The sort keys that order a batch for rpkt_gpu_reassemble_batch.  Flow events key on the
 * 5-tuple of an L4 header that fragments after the first do not have, so they cannot order
 * fragments.  keys_dev[i] (n entries, 8-byte aligned), with the eligibility above (same flags):
 *   an eligible fragment   (h & 0x7fffffff) << 32 | off / 8, h = rpkt_flow_hash(src, dst,
 *                          ident & 0xffff, ident >> 16, proto): IPv4 the record's ip_src / ip_dst,
 *                          the 16-bit ident and the protocol from the frame; IPv6 the record's
 *                          ip6_src_fold / ip6_dst_fold, the 32-bit identification and 44;
 *   every other frame      1 << 63 | i.
 * A stable ascending sort of the keys as unsigned 64-bit numbers (the caller's: any device or
 * host sort) is an order_dev: each datagram's fragments adjacent and ascending in offset
 * whatever their arrival order, every non-fragment after them in arrival order.  A hash collision
 * only interleaves two datagrams, which then merge less: the link compares the real bytes.
 * One launch on `stream`. */
int rpkt_gpu_reassemble_keys(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev,
                             uint32_t flags, uint64_t* keys_dev /* n, 8-B aligned */, void* stream);

/* ---- TCP and UDP receive coalescing (GRO / LRO, UDP GRO) --------------------------- */

/* The receive-side counterpart of rpkt_gpu_segment_batch: rpkt-dpdk/examples/lro_rx.rs turns
 * on the port's LRO offload (rx_offloads bit 4, with scatter) and reads each COALESCED TCP
 * frame's seq_num, ack_num, psh, window_size and payload_len (lro_rx.rs:81-99).
 * rpkt_gpu_coalesce_batch merges consecutive in-order TCP segments of one flow into one frame
 * on the device, for frames that stay in HBM, so a receive loop pays one record and one
 * downstream step per application write instead of one per wire segment.  The output is the
 * complete batch in position order: every position ends up in exactly one output frame.
 *
 * recs_dev: the rpkt_rec_t records of a parse of this same batch (RPKT_F_IPV6 for IPv6
 * frames; RPKT_F_IP_SUM | RPKT_F_L4_SUM unless RPKT_COALESCE_TRUST_SUMS).  As for
 * rpkt_gpu_segment_batch the records locate things and give the verdicts -- status, the
 * dispatch ethertype, ip_protocol, ip_frag, l3_off, l4_off, payload_off, payload_len,
 * ip6_pdst_off, ip_sum, l4_sum -- and every header byte is taken from the frame.
 * order_dev (optional, n entries): position i holds frame order[i] (NULL: frame i), for
 * bursts whose flows interleave (a stable sort of the flow events' buckets).  An entry >= n
 * makes its position an empty frame: never read, a zero-length output.  It need not be a
 * permutation.  max_payload: 1..65535, the largest merged payload.  flags: 0 or any of
 * RPKT_COALESCE_TRUST_SUMS and RPKT_COALESCE_UDP (coalesce UDP datagrams too, below).
 *
 * A frame is ELIGIBLE iff status == RPKT_S_OK, ip_protocol == 6, for IPv4
 * (ip_frag & 0x3fff) == 0, payload_len >= 1, its offsets nest as segmentation requires, SYN
 * (0x02), RST (0x04) and URG (0x20) are clear in TCP byte 13 and, without TRUST_SUMS,
 * l4_sum == 0xffff and for IPv4 ip_sum == 0xffff (a coalescer that refreshes checksums must
 * not launder a corrupt segment).
 * B(i), "position i continues position i - 1" (B(0) false): both frames eligible, the same IP
 * version, equal l3_off, l4_off and payload_off; header bytes [0, payload_off) equal, ignoring
 * only IPv4 bytes l3+2..5 (length, ident) and l3+10..11 (checksum), IPv6 bytes l3+4..5, TCP
 * bytes l4+4..7 (seq), the FIN, PSH and CWR bits of byte l4+13 and bytes l4+16..17 (checksum)
 * -- so MACs, tags, addresses, TOS, TTL, DF, IP options and extension headers, ports, ack,
 * window, the other flag bits and every TCP option byte match; seq_i == seq_{i-1} +
 * payload_len_{i-1} (mod 2^32); for IPv4 with DF clear ident_i == ident_{i-1} + 1 (mod 2^16),
 * with DF set ident is ignored; frame i - 1 carries neither FIN nor PSH; frame i no CWR.
 * With p = payload_len:  short(i) = B(i) && p_i < p_{i-1};
 *                        link(i)  = B(i) && p_i <= p_{i-1} && !short(i-1).
 * So within a run of links every frame but the last has the head's payload length, and a
 * short frame ends its run.  The rule looks at three neighbouring positions only (it is not
 * Linux's sequential state machine): it loses a merge only after two successive shrinking
 * segments.  A run is cut greedily into groups: a linked frame joins the current group while
 * the group's payload stays <= min(max_payload, 65535 - ip_hdrs), ip_hdrs = payload_off -
 * l3_off (IPv4) or payload_off - l3_off - 40 (IPv6).
 *
 * With RPKT_COALESCE_UDP, TCP frames are handled as above and UDP datagrams are merged under
 * the Linux udp_gro_receive_segment rules (the UDP_GRO socket option, DPDK's rte_gro UDP
 * path).  A UDP frame is ELIGIBLE iff status == RPKT_S_OK, ip_protocol == 17, it is no IPv4
 * fragment, payload_len >= 1, its offsets nest with payload_off - l4_off == 8, its UDP checksum
 * field is not 0 (also under TRUST_SUMS: a datagram sent without a checksum is never merged)
 * and, without TRUST_SUMS, l4_sum == 0xffff and for IPv4 ip_sum == 0xffff.  B(i) for two UDP
 * frames: both eligible, the same IP version, equal l3_off, l4_off and payload_off; header
 * bytes [0, payload_off) equal, ignoring the IP bytes above and UDP bytes l4+4..7 (length,
 * checksum); the IPv4 ident rule as for TCP; no sequence and no flag condition.  The protocol
 * byte is compared, so a TCP frame never continues a UDP one.  short, link and the greedy cut
 * are the same, so a run is datagrams of one size ending in at most one shorter one.  The
 * rule is not Linux's sequential state machine here either, and Linux's cap of 64 datagrams
 * per merge is not applied: min(max_payload, 65535 - ip_hdrs) is the only limit.
 *
 * Outputs, in position order, one per group:
 *   a group of one frame   a byte copy of [0, frame_len), padding included;
 *   a merged group         the head's bytes [0, payload_off), then every member's
 *                          [payload_off, + payload_len) in order (Ethernet padding is not
 *                          carried); IPv4 packet_len / IPv6 payload_len set for the total; the
 *                          head's IPv4 ident; the IPv4 checksum filled as RPKT_BUILD_IP_CSUM
 *                          fills it; the head's TCP seq, ack, window and options; flags = the
 *                          head's ORed with the last member's FIN and PSH; the TCP checksum
 *                          filled as segmentation fills it (the IPv6 pseudo destination from the
 *                          head's ip6_pdst_off under rpkt_gpu_build_batch's rule; 0 stays 0);
 *                          for UDP the head's ports, UDP length = 8 + the total payload and the
 *                          UDP checksum filled as segmentation fills it (0 written as 0xffff);
 *   src_first_dev  n + 1 entries: output j is made of positions [src_first[j],
 *                  src_first[j+1]); entries n_out+1..n equal n; exact whatever the capacities;
 *   out_mss_dev    optional, n entries: the head's payload_len for a merged output, 0 for a
 *                  copied one and for entries >= n_out -- the gso_size a later
 *                  rpkt_gpu_segment_batch needs, and the one UDP_GRO hands the socket; exact
 *                  whatever the capacities;
 *   totals_dev, out_frames_dev, out_offsets_dev, out_cap: rpkt_gpu_segment_batch's contract
 *                  exactly -- totals {n_out, out_bytes_needed} exact on overflow, spare offset
 *                  slots equal out_bytes_needed, nothing written outside the buffers.
 * Bounds for sizing: n_out <= n; out_bytes_needed <= the sum of the positions' frame lengths.
 * workspace_dev: rpkt_gpu_coalesce_workspace_bytes(n) bytes, 16-byte aligned; calls that share
 * one must be ordered.  The call is plan, prefix sums and write on `stream` with no host step:
 * parse -> coalesce captures as one graph.  Records from another batch give unspecified output
 * but never a fault: all loads go through the frames buffer resource and offsets that do not
 * nest make a frame ineligible.
 * Not covered: mbuf chains, the inner TCP or UDP of tunnelled frames (to this entry a tunnelled
 * frame is what its outer record says; rpkt_gpu_coalesce_tunnel_batch, below, merges the inner
 * flow), keeping an IPv4 "no checksum" across a merge. */
#define RPKT_COALESCE_TRUST_SUMS 1u   /* do not require valid sums in the records */
#define RPKT_COALESCE_UDP 16u   /* also coalesce UDP datagrams */

size_t rpkt_gpu_coalesce_workspace_bytes(uint32_t n);
int rpkt_gpu_coalesce_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev,
                            const uint32_t* order_dev,      /* optional, n entries */
                            uint32_t max_payload, uint32_t flags,
                            uint8_t* out_frames_dev, uint64_t out_bytes,
                            uint32_t* out_offsets_dev, uint32_t out_cap,
                            uint32_t* src_first_dev,        /* n + 1 entries */
                            uint16_t* out_mss_dev,          /* optional, n entries */
                            uint64_t* totals_dev, void* workspace_dev, void* stream);

/* Coalescing of the inner TCP / UDP of tunnels: the receive side of a VTEP or UPF, the inverse
 * of rpkt_gpu_segment_tunnel_batch.  To rpkt_gpu_coalesce_batch a tunnelled frame is an outer UDP
 * datagram or a GRE packet; this entry merges the segments of the INNER flow and repairs every
 * outer length and checksum, as Linux does in udp_gro_receive -> vxlan_gro_receive and in
 * gre_gro_receive.  coalesce(segment(F)) == F for every frame the tunnel cut accepts.
 *
 * outer_dev, tun_dev, inner_dev: the three outputs of rpkt_gpu_parse_tunnel_batch on this same
 * batch (level 1; RPKT_F_IPV6 for IPv6 at either level; RPKT_F_IP_SUM | RPKT_F_L4_SUM unless
 * RPKT_COALESCE_TRUST_SUMS).  The records locate things and give the verdicts; every header byte
 * is taken from the frame.  order_dev (entries >= n make empty positions; it need not be a
 * permutation), max_payload 1..65535, flags (0 or any of RPKT_COALESCE_TRUST_SUMS and
 * RPKT_COALESCE_UDP), the outputs, src_first_dev, out_mss_dev, totals_dev, the overflow
 * behaviour, the spare offset slots, "nothing written outside the buffers" and "plan, prefix
 * sums and write on `stream` with no host step" are rpkt_gpu_coalesce_batch's contract word for
 * word.  Below O, T, I are position i's outer, tunnel and inner record; ipo = I.payload_off, p =
 * I.payload_len clamped to the frame, tot = ipo + p, toff = T.tun_off, ioff = T.inner_off.
 *
 * ELIGIBLE:
 *   No tunnel   T.kind == RPKT_TUN_NONE: the position is eligible, compared and merged exactly
 *               as rpkt_gpu_coalesce_batch treats it with record O.  It never continues a
 *               tunnelled position and a tunnelled position never continues it: a mixed receive
 *               burst needs this one call only.
 *   Undecoded   T.kind != NONE and T.status != RPKT_T_OK: never eligible, a byte copy.  Its
 *               outer UDP is never merged, with or without RPKT_COALESCE_UDP.
 *   Decoded     eligible iff all of these hold:
 *               - inner: I is eligible under rpkt_gpu_coalesce_batch's TCP rule, or with
 *                 RPKT_COALESCE_UDP its UDP rule (a zero inner UDP checksum is never merged);
 *                 I's offsets are positions in the outer frame and nest within frame_len; the
 *                 verdicts (status, ip_sum, l4_sum) are I's;
 *               - carrier: what rpkt_gpu_segment_tunnel_batch asks of a frame it cuts: O IPv4 or
 *                 IPv6 by its dispatch ethertype and no fragment, O.l3_off + 20 (IPv6: + 40) <=
 *                 O.l4_off, an IPv4 header within 60 bytes; VXLAN / GTP-U: O.status ==
 *                 RPKT_S_OK, ip_protocol 17, O.l4_off + 8 <= toff; GRE: ip_protocol 47, O.l4_off
 *                 == toff; toff + 8 (GRE: + 4, with the C bit + 8) <= ioff <= I.l3_off; the GRE S
 *                 and R bits clear;
 *               - lengths agree, with or without TRUST_SUMS: every length field a merge rewrites
 *                 says tot already: outer IPv4 packet_len == tot - O.l3_off or outer IPv6
 *                 payload_len == tot - O.l3_off - 40; VXLAN / GTP-U: outer UDP length == tot -
 *                 O.l4_off; GTP-U length == tot - toff - 8.  Bytes of the frame past tot (outer
 *                 Ethernet padding) are allowed and not carried, as in the flat rule.  A frame
 *                 with bytes between the inner packet's end and the outer packet's end (the
 *                 padding of an inner Ethernet frame) is not merged: a merge would drop bytes a
 *                 length field counts (Linux's inet_gro_receive flushes on the same mismatch);
 *               - outer sums, without TRUST_SUMS: outer IPv4: O.ip_sum == 0xffff; VXLAN / GTP-U:
 *                 the frame's outer UDP checksum field is 0, or O.l4_sum == 0xffff; GRE with C:
 *                 O.l4_sum == 0xffff.
 * B(i) for two decoded positions: both eligible; equal T.kind, outer IP version, inner IP
 * version and L4 protocol; equal O.l3_off, O.l4_off, toff, ioff, I.l3_off, I.l4_off, ipo; header
 * bytes [0, ipo) equal, ignoring only the inner bytes the flat rule ignores (relative to I's
 * l3_off / l4_off), outer IPv4 bytes ol3+2..5 and ol3+10..11, outer IPv6 bytes ol3+4..5, outer
 * UDP bytes ol4+4..7, GTP-U bytes toff+2..3 and GRE-with-C bytes toff+4..5; the two outer UDP
 * checksum fields both 0 or both not 0 (Linux: !uh->check ^ !uh2->check); the flat rule's inner
 * sequence, inner ident and FIN / PSH / CWR conditions; for outer IPv4 with DF clear ident_i ==
 * ident_{i-1} + 1 (mod 2^16), with DF set the outer ident is ignored.  So outer MACs, tags,
 * addresses, TOS / TTL and ports (VXLAN source-port entropy is per inner flow), VNI / TEID / key
 * and every other tunnel header byte match, GTP-U sequence, N-PDU and extension headers
 * included.
 * short, link and the greedy cut are the flat rule's with p the inner payload length; a group's
 * payload stays <= min(max_payload, 65535 - inner ip_hdrs, 65535 - (ipo - O.l3_off)) (outer
 * IPv6: 65535 - (ipo - O.l3_off - 40)), so every 16-bit length field fits.
 * A merged output: the head's bytes [0, ipo), then every member's [ipo, + p) in order; the inner
 * headers as rpkt_gpu_coalesce_batch writes a merged frame's; the tunnel and outer headers as
 * rpkt_gpu_segment_tunnel_batch writes them for segment 0 of a frame whose total is the merged
 * one: the GTP-U length; the GRE checksum with C (0 stays 0); the outer UDP length; the outer
 * UDP checksum (an input field of 0 stays 0 over IPv4 and IPv6, else filled, 0 written as
 * 0xffff, the IPv6 pseudo destination under rpkt_gpu_build_batch's rule); the outer IPv4
 * packet_len, the head's ident, the checksum refilled; the outer IPv6 payload_len.
 * out_mss_dev[j] is the head's inner payload length.  A group of one is a byte copy of
 * [0, frame_len).  rpkt_gpu_parse_tunnel_batch with RPKT_F_FLOW_EV keys its events by the inner
 * flow, so a stable sort of their buckets is the order_dev of an interleaved burst.
 * workspace_dev: rpkt_gpu_coalesce_tunnel_workspace_bytes(n) bytes, 16-byte aligned.
 * Argument checks: rpkt_gpu_coalesce_batch's in its order, with tun_dev and inner_dev required
 * and 16-byte aligned along with outer_dev, as in rpkt_gpu_segment_tunnel_batch.
 * Records from another batch give unspecified frames but never a fault: every frame load goes
 * through the frames buffer resource, every output store through the output's, and offsets
 * that do not nest make a position ineligible.
 * Not covered: mbuf chains, nested tunnels (only the level-1 records are accepted), a stream
 * whose GTP-U sequence number runs on (the sequence bytes are compared, so it does not merge),
 * GRE sequence numbers, turning a zero outer UDP checksum into a filled one, Linux's sequential
 * state machine. */
size_t rpkt_gpu_coalesce_tunnel_workspace_bytes(uint32_t n);
int rpkt_gpu_coalesce_tunnel_batch(const rpkt_batch_t* batch, const rpkt_rec_t* outer_dev,
                                   const rpkt_tun_t* tun_dev, const rpkt_rec_t* inner_dev,
                                   const uint32_t* order_dev,      /* optional, n entries */
                                   uint32_t max_payload, uint32_t flags,
                                   uint8_t* out_frames_dev, uint64_t out_bytes,
                                   uint32_t* out_offsets_dev, uint32_t out_cap,
                                   uint32_t* src_first_dev,        /* n + 1 entries */
                                   uint16_t* out_mss_dev,          /* optional, n entries */
                                   uint64_t* totals_dev, void* workspace_dev, void* stream);

/* ---- Option iterators ----------------------------------------------------------- */

/* Why an option walk stopped (the iterator's next() returned None). */
enum rpkt_opt_stop {
    RPKT_OPT_NONE = 0,       /* no option slice: that header was not parsed */
    RPKT_OPT_END = 1,        /* the slice was consumed (buf.len() < 1) */
    RPKT_OPT_UNKNOWN = 2,    /* a type outside the option group */
    RPKT_OPT_MALFORMED = 3   /* the type's parse returned Err (short or bad length) */
};

/* Option kind indices (bits of *_kinds, 4-bit codes index + 1 in *_trace).
 * TCP (tcp/generated.rs:1357-1366): 0 Eol, 1 Nop, 2 Mss, 3 WindowScale,
 *   4 SackPermitted, 5 Sack, 6 Timestamp, 7 FastOpen.
 * IPv4 (ipv4/generated.rs:1595-1604): 0 Eol, 1 Nop, 2 Timestamp (68),
 *   3 RecordRoute (7), 4 RouteAlert (148), 5 CommercialSecurity (134),
 *   6 StrictSourceRoute (137), 7 LooseSourceRoute (131). */

/* One frame's option walks, 64 bytes: TcpOptionsIter over tcp.var_header_slice()
 * and Ipv4OptionsIter over ipv4.var_header_slice(), with the getters of the options
 * they yield (the last one of each kind). */
typedef struct rpkt_opts {
    uint8_t  tcp_count;         /*  0 options yielded                         */
    uint8_t  tcp_stop;          /*  1 rpkt_opt_stop                           */
    uint8_t  tcp_wscale;        /*  2 WindowScale::shift_count                */
    uint8_t  tcp_sack_blocks;   /*  3 (Sack::header_len - 2) / 8              */
    uint16_t tcp_kinds;         /*  4 bit k: kind index k yielded             */
    uint16_t tcp_mss;           /*  6 Mss::mss                                */
    uint32_t tcp_ts;            /*  8 Timestamp::ts                           */
    uint32_t tcp_ts_echo;       /* 12 Timestamp::ts_echo                      */
    uint32_t tcp_sack_left;     /* 16 first SACK block (Sack var_header_slice) */
    uint32_t tcp_sack_right;    /* 20                                         */
    uint16_t tcp_fo_len;        /* 24 FastOpen::header_len                    */
    uint8_t  tcp_end;           /* 26 slice bytes consumed when the walk stopped */
    uint8_t  ip_end;            /* 27                                         */
    uint8_t  ip_count;          /* 28                                         */
    uint8_t  ip_stop;           /* 29                                         */
    uint16_t ip_kinds;          /* 30                                         */
    uint16_t ip_route_alert;    /* 32 RouteAlert::data                        */
    uint8_t  ip_rr_len;         /* 34 RecordRoute::header_len                 */
    uint8_t  ip_rr_pointer;     /* 35 RecordRoute::pointer                    */
    uint8_t  ip_ts_len;         /* 36 Timestamp::header_len                   */
    uint8_t  ip_ts_pointer;     /* 37 Timestamp::pointer                      */
    uint8_t  ip_ts_oflw_flg;    /* 38 oflw << 4 | flg                         */
    uint8_t  ip_sr_pointer;     /* 39 Strict/LooseSourceRoute::pointer        */
    uint32_t ip_sr_dest;        /* 40 Strict/LooseSourceRoute::dest_addr      */
    uint32_t ip_cs_doi;         /* 44 CommercialSecurity::doi                 */
    uint64_t tcp_trace;         /* 48 kinds of the first 16 options, 4 bits each (index + 1) */
    uint64_t ip_trace;          /* 56                                         */
} rpkt_opts_t;

#define RPKT_OPTS_BYTES 64u

/* IPv6 frames (records of an RPKT_F_IPV6 parse): TcpOptionsIter as for IPv4, and in
 * place of the IPv4 walk, Ipv6OptionsIter (ipv6/generated.rs:1556-1615) over the
 * var_header_slice() of every HopByHopOption / DestOptions header of the extension chain
 * the parse walked ([l3 + 40, l4)), in order (ipv6_test.rs:47-69, 154-175); a malformed
 * option ends the walking.  Kinds (bits of ip_kinds, codes index + 1 in ip_trace):
 * 0 Pad0, 1 PadN, 2 RouterAlert, 3 Generic (every other type).  The IPv6 view of bytes
 * 27..47:
 *   27 ip_end          bytes consumed in the last header walked
 *   28 ip_count        options yielded over every header walked
 *   29 ip_stop         NONE (no options header), END, or MALFORMED
 *   30 ip_kinds
 *   32 ip_route_alert  RouterAlert::router_alert (the last one)
 *   34 u8 generic type / 35 u8 generic data length: Generic::type_ and header_len - 2
 *   36 u8 option headers walked / 37 u8 the first one's type (0 HopByHop, 60 DestOptions)
 *   40 u32 generic data: the first <= 4 bytes of that Generic's var_header_slice(),
 *          big-endian, zero-filled (ipv6_test.rs:54)
 * other bytes of the half are 0. */

/* Walk the IPv4 and TCP options of every frame of a parsed batch: recs_dev from
 * rpkt_gpu_parse_batch on the same batch locates the slices (ip: [l3 + 20, l4),
 * tcp: [l4 + 20, payload_off) for status OK / TCP).  opts_dev n * 64 B, 16-B aligned.
 * For an IPv6 record the first header of the extension chain is the record's
 * ip6_next_header (byte 30), which the parse copied from frame byte l3 + 6: the records
 * must come from a parse of these same frames (the compact entry below, whose record has
 * no such field, reads frame byte l3 + 6 itself; both agree whenever that holds). */
int rpkt_gpu_options_batch(const rpkt_batch_t* batch, const rpkt_rec_t* recs_dev,
                           rpkt_opts_t* opts_dev, void* stream);

/* The same walks located by compact records (rpkt_gpu_parse_batch_compact on the same
 * batch): status, ip_protocol, l3_off, l4_off and payload_off (the TCP slice's end)
 * are all the walks read, so the 16-B record serves as well as the 80-B one and the
 * results are identical.  recs_dev n * 16 B, opts_dev n * 64 B, both 16-byte aligned. */
int rpkt_gpu_options_batch_compact(const rpkt_batch_t* batch, const rpkt_rec16_t* recs_dev,
                                   rpkt_opts_t* opts_dev, void* stream);

/* Parse + verify and the option walks in one pass: rpkt_gpu_parse_batch's records (and
 * flow events) plus, per frame, the rpkt_opts_t that rpkt_gpu_options_batch would
 * produce from those records -- the walks run on the header bytes the parse has just
 * read, as rpkt's iterators walk the var_header_slice() of the views the parse returned
 * (ipv4/generated.rs:57-60, 1625-1722; tcp/generated.rs:1387-1484), so the option bytes
 * are not fetched a second time.  Outputs are byte-identical to the two separate calls.
 * opts_dev n * 64 B, 16-byte aligned. */
int rpkt_gpu_parse_options_batch(const rpkt_batch_t* batch, uint32_t flags,
                                 rpkt_rec_t* recs_dev, rpkt_opts_t* opts_dev,
                                 rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets, void* stream);
/* The same with compact records (rpkt_gpu_parse_batch_compact's rpkt_rec16_t). */
int rpkt_gpu_parse_options_batch_compact(const rpkt_batch_t* batch, uint32_t flags,
                                         rpkt_rec16_t* recs_dev, rpkt_opts_t* opts_dev,
                                         rpkt_flow_ev_t* flow_ev_dev, uint32_t n_buckets,
                                         void* stream);

/* ---- Protocol layer walk ---------------------------------------------------------- */

/* The protocol stack of each frame, walked with the header views of every protocol
 * rpkt generates from its pktfmt specs (include/rpkt_protocols.h): each layer is the
 * protocol's group_parse / parse (the pktfmt codegen rules: header_len, payload_len /
 * packet_len checks against chunk() and remaining()) and payload() (trim, advance).
 * Which group follows a layer is the dispatch a receive loop writes by hand in the
 * reference (ethertype, IP protocol / next header, UDP ports 4789 VXLAN and
 * 2152 / 2123 GTP, GRE protocol type, MPLS bottom of stack, PPPoE data type,
 * LLC 0x42 STP); DESIGN.md lists it. */
enum rpkt_layer_stop {
    RPKT_L_END = 1,        /* a terminal protocol (TCP, UDP payload, ICMP, ARP, STP, ...) */
    RPKT_L_UNKNOWN = 2,    /* the next protocol is outside the graph: next_key holds it */
    RPKT_L_ERR = 3,        /* the next group's parse returned Err: err_group names it */
    RPKT_L_MAX = 4         /* RPKT_MAX_LAYERS layers walked */
};
#define RPKT_MAX_LAYERS 16

typedef struct rpkt_layers {
    uint8_t  n;                       /*  0 layers parsed                           */
    uint8_t  stop;                    /*  1 rpkt_layer_stop                         */
    uint8_t  err_group;               /*  2 RPKT_GROUP_* the walk failed in (ERR)   */
    uint8_t  key_proto;               /*  3 UNKNOWN: protocol whose next key it is  */
    uint16_t payload_off;             /*  4 cursor after the last layer's payload() */
    uint16_t reserved;                /*  6                                         */
    uint32_t payload_len;             /*  8 remaining() of that payload             */
    uint32_t next_key;                /* 12 UNKNOWN: the unrecognised value         */
    uint8_t  proto[RPKT_MAX_LAYERS];  /* 16 RPKT_P_* of layer k                     */
    uint16_t off[RPKT_MAX_LAYERS];    /* 32 offset of layer k in the frame          */
} rpkt_layers_t;

#define RPKT_LAYERS_BYTES 64u

/* layers_dev n * 64 B, 16-byte aligned. */
int rpkt_gpu_layers_batch(const rpkt_batch_t* batch, rpkt_layers_t* layers_dev, void* stream);

/* ---- Field getters over the layer walk ---------------------------------------------- */

/* The header-field getters rpkt generates for every protocol of the walk
 * (pktfmt/src/codegen/field.rs:115-250, `read_repr` / `read_multi_bytes`): a field of
 * `bits` bits at bit `bit_off` of the protocol's header is the big-endian integer of
 * bytes [bit_off/8, (bit_off+bits-1)/8], shifted right by 7 - (end bit in its byte)
 * and masked to `bits` bits.  Byte-slice fields (MAC, IPv6 addresses) are
 * byte-aligned: a request of up to 64 bits of one returns those bytes as a big-endian
 * integer (ask for a 128-bit address as two 64-bit halves).  Offsets and widths per
 * field come from the same specs (rpkt_amd/proto_fields.json).
 *
 * Request r of frame i reads the `nth` (0 = outermost) layer k of rpkt_layers_t i
 * whose proto[k] == proto.  values_dev[i * n_req + r] is the field, or 0 when the
 * frame has no such layer or the field's bytes pass the frame's end; bit r of
 * present_dev[i] (optional, may be NULL) says which.  Replaces, per frame, the
 * getter calls a receive loop makes on the header views it parsed, e.g.
 * Ipv6::src_addr (ipv6/generated.rs), Arp::operation, Vxlan::vni, Gtpv1::teid. */
typedef struct rpkt_field_req {
    uint8_t  proto;      /* RPKT_P_*                                             */
    uint8_t  nth;        /* occurrence of proto in the stack, 0 = outermost      */
    uint8_t  bits;       /* 1..64                                                */
    uint8_t  reserved;   /* 0                                                    */
    uint16_t bit_off;    /* from the start of the protocol's header              */
    uint16_t reserved2;  /* 0                                                    */
} rpkt_field_req_t;

#define RPKT_MAX_FIELD_REQS 32

/* reqs: host memory, n_req in 1..RPKT_MAX_FIELD_REQS; layers_dev from
 * rpkt_gpu_layers_batch on the same batch; values_dev n * n_req * 8 B, 8-B aligned;
 * present_dev n * 4 B or NULL. */
int rpkt_gpu_fields_batch(const rpkt_batch_t* batch, const rpkt_layers_t* layers_dev,
                          const rpkt_field_req_t* reqs, uint32_t n_req, uint64_t* values_dev,
                          uint32_t* present_dev, void* stream);

/* 5-tuple hash used for flow buckets (host copy of the device function). */
uint32_t rpkt_flow_hash(uint32_t ip_src, uint32_t ip_dst, uint16_t src_port,
                        uint16_t dst_port, uint8_t protocol);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RPKT_GPU_H */
