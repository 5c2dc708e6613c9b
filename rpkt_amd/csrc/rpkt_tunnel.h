// rpkt_tunnel.h — device code shared by the tunnel entries (rpkt_tunnel.hip and
// rpkt_tunnel_next.hip: flat frames; rpkt_tunnel_chains.hip: mbuf chains): the tunnel record
// in registers, the decode of one tunnel level over either view (rpkt_common.h), the
// NO_INNER record and the tunnel-record store, the staged-record flush, the window range
// sum, and a staged record's status and flow event.
#pragma once
#include "rpkt_common.h"

namespace {

struct Tunnel {
    uint32_t w[4];      // rpkt_tun_t as 4 little-endian words
    uint32_t is, ie;    // the inner frame, frame offsets [is, ie)
    uint32_t start_et;  // the inner frame's first header: 0 Ethernet, 0x0800, 0x86DD
    bool ok;
};

__device__ __forceinline__ void tun_set(Tunnel& T, uint32_t kind, uint32_t status, uint32_t tun_off,
                                        uint32_t inner_off, uint32_t inner_type) {
    T.w[0] = kind | (status << 8) | (tun_off << 16);
    T.w[1] = (inner_off & 0xffffu) | (inner_type << 16);
}

// The inner packet of a GTP-U T-PDU or a GRE payload by its first header's type:
// 0x0800 IPv4, 0x86DD IPv6 (with RPKT_F_IPV6), 0x6558 Ethernet; anything else is
// INNER_UNKNOWN.
__device__ __forceinline__ void tun_inner(Tunnel& T, uint32_t kind, uint32_t ts, uint32_t is,
                                          uint32_t ie, uint32_t type, uint32_t flags) {
    const bool eth = type == 0x6558u, ip4 = type == 0x0800u;
    const bool ip6 = type == 0x86ddu && (flags & RPKT_F_IPV6);
    T.ok = eth || ip4 || ip6;
    T.start_et = eth ? 0u : type;
    T.is = is;
    T.ie = ie;
    tun_set(T, kind, T.ok ? RPKT_T_OK : RPKT_T_INNER_UNKNOWN, ts, is, type);
}

// The tunnel of one parsed packet (L: its outer record; V: its bytes, a FlatView or a
// ChainView).  ts, te, T.is, T.ie are logical positions in the packet.  Each parse's
// header-size tests take chunk() at its cursor and its total-length tests remaining() (the
// views' own split: over a Pbuf a header that straddles a segment boundary is Err there,
// T_BAD / T_EXT_BAD here; over a flat frame the two are one number).  Every byte read lies
// inside the chunk its parse tested.
template <class View>
__device__ __forceinline__ Tunnel decode_tunnel(const LaneRec& L, const View& V, uint32_t flags) {
    Tunnel T;
    T.w[0] = RPKT_TUN_NONE | (RPKT_T_NONE << 8);
    T.w[1] = T.w[2] = T.w[3] = 0u;
    T.is = T.ie = T.start_et = 0u;
    T.ok = false;
    const uint32_t* w = L.w;
    const uint32_t proto = (w[8] >> 8) & 0xffu;              // ip_protocol (IPv4 and IPv6)
    uint32_t kind = RPKT_TUN_NONE, ts = 0u, te = 0u;
    if (L.status == RPKT_S_OK && proto == 17u) {
        // Udp::payload() (udp/generated.rs:66-76): [payload_off, + payload_len)
        const uint32_t dp = w[11] >> 16, sp = w[11] & 0xffffu;
        const uint32_t port = (dp == 4789u || dp == 2152u) ? dp
                            : ((sp == 4789u || sp == 2152u) ? sp : 0u);
        if (port != 0u) {
            kind = port == 4789u ? RPKT_TUN_VXLAN : RPKT_TUN_GTPU;
            ts = w[17] & 0xffffu;
            te = ts + (w[17] >> 16);
        }
    } else if (L.status == RPKT_S_L4_OTHER && proto == 47u &&
               (L.is6 || ((w[7] >> 16) & 0x1fffu) == 0u)) {
        // Ipv4|Ipv6::payload() of a first (or only) fragment: [l4_off, + payload_len)
        kind = RPKT_TUN_GRE;
        ts = w[16] >> 16;
        te = ts + (w[17] >> 16);
    }
    if (kind == RPKT_TUN_NONE) return T;
    uint32_t at;
    const uint32_t cl = V.chunk(ts, te, at), rm = te - ts;   // chunk().len(), remaining()
    tun_set(T, kind, RPKT_T_BAD, ts, 0u, 0u);
    if (kind == RPKT_TUN_VXLAN) {
        // Vxlan::parse (vxlan/generated.rs:32-39): chunk_len >= 8; getters :44-87;
        // payload() :91-96 advance 8 -> EtherFrame::parse (vlan_mpls_tests.rs:250)
        if (cl < 8u) return T;
        const uint32_t d0 = V.dw(at), d1 = V.dw(at + 4u);
        T.w[2] = bswap32(d1) >> 8;                            // vni, bytes 4..6
        T.w[3] = (d0 & 0xffffu) | (be16_hi(d0) << 16);        // flags bytes 0, 1; group_id
        tun_inner(T, kind, ts, ts + 8u, te, 0x6558u, flags);
        return T;
    }
    if (kind == RPKT_TUN_GTPU) {
        // Gtpv1::parse (gtpv1/generated.rs:33-49): chunk_len >= 8, header_len (8, or 12
        // with any of E/S/PN, :239-250) <= chunk_len, header_len <= packet_len (length +
        // 8, :81-84) <= remaining
        if (cl < 8u) return T;
        const uint32_t d0 = V.dw(at);
        const uint32_t b0 = d0 & 0xffu, msg = (d0 >> 8) & 0xffu;
        const uint32_t hl = (b0 & 7u) ? 12u : 8u;
        const uint32_t plen = be16_hi(d0) + 8u;
        if (hl > cl || plen < hl || plen > rm) return T;
        const uint32_t d2 = hl == 12u ? V.dw(at + 8u) : 0u;
        T.w[2] = bswap32(V.dw(at + 4u));                      // teid :74-76
        T.w[3] = (d0 & 0xffffu) | (be16_lo(d2) << 16);        // byte 0, message_type; sequence
        // payload() :98-108: trim to packet_len, advance header_len
        uint32_t c = ts + hl;
        const uint32_t end = ts + plen;
        if ((b0 >> 5) != 1u || msg != 255u) {                 // not a GTPv1 G-PDU
            tun_set(T, kind, RPKT_T_NOT_TPDU, ts, c, 0u);
            return T;
        }
        // the extension headers (gtpv1_test.rs:222-229, 306-318, 494-503): the type named
        // by the previous header's next_extention_header (Gtpv1::next_extention_header
        // :275-278 reads byte 11), each its parse against its own chunk, header_len and
        // payload() (advance)
        uint32_t nx = (b0 & 4u) ? (d2 >> 24) : 0u;
        for (int k = 0; k < RPKT_MAX_GTP_EXT && nx != 0u; ++k) {
            const uint32_t rem = V.chunk(c, end, at), x = V.dw(at);
            const uint32_t e0 = x & 0xffu, t = (x >> 12) & 0xfu;
            uint32_t need, mn, ehl;
            if (nx == 0x40u || nx == 0xc0u || nx == 0x20u) {
                need = 4u; mn = 4u; ehl = 4u;                 // ExtUdpPort :336-341,
            } else if (nx == 0x03u || nx == 0x82u) {          //   ExtPduNumber :461-466,
                need = 8u; mn = 8u; ehl = 8u;                 //   ExtServiceClassIndicator
            } else if (nx == 0x81u || nx == 0x83u) {          //   :747-752; ExtLongPduNumber
                need = 1u; mn = 1u; ehl = e0 * 4u;            //   :587-592; ExtContainer
            } else if (nx == 0x84u && t <= 2u) {              //   :880-892 (header_len :902);
                need = 2u; mn = t == 0u ? 6u : (t == 1u ? 7u : 3u); ehl = e0 * 4u;  // NrUp
            } else if (nx == 0x85u && t <= 1u) {              //   :2308-2320; PduSessionUp
                need = 2u; mn = 3u; ehl = e0 * 4u;            //   :1507-1518
            } else {
                need = ~0u; mn = 0u; ehl = 0u;                // unknown type / group Err
            }
            if (rem < need || rem < mn || ehl < mn || ehl > rem) {
                tun_set(T, kind, RPKT_T_EXT_BAD, ts, c, 0u);
                return T;
            }
            nx = V.dw(at + ehl - 1u) & 0xffu;                 // next_extention_header: last byte
            c += ehl;
        }
        if (nx != 0u) {
            tun_set(T, kind, RPKT_T_EXT_BAD, ts, c, 0u);
            return T;
        }
        // the T-PDU: Ipv4 / Ipv6 by the version nibble of the cursor's first byte
        // (gtpv1_test.rs:229)
        const uint32_t v = V.chunk(c, end, at) ? (V.dw(at) >> 4) & 0xfu : 0u;
        tun_inner(T, kind, ts, c, end, v == 4u ? 0x0800u : (v == 6u ? 0x86ddu : 0u), flags);
        return T;
    }
    // GreGroup::group_parse (gre/generated.rs:800-820): chunk >= 4; (C, R, K, version,
    // protocol_type) == (0, 0, 1, 1, 0x880B) -> GreForPPTP::parse (:371-386: chunk >= 8,
    // header_len <= chunk, payload_len + header_len <= remaining), version 0 -> Gre::parse
    // (:33-44, header_len gre/mod.rs:68-85, in [4, chunk]), else Err
    // (a header that fails its parse leaves id / hdr0 / hdr1 / aux 0)
    if (cl < 4u) return T;
    const uint32_t d0 = V.dw(at);
    const uint32_t b0 = d0 & 0xffu, b1 = (d0 >> 8) & 0xffu, pt = be16_hi(d0), ver = b1 & 7u;
    if ((b0 & 0xe0u) == 0x20u && ver == 1u && pt == 0x880bu) {
        if (cl < 8u) return T;
        const uint32_t d1 = V.dw(at + 4u);
        const uint32_t phl = 8u + ((b0 & 0x10u) ? 4u : 0u) + ((b1 & 0x80u) ? 4u : 0u);
        if (phl > cl || be16_lo(d1) + phl > rm) return T;     // payload_len + header_len
        T.w[2] = bswap32(d1);                                 // payload_len, call_id
        T.w[3] = d0 & 0xffffu;
        tun_set(T, kind, RPKT_T_INNER_UNKNOWN, ts, ts + phl, pt);   // PPP, not IP
        return T;
    }
    if (ver != 0u) return T;
    const uint32_t cr = (b0 & 0xc0u) ? 4u : 0u;
    const uint32_t hl = 4u + cr + ((b0 & 0x20u) ? 4u : 0u) + ((b0 & 0x10u) ? 4u : 0u);
    if (hl > cl) return T;
    T.w[3] = (d0 & 0xffffu) | (cr ? be16_lo(V.dw(at + 4u)) << 16 : 0u);   // checksum :236-241
    if (b0 & 0x20u) T.w[2] = bswap32(V.dw(at + 4u + cr));      // key :260-267
    tun_inner(T, kind, ts, ts + hl, te, pt, flags);           // payload() advance header_len
    return T;
}

// The inner record of a packet whose tunnel did not decode: all zero but its status, no sum.
__device__ __forceinline__ void no_inner(LaneRec& L) {
#pragma unroll
    for (int k = 0; k < 20; ++k) L.w[k] = 0u;
    L.w[0] = RPKT_S_NO_INNER;
    L.want_l4 = false;
    L.stream_s = L.stream_e = 0u;
}

// The 16-byte tunnel record of packet i.  (T by value: by reference tunnel_kernel<true>
// allocates a 129th VGPR and loses its fourth wave per SIMD.)
__device__ __forceinline__ void store_tun(rpkt_tun_t* tun, uint32_t i, const Tunnel T) {
    __builtin_nontemporal_store(u32x4{T.w[0], T.w[1], T.w[2], T.w[3]},
                                reinterpret_cast<u32x4*>(tun) + i);
}

// Records staged at rl (stride 21 dwords) -> recs[p0 .. p0 + 64), 1-KiB wave stores.
__device__ __forceinline__ void flush_stage(const uint32_t* rl, int lane, rpkt_rec_t* recs,
                                            uint32_t p0, uint32_t n) {
    wave_sync();
    const uint32_t nrec = n - p0 < (uint32_t)kWave ? n - p0 : (uint32_t)kWave;
    u32x4* out = reinterpret_cast<u32x4*>(recs + p0);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t c = k * kWave + lane, r = c / 5, pc = c % 5;
        const uint32_t* src = rl + r * 21 + pc * 4;
        if (r < nrec) __builtin_nontemporal_store(u32x4{src[0], src[1], src[2], src[3]}, &out[c]);
    }
}

// Absolute-phase word sum of LDS slot bytes [s, e) (slot byte 0 on a 16-B boundary).
__device__ __forceinline__ uint32_t slot_range_sum(const uint8_t* slot, uint32_t s, uint32_t e) {
    if (e <= s) return 0u;
    uint32_t acc = 0;
    uint32_t a = s & ~3u;
    for (; a + 12u < e; a += 16u) {
        const uint32_t x0 = lds32(slot, a), x1 = lds32(slot, a + 4u);
        const uint32_t x2 = lds32(slot, a + 8u), x3 = lds32(slot, a + 12u);
        acc = hsum(x3, hsum(x2, hsum(x1, hsum(x0, acc))));
    }
    for (; a < e; a += 4) acc = hsum(lds32(slot, a), acc);
    acc -= halves(low_bytes(lds32(slot, s & ~3u), s & 3u));
    if (e & 3u) acc -= halves(lds32(slot, e & ~3u) & ~((1u << (8u * (e & 3u))) - 1u));
    return acc;
}

// A record's status and IPv6 dispatch from its words alone: the status is byte 0; the IPv6
// block is used when the dispatch ethertype -- the last tag's, or the frame's, or an inner
// IP packet's start type -- is 0x86DD and the IPv6 header was reached.
template <typename WordsT>
__device__ __forceinline__ void rec_status_is6(const WordsT& w, uint32_t& status, bool& is6) {
    status = w[0] & 0xffu;
    const uint32_t nv = (w[0] >> 8) & 0xffu;
    const uint32_t det = nv == 0u ? w[0] >> 16 : (nv == 1u ? w[5] & 0xffffu : w[5] >> 16);
    is6 = det == 0x86ddu && status != RPKT_S_ETH_SHORT && status != RPKT_S_VLAN_SHORT &&
          status != RPKT_S_NOT_IPV4;
}

// The flow event of a record from its words alone, as flow_event forms it.
template <typename WordsT>
__device__ __forceinline__ uint64_t record_event(const WordsT& w, uint32_t n_buckets) {
    LaneRec R;
    rec_status_is6(w, R.status, R.is6);
    uint32_t x[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) x[k] = w[k];
    return flow_event(R, x, n_buckets);
}

}  // namespace
