"""A plain model of rpkt_gpu_segment_tunnel_batch (include/rpkt_gpu.h, "Segmentation of the
inner TCP / UDP of tunnels"): host frames and the oracle's three tunnel records in, the output
frames, seg_first and totals out.  The inner frame is cut by tests/segment_model.py /
tests/udp_reframe_model.py with the inner record (its offsets are positions in the outer
frame already); this module adds the rule that decides and the outer fix-ups: the GTP-U
length, the GRE checksum, the outer UDP length and checksum, the outer IP header.
tests/test_segment_tunnel_model.py anchors it to the oracle's tunnel parse.  Also the
hand-built tunnel frames the tests use."""
import struct

import numpy as np

from oracle import oracle
from rpkt_amd.records import dispatch_ethertype, ip6_block

import segment_model as sm
import tunnel_frames as tf
import udp_reframe_model as um

NONE, VXLAN, GTPU, GRE = 0, 1, 2, 3
KINDS = {VXLAN: "VXLAN", GTPU: "GTP-U", GRE: "GRE"}


def tunnel_records(hb, flags=sm.F6):
    """The oracle's (outer, tun, inner) records of a HostBatch."""
    return oracle.tunnel_batch(hb.frames, hb.n, flags, offsets=hb.offsets, stride=hb.stride,
                               frame_len=hb.frame_len)


def inner_nests(I, v6, udp, flen):
    """The inner record's offsets nest as rpkt_gpu_segment_batch requires."""
    l3, l4, po = int(I["l3_off"]), int(I["l4_off"]), int(I["payload_off"])
    l4_ok = po - l4 == 8 if udp else 20 <= po - l4 <= 60
    l3_ok = l4 - l3 >= 40 if v6 else 20 <= l4 - l3 <= 60
    return l3 <= l4 <= po <= flen and l4_ok and l3_ok


def is_cut(f, O, T, I, o_et, i_et, mss, udp=False):
    """Rule 3 of the header: the frame `f` with a decoded tunnel is segmented."""
    o_v6, i_v6 = o_et == 0x86DD, i_et == 0x86DD
    proto = int(I["ip_protocol"])
    as_udp = udp and proto == 17
    if not (I["status"] == 0 and (proto == 6 or as_udp) and i_et in (0x0800, 0x86DD) and
            (i_v6 or (int(I["ip_frag"]) & 0x3fff) == 0) and inner_nests(I, i_v6, as_udp, len(f))):
        return False
    if min(int(I["payload_len"]), len(f) - int(I["payload_off"])) <= mss:
        return False
    ol3, ol4 = int(O["l3_off"]), int(O["l4_off"])
    toff, ioff, kind = int(T["tun_off"]), int(T["inner_off"]), int(T["kind"])
    if o_et not in (0x0800, 0x86DD) or not (o_v6 or (int(O["ip_frag"]) & 0x3fff) == 0):
        return False
    if not (ol4 - ol3 >= 40 if o_v6 else 20 <= ol4 - ol3 <= 60):
        return False
    if kind in (VXLAN, GTPU):
        if not (O["status"] == 0 and O["ip_protocol"] == 17 and ol4 + 8 <= toff):
            return False
        need = 8
    elif kind == GRE:
        if not (O["ip_protocol"] == 47 and ol4 == toff and toff < len(f)):
            return False
        if f[toff] & 0x50:                                  # S (sequence) or R
            return False
        need = 8 if f[toff] & 0x80 else 4
    else:
        return False
    return toff + need <= ioff <= int(I["l3_off"])


def outer_fixups(seg, O, T, o_v6, o_pdst, ident):
    """The outer headers of one output `seg` (its inner headers already written): the GTP-U
    length, the GRE checksum, the outer UDP length and checksum, the outer IP header with
    `ident`.  Length fields are taken mod 2^16."""
    h = bytearray(seg)
    tot = len(h)
    ol3, ol4 = int(O["l3_off"]), int(O["l4_off"])
    toff, kind = int(T["tun_off"]), int(T["kind"])
    if kind == GTPU:
        h[toff + 2:toff + 4] = ((tot - toff - 8) & 0xffff).to_bytes(2, "big")
    if kind == GRE:
        if h[toff] & 0x80:                                  # C: RFC 2784, a result of 0 stays 0
            h[toff + 4:toff + 6] = b"\0\0"
            h[toff + 4:toff + 6] = sm.csum_field(h[toff:]).to_bytes(2, "big")
    else:
        ulen = (tot - ol4) & 0xffff
        keep_zero = bytes(h[ol4 + 6:ol4 + 8]) == b"\0\0"
        h[ol4 + 4:ol4 + 6] = ulen.to_bytes(2, "big")
        if not keep_zero:
            h[ol4 + 6:ol4 + 8] = b"\0\0"
            pseudo = um.pseudo_header(h, o_v6, ol3, ol4, o_pdst, 17, ulen)
            h[ol4 + 6:ol4 + 8] = um.udp_csum_field(pseudo, h[ol4:]).to_bytes(2, "big")
    if o_v6:
        h[ol3 + 4:ol3 + 6] = ((tot - ol3 - 40) & 0xffff).to_bytes(2, "big")
    else:
        h[ol3 + 2:ol3 + 4] = ((tot - ol3) & 0xffff).to_bytes(2, "big")
        h[ol3 + 4:ol3 + 6] = (ident & 0xffff).to_bytes(2, "big")
        h[ol3 + 10:ol3 + 12] = b"\0\0"
        h[ol3 + 10:ol3 + 12] = sm.csum_field(h[ol3:ol4]).to_bytes(2, "big")
    return bytes(h)


def segment_frame(f, O, T, I, o_et, o_pdst, i_et, i_pdst, mss, udp=False):
    """The output frames of frame `f` with outer, tunnel and inner records O, T, I (o_et, i_et:
    their dispatch ethertypes; o_pdst, i_pdst: their ip6_pdst_off)."""
    if T["kind"] == NONE:                                   # rule 1: the flat entry's frame
        return um.segment_frame(f, O, o_et == 0x86DD, o_pdst, mss, udp)
    if T["status"] != 0 or not is_cut(f, O, T, I, o_et, i_et, mss, udp):
        return [f]                                          # rules 2 and 3: a byte copy
    r = I.copy()
    r["payload_len"] = min(int(I["payload_len"]), len(f) - int(I["payload_off"]))
    inner = um.segment_frame(f, r, i_et == 0x86DD, i_pdst, mss, udp)
    ol3 = int(O["l3_off"])
    ident = int.from_bytes(f[ol3 + 4:ol3 + 6], "big")
    return [outer_fixups(s, O, T, o_et == 0x86DD, o_pdst, ident + k) for k, s in enumerate(inner)]


def segment(hb, outer, tun, inner, mss, udp=False):
    """(out_frames, seg_first, totals) as segment_model.segment returns them."""
    o_et, i_et = dispatch_ethertype(outer), dispatch_ethertype(inner)
    o_pd, i_pd = ip6_block(outer)["ip6_pdst_off"], ip6_block(inner)["ip6_pdst_off"]
    out, first = [], np.zeros(hb.n + 1, dtype=np.uint32)
    for i, f in enumerate(sm.frames_of(hb)):
        out += segment_frame(f, outer[i], tun[i], inner[i], int(o_et[i]), int(o_pd[i]),
                             int(i_et[i]), int(i_pd[i]), mss, udp)
        first[i + 1] = len(out)
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64)


def cut_kinds(first, tun):
    """{kind: how many frames of that tunnel kind a call with seg_first `first` cut}."""
    cut = np.diff(first.astype(np.int64)) > 1
    return {k: int((cut & (tun["kind"] == k)).sum()) for k in (NONE, VXLAN, GTPU, GRE)}


# ---- hand-built frames -------------------------------------------------------------------

def ip4(proto, payload, frag=0, ident=0x4321, zero_udp_csum=False):
    """tunnel_frames.ipv4_packet with a fragment word, an ident and (UDP) a zero checksum."""
    p = bytearray(tf.ipv4_packet(proto, payload))
    p[4:6] = ident.to_bytes(2, "big")
    p[6:8] = frag.to_bytes(2, "big")
    p[10:12] = b"\0\0"
    p[10:12] = struct.pack("!H", tf.rfc1071(bytes(p[:20])))
    if zero_udp_csum:
        p[26:28] = b"\0\0"
    return bytes(p)


def ip_only(frame):
    """The IP packet of an untagged segment_model / udp_reframe_model frame."""
    return frame[14:]


def gre_seq(inner, seq=7):
    """GRE with the S bit: flags, protocol 0x0800, a sequence word."""
    return struct.pack("!BBHI", 0x10, 0, 0x0800, seq) + inner


def cut_frames(p):
    """The hand shapes that are cut (the VXLAN-around-UDP and the plain UDP one with the flag
    only), inner payload length p."""
    pay = sm.payload_bytes(p, 3)
    both = sm.both_flags()
    e4, e6 = (lambda x, **kw: tf.ether(0x0800, x, **kw)), (lambda x, **kw: tf.ether(0x86dd, x, **kw))
    vx = lambda inner: tf.udp(40000, 4789, tf.vxlan(inner))
    gt = lambda inner, **kw: tf.udp(2152, 2152, tf.gtpu(inner, **kw))
    return [
        e4(ip4(17, vx(sm.tcp4(pay)))),
        e4(ip4(17, vx(sm.tcp4(pay, tags=1, ihl=7, doff=8, flags=both)), ident=0xffff)),
        e6(tf.ipv6_packet(17, vx(sm.tcp6(pay, exts=(sm.hop_by_hop(), sm.routing(0, 2, 1)))))),
        e4(ip4(17, gt(ip_only(sm.tcp4(pay)))), tags=((0x8100, 100),)),
        e4(ip4(17, gt(ip_only(sm.tcp6(pay)), exts=[(0xc0, b"\x09\x04"), (0x85, bytes([0x10, 1]))],
                      seq=5))),
        e6(tf.ipv6_packet(17, gt(ip_only(sm.tcp4(pay, doff=15))))),
        e4(ip4(47, tf.gre(ip_only(sm.tcp4(pay)), checksum=True, key=7))),
        e4(ip4(47, tf.gre(ip_only(sm.tcp4(pay, flags=both))))),
        e6(tf.ipv6_packet(47, tf.gre(ip_only(sm.tcp6(pay)), proto=0x86dd, checksum=True))),
        e4(ip4(47, tf.gre(sm.tcp4(pay), proto=0x6558, key=0xfde8))),
        e4(ip4(17, vx(sm.tcp4(pay)), zero_udp_csum=True)),
        e4(ip4(17, vx(um.udp4(pay)))),
        sm.tcp4(pay, tags=1), um.udp4(pay),
    ]


N_CUT_TCP = 12                                  # of cut_frames: cut without the flag


def through_frames(p, mss):
    """Tunnel frames that must pass through whatever the flag."""
    pay = sm.payload_bytes(p, 4)
    e4 = lambda x: tf.ether(0x0800, x)
    vx = lambda inner: tf.udp(40000, 4789, tf.vxlan(inner))
    not_tpdu = bytearray(tf.gtpu(ip_only(sm.tcp4(pay))))
    not_tpdu[1] = 1                                                # an echo request
    return [
        e4(ip4(47, gre_seq(ip_only(sm.tcp4(pay))))),               # GRE with S
        e4(ip4(47, tf.gre(ip_only(sm.tcp4(pay))), frag=0x2000)),   # an outer first fragment
        e4(ip4(17, vx(sm.tcp4(pay, frag=0x2000)))),                # an inner fragment
        e4(ip4(17, vx(sm.tcp4(pay)[:50]))),                        # a truncated inner TCP header
        e4(ip4(17, tf.udp(40000, 4789, b"\x08\0\0"))),             # T.status BAD
        e4(ip4(17, tf.udp(2152, 2152, bytes(not_tpdu)))),          # NOT_TPDU
        e4(ip4(47, tf.gre(ip_only(sm.tcp4(pay)), proto=0x1234))),  # INNER_UNKNOWN
        e4(ip4(17, vx(sm.tcp4(sm.payload_bytes(mss, 6))))),        # ipl <= mss
        b"",
    ]


def padded_frames(p):
    """Inner and outer Ethernet padding: bytes after the inner IP packet's end inside the
    tunnel payload, bytes after the outer IP packet's end, and both."""
    pay = sm.payload_bytes(p, 8)
    e4 = lambda x: tf.ether(0x0800, x)
    vx = lambda inner: tf.udp(40000, 4789, tf.vxlan(inner))
    return [
        e4(ip4(17, vx(sm.tcp4(pay, pad=6)))),
        e4(ip4(17, vx(sm.tcp4(pay)))) + b"\x5a" * 5,
        e4(ip4(47, tf.gre(sm.tcp4(pay, pad=3), proto=0x6558, checksum=True))) + b"\x5a" * 2,
    ]


MSS_VALUES = (1, 2, 3, 7, 16, 17, 536, 1448)


def hand_frames(mss):
    """The hand-built set for one mss: the cut shapes at an inner payload of two segments and a
    bit, the padded ones, then the frames that pass through."""
    p = min(2 * mss + 1, 2000)
    return cut_frames(p) + padded_frames(p) + through_frames(p, mss)
