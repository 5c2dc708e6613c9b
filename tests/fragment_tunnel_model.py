"""A plain model of rpkt_gpu_fragment_tunnel_batch (include/rpkt_gpu.h, "Fragmenting the inner
packet of a tunnel"): host frames and the oracle's three tunnel records in, the output frames,
frag_first and totals out.  It is composed, with no rule of its own beyond `over`, `mtu - over`
and the flag: the inner packet is cut by tests/fragment_model.py's fragment_ip4 with the inner
record (its offsets are positions in the outer frame already), the carrier is judged by
tests/segment_tunnel_model.py's is_cut, the outer headers are its outer_fixups, and everything
that is not an inner cut is fragment_model.fragment_frame with the outer record or a copy.
tests/test_fragment_tunnel_model.py anchors it to the oracle's tunnel parse and to a reassembly.
Also the hand-built frames the tests use."""
import functools
import struct

import numpy as np

from rpkt_amd.records import dispatch_ethertype, ip6_block

import fragment_model as fm
import segment_model as sm
import segment_tunnel_model as stm
import tunnel_frames as tf
from fragment_model import DF, MF, OPTIONS_MIX, OPTIONS_40
from segment_tunnel_model import NONE, VXLAN, GTPU, GRE, KINDS, tunnel_records  # noqa: F401

KIND_LIST = (VXLAN, GTPU, GRE)


def carrier_ok(f, O, T, I, o_et):
    """The carrier part of segment_tunnel_model.is_cut: the outer headers are ones whose lengths
    and sums can be fixed up and the offsets nest up to I.l3_off.  is_cut also judges the inner
    TCP / UDP frame, so it is asked about a stand-in inner record that passes that part: an
    unfragmented UDP datagram with a 20-byte IPv4 header at I.l3_off and more payload than the
    mss 0.  (The stand-in needs l3 + 28 < len(f); an inner packet that fragment_ip4 cuts is
    longer than that, since L > mtu' >= ihl + 8.)
    Why this way: the carrier rule is stated once, inside is_cut, and
    tests/segment_tunnel_model.py is an existing test file that stays as it is, so its carrier
    half cannot be split out for reuse; asking is_cut through a stand-in keeps this model
    without a second statement of the rule.  The two guards below are not rules of the entry:
    they only keep the stand-in's offsets inside the frame and inside the record's 16-bit
    fields, and cannot fire for a frame that is cut."""
    l3 = int(I["l3_off"])
    if l3 + 28 >= len(f) or l3 + 28 > 0xffff:
        return False
    r = I.copy()
    r["status"], r["ip_protocol"], r["ip_frag"] = 0, 17, 0
    r["l4_off"], r["payload_off"], r["payload_len"] = l3 + 20, l3 + 28, 0xffff
    return stm.is_cut(f, O, T, r, o_et, 0x0800, 0, udp=True)


def inner_cut(f, O, T, I, o_et, o_pdst, i_et, mtu, ignore_df):
    """Rule 2: the outputs of a frame whose inner IPv4 packet is cut, or None."""
    if T["status"] != 0 or i_et != 0x0800 or int(I["status"]) not in fm.IP4_STATUSES:
        return None
    if not carrier_ok(f, O, T, I, o_et):
        return None
    over = int(I["l3_off"]) - int(O["l3_off"])
    if mtu <= over:
        return None
    inner = fm.fragment_ip4(f, int(I["l3_off"]), int(I["l4_off"]), mtu - over, ignore_df)
    if inner is None:
        return None
    ol3 = int(O["l3_off"])
    ident = int.from_bytes(f[ol3 + 4:ol3 + 6], "big")
    return [stm.outer_fixups(s, O, T, o_et == 0x86DD, o_pdst, ident + k) for k, s in enumerate(inner)]


def fragment_frame(f, O, T, I, o_et, o_pdst, i_et, i, mtu, ignore_df=False, outer_fallback=False,
                   ip6_ident=0):
    """The output frames of frame `f`, the batch's i-th, with outer, tunnel and inner records
    O, T, I (o_et, i_et: their dispatch ethertypes; o_pdst: the outer ip6_pdst_off)."""
    if T["kind"] == NONE:                                   # rule 1: the flat entry's frame
        return fm.fragment_frame(f, O, o_et, i, mtu, ignore_df, ip6_ident)
    out = inner_cut(f, O, T, I, o_et, o_pdst, i_et, mtu, ignore_df)
    if out is not None:
        return out
    if outer_fallback:                                      # rule 3 with the flag: as rule 1
        return fm.fragment_frame(f, O, o_et, i, mtu, ignore_df, ip6_ident)
    return [f]


def fragment(hb, outer, tun, inner, mtu, ignore_df=False, outer_fallback=False, ip6_ident=0):
    """(out_frames, frag_first, totals) as fragment_model.fragment returns them."""
    o_et, i_et = dispatch_ethertype(outer), dispatch_ethertype(inner)
    o_pd = ip6_block(outer)["ip6_pdst_off"]
    out, first = [], np.zeros(hb.n + 1, dtype=np.uint32)
    for i, f in enumerate(sm.frames_of(hb)):
        out += fragment_frame(f, outer[i], tun[i], inner[i], int(o_et[i]), int(o_pd[i]),
                              int(i_et[i]), i, mtu, ignore_df, outer_fallback, ip6_ident)
        first[i + 1] = len(out)
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64)


def inner_cuts(hb, outer, tun, inner, mtu, ignore_df=False):
    """A bool per frame: rule 2 cuts it."""
    o_et, i_et = dispatch_ethertype(outer), dispatch_ethertype(inner)
    o_pd = ip6_block(outer)["ip6_pdst_off"]
    return np.array([tun[i]["kind"] != NONE and
                     inner_cut(f, outer[i], tun[i], inner[i], int(o_et[i]), int(o_pd[i]),
                               int(i_et[i]), mtu, ignore_df) is not None
                     for i, f in enumerate(sm.frames_of(hb))], dtype=bool)


def cut_kinds(first, tun, inner_cut_mask):
    """({kind: frames of that tunnel kind whose INNER packet a call with frag_first `first`
    cut}, how many frames had their own / OUTER packet cut)."""
    cut = np.diff(first.astype(np.int64)) > 1
    assert not (inner_cut_mask & ~cut).any()
    return ({k: int((inner_cut_mask & (tun["kind"] == k)).sum()) for k in KIND_LIST},
            int((cut & ~inner_cut_mask).sum()))


# ---- hand-built frames -------------------------------------------------------------------

def e4(pkt, **kw):
    return tf.ether(0x0800, pkt, **kw)


def ip6_hbh(nh, payload):
    """Ether / IPv6 / an 8-byte Hop-by-Hop header / payload (UDP: its checksum filled)."""
    src, dst = b"\xfd\x00" + bytes(13) + b"\x01", b"\xfd\x00" + bytes(13) + b"\x02"
    if nh == 17:
        u = bytearray(payload)
        ps = src + dst + struct.pack("!I", len(u)) + b"\0\0\0\x11"
        u[6:8] = struct.pack("!H", tf.rfc1071(ps + bytes(u[:6]) + b"\0\0" + bytes(u[8:])) or 0xffff)
        payload = bytes(u)
    body = bytes([nh, 0, 1, 4, 0, 0, 0, 0]) + payload
    return tf.ether(0x86dd, tf.ipv6_packet(0, body, src=src, dst=dst))


def vx(inner_frame):
    return tf.udp(40000, 4789, tf.vxlan(inner_frame))


def gt(inner_pkt, **kw):
    return tf.udp(2152, 2152, tf.gtpu(inner_pkt, **kw))


GTP_EXTS = [(0xc0, b"\x09\x04"), (0x85, bytes([0x10, 1])), (0x20, b"\x00\x07")]
# the three carriers the boundary sizes are built around, and their `over`
BASE = ((VXLAN, 50, lambda fr: e4(stm.ip4(17, vx(fr)))),
        (GTPU, 36, lambda fr: e4(stm.ip4(17, gt(fr[14:])))),
        (GRE, 24, lambda fr: e4(stm.ip4(47, tf.gre(fr[14:])))))
# 24: mtu <= over for the three; 51: mtu' - ihl < 8 for the three; 52, 64, 78: c == 8 behind
# GRE, GTP-U, VXLAN; then a small one with several fragments, and the issue's 576, 1500, 65535
MTU_VALUES = (24, 51, 52, 64, 78, 120, 576, 1500, 65535)


@functools.lru_cache(maxsize=None)
def hand_frames(mtu):
    """The hand-built set for one mtu: behind each base carrier inner IPv4 payloads of c - 1, c,
    c + 1, 2c + 1 bytes (a last fragment of 1 byte) and inner packets 1 and 0 bytes over mtu',
    then at an inner packet of three fragments or so the variety of carriers and inner headers,
    the tunnel frames that are not inner-cut, and plain frames."""
    frames = []
    for _, over, wrap in BASE:
        m = mtu - over
        if m >= 28 and mtu <= 1500:
            c = (m - 20) & ~7
            sizes = (c - 1, c, c + 1, 2 * c + 1, m + 1 - 20, m - 20)
        elif m >= 28:
            sizes = (m - 20, 3000)                          # L == mtu' at the 16-bit limit
        else:
            sizes = (64,)
        frames += [wrap(fm.udp4(max(p, 8), ident=0x200 + k)) for k, p in enumerate(sizes)]
    big = 2 * max(mtu, 100) + 9 if mtu <= 1500 else 3000            # inner IP payload
    u, t, ic = fm.udp4, fm.tcp4, fm.icmp4
    gre = lambda fr, **kw: tf.gre(fr[14:], **kw)
    frames += [
        # VXLAN: a zero outer UDP checksum, outer IPv6 with an extension header, tags on both
        e4(stm.ip4(17, vx(u(big)), zero_udp_csum=True)),
        ip6_hbh(17, vx(t(big, options=OPTIONS_MIX))),
        e4(stm.ip4(17, vx(u(big, options=OPTIONS_40, tags=1)), ident=0xffff), tags=((0x8100, 100),)),
        e4(stm.ip4(17, vx(ic(big, tags=2)))),
        # GTP-U: 0..3 extension headers, with and without a sequence number
        e4(stm.ip4(17, gt(u(big)[14:], seq=5))),
        e4(stm.ip4(17, gt(u(big, options=OPTIONS_MIX)[14:], exts=GTP_EXTS[:1]))),
        e4(stm.ip4(17, gt(t(big)[14:], exts=GTP_EXTS[:2], seq=9), zero_udp_csum=True)),
        e4(stm.ip4(17, gt(ic(big)[14:], exts=GTP_EXTS))),
        ip6_hbh(17, gt(u(big, options=OPTIONS_40)[14:])),
        # GRE: plain, K, C, C + K, an inner Ethernet frame, outer IPv6
        e4(stm.ip4(47, gre(t(big)))),
        e4(stm.ip4(47, gre(u(big, options=OPTIONS_MIX), key=7))),
        e4(stm.ip4(47, gre(u(big, options=OPTIONS_40), checksum=True))),
        e4(stm.ip4(47, gre(ic(big), checksum=True, key=0xfde8))),
        e4(stm.ip4(47, tf.gre(u(big, tags=1), proto=0x6558, checksum=True))),
        ip6_hbh(47, gre(u(big), checksum=True)),
        # inner DF; inner packets that are fragments already; an offset that would overflow
        e4(stm.ip4(17, vx(u(big, frag=DF)))),
        e4(stm.ip4(47, gre(u(big, frag=DF, options=OPTIONS_MIX), checksum=True))),
        e4(stm.ip4(17, gt(u(big, frag=MF | 0x0123, options=OPTIONS_MIX)[14:]))),
        e4(stm.ip4(17, vx(u(big, frag=0x0040)))),
        e4(stm.ip4(47, gre(u(big, frag=MF)))),
        e4(stm.ip4(17, vx(u(big, frag=0x1ff0)))),
        # padding: after the inner IP packet, after the outer one, both
        e4(stm.ip4(17, vx(u(big, pad=6)))),
        e4(stm.ip4(17, gt(u(big)[14:]))) + b"\x5a" * 5,
        e4(stm.ip4(47, tf.gre(u(big, pad=3), proto=0x6558, checksum=True))) + b"\x5a" * 2,
        # not inner-cut: inner IPv6, GRE with S, a tunnel that decodes BAD, an outer fragment
        e4(stm.ip4(17, vx(fm.udp6(big)))),
        e4(stm.ip4(17, gt(fm.tcp6(big)[14:]))),
        e4(stm.ip4(47, stm.gre_seq(u(big)[14:]))),
        e4(stm.ip4(17, tf.udp(40000, 4789, b"\x08\0\0" + bytes(big)))),
        e4(stm.ip4(47, gre(u(big)), frag=0x2000)),
        # plain frames
        u(big), u(big, frag=DF, options=OPTIONS_MIX), fm.udp6(big, (fm.HBH,)), t(big, tags=1), b"",
    ]
    return tuple(frames)


def df_clear(f, I):
    """The inner IPv4 packet of frame `f` has DF clear."""
    return not f[int(I["l3_off"]) + 6] & 0x40
