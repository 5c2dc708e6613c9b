"""A plain model of rpkt_gpu_fragment_batch (include/rpkt_gpu.h, "IPv4 / IPv6 fragmentation"):
host frames and oracle records in, the output frames, frag_first and totals out, over
tests/segment_model.py's pack, frames_of, oracle_records and packed_output.  It restates the two
rules in plain Python; tests/test_fragment_model.py checks it against known answers written
out as bytes, the oracle's parse of its output and a reassembly.  Also the hand-built frames
the fragment tests use."""
import functools

import numpy as np

from rpkt_amd.records import STATUS, dispatch_ethertype

import segment_model as sm
from segment_model import csum_field, payload_bytes, ether

MAX_IP6_EXT = 8
IP4_STATUSES = tuple(STATUS[k] for k in ("OK", "L4_OTHER", "UDP_SHORT", "UDP_BAD_LEN", "TCP_SHORT",
                                         "TCP_BAD_DOFF", "ICMP_EMPTY"))
IP6_STATUSES = IP4_STATUSES[:-1]
DF, MF = 0x4000, 0x2000


def noop_options(opts):
    """ip_options_fragment on the option bytes of an IPv4 header: what fragments after the
    first carry."""
    o, x = bytearray(opts), 0
    while x < len(o):
        if o[x] == 0:
            break
        if o[x] == 1:
            x += 1
            continue
        if x + 1 >= len(o) or o[x + 1] < 2 or o[x + 1] > len(o) - x:
            break
        n = o[x + 1]
        if not o[x] & 0x80:
            o[x:x + n] = b"\x01" * n
        x += n
    return bytes(o)


def fragment_ip4(f, l3, l4, mtu, ignore_df):
    ihl = (f[l3] & 0xf) * 4 if l3 < len(f) else 0
    L = int.from_bytes(f[l3 + 2:l3 + 4], "big")
    fw = int.from_bytes(f[l3 + 6:l3 + 8], "big")
    if ihl < 20 or l4 != l3 + ihl or l3 + L > len(f) or L <= mtu:
        return None
    if fw & DF and not ignore_df:
        return None
    c = (mtu - ihl) & ~7
    if c < 8:
        return None
    P, o = L - ihl, fw & 0x1fff
    n = -(-P // c)
    if o + (n - 1) * c // 8 > 0x1fff:
        return None
    out = []
    for k in range(n):
        pay = f[l4 + k * c:l4 + min((k + 1) * c, P)]
        h = bytearray(f[:l4])
        if k:
            h[l3 + 20:l4] = noop_options(h[l3 + 20:l4])
        h[l3 + 2:l3 + 4] = (ihl + len(pay)).to_bytes(2, "big")
        more = k != n - 1 or fw & MF
        h[l3 + 6:l3 + 8] = ((o + k * c // 8) | (MF if more else 0)).to_bytes(2, "big")
        h[l3 + 10:l3 + 12] = b"\0\0"
        h[l3 + 10:l3 + 12] = csum_field(h[l3:l4]).to_bytes(2, "big")
        out.append(bytes(h) + pay)
    return out


def fragment_ip6(f, l3, l4, mtu, ident):
    plen = int.from_bytes(f[l3 + 4:l3 + 6], "big")
    E = l3 + 40 + plen
    if not (l3 + 40 <= l4 <= E <= len(f)) or 40 + plen <= mtu:
        return None
    nh, x, U, nhoff = f[l3 + 6], l3 + 40, l3 + 40, l3 + 6
    for _ in range(MAX_IP6_EXT):
        if x >= l4:
            break
        if nh == 44:
            return None
        if nh in (0, 43, 60):
            n = 8 * (1 + f[x + 1])
        elif nh == 51:
            n = 4 * (2 + f[x + 1])
        else:
            break
        if x + n > l4:
            return None
        if nh == 43 or (nh == 0 and x == l3 + 40):
            U, nhoff = x + n, x
        nh, x = f[x], x + n
    if mtu < (U - l3) + 16:
        return None
    c = (mtu - (U - l3) - 8) & ~7
    F = E - U
    n = -(-F // c)
    out = []
    for k in range(n):
        pay = f[U + k * c:U + min((k + 1) * c, F)]
        h = bytearray(f[:U])
        h[l3 + 4:l3 + 6] = (U - l3 - 40 + 8 + len(pay)).to_bytes(2, "big")
        fh = bytes([h[nhoff], 0]) + ((k * c) | (k < n - 1)).to_bytes(2, "big") + \
            (ident & 0xffffffff).to_bytes(4, "big")
        h[nhoff] = 44
        out.append(bytes(h) + fh + pay)
    return out


def fragment_frame(f, r, det, i, mtu, ignore_df=False, ip6_ident=0):
    """The output frames of frame `f`, the batch's i-th, with record `r` and dispatch
    ethertype `det`."""
    l3, l4, status = int(r["l3_off"]), int(r["l4_off"]), int(r["status"])
    out = None
    if det == 0x0800 and status in IP4_STATUSES:
        out = fragment_ip4(f, l3, l4, mtu, ignore_df)
    elif det == 0x86DD and status in IP6_STATUSES:
        out = fragment_ip6(f, l3, l4, mtu, ip6_ident + i)
    return [f] if out is None else out


def fragment(hb, recs, mtu, ignore_df=False, ip6_ident=0):
    """(out_frames, frag_first, totals): the output frames as byte strings in order, frag_first
    (u32, n + 1) and totals (u64: n_out, out_bytes_needed)."""
    det = dispatch_ethertype(recs)
    out, first = [], np.zeros(hb.n + 1, dtype=np.uint32)
    for i, f in enumerate(sm.frames_of(hb)):
        out += fragment_frame(f, recs[i], int(det[i]), i, mtu, ignore_df, ip6_ident)
        first[i + 1] = len(out)
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64)


# ---- hand-built frames -------------------------------------------------------------------

SRC4, DST4 = b"\xc0\xa8\x38\x0b", b"\xc0\xa8\x38\x0c"
SRC6, DST6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
# NOOP, Record Route (7, not copied, 7 bytes), LSRR (0x83, copied, 7 bytes), EOL: 16 bytes
OPTIONS_MIX = bytes([1, 7, 7, 4, 0xa, 0xb, 0xc, 0xd, 0x83, 7, 4, 0x21, 0x22, 0x23, 0x24, 0])
# 40 bytes: the mix without its EOL, Router Alert (0x94, copied), Timestamp (0x44, not copied),
# NOOP, a Record Route of 11 bytes, EOL
OPTIONS_40 = (OPTIONS_MIX[:15] + bytes([0x94, 4, 0, 0]) + bytes([0x44, 8, 5, 0, 0, 0, 0, 9]) + b"\x01" +
              bytes([7, 11, 4, 1, 2, 3, 4, 5, 6, 7, 8]) + b"\0")
assert len(OPTIONS_40) == 40


def ip4(l4, proto=17, options=b"", frag=0, tags=0, ident=0x1234, pad=0, tos=0):
    """Ether [+ tags] / IPv4 with `options` (a multiple of 4 bytes) / the bytes `l4`, valid
    header sum, `pad` bytes of Ethernet padding after the IP packet."""
    ihl = 20 + len(options)
    ip = bytearray(20) + bytes(options)
    ip[0], ip[1] = 0x40 | ihl // 4, tos
    ip[2:4] = (ihl + len(l4)).to_bytes(2, "big")
    ip[4:6], ip[6:8] = ident.to_bytes(2, "big"), frag.to_bytes(2, "big")
    ip[8], ip[9] = 64, proto
    ip[12:16], ip[16:20] = SRC4, DST4
    ip[10:12] = csum_field(ip).to_bytes(2, "big")
    return ether(tags) + bytes(ip) + bytes(l4) + b"\x5a" * pad


def udp(payload, pseudo):
    """A UDP datagram with a filled checksum over pseudo(length)."""
    h = bytearray(b"\x13\x88\x01\xbb" + (8 + len(payload)).to_bytes(2, "big") + b"\0\0")
    ck = csum_field(pseudo(8 + len(payload)), h, payload)
    h[6:8] = (ck or 0xffff).to_bytes(2, "big")
    return bytes(h) + payload


def udp4(n, **kw):
    """An IPv4 packet whose payload is `n` bytes: a UDP datagram with a filled checksum (n >= 8)."""
    d = udp(payload_bytes(n - 8, n), lambda ln: SRC4 + DST4 + b"\0\x11" + ln.to_bytes(2, "big"))
    return ip4(d, 17, **kw)


def icmp4(n, **kw):
    """An ICMP echo of n bytes (n >= 8), valid sum."""
    m = bytearray(b"\x08\0\0\0\x12\x34\0\x01" + payload_bytes(n - 8, n + 1))
    m[2:4] = csum_field(m).to_bytes(2, "big")
    return ip4(bytes(m), 1, **kw)


def tcp4(n, **kw):
    """An IPv4 packet whose payload is n bytes of TCP (header 20 B, n >= 20)."""
    pay = payload_bytes(n - 20, n + 2)
    t = sm.tcp_header(pay, lambda ln: SRC4 + DST4 + b"\0\x06" + ln.to_bytes(2, "big"))
    return ip4(t + pay, 6, **kw)


def ext(kind, body_len=8, fill=0):
    """(type, bytes) of a Hop-by-Hop (0) / Destination options (60) header of body_len bytes (a
    multiple of 8): one PadN; byte 0 (next header) is filled in by ip6()."""
    return (kind, bytes([0, body_len // 8 - 1, 1, body_len - 4]) + bytes([fill]) * (body_len - 4))


def ip6(l4, proto=17, exts=(), tags=0, pad=0):
    """Ether [+ tags] / IPv6 / extension headers ((type, bytes), byte 0 filled in here) / l4."""
    types = [t for t, _ in exts] + [proto]
    chain = b"".join(bytes([types[k + 1]]) + bytes(b[1:]) for k, (_, b) in enumerate(exts))
    ip = bytearray(40)
    ip[0] = 0x60
    ip[4:6] = (len(chain) + len(l4)).to_bytes(2, "big")
    ip[6], ip[7] = types[0], 64
    ip[8:24], ip[24:40] = SRC6, DST6
    return ether(tags, 0x86DD) + bytes(ip) + chain + bytes(l4) + b"\x5a" * pad


def udp6(n, exts=(), **kw):
    """An IPv6 packet with `exts` and then n bytes of UDP (filled checksum; the pseudo header
    takes the fixed header's destination: no routing header here has segments left)."""
    d = udp(payload_bytes(n - 8, n + 3), lambda ln: SRC6 + DST6 + ln.to_bytes(4, "big") + b"\0\0\0\x11")
    return ip6(d, 17, exts, **kw)


def tcp6(n, exts=(), **kw):
    pay = payload_bytes(n - 20, n + 4)
    t = sm.tcp_header(pay, lambda ln: SRC6 + DST6 + ln.to_bytes(4, "big") + b"\0\0\0\x06")
    return ip6(t + pay, 6, exts, **kw)


def fragment_header(nh, off=0, more=0, ident=7):
    return (44, bytes([nh, 0]) + (off | more).to_bytes(2, "big") + ident.to_bytes(4, "big"))


HBH, DEST, RT0, AUTH = ext(0), ext(60, 16, 3), sm.routing(0, 1, 0), sm.auth_header(24)
LONG_EXTS = (ext(0, 40, 5), ext(60, 48, 6), sm.routing(0, 3, 0))     # U = l3 + 40 + 40 + 48 + 56
MTU_VALUES = (28, 29, 35, 36, 48, 68, 576, 1280, 1500, 65535)


@functools.lru_cache(maxsize=None)
def hand_frames(mtu):
    """The hand-built set for one mtu: for IPv4 (ihl 20) and IPv6 (no extension header) IP
    payloads of c - 1, c, c + 1, 2c, 2c + 1 bytes and packets 1 and 0 bytes over the mtu; then
    at a packet that gives three fragments or so the header variety (options, tags, extension
    headers, padding, UDP / ICMP / TCP, DF, input fragments) and the frames that must pass
    through.  Lengths are capped so that an IP packet stays within 65,535 bytes."""
    def cap(n, hdr, low):
        return max(low, min(n, 65535 - hdr))
    frames = []
    c4, c6 = max((mtu - 20) & ~7, 8), max((mtu - 48) & ~7, 8)
    for k, p in enumerate((c4 - 1, c4, c4 + 1, 2 * c4, 2 * c4 + 1, mtu + 1 - 20, mtu - 20)):
        frames.append(udp4(cap(p, 20, 8), ident=0x100 + k))
    for k, p in enumerate((c6 - 1, c6, c6 + 1, 2 * c6, 2 * c6 + 1, mtu + 1 - 40, mtu - 40)):
        frames.append(udp6(cap(p, 40, 8)))
    big = 2 * mtu + 9 if mtu <= 1500 else 3000                     # IP payload of the variety
    b4, b6 = cap(big, 60, 20), cap(big, 40 + 160, 20)
    frames += [
        # ihl 6 (a Record Route cut short by the header's end: the walk stops), 9 and 15
        udp4(b4, options=OPTIONS_MIX[:4]), udp4(b4, options=OPTIONS_MIX),
        udp4(b4, options=OPTIONS_40, tags=2),
        udp4(b4, tags=1), udp4(b4, tags=2, pad=5), icmp4(b4, pad=1), tcp4(b4), tcp4(b4, tags=1),
        udp4(b4, frag=DF), udp4(b4, frag=DF, options=OPTIONS_MIX),
        # input fragments: a first one (MF), a middle one (MF, offset), a last one (offset); one
        # whose offset leaves no room for the cut's offsets
        udp4(b4, frag=MF), udp4(b4, frag=MF | 0x0123, options=OPTIONS_MIX), udp4(b4, frag=0x0040),
        udp4(b4, frag=0x1ff0), udp4(b4, frag=0x8000),
        udp6(b6, (HBH,)), udp6(b6, LONG_EXTS, tags=1), tcp6(b6, (HBH, RT0)),
        udp6(b6, (AUTH,)), udp6(b6, (DEST,), pad=3), tcp6(b6, tags=2),
        udp6(b6, (DEST, RT0, ext(60, 8, 9))), ip6(payload_bytes(b6, 5), 59),
        ip6(payload_bytes(b6, 6), 58, (HBH, AUTH, RT0, DEST)),
        # pass-through: a Fragment header (atomic, and a real fragment), ARP, truncated frames,
        # an empty frame
        udp6(b6, (fragment_header(17),)), udp6(b6, (HBH, fragment_header(17, 8, 1))),
        ether(0, 0x0806) + bytes(28), udp4(b4)[:30], udp4(b4)[:-1], udp6(b6)[:-1], b"",
    ]
    return tuple(frames)
