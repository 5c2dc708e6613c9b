"""A plain model of rpkt_gpu_segment_batch (include/rpkt_gpu.h, "TCP segmentation"): host
frames and oracle records in, the output frames, seg_first and totals out.  It does its own
checksum arithmetic; tests/test_segment_model.py anchors it to the oracle's parse.  Also
the hand-built frames both segment tests use."""
import numpy as np

from oracle import oracle
from rpkt_amd import gen
from rpkt_amd.records import F_IPV6, dispatch_ethertype, ip6_block

F6 = 3 | F_IPV6
FIN, PSH, ACK, CWR = 0x01, 0x08, 0x10, 0x80


def fold_sum(data):
    """RFC 1071 sum of `data` as big-endian 16-bit words (an odd tail byte is the high byte
    of a last word), carries folded: 2^16 = 1 (mod 0xffff), so the sum's residue is the
    residue of the bytes read as one big number; a non-zero sum folds into 1..0xffff."""
    data = bytes(data)
    x = int.from_bytes(data + (b"\0" if len(data) & 1 else b""), "big")
    return 0 if x == 0 else (x - 1) % 0xffff + 1


def csum_field(*parts):
    """The checksum field for the parts' bytes (the field itself zeroed in them): the
    complement of the folded sum; 0 stays 0."""
    s = sum(fold_sum(p) for p in parts)
    return ~((s - 1) % 0xffff + 1) & 0xffff if s else 0xffff


def frames_of(hb):
    if hb.offsets is not None:
        return [hb.frames[int(hb.offsets[i]):int(hb.offsets[i + 1])].tobytes() for i in range(hb.n)]
    flen = hb.frame_len or hb.stride
    return [hb.frames[i * hb.stride:i * hb.stride + flen].tobytes() for i in range(hb.n)]


def oracle_records(hb, flags=F6):
    return oracle.parse_batch(hb.frames, hb.n, flags, offsets=hb.offsets, stride=hb.stride,
                              frame_len=hb.frame_len)


def is_segmented(r, v6, mss):
    return bool(r["status"] == 0 and r["ip_protocol"] == 6 and
                (v6 or (int(r["ip_frag"]) & 0x3fff) == 0) and int(r["payload_len"]) > mss)


def segment_frame(f, r, v6, pdst, mss):
    """The output frames of frame `f` with record `r` (v6: an IPv6 record, pdst its
    ip6_pdst_off)."""
    if not is_segmented(r, v6, mss):
        return [f]
    l3, l4, po, pl = int(r["l3_off"]), int(r["l4_off"]), int(r["payload_off"]), int(r["payload_len"])
    n = -(-pl // mss)
    ident = int.from_bytes(f[l3 + 4:l3 + 6], "big")
    seq = int.from_bytes(f[l4 + 4:l4 + 8], "big")
    out = []
    for k in range(n):
        pay = f[po + k * mss:po + min((k + 1) * mss, pl)]
        h = bytearray(f[:po])
        if v6:
            h[l3 + 4:l3 + 6] = (po - l3 - 40 + len(pay)).to_bytes(2, "big")
            pd = pdst if l3 + 24 <= pdst <= l4 - 16 else l3 + 24
            pseudo = bytes(h[l3 + 8:l3 + 24]) + bytes(h[pd:pd + 16]) + \
                (po - l4 + len(pay)).to_bytes(4, "big") + b"\0\0\0\x06"
        else:
            h[l3 + 2:l3 + 4] = (po - l3 + len(pay)).to_bytes(2, "big")
            h[l3 + 4:l3 + 6] = ((ident + k) & 0xffff).to_bytes(2, "big")
            h[l3 + 10:l3 + 12] = b"\0\0"
            h[l3 + 10:l3 + 12] = csum_field(h[l3:l4]).to_bytes(2, "big")
            pseudo = bytes(h[l3 + 12:l3 + 20]) + b"\0\x06" + (po - l4 + len(pay)).to_bytes(2, "big")
        h[l4 + 4:l4 + 8] = ((seq + k * mss) & 0xffffffff).to_bytes(4, "big")
        if k != n - 1:
            h[l4 + 13] &= ~(FIN | PSH) & 0xff
        if k != 0:
            h[l4 + 13] &= ~CWR & 0xff
        h[l4 + 16:l4 + 18] = b"\0\0"
        h[l4 + 16:l4 + 18] = csum_field(pseudo, h[l4:po], pay).to_bytes(2, "big")
        out.append(bytes(h) + pay)
    return out


def segment(hb, recs, mss):
    """(out_frames, seg_first, totals): the output frames as byte strings in order, seg_first
    (u32, n + 1) and totals (u64: n_out, out_bytes_needed)."""
    v6 = dispatch_ethertype(recs) == 0x86DD
    pd = ip6_block(recs)["ip6_pdst_off"]
    out, first = [], np.zeros(hb.n + 1, dtype=np.uint32)
    for i, f in enumerate(frames_of(hb)):
        out += segment_frame(f, recs[i], bool(v6[i]), int(pd[i]), mss)
        first[i + 1] = len(out)
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64)


def packed_output(out_frames, out_cap):
    """The packed batch the entry writes for `out_frames` over out_cap slots: the bytes and
    the out_cap + 1 offsets (spare slots empty, at the end)."""
    offs = np.zeros(out_cap + 1, dtype=np.uint32)
    ends = np.cumsum([len(o) for o in out_frames])
    offs[1:len(out_frames) + 1] = ends
    offs[len(out_frames) + 1:] = ends[-1] if len(ends) else 0
    return np.frombuffer(b"".join(out_frames), dtype=np.uint8), offs


def pack(frames, lead=0):
    """Packed HostBatch of byte strings; a `lead`-byte junk frame first shifts every
    following frame's alignment (16 spare bytes at the end)."""
    parts = ([b"\xee" * lead] if lead else []) + [bytes(f) for f in frames]
    offs = np.zeros(len(parts) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(p) for p in parts])
    blob = np.frombuffer(b"".join(parts) + bytes(16), dtype=np.uint8).copy()
    return gen.HostBatch(0, len(parts), 0, blob, offs, 0, 0)


# ---- hand-built frames -------------------------------------------------------------------

def payload_bytes(n, salt=0):
    return bytes((17 * k + 31 * (k >> 8) + salt + 1) & 0xff for k in range(n))


def ether(tags=0, ethertype=0x0800):
    f = b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02"
    if tags == 2:
        f += b"\x88\xa8\x20\x64"
    if tags >= 1:
        f += b"\x81\x00\x60\x07"
    return f + ethertype.to_bytes(2, "big")


def tcp_header(payload, pseudo_of, doff=5, seq=0x01020304, flags=ACK | PSH):
    h = bytearray(doff * 4)
    h[0:4] = b"\x13\x88\x01\xbb"
    h[4:8] = seq.to_bytes(4, "big")
    h[8:12] = b"\x0a\x0b\x0c\x0d"
    h[12], h[13] = doff << 4, flags
    h[14:16] = b"\x20\x00"
    for k in range(20, doff * 4):                       # options: NOPs, then a timestamp-like run
        h[k] = 1 if k < 24 else (k * 7) & 0xff
    h[16:18] = csum_field(pseudo_of(len(h) + len(payload)), h, payload).to_bytes(2, "big")
    return bytes(h)


def tcp4(payload, tags=0, ihl=5, doff=5, ident=0x1234, seq=0x01020304, flags=ACK | PSH, frag=0,
         pad=0, proto=6):
    """Ether [+ tags] / IPv4 (ihl words) / TCP (doff words) / payload, valid sums, `pad` bytes
    of Ethernet padding after the IP packet."""
    src, dst = b"\xc0\xa8\x38\x0b", b"\xc0\xa8\x38\x0c"
    tcp = tcp_header(payload, lambda n: src + dst + b"\0" + bytes([proto]) + n.to_bytes(2, "big"),
                     doff, seq, flags)
    ip = bytearray(ihl * 4)
    ip[0] = 0x40 | ihl
    ip[2:4] = (ihl * 4 + len(tcp) + len(payload)).to_bytes(2, "big")
    ip[4:6] = ident.to_bytes(2, "big")
    ip[6:8] = frag.to_bytes(2, "big")
    ip[8], ip[9] = 64, proto
    ip[12:16], ip[16:20] = src, dst
    for k in range(20, ihl * 4):
        ip[k] = 1                                       # NOP options
    ip[10:12] = csum_field(ip).to_bytes(2, "big")
    return ether(tags) + bytes(ip) + tcp + payload + b"\x5a" * pad


def tcp6(payload, exts=(), tags=0, doff=5, seq=0x01020304, flags=ACK | PSH, pad=0):
    """Ether [+ tags] / IPv6 / extension headers / TCP / payload.  exts: (type, bytes) with
    byte 0 (next header) filled in here; the pseudo destination follows a Routing header with
    segments left (types 0 and 2: the last address, type 4: the first)."""
    src, dst = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
    pdst, chain = dst, b""
    types = [t for t, _ in exts] + [6]
    for k, (t, body) in enumerate(exts):
        body = bytes([types[k + 1]]) + bytes(body[1:])
        if t == 43 and body[3] > 0 and len(body) >= 24:
            n = (len(body) - 8) // 16
            at = 8 if body[2] == 4 else 8 + 16 * (n - 1)
            if body[2] in (0, 2, 4):
                pdst = body[at:at + 16]
        chain += body
    tcp = tcp_header(payload, lambda n: src + pdst + n.to_bytes(4, "big") + b"\0\0\0\x06", doff,
                     seq, flags)
    ip = bytearray(40)
    ip[0] = 0x60
    ip[4:6] = (len(chain) + len(tcp) + len(payload)).to_bytes(2, "big")
    ip[6], ip[7] = types[0], 64
    ip[8:24], ip[24:40] = src, dst
    return ether(tags, 0x86DD) + bytes(ip) + chain + tcp + payload + b"\x5a" * pad


def hop_by_hop():
    return (0, bytes([0, 0, 1, 4, 0, 0, 0, 0]))                            # PadN


def routing(rtype, n_addr, left):
    body = bytes([0, 2 * n_addr, rtype, left, 0, 0, 0, 0])
    return (43, body + b"".join(bytes([0xa0 + a]) * 16 for a in range(n_addr)))


def auth_header(total):
    """An AH of `total` bytes (a multiple of 4, >= 12)."""
    return (51, bytes([0, total // 4 - 2, 0, 0]) + bytes((3 * k + 1) & 0xff for k in range(total - 4)))


def udp4(payload):
    f = bytearray(tcp4(b"", proto=17)[:34])
    f[16:18] = (28 + len(payload)).to_bytes(2, "big")
    f[24:26] = b"\0\0"
    f[24:26] = csum_field(f[14:34]).to_bytes(2, "big")
    udp = b"\x13\x88\x01\xbb" + (8 + len(payload)).to_bytes(2, "big") + b"\0\0"
    return bytes(f) + udp + payload


def variety(p):
    """Frames of TCP payload length p in every header shape the entry handles, then the
    frames it must pass through."""
    pay = payload_bytes(p, 3)
    both = FIN | PSH | CWR | ACK
    frames = [
        tcp4(pay, tags=1), tcp4(pay, tags=2), tcp4(pay, ihl=6), tcp4(pay, ihl=15),
        tcp4(pay, doff=6), tcp4(pay, doff=15), tcp4(pay, tags=2, ihl=15, doff=15),
        tcp6(pay), tcp6(pay, tags=1, doff=8),
        tcp6(pay, exts=(hop_by_hop(), routing(0, 2, 1))),
        tcp6(pay, exts=(hop_by_hop(), routing(4, 3, 2)), flags=both),
        tcp6(pay, exts=(routing(0, 1, 0),)),                       # none left: dst_addr
        tcp6(pay, exts=(auth_header(96),)),                        # TCP header at 54 + 96
        tcp6(pay, exts=(hop_by_hop(), auth_header(120), routing(4, 2, 1)), doff=15),
        tcp4(pay, ident=0xffff, seq=0xfffffff0, flags=both),
        tcp4(pay, ident=0xfffe, seq=0xffffffff - p // 2, flags=FIN | ACK),
        tcp4(pay, pad=6), tcp4(pay, tags=1, pad=1), tcp6(pay, pad=3),
        # not segmented: a first fragment (MF), a later fragment
        tcp4(pay, frag=0x2000), tcp4(pay, frag=0x0010),
        # pass-through: UDP, ARP, a truncated TCP header, a zero-length frame
        udp4(pay), ether(0, 0x0806) + bytes(28), tcp4(pay)[:50], b"",
    ]
    return frames


MSS_VALUES = (1, 2, 3, 7, 16, 17, 536, 1448, 65535)


def hand_frames(mss):
    """The hand-built set for one mss: payload lengths around it, the header variety at a
    payload of two segments and a bit, and for 536 / 1448 one 65,535-byte IP packet."""
    top = 65535 - 40                                               # IPv4 + TCP headers
    lens = [5] if mss == 1 else []
    lens += [min(x, top) for x in (mss, mss + 1, 2 * mss, 2 * mss - 1, 1, 0)]
    frames = [tcp4(payload_bytes(p, k), seq=0x10000000 * k + 7) for k, p in enumerate(lens)]
    frames += variety(min(2 * mss + 1, 2000) if mss < 65535 else 100)
    if mss in (536, 1448):
        frames.append(tcp4(payload_bytes(top, 9), flags=both_flags()))
    return frames


def both_flags():
    return FIN | PSH | CWR | ACK


def tso_tx_frame():
    """rpkt-dpdk/examples/tso_tx.rs:36-64 as bytes: Ether / IPv4 / TCP with a 4000-byte
    payload of 0xae (the example leaves the checksums to the port; they are zero here)."""
    pay = b"\xae" * 4000
    tcp = bytearray(20)
    tcp[0:2], tcp[2:4] = (60376).to_bytes(2, "big"), (161).to_bytes(2, "big")
    tcp[4:8], tcp[8:12] = (0x8e501902).to_bytes(4, "big"), (0xc7529d89).to_bytes(4, "big")
    tcp[12], tcp[13] = 0x50, ACK | PSH
    tcp[14:16] = (46).to_bytes(2, "big")
    ip = bytearray(20)                                             # the template: ident, frag 0
    ip[0] = 0x45
    ip[2:4] = (20 + 20 + 4000).to_bytes(2, "big")
    ip[8], ip[9] = 128, 6
    ip[12:16], ip[16:20] = bytes([172, 0, 10, 17]), bytes([192, 168, 23, 2])
    eth = bytes([0xac, 0xdc, 0xca, 0x79, 0xe5, 0xc6]) + bytes([0xac, 0xdc, 0xca, 0x79, 0xca, 0x86])
    return eth + b"\x08\x00" + bytes(ip) + bytes(tcp) + pay
