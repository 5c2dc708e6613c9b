"""A plain model of the UDP side of the re-framing entries (include/rpkt_gpu.h:
RPKT_SEGMENT_UDP for rpkt_gpu_segment_batch / rpkt_gpu_segment_chains, RPKT_COALESCE_UDP for
rpkt_gpu_coalesce_batch).  segment / segment_frame / coalesce here are
tests/segment_model.py's and tests/coalesce_model.py's with a `udp` argument: TCP frames go to
those models, UDP datagrams are cut under the __udp_gso_segment rules and merged under the
udp_gro_receive_segment rules as the header states them.  The checksum arithmetic is
segment_model.csum_field with UDP's "0 is sent as 0xffff"; tests/test_udp_reframe_model.py
anchors it to the oracle's parse.  Also the hand-built UDP frames the tests use."""
import numpy as np

from rpkt_amd.records import dispatch_ethertype, ip6_block

import coalesce_model as cm
import segment_model as sm

DF = 0x4000
TOP = 65535 - 28                                # the largest UDP payload over IPv4: 65,507


def udp_csum_field(*parts):
    """The UDP checksum field for the parts' bytes: csum_field's, a result of 0 sent as 0xffff."""
    return sm.csum_field(*parts) or 0xffff


# ---- segmentation ------------------------------------------------------------------------

def is_udp_segmented(r, v6, mss):
    return bool(r["status"] == 0 and r["ip_protocol"] == 17 and
                (v6 or (int(r["ip_frag"]) & 0x3fff) == 0) and
                int(r["payload_off"]) - int(r["l4_off"]) == 8 and int(r["payload_len"]) > mss)


def pseudo_header(h, v6, l3, l4, pdst, proto, l4_len):
    """The pseudo header of the header bytes `h`: for IPv6 the destination at pdst under
    rpkt_gpu_build_batch's rule."""
    if v6:
        pd = pdst if l3 + 24 <= pdst <= l4 - 16 else l3 + 24
        return bytes(h[l3 + 8:l3 + 24]) + bytes(h[pd:pd + 16]) + l4_len.to_bytes(4, "big") + \
            bytes([0, 0, 0, proto])
    return bytes(h[l3 + 12:l3 + 20]) + bytes([0, proto]) + l4_len.to_bytes(2, "big")


def udp_output(head, v6, l3, l4, po, pdst, pay, ident=None):
    """The header head[:po] re-written for the payload `pay`: the IP lengths, the IPv4 ident
    (None: the header's own) and checksum, the UDP length and checksum."""
    h = bytearray(head[:po])
    if v6:
        h[l3 + 4:l3 + 6] = (po - l3 - 40 + len(pay)).to_bytes(2, "big")
    else:
        h[l3 + 2:l3 + 4] = (po - l3 + len(pay)).to_bytes(2, "big")
        if ident is not None:
            h[l3 + 4:l3 + 6] = (ident & 0xffff).to_bytes(2, "big")
        h[l3 + 10:l3 + 12] = b"\0\0"
        h[l3 + 10:l3 + 12] = sm.csum_field(h[l3:l4]).to_bytes(2, "big")
    h[l4 + 4:l4 + 6] = (8 + len(pay)).to_bytes(2, "big")
    h[l4 + 6:l4 + 8] = b"\0\0"
    pseudo = pseudo_header(h, v6, l3, l4, pdst, 17, 8 + len(pay))
    h[l4 + 6:l4 + 8] = udp_csum_field(pseudo, h[l4:po], pay).to_bytes(2, "big")
    return bytes(h) + pay


def segment_frame(f, r, v6, pdst, mss, udp=False):
    """segment_model.segment_frame with RPKT_SEGMENT_UDP as `udp`."""
    if not (udp and is_udp_segmented(r, v6, mss)):
        return sm.segment_frame(f, r, v6, pdst, mss)
    l3, l4, po, pl = int(r["l3_off"]), int(r["l4_off"]), int(r["payload_off"]), int(r["payload_len"])
    ident = int.from_bytes(f[l3 + 4:l3 + 6], "big")
    return [udp_output(f, v6, l3, l4, po, pdst, f[po + k * mss:po + min((k + 1) * mss, pl)], ident + k)
            for k in range(-(-pl // mss))]


def segment(hb, recs, mss, udp=False):
    """segment_model.segment with RPKT_SEGMENT_UDP as `udp`: (out_frames, seg_first, totals)."""
    v6 = dispatch_ethertype(recs) == 0x86DD
    pd = ip6_block(recs)["ip6_pdst_off"]
    out, first = [], np.zeros(hb.n + 1, dtype=np.uint32)
    for i, f in enumerate(sm.frames_of(hb)):
        out += segment_frame(f, recs[i], bool(v6[i]), int(pd[i]), mss, udp)
        first[i + 1] = len(out)
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64)


def cut_counts(recs, mss):
    """(UDP frames, TCP frames) of the records that are cut at mss with the flag."""
    v6 = dispatch_ethertype(recs) == 0x86DD
    return (sum(is_udp_segmented(r, bool(v), mss) for r, v in zip(recs, v6)),
            sum(sm.is_segmented(r, bool(v), mss) for r, v in zip(recs, v6)))


# ---- coalescing --------------------------------------------------------------------------

class Pos(cm.Pos):
    """coalesce_model.Pos; with `udp` a UDP datagram is eligible under its own rule."""

    def __init__(self, f=b"", r=None, ethertype=0, pdst=0, trust=False, udp=False):
        super().__init__(f, r, ethertype, pdst, trust)
        self.udp = False
        if not udp or r is None or r["ip_protocol"] != 17:
            return
        l3, l4, po, v6 = self.l3, self.l4, self.po, self.v6
        nest = l3 <= l4 <= po <= len(f) and po - l4 == 8 and \
            (l4 - l3 >= 40 if v6 else 20 <= l4 - l3 <= 60)
        if not nest:
            return
        self.udp = True
        self.p = min(int(r["payload_len"]), len(f) - po)
        sums = trust or (int(r["l4_sum"]) == 0xffff and (v6 or int(r["ip_sum"]) == 0xffff))
        self.elig = bool(r["status"] == 0 and ethertype in (0x0800, 0x86DD) and
                         (v6 or (int(r["ip_frag"]) & 0x3fff) == 0) and self.p >= 1 and sums and
                         f[l4 + 6:l4 + 8] != b"\0\0")

    def udp_masked_header(self):
        h = bytearray(self.f[:self.po])
        l3, l4 = self.l3, self.l4
        for a, b in (((l3 + 4, l3 + 6),) if self.v6 else ((l3 + 2, l3 + 6), (l3 + 10, l3 + 12))) + \
                ((l4 + 4, l4 + 8),):
            h[a:b] = bytes(b - a)
        return bytes(h)


def base(a, b):
    """B: position b continues position a."""
    if not (a.udp or b.udp):
        return cm.base(a, b)
    if not (a.udp and b.udp and a.elig and b.elig) or a.v6 != b.v6 or \
            (a.l3, a.l4, a.po) != (b.l3, b.l4, b.po):
        return False
    if a.udp_masked_header() != b.udp_masked_header():
        return False
    return bool(b.v6 or b.f[b.l3 + 6] & 0x40 or
                b.be(b.l3 + 4, 2) == (a.be(a.l3 + 4, 2) + 1) & 0xffff)


def merge(group):
    head = group[0]
    if not head.udp:
        return cm.merge(group)
    pay = b"".join(m.f[m.po:m.po + m.p] for m in group)
    return udp_output(head.f, head.v6, head.l3, head.l4, head.po, head.pdst, pay)


def coalesce(hb, recs, order=None, max_payload=65535, trust_sums=False, udp=False):
    """coalesce_model.coalesce with RPKT_COALESCE_UDP as `udp`: (out_frames, src_first, totals,
    out_mss).  short, link and the greedy cut are written out again: they are the same rule
    over this module's positions."""
    frames = sm.frames_of(hb)
    et = dispatch_ethertype(recs)
    pd = ip6_block(recs)["ip6_pdst_off"]
    idx = range(hb.n) if order is None else [int(x) for x in order]
    P = [Pos(frames[k], recs[k], int(et[k]), int(pd[k]), trust_sums, udp) if k < hb.n else Pos()
         for k in idx]
    n = len(P)
    B = [i > 0 and base(P[i - 1], P[i]) for i in range(n)]
    short = [B[i] and P[i].p < P[i - 1].p for i in range(n)]
    link = [B[i] and P[i].p <= P[i - 1].p and not short[i - 1] for i in range(n)]
    groups, held = [], 0
    for i in range(n):
        if link[i]:
            head = P[groups[-1][0]]
            limit = min(max_payload, 65535 - (head.po - head.l3 - (40 if head.v6 else 0)))
            if held + P[i].p <= limit:
                groups[-1].append(i)
                held += P[i].p
                continue
        groups.append([i])
        held = P[i].p
    out = [P[g[0]].f if len(g) == 1 else merge([P[k] for k in g]) for g in groups]
    first = np.full(n + 1, n, dtype=np.uint32)
    first[:len(groups)] = [g[0] for g in groups]
    mss = np.zeros(n, dtype=np.uint16)
    mss[:len(groups)] = [P[g[0]].p if len(g) > 1 else 0 for g in groups]
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64), mss


# ---- hand-built frames -------------------------------------------------------------------

def udp_header(payload, pseudo_of, sport, zero_csum):
    h = bytearray(sport.to_bytes(2, "big") + b"\x01\xbb" + (8 + len(payload)).to_bytes(2, "big") + b"\0\0")
    if not zero_csum:
        h[6:8] = udp_csum_field(pseudo_of(len(h) + len(payload)), h, payload).to_bytes(2, "big")
    return bytes(h)


def udp4(payload, tags=0, ihl=5, ident=0x1234, df=False, frag=0, pad=0, zero_csum=False,
         sport=5000, ttl=64):
    """Ether [+ tags] / IPv4 (ihl words) / UDP / payload, valid sums (zero_csum: a UDP checksum
    field of 0, "not computed"), `pad` bytes of Ethernet padding after the IP packet."""
    src, dst = b"\xc0\xa8\x38\x0b", b"\xc0\xa8\x38\x0c"
    udp = udp_header(payload, lambda n: src + dst + b"\0\x11" + n.to_bytes(2, "big"), sport, zero_csum)
    ip = bytearray(ihl * 4)
    ip[0] = 0x40 | ihl
    ip[2:4] = (ihl * 4 + 8 + len(payload)).to_bytes(2, "big")
    ip[4:6] = ident.to_bytes(2, "big")
    ip[6:8] = (frag | (DF if df else 0)).to_bytes(2, "big")
    ip[8], ip[9] = ttl, 17
    ip[12:16], ip[16:20] = src, dst
    for k in range(20, ihl * 4):
        ip[k] = 1                                       # NOP options
    ip[10:12] = sm.csum_field(ip).to_bytes(2, "big")
    return sm.ether(tags) + bytes(ip) + udp + payload + b"\x5a" * pad


def udp6(payload, exts=(), tags=0, pad=0, zero_csum=False, sport=5000):
    """Ether [+ tags] / IPv6 / extension headers / UDP / payload; exts as segment_model.tcp6
    takes them (the pseudo destination follows a Routing header with segments left)."""
    src, dst = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
    pdst, chain = dst, b""
    types = [t for t, _ in exts] + [17]
    for k, (t, body) in enumerate(exts):
        body = bytes([types[k + 1]]) + bytes(body[1:])
        if t == 43 and body[3] > 0 and len(body) >= 24 and body[2] in (0, 2, 4):
            n = (len(body) - 8) // 16
            at = 8 if body[2] == 4 else 8 + 16 * (n - 1)
            pdst = body[at:at + 16]
        chain += body
    udp = udp_header(payload, lambda n: src + pdst + n.to_bytes(4, "big") + b"\0\0\0\x11", sport,
                     zero_csum)
    ip = bytearray(40)
    ip[0] = 0x60
    ip[4:6] = (len(chain) + 8 + len(payload)).to_bytes(2, "big")
    ip[6], ip[7] = types[0], 64
    ip[8:24], ip[24:40] = src, dst
    return sm.ether(tags, 0x86DD) + bytes(ip) + chain + udp + payload + b"\x5a" * pad


def solve_last_two(make, n, at, field_of, salt=0):
    """The frame make(payload) of an n-byte payload whose bytes [at, at + 2) are solved so
    that the checksum field_of(frame) reads comes out of a computed 0 (written 0xffff).  With
    the two bytes zero the field is the complement of the sum S of everything else; putting
    that complement there makes the sum S + ~S = 0xffff, whose complement is 0.  (A field of
    0xffff with the bytes zero: S is 0xffff already, the bytes stay zero.)  `at` is an even
    offset into the summed payload, so the two bytes are one word of the sum."""
    pay = bytearray(sm.payload_bytes(n, salt))
    pay[at:at + 2] = b"\0\0"
    c = field_of(make(bytes(pay)))
    pay[at:at + 2] = (0 if c == 0xffff else c).to_bytes(2, "big")
    return make(bytes(pay))


def zero_sum_segment(make, mss, records_of, salt=0):
    """A datagram of two segments at mss whose second segment's computed UDP checksum is 0
    (make(payload) -> frame, records_of(frame) -> (record, v6, pdst)); None where no segment
    can hold the two solved bytes at an even offset (mss 1) or the datagram would pass 65,507."""
    q = mss if mss % 2 == 0 else mss - 1                      # the second segment's payload
    if q < 2 or mss + q > TOP:
        return None

    def field_of(f):
        r, v6, pdst = records_of(f)
        seg = segment_frame(f, r, v6, pdst, mss, True)[1]
        l4 = int(r["l4_off"])
        return int.from_bytes(seg[l4 + 6:l4 + 8], "big")
    return solve_last_two(make, mss + q, mss + q - 2, field_of, salt)


def zero_sum_datagram(make, n, l4_of, salt=0):
    """A datagram of n payload bytes (n even) whose own computed UDP checksum is 0, so its
    field reads 0xffff: what the merge of its segments must write.  l4_of(frame): its l4_off."""
    assert n % 2 == 0 and n >= 2

    def field_of(f):
        l4 = l4_of(f)
        return int.from_bytes(f[l4 + 6:l4 + 8], "big")
    return solve_last_two(make, n, n - 2, field_of, salt)


def record_of(f):
    """(record, v6, ip6_pdst_off) of one frame from the oracle."""
    recs = sm.oracle_records(sm.pack([f]))
    return recs[0], bool(dispatch_ethertype(recs)[0] == 0x86DD), int(ip6_block(recs)["ip6_pdst_off"][0])


def udp_variety(p):
    """Datagrams of payload length p in every header shape the entries handle, then the UDP
    frames that pass through."""
    pay = sm.payload_bytes(p, 5)
    hop, routing, ah = sm.hop_by_hop, sm.routing, sm.auth_header
    return [
        udp4(pay, tags=1), udp4(pay, tags=2), udp4(pay, ihl=6), udp4(pay, tags=2, ihl=15),
        udp6(pay), udp6(pay, tags=1),
        udp6(pay, exts=(hop(), routing(0, 2, 1))),                 # a moved pseudo destination
        udp6(pay, exts=(hop(), routing(4, 3, 2))),
        udp6(pay, exts=(routing(0, 1, 0),)),                       # none left: dst_addr
        udp6(pay, exts=(ah(96),)),                                 # the UDP header at 54 + 96
        udp6(pay, exts=(hop(), ah(120), routing(4, 2, 1))),
        udp4(pay, ident=0xffff), udp4(pay, ident=0xfffe, df=True),
        udp4(pay, pad=6), udp4(pay, tags=1, pad=1), udp6(pay, pad=3),
        udp4(pay, zero_csum=True), udp6(pay, zero_csum=True),
        # not segmented: a first fragment (MF), a later fragment, a truncated UDP header
        udp4(pay, frag=0x2000), udp4(pay, frag=0x0010), udp4(pay)[:38],
    ]


MSS_VALUES = (1, 7, 16, 17, 536, 1448, 65535)


def hand_frames(mss):
    """The hand-built set for one mss: UDP payload lengths around it, the header variety at a
    payload of two segments and a bit, the datagram whose second segment's checksum computes
    to 0, TCP frames mixed in, and for 536 / 1448 the 65,507-byte datagram."""
    lens = [min(x, TOP) for x in (mss, mss + 1, 2 * mss, 2 * mss - 1, 1, 0)]
    frames = [udp4(sm.payload_bytes(p, k), ident=0x0100 * k + 3, sport=5000 + k)
              for k, p in enumerate(lens)]
    p = min(2 * mss + 1, 2000) if mss < 65535 else 100
    frames += udp_variety(p)
    for make in (lambda pay: udp4(pay, tags=1, ident=0xfffe), lambda pay: udp6(pay, exts=(sm.routing(0, 2, 1),))):
        f = zero_sum_segment(make, mss, record_of, salt=mss)
        if f is not None:
            frames.append(f)
    tcp = sm.payload_bytes(p, 3)
    frames += [sm.tcp4(tcp, tags=1), sm.tcp6(tcp, exts=(sm.hop_by_hop(), sm.routing(0, 2, 1))),
               sm.tcp4(tcp, flags=sm.both_flags(), pad=6), sm.tcp4(tcp)[:50], b""]
    if mss in (536, 1448):
        frames.append(udp4(sm.payload_bytes(TOP, 9), ident=0xfff0))
    return frames


def zero_sum_segments(out_frames, recs):
    """How many of the output frames are UDP with a checksum field of 0xffff."""
    return sum(1 for f, r in zip(out_frames, recs) if r["status"] == 0 and r["ip_protocol"] == 17 and
               f[int(r["l4_off"]) + 6:int(r["l4_off"]) + 8] == b"\xff\xff")


def round_trip_frames(mss):
    """Super-frames for coalesce(segment(F)) == F: filled checksums, no padding, neighbours
    that differ in a compared byte (the source port); payloads of exactly 2 * mss, of mss + 1
    and of 65,507, DF set and clear, IPv6 with a moved pseudo destination, and one whose own
    checksum computes to 0."""
    two = min(2 * mss, TOP)
    frames = [
        udp4(sm.payload_bytes(two, 1), sport=6000, ident=0x1000),
        udp4(sm.payload_bytes(mss + 1, 2), sport=6001, ident=0xffff),
        udp4(sm.payload_bytes(TOP, 3), sport=6002, ident=0x2000, df=True),
        udp4(sm.payload_bytes(3 * mss + 2, 4), sport=6003, tags=2, ihl=7, ident=0x3000),
        udp6(sm.payload_bytes(two, 5), sport=6004),
        udp6(sm.payload_bytes(4 * mss + 1, 6), sport=6005, exts=(sm.hop_by_hop(), sm.routing(0, 2, 1))),
        sm.tcp4(sm.payload_bytes(3 * mss, 7), flags=sm.ACK),
        zero_sum_datagram(lambda pay: udp4(pay, sport=6006, ident=0x4000), 2 * mss + 2,
                          lambda f: 34, salt=8),
        udp4(sm.payload_bytes(TOP, 9), sport=6007, ident=0x5000),
    ]
    return frames
