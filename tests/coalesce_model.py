"""A plain model of rpkt_gpu_coalesce_batch (include/rpkt_gpu.h, "TCP receive coalescing"):
host frames, oracle records and an optional order in, the output frames, src_first, totals
and out_mss out.  The rules are written as the header states them -- eligibility, the base
predicate B, short / link over three neighbouring positions, the greedy cut of a run into
groups -- with no closed forms; frames, packing and checksum arithmetic come from
tests/segment_model.py."""
import numpy as np

from rpkt_amd.records import dispatch_ethertype, ip6_block

import segment_model as sm

SYN, RST, URG = 0x02, 0x04, 0x20
F_ALL = sm.F6                                   # both sums and IPv6: what coalescing wants


class Pos:
    """One position: its frame's bytes and what its record says (None fields: an empty frame)."""

    def __init__(self, f=b"", r=None, ethertype=0, pdst=0, trust=False):
        self.f, self.elig, self.v6, self.p = f, False, ethertype == 0x86DD, 0
        if r is None:
            return
        self.l3, self.l4, self.po = int(r["l3_off"]), int(r["l4_off"]), int(r["payload_off"])
        self.pdst = pdst
        l3, l4, po, v6 = self.l3, self.l4, self.po, self.v6
        nest = l3 <= l4 <= po <= len(f) and 20 <= po - l4 <= 60 and \
            (l4 - l3 >= 40 if v6 else 20 <= l4 - l3 <= 60)
        if not nest:
            return
        self.p = min(int(r["payload_len"]), len(f) - po)
        sums = trust or (int(r["l4_sum"]) == 0xffff and (v6 or int(r["ip_sum"]) == 0xffff))
        self.elig = bool(r["status"] == 0 and r["ip_protocol"] == 6 and ethertype in (0x0800, 0x86DD)
                         and (v6 or (int(r["ip_frag"]) & 0x3fff) == 0) and self.p >= 1 and sums
                         and not f[l4 + 13] & (SYN | RST | URG))

    def masked_header(self):
        h = bytearray(self.f[:self.po])
        l3, l4 = self.l3, self.l4
        for a, b in (((l3 + 4, l3 + 6),) if self.v6 else ((l3 + 2, l3 + 6), (l3 + 10, l3 + 12))) + \
                ((l4 + 4, l4 + 8), (l4 + 16, l4 + 18)):
            h[a:b] = bytes(b - a)
        h[l4 + 13] &= 0xff & ~(sm.FIN | sm.PSH | sm.CWR)
        return bytes(h)

    def be(self, at, n):
        return int.from_bytes(self.f[at:at + n], "big")


def base(a, b):
    """B: position b continues position a."""
    if not (a.elig and b.elig) or a.v6 != b.v6 or (a.l3, a.l4, a.po) != (b.l3, b.l4, b.po):
        return False
    if a.masked_header() != b.masked_header():
        return False
    if b.be(b.l4 + 4, 4) != (a.be(a.l4 + 4, 4) + a.p) & 0xffffffff:
        return False
    if not b.v6 and not b.f[b.l3 + 6] & 0x40 and b.be(b.l3 + 4, 2) != (a.be(a.l3 + 4, 2) + 1) & 0xffff:
        return False
    return not a.f[a.l4 + 13] & (sm.FIN | sm.PSH) and not b.f[b.l4 + 13] & sm.CWR


def merge(group):
    """The merged frame of a group of two positions or more."""
    head, last = group[0], group[-1]
    l3, l4, po = head.l3, head.l4, head.po
    pay = b"".join(m.f[po:po + m.p] for m in group)
    h = bytearray(head.f[:po])
    if head.v6:
        h[l3 + 4:l3 + 6] = (po - l3 - 40 + len(pay)).to_bytes(2, "big")
        pd = head.pdst if l3 + 24 <= head.pdst <= l4 - 16 else l3 + 24
        pseudo = bytes(h[l3 + 8:l3 + 24]) + bytes(h[pd:pd + 16]) + \
            (po - l4 + len(pay)).to_bytes(4, "big") + b"\0\0\0\x06"
    else:
        h[l3 + 2:l3 + 4] = (po - l3 + len(pay)).to_bytes(2, "big")
        h[l3 + 10:l3 + 12] = b"\0\0"
        h[l3 + 10:l3 + 12] = sm.csum_field(h[l3:l4]).to_bytes(2, "big")
        pseudo = bytes(h[l3 + 12:l3 + 20]) + b"\0\x06" + (po - l4 + len(pay)).to_bytes(2, "big")
    h[l4 + 13] |= last.f[l4 + 13] & (sm.FIN | sm.PSH)
    h[l4 + 16:l4 + 18] = b"\0\0"
    h[l4 + 16:l4 + 18] = sm.csum_field(pseudo, h[l4:po], pay).to_bytes(2, "big")
    return bytes(h) + pay


def positions(hb, recs, order=None, trust_sums=False):
    frames = sm.frames_of(hb)
    et = dispatch_ethertype(recs)
    pd = ip6_block(recs)["ip6_pdst_off"]
    idx = range(hb.n) if order is None else [int(x) for x in order]
    return [Pos(frames[k], recs[k], int(et[k]), int(pd[k]), trust_sums) if k < hb.n else Pos()
            for k in idx]


def coalesce(hb, recs, order=None, max_payload=65535, trust_sums=False):
    """(out_frames, src_first, totals, out_mss): the output frames as byte strings in order,
    src_first (u32, n + 1), totals (u64: n_out, out_bytes_needed) and out_mss (u16, n)."""
    P = positions(hb, recs, order, trust_sums)
    n = len(P)
    B = [i > 0 and base(P[i - 1], P[i]) for i in range(n)]
    short = [B[i] and P[i].p < P[i - 1].p for i in range(n)]
    link = [B[i] and P[i].p <= P[i - 1].p and not short[i - 1] for i in range(n)]
    groups, held = [], 0                        # held: the current group's payload
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


def flow_order_host(hb, n_buckets=4096):
    """engine.flow_order over the oracle's flow events of hb (CPU tensors)."""
    import torch
    from oracle import oracle
    from rpkt_amd import engine
    _, ev = oracle.parse_batch(hb.frames, hb.n, F_ALL, offsets=hb.offsets, stride=hb.stride,
                               frame_len=hb.frame_len, n_buckets=n_buckets, flow_ev=True)
    return engine.flow_order(torch.from_numpy(ev.view(np.int64).copy())).numpy().view(np.uint32)
