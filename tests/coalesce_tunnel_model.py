"""A plain model of rpkt_gpu_coalesce_tunnel_batch (include/rpkt_gpu.h, "Coalescing of the
inner TCP / UDP of tunnels"): host frames, the oracle's three tunnel records and an optional
order in, the output frames, src_first, totals and out_mss out.  The inner frame is judged,
compared and merged by tests/udp_reframe_model.py with the inner record (its offsets are
positions in the outer frame already); the carrier rule and the outer headers of a merged
frame are tests/segment_tunnel_model.py's (is_cut at mss 0, outer_fixups).  This module adds
what is the tunnel entry's own: the length agreement, the outer sums, the outer bytes B(i)
ignores, the outer ident and zero-checksum rules and the tighter limit of the greedy cut."""
import copy

import numpy as np

from rpkt_amd.records import dispatch_ethertype, ip6_block

import segment_model as sm
import segment_tunnel_model as stm
import udp_reframe_model as um

NONE, VXLAN, GTPU, GRE = stm.NONE, stm.VXLAN, stm.GTPU, stm.GRE


def be(f, at, n=2):
    return int.from_bytes(f[at:at + n], "big")


class TPos:
    """One position.  `pos`: the udp_reframe_model.Pos that is compared and merged -- the frame
    under its outer record (no tunnel) or under its inner record (a decoded tunnel); `cmp`: the
    same over the frame with the outer bytes B(i) ignores zeroed.  An empty position, an
    undecoded tunnel and a decoded one that fails a carrier, length or outer sum condition are
    not eligible."""

    def __init__(self, f=b"", O=None, T=None, I=None, o_et=0, o_pdst=0, i_et=0, i_pdst=0,
                 trust=False, udp=False):
        self.f, self.tunnel, self.elig, self.p = f, False, False, 0
        self.pos = self.cmp = um.Pos()
        if O is None:
            return
        if T["kind"] == NONE:                               # the flat entry's position
            self.pos = self.cmp = um.Pos(f, O, o_et, o_pdst, trust, udp)
            self.elig, self.p = self.pos.elig, self.pos.p
            return
        self.tunnel = True
        if T["status"] != 0:                                # undecoded: a byte copy
            return
        pos = um.Pos(f, I, i_et, i_pdst, trust, udp)        # the inner rule, I's verdicts
        # the carrier: what rpkt_gpu_segment_tunnel_batch asks of a frame it cuts
        if not (pos.elig and stm.is_cut(f, O, T, I, o_et, i_et, 0, udp)):
            return
        self.kind, self.o_v6, self.o_pdst = int(T["kind"]), o_et == 0x86DD, o_pdst
        self.ol3, self.ol4 = int(O["l3_off"]), int(O["l4_off"])
        self.toff, self.ioff = int(T["tun_off"]), int(T["inner_off"])
        self.O, self.T = O, T
        ol3, ol4, toff, kind = self.ol3, self.ol4, self.toff, self.kind
        tot = pos.po + pos.p
        # every length field a merge rewrites says tot already
        if self.o_v6:
            agree = be(f, ol3 + 4) == tot - ol3 - 40
        else:
            agree = be(f, ol3 + 2) == tot - ol3
        if kind in (VXLAN, GTPU):
            agree = agree and be(f, ol4 + 4) == tot - ol4
        if kind == GTPU:
            agree = agree and be(f, toff + 2) == tot - toff - 8
        if not agree:
            return
        self.o_csum = kind != GRE and be(f, ol4 + 6) != 0   # the outer UDP checksum is filled
        if not trust:
            if not self.o_v6 and int(O["ip_sum"]) != 0xffff:
                return
            l4_ok = int(O["l4_sum"]) == 0xffff
            if kind == GRE:
                if f[toff] & 0x80 and not l4_ok:
                    return
            elif self.o_csum and not l4_ok:
                return
        self.pos, self.elig, self.p = pos, True, pos.p
        # the outer bytes B(i) ignores
        g = bytearray(f)
        holes = [(ol3 + 4, ol3 + 6)] if self.o_v6 else [(ol3 + 2, ol3 + 6), (ol3 + 10, ol3 + 12)]
        if kind != GRE:
            holes.append((ol4 + 4, ol4 + 8))
        if kind == GTPU:
            holes.append((toff + 2, toff + 4))
        if kind == GRE and f[toff] & 0x80:
            holes.append((toff + 4, toff + 6))
        for a, b in holes:
            g[a:b] = bytes(b - a)
        self.cmp = copy.copy(pos)
        self.cmp.f = bytes(g)

    def limit(self, max_payload):
        """The largest payload of a group this position heads."""
        h = self.pos
        lim = min(max_payload, 65535 - (h.po - h.l3 - (40 if h.v6 else 0)))
        if self.tunnel:
            lim = min(lim, 65535 - (h.po - self.ol3 - (40 if self.o_v6 else 0)))
        return lim


def base(a, b):
    """B: position b continues position a."""
    if not (a.elig and b.elig) or a.tunnel != b.tunnel:
        return False
    if not a.tunnel:
        return um.base(a.pos, b.pos)
    if (a.kind, a.o_v6, a.ol3, a.ol4, a.toff, a.ioff) != (b.kind, b.o_v6, b.ol3, b.ol4, b.toff, b.ioff):
        return False
    if a.o_csum != b.o_csum:                                # !uh->check ^ !uh2->check
        return False
    # the inner rule (IP version, protocol, offsets, seq, ident, flags) and the header bytes
    # [0, ipo) under both sets of ignored bytes
    if not um.base(a.cmp, b.cmp):
        return False
    return bool(b.o_v6 or b.f[b.ol3 + 6] & 0x40 or
                be(b.f, b.ol3 + 4) == (be(a.f, a.ol3 + 4) + 1) & 0xffff)


def merge(group):
    """The merged frame of a group of two positions or more."""
    head = group[0]
    inner = um.merge([m.pos for m in group])
    if not head.tunnel:
        return inner
    return stm.outer_fixups(inner, head.O, head.T, head.o_v6, head.o_pdst, be(head.f, head.ol3 + 4))


def positions(hb, outer, tun, inner, order=None, trust_sums=False, udp=False):
    frames = sm.frames_of(hb)
    o_et, i_et = dispatch_ethertype(outer), dispatch_ethertype(inner)
    o_pd, i_pd = ip6_block(outer)["ip6_pdst_off"], ip6_block(inner)["ip6_pdst_off"]
    idx = range(hb.n) if order is None else [int(x) for x in order]
    return [TPos(frames[k], outer[k], tun[k], inner[k], int(o_et[k]), int(o_pd[k]), int(i_et[k]),
                 int(i_pd[k]), trust_sums, udp) if k < hb.n else TPos() for k in idx]


def groups_of(P, max_payload):
    """short, link and the greedy cut: the flat rule over these positions."""
    n = len(P)
    B = [i > 0 and base(P[i - 1], P[i]) for i in range(n)]
    short = [B[i] and P[i].p < P[i - 1].p for i in range(n)]
    link = [B[i] and P[i].p <= P[i - 1].p and not short[i - 1] for i in range(n)]
    groups, held = [], 0
    for i in range(n):
        if link[i] and held + P[i].p <= P[groups[-1][0]].limit(max_payload):
            groups[-1].append(i)
            held += P[i].p
            continue
        groups.append([i])
        held = P[i].p
    return groups


def coalesce(hb, outer, tun, inner, order=None, max_payload=65535, trust_sums=False, udp=False):
    """(out_frames, src_first, totals, out_mss) as udp_reframe_model.coalesce returns them."""
    P = positions(hb, outer, tun, inner, order, trust_sums, udp)
    n = len(P)
    groups = groups_of(P, max_payload)
    out = [P[g[0]].f if len(g) == 1 else merge([P[k] for k in g]) for g in groups]
    first = np.full(n + 1, n, dtype=np.uint32)
    first[:len(groups)] = [g[0] for g in groups]
    mss = np.zeros(n, dtype=np.uint16)
    mss[:len(groups)] = [P[g[0]].p if len(g) > 1 else 0 for g in groups]
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64), mss


def merged_kinds(first, n_out, tun, order=None):
    """{kind: how many merged groups (two positions or more) a result heads with that kind}."""
    f = first.astype(np.int64)
    heads = [int(f[j]) for j in range(int(n_out)) if f[j + 1] - f[j] > 1]
    at = (lambda i: i) if order is None else (lambda i: int(order[i]))
    kinds = [int(tun["kind"][at(i)]) for i in heads]
    return {k: kinds.count(k) for k in (NONE, VXLAN, GTPU, GRE)}


def segment_then_records(frames, mss, udp=False):
    """The frames cut in the tunnel at mss (the model) as a packed HostBatch, with the oracle's
    three records of the segments: a receive burst for the entry."""
    hb = sm.pack(frames)
    O, T, I = stm.tunnel_records(hb)
    segs, first, _ = stm.segment(hb, O, T, I, mss, udp)
    hs = sm.pack(segs)
    return hs, stm.tunnel_records(hs), first
