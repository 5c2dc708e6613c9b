"""A plain model of rpkt_gpu_reassemble_batch and rpkt_gpu_reassemble_keys (include/rpkt_gpu.h,
"IPv4 / IPv6 reassembly"): host frames, oracle records and an optional order in, the output
frames, src_first and totals out, over tests/segment_model.py's pack, frames_of, oracle_records
and packed_output.  It restates both fragment rules, the link and the key in plain Python, with
the host copy of rpkt_flow_hash (engine.lib()) for the key; tests/test_reassemble_model.py
checks it against known answers written out as bytes, the round trip through
tests/fragment_model.py and the oracle's parse of its output."""
import numpy as np

from rpkt_amd.records import STATUS, dispatch_ethertype, ip6_block

import fragment_model as fm
import segment_model as sm

MAX_IP6_EXT = fm.MAX_IP6_EXT
MF = fm.MF


class Pos:
    """One position: its frame's bytes and, when it is an eligible fragment (`on`), where its
    headers are, the P payload bytes it carries at datagram offset `off`, MF / M (`more`) and
    what the key hashes (ident, proto)."""

    def __init__(self, f=b"", r=None, ethertype=0, trust=False):
        self.f, self.on, self.v6 = f, False, ethertype == 0x86DD
        if r is None:
            return
        l3, l4, status = int(r["l3_off"]), int(r["l4_off"]), int(r["status"])
        self.l3, self.l4 = l3, l4
        if ethertype == 0x0800 and status in fm.IP4_STATUSES:
            self.ip4(f, l3, l4, trust or int(r["ip_sum"]) == 0xffff)
        elif ethertype == 0x86DD and status == STATUS["IP6_FRAGMENT"]:
            self.ip6(f, l3, l4)

    def be(self, at, n=2):
        """The frame's bytes [at, at + n) as a big-endian number; past the frame they read 0."""
        return int.from_bytes((self.f[at:at + n] + bytes(n))[:n], "big")

    def ip4(self, f, l3, l4, sum_ok):
        ihl, L, fw = (self.be(l3, 1) & 0xf) * 4, self.be(l3 + 2), self.be(l3 + 6)
        if ihl < 20 or l4 != l3 + ihl or l3 + L > len(f) or L - ihl < 1 or not fw & 0x3fff:
            return
        P, off = L - ihl, (fw & 0x1fff) * 8
        if ihl + off + P > 65535 or not sum_ok:
            return
        self.P, self.off, self.more = P, off, bool(fw & MF)
        self.ident, self.proto = self.be(l3 + 4), f[l3 + 9]
        self.on = True

    def ip6(self, f, l3, l4):
        x = l4 - 8
        if x < l3 + 40:
            return
        nh, y, nhoff = self.be(l3 + 6, 1), l3 + 40, l3 + 6
        for _ in range(MAX_IP6_EXT):
            if y >= x:
                break
            if nh in (0, 43, 60):
                n = 8 * (1 + self.be(y + 1, 1))
            elif nh == 51:
                n = 4 * (2 + self.be(y + 1, 1))
            else:
                return
            if y + n > x:
                return
            nhoff, nh, y = y, self.be(y, 1), y + n
        if y != x or nh != 44:
            return
        E = l3 + 40 + self.be(l3 + 4)
        P = E - (x + 8)
        if E > len(f) or P < 1:
            return
        off = self.be(x + 2) & 0xfff8
        if (x - l3 - 40) + 8 + off + P > 65535:
            return
        self.P, self.off, self.more = P, off, bool(self.be(x + 2) & 1)
        self.x, self.nhoff, self.ident, self.proto = x, nhoff, self.be(x + 4, 4), 44
        self.on = True

    def compared(self):
        """The bytes B compares."""
        f, l3 = self.f, self.l3
        if not self.v6:
            return f[:l3], f[l3 + 4:l3 + 6], f[l3 + 9], f[l3 + 12:l3 + 20]
        h = bytearray(f[:self.x + 8])
        h[l3 + 4:l3 + 6] = h[self.x + 2:self.x + 4] = b"\0\0"
        return bytes(h)


def base(a, b):
    """B: position b continues position a."""
    if not (a.on and b.on) or a.v6 != b.v6 or (a.l3, a.l4) != (b.l3, b.l4):
        return False
    if not a.more or a.P % 8 or b.off != a.off + a.P:
        return False
    return a.compared() == b.compared()


def merge(group):
    """The merged frame of a run of two positions or more."""
    head, last = group[0], group[-1]
    l3, l4 = head.l3, head.l4
    pay = b"".join(m.f[l4:l4 + m.P] for m in group)
    if not head.v6:
        h = bytearray(head.f[:l4])
        h[l3 + 2:l3 + 4] = (l4 - l3 + len(pay)).to_bytes(2, "big")
        fw = (head.be(l3 + 6) & ~MF) | (MF if last.more else 0)
        h[l3 + 6:l3 + 8] = fw.to_bytes(2, "big")
        h[l3 + 10:l3 + 12] = b"\0\0"
        h[l3 + 10:l3 + 12] = sm.csum_field(h[l3:l4]).to_bytes(2, "big")
        return bytes(h) + pay
    x = head.x
    if head.off == 0 and not last.more:                            # complete: no Fragment header
        h = bytearray(head.f[:x])
        h[head.nhoff] = head.f[x]
        h[l3 + 4:l3 + 6] = (x - l3 - 40 + len(pay)).to_bytes(2, "big")
        return bytes(h) + pay
    h = bytearray(head.f[:x + 8])
    h[l3 + 4:l3 + 6] = (x - l3 - 40 + 8 + len(pay)).to_bytes(2, "big")
    h[x + 2:x + 4] = (head.off | last.more).to_bytes(2, "big")
    return bytes(h) + pay


def positions(hb, recs, order=None, trust_sums=False):
    frames = sm.frames_of(hb)
    et = dispatch_ethertype(recs)
    idx = range(hb.n) if order is None else [int(x) for x in order]
    return [Pos(frames[k], recs[k], int(et[k]), trust_sums) if k < hb.n else Pos() for k in idx]


def reassemble(hb, recs, order=None, trust_sums=False):
    """(out_frames, src_first, totals): the output frames as byte strings in order, src_first
    (u32, n + 1) and totals (u64: n_out, out_bytes_needed)."""
    P = positions(hb, recs, order, trust_sums)
    n = len(P)
    groups = []
    for i in range(n):
        if i > 0 and base(P[i - 1], P[i]):
            groups[-1].append(i)
        else:
            groups.append([i])
    out = [P[g[0]].f if len(g) == 1 else merge([P[k] for k in g]) for g in groups]
    first = np.full(n + 1, n, dtype=np.uint32)
    first[:len(groups)] = [g[0] for g in groups]
    return out, first, np.array([len(out), sum(len(o) for o in out)], dtype=np.uint64)


def keys(hb, recs, trust_sums=False):
    """rpkt_gpu_reassemble_keys' keys (u64, n)."""
    from rpkt_amd import engine
    h = engine.lib().rpkt_flow_hash
    v6 = ip6_block(recs)
    out = np.zeros(hb.n, dtype=np.uint64)
    for i, p in enumerate(positions(hb, recs, None, trust_sums)):
        if not p.on:
            out[i] = (1 << 63) | i
            continue
        src, dst = ((int(v6[i]["ip6_src_fold"]), int(v6[i]["ip6_dst_fold"])) if p.v6 else
                    (int(recs[i]["ip_src"]), int(recs[i]["ip_dst"])))
        out[i] = ((h(src, dst, p.ident & 0xffff, p.ident >> 16, p.proto) & 0x7fffffff) << 32) | p.off // 8
    return out


def order_of(k):
    """The order_dev a stable ascending sort of the keys gives (u32, n)."""
    return np.argsort(k, kind="stable").astype(np.uint32)


def fragmented(frames, mtu, ignore_df=False, ip6_ident=0, lead=0):
    """A packed HostBatch of fragment_model's fragments of `frames` at mtu, and the model's
    frag_first."""
    hb = sm.pack(frames)
    out, first, _ = fm.fragment(hb, sm.oracle_records(hb), mtu, ignore_df, ip6_ident)
    return sm.pack(out, lead), first


def strip(f, r, det):
    """Frame `f` (record r, dispatch ethertype det) as a round trip through fragmentation leaves
    it when it was cut: without the bytes after its IP packet and, IPv4, without DF and the
    reserved bit (the header checksum refilled)."""
    l3, l4 = int(r["l3_off"]), int(r["l4_off"])
    if det == 0x0800 and int(r["status"]) in fm.IP4_STATUSES:
        L = int.from_bytes(f[l3 + 2:l3 + 4], "big")
        h = bytearray(f[:l3 + L])
        h[l3 + 6] &= 0x3f
        h[l3 + 10:l3 + 12] = b"\0\0"
        h[l3 + 10:l3 + 12] = sm.csum_field(h[l3:l4]).to_bytes(2, "big")
        return bytes(h)
    if det == 0x86DD and int(r["status"]) in fm.IP6_STATUSES:
        return f[:l3 + 40 + int.from_bytes(f[l3 + 4:l3 + 6], "big")]
    return f
