"""Reference model of rpkt_gpu_parse_tunnel_chains, composed from the two committed oracles
(pure Python + numpy over oracle.parse_chains; no new C):

  outer  = oracle.parse_chains on the chains;
  tun    = oracle/rpkt_oracle_tunnel.c's vxlan / gtpu / gtp_ext / gre restated over a Pbuf
           view (s, e): header sizes against chunk_len(s, e) -- the rest of the first segment
           whose end passes s, cut at e (pbuf.rs:49-104) -- totals against remaining() = e - s;
  inner  = oracle.parse_chains on the derived sub-chain: the pieces of the chain's segments
           that intersect [is, ie), empty ones dropped; an inner packet that starts at its
           IP header gets a leading 14-byte segment (12 zero bytes + inner_type), and 14 is
           taken off frame_len and the offsets again.  The offsets the record reached are
           moved by `is` (oracle_tunnel_one, rpkt_oracle_tunnel.c:236-252).

tests/test_tunnel_chain_model.py pins this to oracle.tunnel_batch."""
import numpy as np

from oracle import oracle
from rpkt_amd import gen
from rpkt_amd.records import (F_IPV6, MAX_GTP_EXT, REC_DTYPE, STATUS, TUN_DTYPE, TUN_KIND,
                              TUN_STATUS, is_ip6)


class Pbuf:
    """One chain as the ABI reads it (include/rpkt_gpu.h, rpkt_chains_t: indices and
    segments clamped), with its bytes concatenated."""

    def __init__(self, buf, segs, chain_first, p):
        n_segs, fb = len(segs), len(buf)
        a = min(int(chain_first[p]), n_segs)
        b = min(max(int(chain_first[p + 1]), a), n_segs)
        self.pieces = []                      # (absolute offset, length)
        for off, ln in segs[a:b].tolist():
            off = min(off, fb)
            self.pieces.append((off, min(ln, fb - off)))
        self.flat = b"".join(buf[o:o + l].tobytes() for o, l in self.pieces)

    def chunk_len(self, s, e):
        """chunk().len() of the view [s, e): the rest of the first segment whose end passes
        s (empty segments skipped, as advance_common walks), cut at e."""
        if s >= e:
            return 0
        cum = 0
        for _, ln in self.pieces:
            if cum + ln > s:
                return min(cum + ln, e) - s
            cum += ln
        return 0

    def sub(self, s, e):
        """The pieces of the segments that intersect [s, e), empty ones dropped."""
        out, cum = [], 0
        for off, ln in self.pieces:
            lo, hi = max(cum, s), min(cum + ln, e)
            if hi > lo:
                out.append((off + lo - cum, hi - lo))
            cum += ln
        return out


def _be16(b, k):
    return (b[k] << 8) | b[k + 1]


def _be32(b, k):
    return (b[k] << 24) | (b[k + 1] << 16) | (b[k + 2] << 8) | b[k + 3]


def _inner_by_type(t, typ, s, e, flags):
    t["inner_off"], t["inner_type"] = s & 0xffff, typ
    if typ == 0x6558:
        start = 0
    elif typ == 0x0800 or (typ == 0x86dd and flags & F_IPV6):
        start = typ
    else:
        t["status"] = TUN_STATUS["INNER_UNKNOWN"]
        return None
    t["status"] = TUN_STATUS["OK"]
    return (s, e, start)


def _vxlan(pb, s, e, flags, t):
    if pb.chunk_len(s, e) < 8:                        # Vxlan::parse vxlan/generated.rs:32-39
        return None
    p = pb.flat[s:s + 8]
    t["hdr0"], t["hdr1"], t["aux"] = p[0], p[1], _be16(p, 2)
    t["id"] = (p[4] << 16) | (p[5] << 8) | p[6]
    return _inner_by_type(t, 0x6558, s + 8, e, flags)


def _gtp_ext(pb, s, e, typ):
    """(header_len, next type) of one extension header at view [s, e), or None: each parse
    tests its own chunk (gtpv1/generated.rs:336-341, :461-466, :587-592, :747-752, :880-892,
    NrUp::group_parse :2308-2320, PduSessionUp::group_parse :1507-1518)."""
    cl = pb.chunk_len(s, e)
    p = pb.flat[s:s + cl]
    if typ in (0x40, 0xc0, 0x20):
        if cl < 4:
            return None
        hl = 4
    elif typ in (0x03, 0x82):
        if cl < 8:
            return None
        hl = 8
    elif typ in (0x81, 0x83):
        if cl < 1:
            return None
        hl = p[0] * 4
        if hl < 1 or hl > cl:
            return None
    elif typ == 0x84:
        if cl < 2:
            return None
        mn = {0: 6, 1: 7, 2: 3}.get(p[1] >> 4)
        if mn is None or cl < mn:
            return None
        hl = p[0] * 4
        if hl < mn or hl > cl:
            return None
    elif typ == 0x85:
        if cl < 2 or (p[1] >> 4) > 1 or cl < 3:
            return None
        hl = p[0] * 4
        if hl < 3 or hl > cl:
            return None
    else:
        return None
    return hl, p[hl - 1]


def _gtpu(pb, s, e, flags, t):
    # Gtpv1::parse gtpv1/generated.rs:33-49: chunk >= 8, header_len <= chunk, header_len <=
    # packet_len <= remaining
    cl = pb.chunk_len(s, e)
    if cl < 8:
        return None
    p = pb.flat[s:s + min(cl, 12)]
    hl = 8 if (p[0] & 7) == 0 else 12
    plen = _be16(p, 2) + 8
    if hl > cl or plen < hl or plen > e - s:
        return None
    t["hdr0"], t["hdr1"], t["id"] = p[0], p[1], _be32(p, 4)
    t["aux"] = _be16(p, 8) if hl == 12 else 0
    x, xe = s + hl, s + plen                          # payload(): trim, advance :98-108
    if (p[0] >> 5) != 1 or p[1] != 255:
        t["status"], t["inner_off"] = TUN_STATUS["NOT_TPDU"], x & 0xffff
        return None
    nxt = p[11] if (p[0] & 4) else 0
    k = 0
    while nxt != 0:
        r = _gtp_ext(pb, x, xe, nxt) if k < MAX_GTP_EXT else None
        if r is None:
            t["status"], t["inner_off"] = TUN_STATUS["EXT_BAD"], x & 0xffff
            return None
        x += r[0]
        nxt = r[1]
        k += 1
    ver = pb.flat[x] >> 4 if pb.chunk_len(x, xe) else 0
    return _inner_by_type(t, 0x0800 if ver == 4 else (0x86dd if ver == 6 else 0), x, xe, flags)


def _gre(pb, s, e, flags, t):
    # GreGroup::group_parse gre/generated.rs:800-820: chunk >= 4
    cl = pb.chunk_len(s, e)
    if cl < 4:
        return None
    p = pb.flat[s:s + min(cl, 16)]
    c, r, k, ver = p[0] >> 7, (p[0] >> 6) & 1, (p[0] >> 5) & 1, p[1] & 7
    pt = _be16(p, 2)
    if c == 0 and r == 0 and k == 1 and ver == 1 and pt == 0x880b:
        # GreForPPTP::parse :371-386: chunk >= 8, header_len <= chunk, payload_len +
        # header_len <= remaining
        if cl < 8:
            return None
        ind = _be16(p, 0)
        hl = 8 + (4 if ind & 0x1000 else 0) + (4 if ind & 0x0080 else 0)
        if hl > cl or _be16(p, 4) + hl > e - s:
            return None
        t["hdr0"], t["hdr1"], t["id"] = p[0], p[1], _be32(p, 4)
        t["status"] = TUN_STATUS["INNER_UNKNOWN"]
        t["inner_off"], t["inner_type"] = (s + hl) & 0xffff, pt
        return None
    if ver != 0:
        return None
    hl = 4 + (4 if (c | r) else 0) + (4 if k else 0) + (4 if (p[0] >> 4) & 1 else 0)
    if hl > cl:                                       # Gre::parse :33-44: header_len in [4, chunk]
        return None
    t["hdr0"], t["hdr1"] = p[0], p[1]
    t["aux"] = _be16(p, 4) if (c | r) else 0
    t["id"] = _be32(p, 8 if (c | r) else 4) if k else 0
    return _inner_by_type(t, pt, s + hl, e, flags)


def decode(pb, o, v6, flags):
    """(rpkt_tun_t fields, inner view (is, ie, start) or None) of one chain from its outer
    record o, as oracle_tunnel_one takes the dispatch and the view bounds."""
    t = dict(kind=0, status=TUN_STATUS["NONE"], tun_off=0, inner_off=0, inner_type=0, id=0,
             hdr0=0, hdr1=0, aux=0)
    proto, view = int(o["ip_protocol"]), None
    if o["status"] == STATUS["OK"] and proto == 17:
        dp, sp = int(o["dst_port"]), int(o["src_port"])
        port = dp if dp in (4789, 2152) else (sp if sp in (4789, 2152) else 0)
        if port:
            s = int(o["payload_off"])
            e = s + int(o["payload_len"])
            t["kind"] = TUN_KIND["VXLAN"] if port == 4789 else TUN_KIND["GTPU"]
            t["status"], t["tun_off"] = TUN_STATUS["BAD"], s
            view = (_vxlan if port == 4789 else _gtpu)(pb, s, e, flags, t)
    elif o["status"] == STATUS["L4_OTHER"] and proto == 47 and (v6 or (int(o["ip_frag"]) & 0x1fff) == 0):
        s = int(o["l4_off"])
        e = s + int(o["payload_len"])
        t["kind"], t["status"], t["tun_off"] = TUN_KIND["GRE"], TUN_STATUS["BAD"], s
        view = _gre(pb, s, e, flags, t)
    return t, view


def tunnel_chains(buf, segs, chain_first, flags=3):
    """(outer records, rpkt_tun_t, inner records) of rpkt_gpu_parse_tunnel_chains."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    segs = np.ascontiguousarray(segs, dtype=np.uint32).reshape(-1, 2)
    chain_first = np.ascontiguousarray(chain_first, dtype=np.uint32)
    n = chain_first.size - 1
    outer = oracle.parse_chains(buf, segs, chain_first, flags & ~4)
    v6 = is_ip6(outer)
    ip6_proto = np.ascontiguousarray(outer).view(np.uint8).reshape(-1, 80)[:, 33]
    tun = np.zeros(n, dtype=TUN_DTYPE)
    sub_segs, sub_first, views = [], [0], []
    extra = bytearray()                               # the 14-byte segments of IP-start inners
    for p in range(n):
        pb = Pbuf(buf, segs, chain_first, p)
        o = {k: outer[p][k] for k in ("status", "dst_port", "src_port", "payload_off",
                                      "payload_len", "l4_off", "ip_frag")}
        o["ip_protocol"] = ip6_proto[p]               # byte 33, IPv4 and IPv6
        t, view = decode(pb, o, bool(v6[p]), flags)
        for k, x in t.items():
            tun[p][k] = x
        if view is not None:
            s, e, start = view
            if start:
                sub_segs.append((buf.size + len(extra), 14))
                extra += bytes(12) + bytes([start >> 8, start & 0xff])
            sub_segs.extend(pb.sub(s, e))
        views.append(view)
        sub_first.append(len(sub_segs))
    arena = np.concatenate([buf, np.frombuffer(bytes(extra), dtype=np.uint8)])
    inner = oracle.parse_chains(arena, np.array(sub_segs, dtype=np.uint32).reshape(-1, 2),
                                np.array(sub_first, dtype=np.uint32), flags & ~4)
    none = np.array([v is None for v in views])
    inner[none] = np.zeros((), dtype=REC_DTYPE)
    inner["status"][none] = STATUS["NO_INNER"]
    # an IP-start inner: take the 14 bytes off again; then the offsets the record reached
    # move by `is` (rpkt_oracle_tunnel.c:236-252)
    base = np.array([0 if v is None else v[0] - (14 if v[2] else 0) for v in views], dtype=np.int64)
    ipstart = np.array([v is not None and v[2] != 0 for v in views])
    inner["frame_len"][ipstart] -= 14
    st, i6 = inner["status"], is_ip6(inner)
    l3_set = ~none & ~np.isin(st, [STATUS["ETH_SHORT"], STATUS["VLAN_SHORT"], STATUS["NOT_IPV4"]])
    l4_set = l3_set & np.where(i6, ~np.isin(st, [STATUS["IP6_SHORT"], STATUS["IP6_BAD_LEN"]]),
                               ~((st >= STATUS["IP_SHORT"]) & (st <= STATUS["IP_TOT_GT_LEN"])))
    mv = lambda x, m: np.where(m, (x.astype(np.int64) + base) & 0xffff, x).astype(np.uint16)
    inner["l3_off"] = mv(inner["l3_off"], l3_set)
    inner["l4_off"] = mv(inner["l4_off"], l4_set)
    inner["payload_off"] = mv(inner["payload_off"], l4_set)
    pd = inner.view(np.uint8).reshape(-1, 80)[:, 34:36]          # ip6_pdst_off
    pdv = pd[:, 0].astype(np.int64) | (pd[:, 1].astype(np.int64) << 8)
    pdn = mv(pdv, l4_set & i6)
    pd[:, 0], pd[:, 1] = pdn & 0xff, pdn >> 8
    return outer, tun, inner


def flow_events(outer, tun, inner, n_buckets):
    return oracle.tunnel_flow_events(outer, tun, inner, n_buckets)


def lay_out(frames, seg_lens, gap=3, lead=1):
    """Frames as chains in one arena: frame k cut into seg_lens[k] (zeros make empty
    segments), the segments `gap` bytes apart from offset `lead`.  Returns a gen.HostChains."""
    segs, first, parts, pos = [], [0], [], lead
    parts.append(bytes(lead))
    for f, lens in zip(frames, seg_lens):
        assert sum(lens) == len(f), (sum(lens), len(f))
        c = 0
        for ln in lens:
            segs.append((pos, ln))
            parts.append(f[c:c + ln] + bytes(gap))
            pos += ln + gap
            c += ln
        first.append(len(segs))
    buf = np.frombuffer(b"".join(parts) + bytes(64), dtype=np.uint8).copy()
    return gen.HostChains(None, len(frames), None, buf,
                          np.array(segs, dtype=np.uint32).reshape(-1, 2),
                          np.array(first, dtype=np.uint32),
                          np.array([len(f) for f in frames], dtype=np.uint32))


def cut_at(length, cuts):
    """Segment lengths of a frame of `length` bytes cut at the sorted positions `cuts`
    (repeated positions give empty segments)."""
    edges = [0] + sorted(min(max(int(c), 0), length) for c in cuts) + [length]
    return [edges[k + 1] - edges[k] for k in range(len(edges) - 1)]
