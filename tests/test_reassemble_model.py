"""tests/reassemble_model.py, the model the GPU test of rpkt_gpu_reassemble_batch compares
against, checked without a GPU: known answers written out as bytes, the round trip
reassemble(fragment(F)) over the hand-built frames of tests/fragment_model.py at every mtu, each
reason two neighbouring fragments do not link, and the oracle's parse of the model's output."""
import numpy as np
import pytest

from rpkt_amd.records import STATUS, dispatch_ethertype

import fragment_model as fm
import reassemble_model as rm
import segment_model as sm

ETH = "020000000001020000000002"
SRC6 = "202122232425262728292a2b2c2d2e2f"
DST6 = "404142434445464748494a4b4c4d4e4f"


def run(frames, order=None, trust_sums=False):
    hb = sm.pack(frames)
    return rm.reassemble(hb, sm.oracle_records(hb), order, trust_sums)


def out_of(frames, **kw):
    return run(frames, **kw)[0]


def hexes(*parts):
    return bytes.fromhex("".join(parts))


# ---- known answers ---------------------------------------------------------------------------

# Ether / IPv4 ihl 7 (LSRR, EOL), tos 0x10, ident 0xbeef, UDP's protocol / 16 + 8 payload bytes
V4_OPTS = "8307040102030400"
V4_A = hexes(ETH, "0800", "4710002cbeef2000" "40111b4e" "c0a8380b" "c0a8380c", V4_OPTS,
             "303132333435363738393a3b3c3d3e3f")
V4_B = hexes(ETH, "0800", "47100024beef0002" "40113b54" "c0a8380b" "c0a8380c", V4_OPTS,
             "4041424344454647")
V4_WHOLE = hexes(ETH, "0800", "47100034beef0000" "40113b46" "c0a8380b" "c0a8380c", V4_OPTS,
                 "303132333435363738393a3b3c3d3e3f4041424344454647")

# Ether / one tag / IPv6 / Hop-by-Hop / Fragment (ident 0x01020304) / 8 + 8 + 4 payload bytes
V6_HBH = "00010400000000"


def v6_frag(plen, off_m, pay):
    return hexes(ETH, "81006007" "86dd", "60000000", plen, "0040", SRC6, DST6, "2c", V6_HBH,
                 "1100", off_m, "01020304", pay)


V6_A = v6_frag("0018", "0001", "5051525354555657")
V6_B = v6_frag("0018", "0009", "58595a5b5c5d5e5f")
V6_C = v6_frag("0014", "0010", "60616263")
V6_WHOLE = hexes(ETH, "81006007" "86dd", "60000000" "001c" "0040", SRC6, DST6, "11", V6_HBH,
                 "505152535455565758595a5b5c5d5e5f60616263")
V6_TAIL = v6_frag("001c", "0008", "58595a5b5c5d5e5f60616263")       # B + C: offset 8, M clear
V6_HEAD = v6_frag("0020", "0001", "505152535455565758595a5b5c5d5e5f")   # A + B: offset 0, M set


def test_known_answer_ip4_pair_with_options():
    out, first, totals = run([V4_A, V4_B])
    assert out == [V4_WHOLE]
    assert first.tolist() == [0, 2, 2] and totals.tolist() == [1, len(V4_WHOLE)]
    # the same bytes are what fragmentation cuts into the pair
    hb, _ = rm.fragmented([V4_WHOLE], 44)
    assert sm.frames_of(hb) == [V4_A, V4_B]


def test_known_answer_ip6_complete_merge():
    out, first, totals = run([V6_A, V6_B, V6_C])
    assert out == [V6_WHOLE]
    assert first.tolist() == [0, 3, 3, 3] and totals.tolist() == [1, len(V6_WHOLE)]
    hb, _ = rm.fragmented([V6_WHOLE], 64, ip6_ident=0x01020304)
    assert sm.frames_of(hb) == [V6_A, V6_B, V6_C]


def test_known_answer_ip6_partial_merges_and_their_composition():
    assert out_of([V6_B, V6_C]) == [V6_TAIL]
    assert out_of([V6_A, V6_B]) == [V6_HEAD]
    # a partial merge is a valid, larger fragment: a second call finishes the merge
    assert out_of([V6_A, V6_TAIL]) == [V6_WHOLE] and out_of([V6_HEAD, V6_C]) == [V6_WHOLE]
    # two datagrams' runs and a frame between them, in position order
    other = fm.udp4(30)
    out, first, totals = run([V6_B, V6_C, other, V4_A, V4_B, b""])
    assert out == [V6_TAIL, other, V4_WHOLE, b""]
    assert first.tolist() == [0, 2, 3, 5, 6, 6, 6]
    assert totals.tolist() == [4, len(V6_TAIL) + len(other) + len(V4_WHOLE)]


def test_order_and_empty_positions():
    out, first, totals = run([V4_B, V6_C, V4_A, V6_A, V6_B], order=[2, 0, 9, 3, 4, 1, 2])
    assert out == [V4_WHOLE, b"", V6_WHOLE, V4_A]
    assert first.tolist() == [0, 2, 3, 6, 7, 7, 7, 7]


# ---- the round trip --------------------------------------------------------------------------

def round_trip(frames, mtu, ignore_df, again=None):
    """(out, exact, cut): the reassembled fragments of `frames` at mtu (fragmented once more at
    `again`), which frames the inverse property covers, which were cut."""
    hb0 = sm.pack(frames)
    r0 = sm.oracle_records(hb0)
    det = dispatch_ethertype(r0)
    hb, first = rm.fragmented(frames, mtu, ignore_df, 0xfffffffe)
    cut = np.diff(first.astype(np.int64)) > 1
    if again:
        hb, _ = rm.fragmented(sm.frames_of(hb), again, ignore_df, 7)
    out, _, totals = rm.reassemble(hb, sm.oracle_records(hb))
    exact = []
    for f, r, d in zip(frames, r0, det):
        l3 = int(r["l3_off"])
        if d == 0x0800 and int(r["status"]) in fm.IP4_STATUSES:
            ends = l3 + int.from_bytes(f[l3 + 2:l3 + 4], "big") == len(f)
            exact.append(ends and not f[l3 + 6] & 0xc0)
        elif d == 0x86DD and int(r["status"]) in fm.IP6_STATUSES:
            exact.append(l3 + 40 + int.from_bytes(f[l3 + 4:l3 + 6], "big") == len(f))
        else:
            exact.append(True)                                     # never cut: a copy of a copy
    stripped = [rm.strip(f, r, int(d)) for f, r, d in zip(frames, r0, det)]
    return out, exact, cut, stripped


@pytest.mark.parametrize("ignore_df", [False, True])
@pytest.mark.parametrize("mtu", fm.MTU_VALUES)
def test_round_trip_over_the_hand_built_frames(mtu, ignore_df):
    frames = list(fm.hand_frames(mtu))
    out, exact, cut, stripped = round_trip(frames, mtu, ignore_df)
    assert len(out) == len(frames) == 45
    assert (cut.sum() > 0) == (mtu < 65535)
    for i, f in enumerate(frames):
        if exact[i] or not cut[i]:
            assert out[i] == f, i
        else:
            assert out[i] == stripped[i] != f, i
    # the only frames outside the property: the padded ones, the DF ones, the reserved bit
    assert set(np.nonzero(~np.array(exact))[0].tolist()) == {18, 19, 22, 23, 28, 33}


def test_twice_fragmented_ip4_comes_back_whole_in_one_call():
    frames = list(fm.hand_frames(300))
    out, exact, cut, stripped = round_trip(frames, 300, True, again=100)
    assert len(out) == 45
    det = dispatch_ethertype(sm.oracle_records(sm.pack(frames)))
    v4 = [i for i in range(45) if det[i] == 0x0800 and cut[i]]
    assert len(v4) >= 15
    for i in v4:
        assert out[i] == (frames[i] if exact[i] else stripped[i]), i
    # an IPv6 fragment is never cut again, so the IPv6 frames come back from their one cut
    for i in range(45):
        if det[i] == 0x86DD and exact[i]:
            assert out[i] == frames[i], i


# ---- each reason not to link -------------------------------------------------------------------

def frag4(off8, n, more=True, ident=0x77, proto=17, salt=0, **kw):
    """An IPv4 fragment at offset off8 * 8 carrying n bytes."""
    return fm.ip4(fm.payload_bytes(n, salt), proto, frag=off8 | (fm.MF if more else 0), ident=ident, **kw)


def frag6(off, n, more=True, ident=9, exts=(), salt=0, **kw):
    e = tuple(exts) + (fm.fragment_header(17, off, int(more), ident),)
    return fm.ip6(fm.payload_bytes(n, salt), 17, e, **kw)


def lone(frames, **kw):
    """True when nothing merges."""
    out = out_of(frames, **kw)
    return out == list(frames)


def test_links_and_each_non_link_reason_ip4():
    a, b = frag4(0, 16), frag4(2, 9, more=False)
    assert len(out_of([a, b])) == 1
    assert lone([a, frag4(3, 9, more=False)])                                   # a gap
    assert lone([a, frag4(1, 9, more=False)])                                   # an overlap
    assert lone([a, a]) and lone([b, a])                                        # a duplicate; out of order
    assert lone([frag4(2, 16, more=False), frag4(4, 8)])                        # the predecessor has no MF
    assert lone([frag4(0, 12), frag4(1, 8)]) and lone([frag4(0, 12), frag4(2, 8)])   # its P % 8 != 0
    assert lone([a, frag4(2, 9, more=False, ident=0x78)])                       # ident
    assert lone([a, frag4(2, 9, more=False, proto=1)])                          # protocol
    c = bytearray(b)
    c[14 + 19] ^= 1                                                             # destination address
    c[14 + 10:14 + 12] = b"\0\0"
    c[14 + 10:14 + 12] = sm.csum_field(c[14:34]).to_bytes(2, "big")
    assert lone([a, bytes(c)])
    assert lone([a, frag4(2, 9, more=False, tags=1)])                           # l3_off
    assert lone([a, frag4(2, 9, more=False, options=fm.OPTIONS_MIX[:4])])       # l4_off
    c = bytearray(frag4(2, 9, more=False, tags=1))
    c[14:16] = b"\x81\x01"
    assert lone([frag4(0, 16, tags=1), bytes(c)])                               # a byte before l3
    # TOS, TTL, options of equal length, DF and the reserved bit are not compared
    d = frag4(2, 9, more=False, tos=4)
    assert len(out_of([a, d])) == 1
    d = fm.ip4(fm.payload_bytes(9), 17, frag=2 | 0xc000, ident=0x77)
    got = out_of([a, d])
    assert len(got) == 1 and got[0][20:22] == b"\0\0"                           # the head's frag word
    # a bad header sum: not eligible, unless the sums are trusted
    c = bytearray(b)
    c[14 + 10] ^= 0x40
    assert lone([a, bytes(c)]) and len(out_of([a, bytes(c)], trust_sums=True)) == 1
    # an unfragmented packet is never eligible
    assert lone([fm.udp4(16), fm.udp4(16)])
    # a truncated frame: l3 + L > frame_len
    assert lone([a, b[:-1]]) and lone([a[:-1], b])


def test_the_65535_bound():
    """ihl + off + P <= 65535: a fragment whose end would overflow packet_len is not eligible,
    whatever precedes it; one that ends exactly there is."""
    off8 = (65535 - 20 - 15) // 8                                  # 8187: off 65496, room for 19
    a = frag4(off8 - 2, 16)
    assert len(out_of([a, frag4(off8, 19, more=False)])) == 1
    assert lone([a, frag4(off8, 20, more=False)])
    assert lone([frag4(off8, 24), frag4(off8 + 3, 8, more=False)])  # the head itself is too long
    x = 65535 - 8 - 8                                              # IPv6: 8 + off + P <= 65535
    off = x & ~7
    a6 = frag6(off - 16, 16)
    fits = frag6(off, 65535 - 8 - off, more=False)
    assert len(out_of([a6, fits])) == 1
    assert lone([a6, frag6(off, 65535 - 8 - off + 1, more=False)])


def test_links_and_each_non_link_reason_ip6():
    a, b = frag6(0, 16), frag6(16, 5, more=False)
    assert len(out_of([a, b])) == 1
    assert lone([a, frag6(24, 5, more=False)]) and lone([a, frag6(8, 5, more=False)])   # gap, overlap
    assert lone([a, a]) and lone([frag6(16, 8, more=False), frag6(24, 8)])      # duplicate; no M
    assert lone([frag6(0, 12), frag6(8, 8)])                                    # P % 8 != 0
    assert lone([a, frag6(16, 5, more=False, ident=10)])                        # identification
    assert lone([a, frag6(16, 5, more=False, tags=1)])                          # l3_off
    assert lone([a, frag6(16, 5, more=False, exts=(fm.HBH,))])                  # l4_off
    assert lone([frag6(0, 16, exts=(fm.HBH,)), frag6(16, 5, more=False, exts=(fm.ext(0, 8, 1),))])
    c = bytearray(b)
    c[14 + 7] = 63                                                              # hop limit
    assert lone([a, bytes(c)])
    c = bytearray(b)
    c[14 + 40 + 1] = 1                                                          # the reserved byte
    assert lone([a, bytes(c)])
    # an atomic fragment parses on and is never eligible
    atom = fm.udp6(24, (fm.fragment_header(17),))
    assert lone([atom, atom]) and lone([atom, frag6(16, 5, more=False, ident=7)])
    # an AH before the Fragment header is walked with its own length rule (4 * (2 + byte 1)):
    # 24 bytes here, where the other rule would say 40
    ah = frag6(0, 16, exts=(fm.HBH, fm.AUTH)), frag6(16, 5, more=False, exts=(fm.HBH, fm.AUTH))
    got = out_of(list(ah))
    assert len(got) == 1 and got[0] == fm.ip6(fm.payload_bytes(16) + fm.payload_bytes(5), 17,
                                             (fm.HBH, fm.AUTH))
    # a truncated frame
    assert lone([a, b[:-1]]) and lone([a[:-1], b])


def test_a_walk_longer_than_the_limit_is_not_eligible():
    exts = tuple(fm.ext(60, 8, k) for k in range(rm.MAX_IP6_EXT))
    a, b = frag6(0, 16, exts=exts[:-1]), frag6(16, 5, more=False, exts=exts[:-1])
    assert len(out_of([a, b])) == 1
    a, b = frag6(0, 16, exts=exts), frag6(16, 5, more=False, exts=exts)
    recs = sm.oracle_records(sm.pack([a, b]))
    assert (recs["status"] != STATUS["IP6_FRAGMENT"]).all() and lone([a, b])


# ---- the oracle's parse of the output; the keys ------------------------------------------------

def test_oracle_parse_of_the_output():
    frames = [fm.udp4(3000), fm.udp4(700, options=fm.OPTIONS_40, tags=2), fm.tcp4(900, tags=1),
              fm.icmp4(600), fm.udp6(3000), fm.udp6(1200, (fm.HBH, fm.RT0), tags=1),
              fm.udp6(800, fm.LONG_EXTS), fm.udp6(900, (fm.AUTH,))]
    hb, first = rm.fragmented(frames, 300, ip6_ident=5)
    assert hb.n > 4 * len(frames)
    out, src_first, totals = rm.reassemble(hb, sm.oracle_records(hb))
    assert out == frames and np.array_equal(src_first[:len(frames) + 1], first)
    blob, offs = sm.packed_output(out, len(out))
    recs = sm.oracle_records(sm.pack(out))
    assert np.isin(recs["status"], (STATUS["OK"], STATUS["L4_OTHER"])).all()     # L4_OTHER: ICMP
    v4 = dispatch_ethertype(recs) == 0x0800
    assert (recs["ip_sum"][v4] == 0xffff).all() and (recs["ip_frag"][v4] == 0).all()
    udp = recs["ip_protocol"] == 17
    assert udp.sum() == 6 and (recs["l4_sum"][udp] == 0xffff).all()   # a complete datagram verifies
    # a partial IPv4 merge: a valid header sum, still a fragment
    part, _, _ = rm.reassemble(sm.pack(sm.frames_of(hb)[:3]), sm.oracle_records(sm.pack(sm.frames_of(hb)[:3])))
    r = sm.oracle_records(sm.pack(part))
    assert len(part) == 1 and int(r["ip_sum"][0]) == 0xffff and int(r["ip_frag"][0]) == fm.MF


def test_keys_order_a_shuffled_burst():
    frames = [fm.udp4(900, ident=k) for k in range(5)] + [fm.udp6(700), fm.udp4(40), b"",
                                                          fm.ether(0, 0x0806) + bytes(28)]
    hb, first = rm.fragmented(frames, 300, ip6_ident=3)
    fr = sm.frames_of(hb)
    perm = np.random.RandomState(5).permutation(hb.n)
    hb = sm.pack([fr[k] for k in perm])
    recs = sm.oracle_records(hb)
    k = rm.keys(hb, recs)
    frag = (k >> np.uint64(63)) == 0
    assert frag.sum() == hb.n - 3 and len(np.unique(k >> np.uint64(32))) == 6 + 1
    assert (k[~frag] & np.uint64(0xffffffff)).tolist() == np.nonzero(~frag)[0].tolist()
    out, _, totals = rm.reassemble(hb, recs, rm.order_of(k))
    assert sorted(out) == sorted(frames) and int(totals[0]) == len(frames)
    assert out[-3:] == [f for f in (fr[k] for k in perm) if f in frames[-3:]]   # arrival order
    plain, _, _ = rm.reassemble(hb, recs)
    assert len(plain) > 2 * len(frames)


def test_engine_has_the_entries():
    import re
    from rpkt_amd import engine
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/rpkt_gpu.h").read()
    for name in ("rpkt_gpu_reassemble_batch", "rpkt_gpu_reassemble_workspace_bytes",
                 "rpkt_gpu_reassemble_keys"):
        assert re.search(r"\b%s\(" % name, hdr) and name in engine.EXPORTS
    assert engine.REASSEMBLE_TRUST_SUMS == 1 and callable(engine.reassemble_batch)
    assert callable(engine.reassemble_keys) and callable(engine.reassemble_order)
    import torch
    k = torch.tensor([(1 << 63) - (1 << 64), 5 << 32 | 2, 5 << 32, (1 << 63) + 1 - (1 << 64), 3 << 32],
                     dtype=torch.int64)
    assert engine.reassemble_order(k).tolist() == [4, 2, 1, 0, 3]
