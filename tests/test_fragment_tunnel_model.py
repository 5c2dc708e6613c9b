"""tests/fragment_tunnel_model.py against what does not depend on it: the oracle's tunnel parse
of its output (the tunnel decodes, the outer packet fits the mtu, every outer sum verifies, the
inner frag words are the expected ones), a reassembly of the inner fragments by
tests/reassemble_model.py, the flat model where there is no tunnel, and the counts of a run of
the rules on the generator's tunnel batches.  Every input tests/test_gpu_fragment_tunnel.py uses
is checked here."""
import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import gen
from rpkt_amd.records import STATUS, dispatch_ethertype

import fragment_model as fm
import fragment_tunnel_model as ftm
import reassemble_model as rm
import segment_model as sm
import tunnel_frames as tf

ETHER = bytes.fromhex("02000000000a02000000000b0800")


@pytest.fixture(scope="module")
def hand():
    """mtu -> (frames, hb, records)."""
    res = {}
    for mtu in ftm.MTU_VALUES:
        frames = ftm.hand_frames(mtu)
        hb = sm.pack(frames)
        res[mtu] = (frames, hb, ftm.tunnel_records(hb))
    return res


@pytest.fixture(scope="module")
def config13():
    hb = gen.make_batch(13, n=2048, seed=3)
    return hb, ftm.tunnel_records(hb)


@pytest.fixture(scope="module")
def config14():
    hb = gen.make_batch(14, n=4096, seed=3)
    return hb, ftm.tunnel_records(hb)


def groups(want, mask):
    """(i, [the outputs of frame i]) for the frames of `mask`."""
    out, first, _ = want
    return [(int(i), out[int(first[i]):int(first[i + 1])]) for i in np.nonzero(mask)[0]]


def check_inner_cuts(hb, recs, mtu, ignore_df, want):
    """Every inner-cut output through the oracle, and the inverse through the reassembly model;
    the number of inner-cut frames."""
    outer, tun, inner = recs
    frames = sm.frames_of(hb)
    mask = ftm.inner_cuts(hb, outer, tun, inner, mtu, ignore_df)
    o_et = dispatch_ethertype(outer)
    for i, outs in groups(want, mask):
        f, I = frames[i], inner[i]
        il3, il4 = int(I["l3_off"]), int(I["l4_off"])
        c = (mtu - (il3 - int(outer[i]["l3_off"])) - (il4 - il3)) & ~7
        fw = int.from_bytes(f[il3 + 6:il3 + 8], "big")
        L = int.from_bytes(f[il3 + 2:il3 + 4], "big")
        assert len(outs) == -(-(L - (il4 - il3)) // c) and c >= 8
        ob = sm.pack(outs)
        O2, T2, I2 = ftm.tunnel_records(ob)
        for k in range(len(outs)):
            what = "mtu %d frame %d fragment %d" % (mtu, i, k)
            assert T2[k]["status"] == 0 and T2[k]["kind"] == tun[i]["kind"], what
            assert len(outs[k]) - int(O2[k]["l3_off"]) <= mtu, what
            ok = (STATUS["OK"], STATUS["L4_OTHER"]) if tun[i]["kind"] == ftm.GRE else (STATUS["OK"],)
            assert int(O2[k]["status"]) in ok, what
            # a status says the headers parsed, not that the sums hold: each outer sum itself
            o, ol4, toff = outs[k], int(O2[k]["l4_off"]), int(T2[k]["tun_off"])
            assert o_et[i] == 0x86DD or int(O2[k]["ip_sum"]) == 0xffff, what
            if o_et[i] == 0x0800:
                assert int(O2[k]["ip_ident"]) == (int(outer[i]["ip_ident"]) + k) & 0xffff, what
            if tun[i]["kind"] != ftm.GRE:
                if f[ol4 + 6:ol4 + 8] == b"\0\0":                   # a zero checksum stays zero
                    assert o[ol4 + 6:ol4 + 8] == b"\0\0", what
                else:
                    assert o[ol4 + 6:ol4 + 8] != b"\0\0" and int(O2[k]["l4_sum"]) == 0xffff, what
                assert int.from_bytes(o[ol4 + 4:ol4 + 6], "big") == len(o) - ol4, what
            elif f[toff] & 0x80:                                    # GRE with C: RFC 1071 over [tun_off, end)
                assert int(O2[k]["l4_sum"]) == 0xffff and tf.rfc1071(o[toff:]) == 0, what
            assert int(I2[k]["ip_sum"]) == 0xffff, what
            if tun[i]["kind"] == ftm.GTPU:
                assert int.from_bytes(o[toff + 2:toff + 4], "big") == len(o) - toff - 8, what
            more = k < len(outs) - 1 or fw & fm.MF
            assert int(I2[k]["ip_frag"]) == ((fw & 0x1fff) + k * c // 8) | (fm.MF if more else 0), what
            assert int(I2[k]["l3_off"]) == il3 and int(I2[k]["l4_off"]) == il4, what
        # the inverse: the inner packets behind one Ethernet header reassemble to the original
        # inner packet (a DF packet cut under IGNORE_DF: but for DF and the header checksum,
        # which reassemble_model.strip takes out of the original)
        inner_frames = [ETHER + o[il3:] for o in outs]
        rb = sm.pack(inner_frames)
        got, _, _ = rm.reassemble(rb, sm.oracle_records(rb))
        orig = sm.pack([ETHER + f[il3:il3 + L]])
        r0 = sm.oracle_records(orig)
        want1 = rm.strip(sm.frames_of(orig)[0], r0[0], int(dispatch_ethertype(r0)[0]))
        if ftm.df_clear(f, I):
            assert want1 == ETHER + f[il3:il3 + L]
        assert got == [want1], "mtu %d frame %d: the inner fragments do not reassemble" % (mtu, i)
    return int(mask.sum())


@pytest.mark.parametrize("mtu", ftm.MTU_VALUES)
def test_hand_frames_inner_cuts_parse_and_reassemble(hand, mtu):
    frames, hb, recs = hand[mtu]
    for ignore_df in (False, True):
        for fallback in (False, True):
            want = ftm.fragment(hb, *recs, mtu, ignore_df, fallback, 0xfffffff0)
            assert sum(len(o) for o in want[0]) == int(want[2][1])
            n_cut = check_inner_cuts(hb, recs, mtu, ignore_df, want)
            assert n_cut > 0 or mtu in (24, 51, 65535)


def test_the_hand_frames_hold_what_the_issue_lists(hand):
    """The carriers, the inner headers and the frames that are not inner-cut are all there."""
    frames, hb, (outer, tun, inner) = hand[576]
    o_et, i_et = dispatch_ethertype(outer), dispatch_ethertype(inner)
    cut = ftm.inner_cuts(hb, outer, tun, inner, 576, False)
    cut_df = ftm.inner_cuts(hb, outer, tun, inner, 576, True)
    ihl = (inner["l4_off"].astype(int) - inner["l3_off"].astype(int))
    for kind in ftm.KIND_LIST:
        k = tun["kind"] == kind
        assert (cut & k & (o_et == 0x0800)).any() and (cut & k & (o_et == 0x86DD)).any(), kind
        assert {20, 36, 60} <= set(ihl[cut & k]), kind                 # ihl 5, OPTIONS_MIX, OPTIONS_40
    protos = set(int(p) for p in inner["ip_protocol"][cut])
    assert {1, 6, 17} <= protos
    assert (cut_df & ~cut).sum() == 2                                   # inner DF
    assert (outer["l3_off"][cut] > 14).any()                            # an outer tag
    l2 = inner["l3_off"].astype(int) - tun["inner_off"].astype(int)
    assert (l2[cut] == 18).any() and (l2[cut] == 14).any() and (l2[cut] == 0).any()
    fw = inner["ip_frag"].astype(int)
    assert (cut & (fw & 0x1fff != 0) & (fw & fm.MF != 0)).any()        # a middle fragment, cut again
    assert (~cut_df & (tun["kind"] != 0) & (fw == 0x1ff0)).any()       # the offset would overflow
    assert (~cut_df & (tun["kind"] != 0) & (i_et == 0x86DD)).sum() == 2
    assert (~cut_df & (tun["status"] != 0)).any()                      # RPKT_T_BAD
    gre_s = [i for i, f in enumerate(frames) if tun[i]["kind"] == ftm.GRE and
             f[int(tun[i]["tun_off"])] & 0x10]
    assert gre_s and not cut_df[gre_s].any()
    assert (tun["kind"] == 0).sum() >= 4                                # plain frames
    # a zero and a non-zero outer UDP checksum, GRE with and without C, among the cut ones
    udp_ck = [int.from_bytes(frames[i][int(outer[i]["l4_off"]) + 6:][:2], "big")
              for i in np.nonzero(cut & (tun["kind"] != ftm.GRE))[0]]
    assert 0 in udp_ck and any(udp_ck)
    gre_c = [frames[i][int(tun[i]["tun_off"])] & 0xa0 for i in np.nonzero(cut & (tun["kind"] == ftm.GRE))[0]]
    assert {0, 0x20, 0x80, 0xa0} <= set(gre_c)
    # GTP-U: 0..3 extension headers, with and without a sequence number
    g = np.nonzero(cut & (tun["kind"] == ftm.GTPU))[0]
    assert len(set(int(inner[i]["l3_off"]) - int(tun[i]["tun_off"]) for i in g)) >= 4
    # padding after the inner packet and after the outer one
    assert any(len(frames[i]) > int(outer[i]["l3_off"]) + int(outer[i]["ip_packet_len"])
               for i in np.nonzero(cut)[0] if o_et[i] == 0x0800)


def test_mtu_values_reach_every_boundary(hand):
    """For every tunnel kind a frame and an mtu with c == 8, with mtu' - ihl < 8, with mtu <=
    over, with a last fragment of 1 byte, with L == mtu' + 1 and with L == mtu'."""
    seen = {k: set() for k in ftm.KIND_LIST}
    for mtu in ftm.MTU_VALUES:
        frames, hb, (outer, tun, inner) = hand[mtu]
        cut = ftm.inner_cuts(hb, outer, tun, inner, mtu, True)
        i_et = dispatch_ethertype(inner)
        for i, f in enumerate(frames):
            kind = int(tun[i]["kind"])
            if kind == 0 or tun[i]["status"] != 0 or i_et[i] != 0x0800:
                continue
            il3, il4 = int(inner[i]["l3_off"]), int(inner[i]["l4_off"])
            over, ihl = il3 - int(outer[i]["l3_off"]), il4 - il3
            L = int.from_bytes(f[il3 + 2:il3 + 4], "big")
            m = mtu - over
            if mtu <= over:
                assert not cut[i]
                seen[kind].add("mtu <= over")
                continue
            if m - ihl < 8:
                assert not cut[i]
                seen[kind].add("mtu' - ihl < 8")
                continue
            c = (m - ihl) & ~7
            if L == m:
                assert not cut[i]
                seen[kind].add("L == mtu'")
            if cut[i]:
                if c == 8:
                    seen[kind].add("c == 8")
                if (L - ihl) % c == 1:
                    seen[kind].add("last fragment of 1 byte")
                if L == m + 1:
                    seen[kind].add("L == mtu' + 1")
    for kind in ftm.KIND_LIST:
        assert seen[kind] == {"c == 8", "mtu' - ihl < 8", "mtu <= over", "last fragment of 1 byte",
                              "L == mtu' + 1", "L == mtu'"}, (kind, seen[kind])
    assert {576, 1500, 65535} <= set(ftm.MTU_VALUES)


@pytest.mark.parametrize("mtu", [576, 120])
def test_config_13_counts(config13, mtu):
    hb, recs = config13
    mask = ftm.inner_cuts(hb, *recs, mtu, True)
    want = ftm.fragment(hb, *recs, mtu, True, False)
    kinds, outer_cuts = ftm.cut_kinds(want[1], recs[1], mask)
    assert min(kinds.values()) >= 100 and outer_cuts == 0, kinds
    assert kinds == {ftm.VXLAN: 596, ftm.GTPU: 611, ftm.GRE: 220}
    both = ftm.fragment(hb, *recs, mtu, True, True)
    assert ftm.cut_kinds(both[1], recs[1], mask) == (kinds, 621)
    # both generators set DF: without IGNORE_DF nothing is cut, inner or outer
    for fallback in (False, True):
        plain = ftm.fragment(hb, *recs, mtu, False, fallback)
        assert plain[0] == sm.frames_of(hb)
    if mtu == 576:
        assert check_inner_cuts(hb, recs, mtu, True, want) == 1427
        assert sum(int(d) for d in np.diff(want[1].astype(np.int64))[mask]) == 4281


def test_config_14_counts(config14):
    hb, recs = config14
    mask = ftm.inner_cuts(hb, *recs, 120, True)
    want = ftm.fragment(hb, *recs, 120, True, True)
    kinds, outer_cuts = ftm.cut_kinds(want[1], recs[1], mask)
    assert min(kinds.values()) >= 100, kinds
    assert kinds == {ftm.VXLAN: 723, ftm.GTPU: 537, ftm.GRE: 239} and outer_cuts == 1577
    assert ftm.fragment(hb, *recs, 120, False, True)[0] == sm.frames_of(hb)


@pytest.mark.parametrize("mtu", [120, 576])
def test_without_tunnels_the_model_is_the_flat_one(hand, config13, mtu):
    for hb, (outer, tun, inner) in (hand[mtu][1:], config13):
        none = tun.copy()
        none["kind"] = 0
        for ignore_df in (False, True):
            a = ftm.fragment(hb, outer, none, inner, mtu, ignore_df, False, 0xfffffff0)
            b = fm.fragment(hb, outer, mtu, ignore_df, 0xfffffff0)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_the_outer_rule_applies_only_with_the_flag(hand):
    """Rule 3: a tunnelled frame that is not inner-cut is a copy without the flag and the flat
    model's frames with it."""
    frames, hb, (outer, tun, inner) = hand[120]
    mask = ftm.inner_cuts(hb, outer, tun, inner, 120, False)
    a = ftm.fragment(hb, outer, tun, inner, 120, False, False)
    b = ftm.fragment(hb, outer, tun, inner, 120, False, True)
    flat = fm.fragment(hb, outer, 120, False)
    rest = ~mask & (tun["kind"] != 0)
    assert rest.sum() >= 8
    for (i, ga), (_, gb), (_, gf) in zip(groups(a, rest), groups(b, rest), groups(flat, rest)):
        assert ga == [frames[i]] and gb == gf
    assert any(len(g) > 1 for _, g in groups(b, rest))


def test_oracle_parse_of_a_whole_output(hand):
    """The packed output of the model parses slot by slot: spare slots are empty frames."""
    frames, hb, recs = hand[120]
    out, first, totals = ftm.fragment(hb, *recs, 120, True, True)
    blob, offs = sm.packed_output(out, int(totals[0]) + 3)
    O, T, I = oracle.tunnel_batch(blob, int(totals[0]) + 3, sm.F6, offsets=offs)
    assert (O["frame_len"][int(totals[0]):] == 0).all()
