"""tests/fragment_chains_model.py on the CPU: the model on single-segment chains is
tests/fragment_model.py, the flattening follows rpkt_chains_t's clamps, and every chain batch
of tests/test_gpu_fragment_chains.py reaches what it was built to reach: which chains the model
cuts, into how many fragments, through which header path.  A batch that stopped reaching its
case fails here instead of passing vacuously on the GPU."""
import numpy as np
import pytest

from rpkt_amd import gen
from rpkt_amd.records import dispatch_ethertype

import fragment_chains_model as fcm
import fragment_model as fm
import reassemble_model as rm
import segment_model as sm


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("mtu", [36, 68, 1500])
def test_single_segment_chains_give_the_flat_models_output(mtu):
    frames = fm.hand_frames(mtu)
    hb = sm.pack(frames)
    for hc in (fcm.chains_of(frames, [[] for _ in frames], lead=3), fcm.single_segment_chains(hb)):
        assert fcm.chain_bytes(hc) == list(frames)
        # one segment per chain: the chain parse sees what the flat parse sees
        recs = fcm.chain_records(hc)
        assert recs.tobytes() == sm.oracle_records(hb).tobytes()
        for ignore_df in (False, True):
            want = fm.fragment(hb, sm.oracle_records(hb), mtu, ignore_df, fcm.IDENT)
            assert same(fcm.fragment_chains(hc, recs, mtu, ignore_df, fcm.IDENT), want)
            assert int(want[2][0]) > hb.n


def test_clamps_of_out_of_range_descriptors():
    """The chains of the GPU test's descriptor case flatten under the documented clamps, and
    the model cuts the shared chain 5 under both kinds of records and chain 0, cut inside its
    IPv4 header, only under the flat ones."""
    hc, frames = fcm.descriptor_edge_chains()
    fb, segs = hc.buf.size, hc.segs
    got = fcm.chain_bytes(hc)
    assert [len(g) for g in got][:2] == [len(frames[0]), 0] and got[4] == b"" and got[5] == frames[1]
    assert got[2] == frames[0][30:] + frames[1] + frames[2] and len(got[3]) == fb - int(segs[7][0])
    assert sm.frames_of(fcm.flatten(hc)) == got
    for kind in ("chain", "flat"):
        _, first, totals = fcm.fragment_chains(hc, fcm.RECORDS[kind](hc), 68, True, fcm.IDENT)
        assert fcm.cut(first)[[0, 5]].tolist() == [kind == "flat", True]
        assert fcm.cut(first)[[1, 4]].tolist() == [False, False]
    hz = fcm.no_segments()
    out, first, totals = fcm.fragment_chains(hz, fcm.flat_records(hz), 100, True, 0)
    assert totals.tolist() == [300, 0] and np.array_equal(first, np.arange(301)) and out == [b""] * 300


# which of cut_frames() each mtu cuts, and the fragments of each (flat records)
EVERY_CUT = {36: {0: 3, 1: 7}, 68: {1: 3, 2: 6, 3: 2, 4: 3, 5: 6}, 120: {6: 5}, 208: {7: 3}}


def test_every_cut_batch_reaches_each_header_rule():
    frames = fcm.cut_frames()
    assert [len(f) for f in frames] == [75, 134, 123, 94, 95, 103, 186, 243]
    ranges = fcm.cut_ranges()
    assert set(EVERY_CUT) == set(fcm.CUT_MTUS)
    cut_by = {kind: {} for kind in fcm.RECORDS}
    for mtu, frags in EVERY_CUT.items():
        for kind in ("flat", "chain"):
            hc, recs, (out, first, totals) = fcm.every_cut(0, kind, mtu)
            assert hc.n == sum(len(f) + 1 for f in frames) and int(totals[0]) == len(out)
            cut, n_out = fcm.cut(first), np.diff(first.astype(np.int64))
            for k, (lo, hi) in enumerate(ranges):
                if k not in frags:
                    assert not cut[lo:hi].any(), (mtu, kind, k)
                elif kind == "flat":
                    # the flat records say "cut" wherever the segments are cut
                    assert (n_out[lo:hi] == frags[k]).all(), (mtu, k)
                else:
                    # the chain parse's: roughly the cuts outside the headers
                    assert 0 < cut[lo:hi].sum() < hi - lo, (mtu, k)
                    assert set(n_out[lo:hi].tolist()) == {1, frags[k]}
                    cut_by[kind][mtu, k] = int(cut[lo:hi].sum())
    assert cut_by["chain"][36, 0] == 43 and cut_by["chain"][208, 7] == 47
    # the arena phase moves no byte of the chains
    assert fcm.chain_bytes(fcm.every_cut(11, "flat", 36)[0]) == fcm.chain_bytes(fcm.every_cut(0, "flat", 36)[0])
    # what the frames are there for
    hb = sm.pack(frames)
    r = sm.oracle_records(hb)
    assert all(int(x) in fm.IP4_STATUSES for x in r["status"])
    assert r["l4_off"][2] - r["l3_off"][2] == 60 and r["l3_off"][2] == 22           # ihl 60, two tags
    hdr = [len(fm.fragment_frame(f, r[k], int(dispatch_ethertype(r)[k]), k, mtu, True)[1]) -
           int(r["l3_off"][k]) - c
           for k, f, mtu, c in ((4, frames[4], 68, 16), (5, frames[5], 68, 8), (7, frames[7], 208, 16))]
    assert hdr == [48, 56, 192]                          # IPv6 per-fragment headers 40, 48, 184 + 8
    out = fm.fragment_frame(frames[1], r[1], 0x0800, 1, 68, True)
    assert [len(o) - 34 for o in out] == [48, 48, 4]     # c = 48 with a last slice of 4 bytes
    out = fm.fragment_frame(frames[3], r[3], 0x0800, 3, 68, True)
    l3 = int(r["l3_off"][3])
    assert all(int.from_bytes(o[l3 + 6:l3 + 8], "big") & fm.MF for o in out)          # MF stays
    assert len(frames[3]) - (l3 + int.from_bytes(frames[3][l3 + 2:l3 + 4], "big")) == 3


def test_three_and_four_segment_cases():
    """The cut lists hold empty first and middle segments, a 1-byte segment inside a slice and
    cuts at the header's end and at slice ends; mtu 68 and 76 cut the IPv4 frame, 104 the IPv6
    frame."""
    cases = fcm.multi_cases()
    assert [(hs, mtu) for _, hs, mtu, _ in cases] == [(50, 68), (50, 76), (86, 68), (86, 76), (86, 104)]
    for f, hs, mtu, c in cases:
        hb = sm.pack([f])
        r = sm.oracle_records(hb)
        assert int(r["l4_off"][0]) == hs and len(f) == hs + 100
        out, _, _ = fm.fragment(hb, r, mtu, True, 0)
        is_cut = not (hs == 86 and mtu < 104)
        assert len(out) == (-(-100 // c) if is_cut else 1) and len(out) != 2
        if is_cut:
            assert len(out[0]) == hs + (8 if hs == 86 else 0) + c
        cuts = fcm.multi_cuts(hs, c)
        assert all(0 <= x <= len(f) for cs in cuts for x in cs)
        assert [0, 0, hs] in cuts and [30, 30, 70] in cuts and [hs, hs + c, hs + 2 * c] in cuts
        hc = fcm.chains_of([f] * len(cuts), cuts, lead=5, seed=hs + mtu)
        assert fcm.chain_bytes(hc) == [f] * len(cuts)
        first = fcm.fragment_chains(hc, fcm.flat_records(hc), mtu, True, 0)[1]
        assert fcm.cut(first).all() == is_cut and fcm.cut(first).any() == is_cut
        # the chain parse accepts the chains cut at or after the header's end
        first = fcm.fragment_chains(hc, fcm.chain_records(hc), mtu, True, 0)[1]
        assert fcm.cut(first)[7:12].all() == is_cut and not fcm.cut(first).all()


@pytest.mark.parametrize("room", [61, 64, 2048])
def test_hand_built_frames_in_data_rooms(room):
    for mtu in fm.MTU_VALUES:
        frames = fm.hand_frames(mtu)
        hc = fcm.chains_of(frames, [fcm.room_cuts(f, room) for f in frames], lead=room & 15, seed=mtu)
        assert fcm.chain_bytes(hc) == list(frames)
        for kind in ("chain", "flat"):
            totals = fcm.fragment_chains(hc, fcm.RECORDS[kind](hc), mtu, True, fcm.IDENT)[2]
            assert (int(totals[0]) > hc.n) == (mtu < 65535)


def test_generator_configs():
    """The shares the GPU test asserts, from the model on the chain parse's records."""
    hc = gen.make_chains(7, 1024, layout="mbuf")
    recs = fcm.chain_records(hc)
    assert recs.tobytes() == fcm.flat_records(hc).tobytes()
    out, first, totals = fcm.fragment_chains(hc, recs, 1500, True, fcm.IDENT)
    assert fcm.cut(first).all() and int(totals[0]) == 6144
    out, first, totals = fcm.fragment_chains(hc, recs, 1500, False, fcm.IDENT)
    assert not fcm.cut(first).any() and out == fcm.chain_bytes(hc)
    for config, share, gathered in ((11, 0.65, 22), (5, 0.52, 51)):
        hc = gen.make_chains(config, 2048, layout="fuzz")
        recs = fcm.chain_records(hc)
        first = fcm.fragment_chains(hc, recs, 300, True, fcm.IDENT)[1]
        assert abs(fcm.cut(first).mean() - share) < 0.01
        assert fcm.header_past_first_segment(hc, recs, first) == gathered
    hc = gen.make_chains(6, 4096, layout="fuzz")
    recs = fcm.chain_records(hc)
    assert len(np.unique(recs["status"])) >= 15
    assert abs(fcm.cut(fcm.fragment_chains(hc, recs, 100, True, fcm.IDENT)[1]).mean() - 0.30) < 0.01


def test_scan_block_and_its_tiling():
    hc1, recs1, want1 = fcm.scan_block()
    assert hc1.n == 700 and int(want1[2][0]) > 2 * hc1.n
    assert fcm.cut(want1[1])[dispatch_ethertype(recs1) == 0x86DD].any()
    hc, recs, want = fcm.tiled(hc1, recs1, want1, 3)
    assert hc.n == 2100 and 2 * hc.n <= hc.n_segs <= 3 * hc.n
    assert same(fcm.fragment_chains(hc, recs, 68, True, 0), want)


def test_capacity_case_and_graph_inputs():
    frames = fm.hand_frames(68)
    hc = fcm.chains_of(frames, [fcm.room_cuts(f, 64) for f in frames], lead=3, seed=64)
    totals = fcm.fragment_chains(hc, fcm.flat_records(hc), 68, True, fcm.IDENT)[2]
    assert int(totals[0]) > hc.n + 16 and int(totals[1]) > 16
    tot = [fcm.fragment_chains(h, fcm.chain_records(h), 300, True, fcm.IDENT)[2]
           for h in (gen.make_chains(5, 512, seed=s, layout="fuzz") for s in (5, 55))]
    assert tot[0][0] != tot[1][0] and tot[0][1] != tot[1][1]


def test_inverse_frames_come_back_from_reassembly():
    """In arrival order every fragment follows its predecessor, so reassembly gives back each
    chain's bytes.  In the order of the reassembly keys a datagram is told from another by
    (source, destination, identification, protocol) alone: hand_frames' IPv4 datagrams share
    one identification, so there only the IPv6 chains (identification ip6_ident + p) and the
    chains that were not cut are sure to come back."""
    frames = fcm.inverse_frames(576)
    assert len(frames) == 34
    hc = fcm.chains_of(frames, [fcm.room_cuts(f, 64) for f in frames], lead=3, seed=576)
    for kind, ncut in (("chain", 17), ("flat", 23)):
        out, first, _ = fcm.fragment_chains(hc, fcm.RECORDS[kind](hc), 576, False, fcm.IDENT)
        assert fcm.cut(first).sum() == ncut
        hb = sm.pack(out)
        r = sm.oracle_records(hb)
        assert rm.reassemble(hb, r)[0] == frames
        keyed = rm.reassemble(hb, r, rm.order_of(rm.keys(hb, r)))[0]
        sure = [f for f, c in zip(frames, fcm.cut(first)) if not c or f[12:14] == b"\x86\xdd"]
        assert len(sure) >= 20 and all(f in keyed for f in sure)
