"""tests/segment_tunnel_chains_model.py pinned, and the input conditions the GPU tests of
rpkt_gpu_segment_tunnel_chains rely on (tests/test_gpu_segment_tunnel_chains.py), so that they
can be checked without a GPU: how many chains of each tunnel kind each case cuts, how many of
them have a header that is gathered through the segment list, and that the two record sources
agree where no header is cut.  CPU only.

The floors are caps against a vacuous test, below what the reference models give on the default
seeds (measured: config 13 fuzz, 2048 chains, mss 300: 466 / 462 / 198 VXLAN / GTP-U / GRE
chains cut with the flag and 224 / 223 / 96 without, 93 and 46 of them with the inner header
past the first non-empty segment, 811 / 813 / 313 with the flat records; config 14 fuzz, 4096
chains, mss 100: 427 / 347 / 164 and all six tunnel statuses)."""
import os
import re

import numpy as np
import pytest

from rpkt_amd import engine, gen

import segment_chains_model as scm
import segment_model as sm
import segment_tunnel_chains_model as stcm
import segment_tunnel_model as stm
import test_segment_tunnel_model as flat_tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNNELS = (stm.VXLAN, stm.GTPU, stm.GRE)


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def same_records(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def config13():
    hc = gen.make_chains(13, 2048, layout="fuzz")
    return hc, stcm.chain_records(hc)


@pytest.mark.parametrize("udp,floor,past", [(True, 150, 40), (False, 80, 20)])
def test_config_13_fuzz_cuts_every_kind_and_gathers_headers(config13, udp, floor, past):
    hc, recs = config13
    out, first, totals = stcm.segment(hc, *recs, 300, udp)
    kinds = stm.cut_kinds(first, recs[1])
    assert min(kinds[k] for k in TUNNELS) >= floor, kinds
    assert stcm.header_past_first_segment(hc, *recs, first) >= past
    assert [kinds[k] for k in TUNNELS] == ([466, 462, 198] if udp else [224, 223, 96])
    assert int(totals[0]) == len(out) == int(first[-1]) > hc.n


def test_config_13_fuzz_flat_records_cut_more(config13):
    """The flat records of the flattened bytes cut the chains whose headers straddle a segment
    end too."""
    hc, recs = config13
    flat = stcm.flat_records(hc)
    kinds = stm.cut_kinds(stcm.segment(hc, *flat, 300, True)[1], flat[1])
    assert [kinds[k] for k in TUNNELS] == [811, 813, 313]


def test_config_14_fuzz_has_every_tunnel_status():
    hc = gen.make_chains(14, 4096, layout="fuzz")
    recs = stcm.chain_records(hc)
    assert sorted(np.unique(recs[1]["status"]).tolist()) == [0, 1, 2, 3, 4, 5]
    kinds = stm.cut_kinds(stcm.segment(hc, *recs, 100, True)[1], recs[1])
    assert min(kinds[k] for k in TUNNELS) >= 100, kinds
    assert [kinds[k] for k in TUNNELS] == [427, 347, 164]


def test_single_segment_chains_are_the_flat_batch():
    for mss, lead in ((17, 5), (536, 0)):
        hb = sm.pack(stm.hand_frames(mss), lead)
        hc = stcm.single_segment_chains(hb)
        flat = stm.tunnel_records(hb)
        assert same_records(stcm.chain_records(hc), flat)
        for udp in (False, True):
            assert same(stcm.segment(hc, *flat, mss, udp), stm.segment(hb, *flat, mss, udp))


def test_mbuf_layout_chain_records_are_the_flat_records():
    """Data rooms of 2048 bytes: every header lies in the first segment."""
    hc = gen.make_chains(13, 2048, layout="mbuf")
    chain, flat = stcm.chain_records(hc), stcm.flat_records(hc)
    assert same_records(chain, flat)
    hb = scm.flatten(hc)
    want = stm.segment(hb, *flat, 300, True)
    assert same(stcm.segment(hc, *chain, 300, True), want)
    kinds = stm.cut_kinds(want[1], flat[1])
    assert min(kinds[k] for k in TUNNELS) >= 100, kinds


@pytest.mark.parametrize("udp", [False, True])
@pytest.mark.parametrize("mss", stm.MSS_VALUES)
def test_hand_built_chains_verify_under_the_oracle(mss, udp):
    """The hand-built set in 64-byte data rooms: the model's output parses back with all four
    sums valid for every cut frame, with either kind of records."""
    frames = stm.hand_frames(mss)
    hc = scm.chains_of(frames, [scm.room_cuts(f, 64) for f in frames], lead=3, seed=mss)
    hb = scm.flatten(hc)
    assert sm.frames_of(hb) == frames
    for kind in ("chain", "flat"):
        recs = stcm.RECORDS[kind](hc)
        first, _ = flat_tests.check_cut(hb, recs, mss, udp, "%s records mss %d" % (kind, mss))
        assert same(stcm.segment(hc, *recs, mss, udp), stm.segment(hb, *recs, mss, udp))
        if kind == "flat":
            n = np.diff(first.astype(np.int64))
            cut = len(stm.cut_frames(1))
            want = [k < stm.N_CUT_TCP - 1 or k == stm.N_CUT_TCP or udp for k in range(cut)] + [True] * 3
            assert [x > 1 for x in n[:cut + 3]] == want


def test_the_entry_in_the_header_the_wrapper_and_the_rust_binding():
    hdr = open(os.path.join(ROOT, "include", "rpkt_gpu.h")).read()
    names = ("rpkt_gpu_segment_tunnel_chains", "rpkt_gpu_segment_tunnel_chains_workspace_bytes")
    for name in names:
        assert re.search(r"\b%s\(" % name, hdr) and name in engine.EXPORTS
    assert "tunnel segmentation over mbuf chains" not in hdr
    assert "takes flat batches only" not in hdr
    assert "nested" in hdr and "Not covered: coalescing over chains" in hdr
    ffi = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "lib.rs")).read()
    for name in names:
        assert "pub fn %s(" % name in ffi
        assert re.search(r"pub (unsafe )?fn %s\(" % name[len("rpkt_gpu_"):], lib_rs)
    assert callable(engine.segment_tunnel_chains) and callable(engine.segment_tunnel_chains_workspace)
