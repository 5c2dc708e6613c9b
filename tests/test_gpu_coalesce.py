"""GPU parity of rpkt_gpu_coalesce_batch (TCP receive coalescing): the output frames, offsets,
src_first, out_mss and totals byte for byte against tests/coalesce_model.py, with every
output pre-filled with 0xa5 and followed by guard bytes that must stay 0xa5, the inputs
unchanged by the call, and the GPU's parse of the GPU's output equal to the oracle's parse of
the model's."""
import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import F_FLOW_EV, as_records

import coalesce_model as cm
import reframe_check as rc
import segment_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes):
    return rc.Outputs(torch, n, out_cap, out_bytes, engine.coalesce_batch, engine.coalesce_workspace(n),
                      "src_first", (("out_mss", n, torch.int16),))


def check_case(torch, hb, order=None, max_payload=65535, trust_sums=False, out_cap=None,
               out_bytes=None, what="", parse_back=True, want=None):
    """One call on hb against the model.  out_cap / out_bytes default to a little more than
    the model's totals (spare slots and spare bytes to check); smaller ones overflow.  Returns
    the model's (out_frames, src_first, totals, out_mss)."""
    if want is None:
        want = cm.coalesce(hb, sm.oracle_records(hb), order, max_payload, trust_sums)
    out, first, totals, mss = want
    n = hb.n
    assert order is None or len(order) == n
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, sm.F6)
    dorder = None
    if order is not None:
        dorder = torch.from_numpy(np.asarray(order, dtype=np.uint32).view(np.int32).copy()).cuda()
    f0, r0 = db.frames.clone(), recs.clone()
    o0 = dorder.clone() if dorder is not None else None
    o = Outputs(torch, n, out_cap, out_bytes)
    odb, _, _ = o.call(db, recs, dorder, max_payload, trust_sums)
    torch.cuda.synchronize()
    assert torch.equal(db.frames, f0) and torch.equal(recs, r0), "%s: the inputs were written" % what
    assert o0 is None or torch.equal(dorder, o0), "%s: the order was written" % what
    # out_mss, as src_first and totals, is exact whatever the capacities; its guard is intact
    gm = o.host()[3]
    assert np.array_equal(gm[:n], mss), "%s: out_mss at %d" % (what, rc.first_diff(gm[:n], mss))
    assert (gm[n:] == 0xa5a5).all(), what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back)
    return want


def segmented(hb, mss):
    """The model's segmentation of hb at mss: (the output frames, the number of frames cut)."""
    out, first, _ = sm.segment(hb, sm.oracle_records(hb), mss)
    return out, int((np.diff(first.astype(np.int64)) > 1).sum())


@pytest.fixture(scope="module")
def hand_segments():
    return {mss: segmented(sm.pack(sm.hand_frames(mss)), mss) for mss in sm.MSS_VALUES}


@pytest.mark.parametrize("lead", list(range(16)))
def test_segmented_hand_frames(torch, hand_segments, lead):
    """The segments of the hand-built frames at every mss (tags, IPv4 / TCP options, IPv6 with
    extension headers and a moved pseudo destination, headers past 128 B, wrap-around, flags,
    padding, fragments, pass-through frames, members of 1..1448 bytes: every source and
    destination phase), at every 16-B phase of the batch."""
    for mss in sm.MSS_VALUES:
        frames, n_seg = hand_segments[mss]
        hb = sm.pack(frames, lead)
        out, first, totals, out_mss = check_case(torch, hb, what="mss %d lead %d" % (mss, lead))
        assert int((out_mss != 0).sum()) == n_seg and (n_seg > 0) == (mss < 65535)
        assert int(totals[0]) == len(sm.hand_frames(mss)) + (1 if lead else 0)


@pytest.fixture(scope="module")
def config3():
    frames, n_seg = segmented(gen.make_batch(3, 4096), 536)
    hb = sm.pack(frames)
    return hb, cm.coalesce(hb, sm.oracle_records(hb)), n_seg


def test_config_3_segments(torch, config3):
    hb, want, n_seg = config3
    assert int(want[2][0]) == 4096 and int((want[3] != 0).sum()) == n_seg == 4096
    check_case(torch, hb, what="config 3", want=want)


@pytest.mark.parametrize("config,n_merged", [(5, 3175), (11, 2059)])
def test_configs_with_options_and_dual_stack(torch, config, n_merged):
    frames, n_seg = segmented(gen.make_batch(config, 4096), 300)
    hb = sm.pack(frames)
    want = cm.coalesce(hb, sm.oracle_records(hb))
    assert int(want[2][0]) == 4096 and int((want[3] != 0).sum()) == n_seg == n_merged
    check_case(torch, hb, what="config %d" % config, want=want)


def test_exact_capacities(torch, config3):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte."""
    hb, want, _ = config3
    check_case(torch, hb, out_cap=int(want[2][0]), out_bytes=int(want[2][1]), what="exact", want=want)


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, config3, short):
    """Capacities below the totals: RPKT_OK, src_first, out_mss and totals exact, nothing
    written past out_bytes or out_cap + 1 offsets."""
    hb, want, _ = config3
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hb, out_cap=cap, out_bytes=nbytes, what="overflow " + short, want=want)


def test_config_6_fuzz(torch):
    """Every parse status passes through."""
    hb = gen.make_batch(6, 8192)
    recs = sm.oracle_records(hb)
    assert len(np.unique(recs["status"])) >= 12
    check_case(torch, hb, what="config 6")
    check_case(torch, hb, trust_sums=True, max_payload=1000, what="config 6, trusted sums")


@pytest.fixture(scope="module")
def long_stream():
    """300 other frames, then the 65,535-byte IP packet as 65,495 one-byte segments."""
    other = sm.frames_of(gen.make_batch(5, 300))
    big = sm.tcp4(sm.payload_bytes(65535 - 40, 9), flags=sm.both_flags())
    segs, _ = segmented(sm.pack([big]), 1)
    assert len(segs) == 65495
    return sm.pack(other + segs), big


@pytest.mark.parametrize("max_payload", [65535, 3])
def test_a_run_across_blocks_and_the_scan_carry(torch, long_stream, max_payload):
    """One run of 65,495 positions: it crosses the 256-position blocks, and the block sums'
    scans their 256-block carry (258 blocks).  One output of 65,495 members, or groups of
    three."""
    hb, big = long_stream
    out, first, totals, mss = check_case(torch, hb, max_payload=max_payload,
                                         what="long stream, max_payload %d" % max_payload)
    members = np.diff(first[:int(totals[0]) + 1].astype(np.int64))
    if max_payload == 65535:
        assert out[-1] == big and members[-1] == 65495 and mss[int(totals[0]) - 1] == 1
    else:
        assert (members[-21832:-1] == 3).all() and members[-1] == 65495 - 3 * 21831


def with_port(f, port):
    """An untagged IPv4 / TCP frame of segment_model with another source port."""
    f = bytearray(f)
    f[34:36] = port.to_bytes(2, "big")
    f[50:52] = b"\0\0"
    pseudo = bytes(f[26:34]) + b"\0\x06" + (len(f) - 34).to_bytes(2, "big")
    f[50:52] = sm.csum_field(pseudo, f[34:]).to_bytes(2, "big")
    return bytes(f)


def test_interleaved_streams_with_flow_order(torch):
    """Five streams cut at 700 and interleaved round robin: nothing merges in arrival order;
    under engine.flow_order of the GPU's flow events every stream comes back whole."""
    src = [with_port(sm.tcp4(sm.payload_bytes(9000 + 13 * s, s), seq=0xfffff000 + s, ident=0xfff8 + s),
                     5000 + 7 * s) for s in range(5)]
    per = [segmented(sm.pack([f]), 700)[0] for f in src]
    assert all(len(p) == 13 for p in per)
    hb = sm.pack([per[k % 5][k // 5] for k in range(65)])
    out, _, totals, _ = check_case(torch, hb, what="interleaved, arrival order")
    assert int(totals[0]) == hb.n
    db = engine.DeviceBatch.from_host(hb)
    _, ev = engine.parse_batch(db, sm.F6 | F_FLOW_EV, n_buckets=4096)
    order = engine.flow_order(ev)
    assert order.is_cuda and order.element_size() == 4
    order = order.cpu().numpy().view(np.uint32)
    assert np.array_equal(order, cm.flow_order_host(hb))
    out, _, totals, _ = check_case(torch, hb, order=order, what="interleaved, flow order")
    assert sorted(out) == sorted(src)


def test_device_only_round_trip(torch):
    """segment -> parse -> coalesce, all on the device, gives back the source frames (a cut
    frame without its Ethernet padding), with out_mss the mss it was cut at."""
    hb = sm.pack(sm.hand_frames(536), 5)
    recs = sm.oracle_records(hb)
    cut = [sm.is_segmented(r, et == 0x86DD, 536) for r, et in zip(recs, cm.dispatch_ethertype(recs))]
    want = [f[:int(r["payload_off"]) + int(r["payload_len"])] if c else f
            for f, r, c in zip(sm.frames_of(hb), recs, cut)]
    db = engine.DeviceBatch.from_host(hb)
    sdb, seg_first, stot = engine.segment_batch(db, engine.parse_batch(db, sm.F6), 536)
    cdb, src_first, ctot = engine.coalesce_batch(sdb, engine.parse_batch(sdb, sm.F6))
    torch.cuda.synchronize()
    spare = sdb.n - int(stot[0])                       # segmentation's spare slots: empty frames
    want += [b""] * spare
    assert spare > 0 and ctot.cpu().tolist() == [hb.n + spare, sum(len(f) for f in want)]
    blob, offs = sm.packed_output(want, cdb.n)
    assert np.array_equal(cdb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(cdb.frames.cpu().numpy()[:blob.size], blob)
    # the inverse mapping: output j is made of the segments of frame j
    assert torch.equal(src_first[:hb.n + 1], seg_first)


def test_graph_capture(torch):
    """Parse, coalesce, parse of the output over out_cap slots, captured once on one stream
    as a graph and replayed over a second batch's contents: no host step between the three."""
    hbs = [sm.pack(segmented(gen.make_batch(5, 256, seed=s), 300)[0]) for s in (5, 55)]
    n = min(hb.n for hb in hbs)
    hbs = [sm.pack(sm.frames_of(hb)[:n]) for hb in hbs]
    wants = [cm.coalesce(hb, sm.oracle_records(hb)) for hb in hbs]
    assert wants[0][0] != wants[1][0]
    size = max(hb.frames.size for hb in hbs) + 16
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    db = engine.DeviceBatch(frames, n, offsets)
    recs, orecs = engine.alloc_records(n), engine.alloc_records(out_cap)
    o = Outputs(torch, n, out_cap, out_bytes)

    def load(hb):
        frames.zero_()
        frames[:hb.frames.size].copy_(torch.from_numpy(hb.frames.copy()))
        offsets.copy_(torch.from_numpy(hb.offsets.view(np.int32).copy()))

    def fn():
        engine.parse_batch(db, sm.F6, recs=recs)
        odb, _, _ = o.call(db, recs)
        engine.parse_batch(odb, sm.F6, recs=orecs)

    load(hbs[0])
    loop = graphs.CapturedLoop(fn)
    for k in (1, 0, 1):
        load(hbs[k])
        o.frames.fill_(0xa5)
        loop.replay()
        torch.cuda.synchronize()
        out, first, totals, mss = wants[k]
        gf, go, gs, gm, gt = o.host()
        blob, offs = sm.packed_output(out, out_cap)
        assert list(gt[:2]) == [int(totals[0]), int(totals[1])] and np.array_equal(gs[:n + 1], first)
        assert np.array_equal(gm[:n], mss)
        assert np.array_equal(go[:out_cap + 1], offs) and np.array_equal(gf[:blob.size], blob)
        assert (gf[blob.size:] == 0xa5).all()
        w = oracle.parse_batch(blob, out_cap, sm.F6, offsets=offs)
        assert as_records(orecs.cpu().numpy()).tobytes() == w.tobytes()


def test_cpp_lro_rx_through_c_abi(torch):
    """examples/lro_rx: streams built, segmented, interleaved, ordered, coalesced and parsed
    back through the C ABI only; the example checks that every stream came back whole."""
    import subprocess
    from rpkt_amd.build import LRO_RX_BIN
    r = subprocess.run([LRO_RX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: every stream came back whole, sums valid" in r.stdout
    assert r.stdout.count("l4_sum=0xffff") == 3 and r.stdout.count("payload_len 8000") == 3


def test_engine_refuses_bad_arguments(torch):
    hb = sm.pack(cm_stream())
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, 3)
    for mp in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.coalesce_batch(db, recs, max_payload=mp)
    with pytest.raises(engine.RpktError):
        engine.coalesce_batch(db, recs, out_cap=0, out_bytes=8192)
    odb, first, totals = engine.coalesce_batch(db, recs)
    assert totals.cpu().tolist() == [1, 54 + 4000] and first.cpu().tolist() == [0, 4, 4, 4, 4]


def cm_stream():
    """The reference's tso_tx frame with valid sums, cut at 1000."""
    f = bytearray(sm.tso_tx_frame())
    f[24:26] = sm.csum_field(f[14:34]).to_bytes(2, "big")
    f = with_port(bytes(f), 60376)
    return segmented(sm.pack([f]), 1000)[0]
