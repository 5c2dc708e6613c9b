"""GPU parity of rpkt_gpu_segment_batch (TCP segmentation): the output frames, offsets,
seg_first and totals byte for byte against tests/segment_model.py, with every output
pre-filled with 0xa5 and followed by guard bytes that must stay 0xa5, and the inputs
unchanged by the call."""
import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records

import reframe_check as rc
import segment_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes):
    return rc.Outputs(torch, n, out_cap, out_bytes, engine.segment_batch, engine.segment_workspace(n),
                      "seg_first")


def check_case(torch, hb, mss, out_cap=None, out_bytes=None, what="", parse_back=True, want=None):
    """One call on hb at mss against the model.  out_cap / out_bytes default to a little more
    than the model's totals (spare slots and spare bytes to check); smaller ones overflow.
    Returns the model's (out_frames, seg_first, totals)."""
    out, first, totals = want if want is not None else sm.segment(hb, sm.oracle_records(hb), mss)
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, sm.F6)
    f0, r0 = db.frames.clone(), recs.clone()
    o = Outputs(torch, hb.n, out_cap, out_bytes)
    odb, _, _ = o.call(db, recs, mss)
    torch.cuda.synchronize()
    assert torch.equal(db.frames, f0) and torch.equal(recs, r0), "%s: the inputs were written" % what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back)
    return out, first, totals


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_frames(torch, lead):
    """Payload lengths around every mss, tags, IPv4 / TCP options, IPv6 with extension headers
    (a moved pseudo destination, headers past 128 B), wrap-around, flags, padding, fragments
    and pass-through frames (tests/segment_model.py: hand_frames), at every 16-B phase."""
    for mss in sm.MSS_VALUES:
        hb = sm.pack(sm.hand_frames(mss), lead)
        out, first, totals = check_case(torch, hb, mss, what="mss %d lead %d" % (mss, lead))
        assert (int(totals[0]) > hb.n) == (mss < 65535)


def test_exact_capacities(torch):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte."""
    hb = sm.pack(sm.hand_frames(17), 5)
    out, first, totals = sm.segment(hb, sm.oracle_records(hb), 17)
    check_case(torch, hb, 17, out_cap=int(totals[0]), out_bytes=int(totals[1]), what="exact",
               want=(out, first, totals))


@pytest.fixture(scope="module")
def config3():
    hb = gen.make_batch(3, 4096)
    return hb, sm.segment(hb, sm.oracle_records(hb), 536)


def test_config_3_strided_1500(torch, config3):
    hb, want = config3
    counts = np.diff(want[1].astype(np.int64))
    assert (counts == 3).mean() >= 0.95
    check_case(torch, hb, 536, what="config 3", want=want)


@pytest.mark.parametrize("config", [5, 11])
def test_configs_with_options_and_dual_stack(torch, config):
    hb = gen.make_batch(config, 4096)
    want = sm.segment(hb, sm.oracle_records(hb), 300)
    assert (np.diff(want[1].astype(np.int64)) > 1).mean() >= 0.40
    check_case(torch, hb, 300, what="config %d" % config, want=want)


def test_config_6_fuzz(torch):
    """Every parse status passes through or segments."""
    hb = gen.make_batch(6, 8192)
    recs = sm.oracle_records(hb)
    assert len(np.unique(recs["status"])) >= 12
    want = sm.segment(hb, recs, 100)
    assert (np.diff(want[1].astype(np.int64)) > 1).any()
    check_case(torch, hb, 100, what="config 6", want=want)


def test_default_sizes_come_from_the_documented_bound(torch):
    """engine.segment_batch with no outputs given sizes them from the bound: never an
    overflow for headers within its header_max."""
    hb = gen.make_batch(5, 1024)
    out, first, totals = sm.segment(hb, sm.oracle_records(hb), 300)
    db = engine.DeviceBatch.from_host(hb)
    odb, gs, gt = engine.segment_batch(db, engine.parse_batch(db, sm.F6), 300)
    assert odb.n == hb.n + hb.frames.size // 300 and odb.n >= int(totals[0])
    assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
    assert odb.frames.numel() >= int(totals[1])
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), first)
    blob, offs = sm.packed_output(out, odb.n)
    assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)


def test_scan_across_blocks(torch):
    """70,000 frames of 64..200 B at mss 32: the prefix sums cross the 256-frame blocks and
    the 256-block carry of the block sums' scan (274 blocks).  700 distinct frames (hand-built
    TCP over IPv4 / IPv6 with every payload length, and config-6 fuzz frames cut to size),
    tiled 100 times: the model's output of the 700 is tiled the same way."""
    fuzz = [f for f in sm.frames_of(gen.make_batch(6, 4096)) if 64 <= len(f) <= 200][:300]
    assert len(fuzz) == 300
    hand = [sm.tcp4(sm.payload_bytes(10 + k % 137, k), seq=k * 977, ident=k) if k % 3 else
            sm.tcp6(sm.payload_bytes(k % 127, k)) for k in range(400)]
    block = [f for pair in zip(hand[:300], fuzz) for f in pair] + hand[300:]
    assert all(64 <= len(f) <= 200 for f in block) and len(set(block)) > 600
    hb1 = sm.pack(block)
    out1, first1, tot1 = sm.segment(hb1, sm.oracle_records(hb1), 32)
    reps = 100
    hb = sm.pack(block * reps)
    assert hb.n == 70000
    first = np.concatenate([first1[:-1].astype(np.uint64) + r * int(tot1[0]) for r in range(reps)] +
                           [np.array([reps * int(tot1[0])], dtype=np.uint64)]).astype(np.uint32)
    want = (out1 * reps, first, tot1 * np.uint64(reps))
    assert int(want[2][0]) > 2 * hb.n
    check_case(torch, hb, 32, what="70,000 frames", want=want, parse_back=False)


@pytest.mark.parametrize("stride", [1104, 1101])
def test_strided_input(torch, stride):
    """frame_len < stride, at strides that are and are not a multiple of 16."""
    frames = [sm.tcp4(sm.payload_bytes(1000, k), seq=k * 4099, ident=k) for k in range(75)]
    flen = len(frames[0])
    assert all(len(f) == flen for f in frames) and flen < stride
    buf = np.full(len(frames) * stride + 16, 0xee, dtype=np.uint8)
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + flen] = np.frombuffer(f, dtype=np.uint8)
    hb = gen.HostBatch(0, len(frames), 0, buf, None, stride, flen)
    out, first, totals = check_case(torch, hb, 400, what="stride %d" % stride)
    assert int(totals[0]) == 3 * hb.n
    packed = sm.segment(sm.pack(frames), sm.oracle_records(sm.pack(frames)), 400)
    assert out == packed[0]


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, config3, short):
    """Capacities below the totals: RPKT_OK, seg_first and totals exact, nothing written past
    out_bytes or out_cap + 1 offsets."""
    hb, want = config3
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hb, 536, out_cap=cap, out_bytes=nbytes, what="overflow " + short, want=want)


def test_graph_capture(torch):
    """Parse, segment, parse of the output over out_cap slots, captured as one graph and
    replayed on two inputs: no host step between the three."""
    hbs = [gen.make_batch(5, 512, seed=s) for s in (5, 55)]
    wants = [sm.segment(hb, sm.oracle_records(hb), 300) for hb in hbs]
    assert wants[0][2][0] != wants[1][2][0]
    size = max(hb.frames.size for hb in hbs) + 16
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(513, dtype=torch.int32, device="cuda")
    db = engine.DeviceBatch(frames, 512, offsets)
    recs, orecs = engine.alloc_records(512), engine.alloc_records(out_cap)
    o = Outputs(torch, 512, out_cap, out_bytes)

    def load(hb):
        frames.zero_()
        frames[:hb.frames.size].copy_(torch.from_numpy(hb.frames.copy()))
        offsets.copy_(torch.from_numpy(hb.offsets.view(np.int32).copy()))

    def fn():
        engine.parse_batch(db, sm.F6, recs=recs)
        odb, _, _ = o.call(db, recs, 300)
        engine.parse_batch(odb, sm.F6, recs=orecs)

    load(hbs[0])
    loop = graphs.CapturedLoop(fn)
    for k in (1, 0, 1):
        load(hbs[k])
        o.frames.fill_(0xa5)
        loop.replay()
        torch.cuda.synchronize()
        out, first, totals = wants[k]
        gf, go, gs, gt = o.host()
        blob, offs = sm.packed_output(out, out_cap)
        assert list(gt[:2]) == [int(totals[0]), int(totals[1])] and np.array_equal(gs[:513], first)
        assert np.array_equal(go[:out_cap + 1], offs) and np.array_equal(gf[:blob.size], blob)
        assert (gf[blob.size:] == 0xa5).all()
        w = oracle.parse_batch(blob, out_cap, sm.F6, offsets=offs)
        assert as_records(orecs.cpu().numpy()).tobytes() == w.tobytes()


def test_cpp_tso_tx_through_c_abi(torch):
    """examples/tso_tx: the reference's tso_tx.rs frame built, segmented at 1024 and parsed
    back through the C ABI only; the example checks its own four segments."""
    import subprocess
    from rpkt_amd.build import TSO_TX_BIN
    r = subprocess.run([TSO_TX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: 4 segments, sums valid" in r.stdout and r.stdout.count("l4_sum=0xffff") == 5


def test_engine_refuses_bad_arguments(torch):
    hb = sm.pack([sm.tso_tx_frame()])
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, 3)
    for mss in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.segment_batch(db, recs, mss, out_cap=8, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.segment_batch(db, recs, 1024, out_cap=0, out_bytes=8192)
    odb, first, totals = engine.segment_batch(db, recs, 1024)
    assert totals.cpu().tolist() == [4, 4000 + 4 * 54] and first.cpu().tolist() == [0, 4]
