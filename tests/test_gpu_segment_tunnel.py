"""GPU parity of rpkt_gpu_segment_tunnel_batch: the output frames, offsets, seg_first and totals
byte for byte against tests/segment_tunnel_model.py, every output pre-filled with 0xa5 and
followed by guard elements that must stay 0xa5, the inputs unchanged by the call, and the GPU's
tunnel parse of the GPU's output equal to the oracle's tunnel parse of the model's."""
import functools
import subprocess

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records, as_tunnels

import reframe_check as rc
import segment_model as sm
import segment_tunnel_model as stm
import udp_reframe_model as um

pytestmark = pytest.mark.gpu

K_SEG_BLOCK = 256                              # frames a plan block (rpkt_segcopy.h kSegBlock)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, udp):
    return rc.Outputs(torch, n, out_cap, out_bytes,
                      functools.partial(engine.segment_tunnel_batch, udp=udp),
                      engine.segment_tunnel_workspace(n), "seg_first")


def model(hb, mss, udp):
    outer, tun, inner = stm.tunnel_records(hb)
    return stm.segment(hb, outer, tun, inner, mss, udp)


def parse_back(odb, out, out_cap, what):
    """The GPU's tunnel parse over all out_cap slots of the GPU's output: the oracle's of the
    model's."""
    blob, offs = sm.packed_output(out, out_cap)
    got = engine.parse_tunnel_batch(odb, sm.F6)
    want = oracle.tunnel_batch(blob, out_cap, sm.F6, offsets=offs)
    for g, w, view, name in zip(got, want, (as_records, as_tunnels, as_records),
                                ("outer", "tunnel", "inner")):
        assert view(g.cpu().numpy()).tobytes() == w.tobytes(), \
            "%s: the %s records of the output differ" % (what, name)


def check_case(torch, hb, mss, want, udp, out_cap=None, out_bytes=None, what="", parse=True,
               records=None):
    """One call on hb at mss against the model's `want` = (out_frames, seg_first, totals).
    out_cap / out_bytes default to a little more than the totals; smaller ones overflow."""
    out, first, totals = want
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, sm.F6) if records is None else records
    before = [t.clone() for t in (db.frames,) + tuple(recs)]
    o = Outputs(torch, hb.n, out_cap, out_bytes, udp)
    odb, _, _ = o.call(db, *recs, mss)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((db.frames,) + tuple(recs), before)), \
        "%s: the inputs were written" % what
    if rc.check_outputs(o, odb, out, first, totals, what, parse_back=False) and parse:
        parse_back(odb, out, out_cap, what)


def with_lead(want, lead):
    """The model's output for the same frames behind a `lead`-byte junk frame."""
    if not lead:
        return want
    out, first, totals = want
    return ([b"\xee" * lead] + out, np.concatenate([[0], first + 1]).astype(np.uint32),
            totals + np.array([1, lead], dtype=np.uint64))


@pytest.fixture(scope="module")
def hand():
    """(mss, udp) -> (frames, the model's output)."""
    res = {}
    for mss in stm.MSS_VALUES:
        frames = stm.hand_frames(mss)
        hb = sm.pack(frames)
        recs = stm.tunnel_records(hb)
        for udp in (False, True):
            res[mss, udp] = (frames, stm.segment(hb, *recs, mss, udp))
    return res


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_frames(torch, hand, lead):
    """VXLAN, GTP-U and GRE over IPv4 and IPv6 around TCP and UDP, tags, options, extension
    headers, GTP-U extension headers, GRE with C and K, a zero outer UDP checksum, padding, plain
    frames, and the frames that pass through, at every 16-B source phase, with and without
    RPKT_SEGMENT_UDP."""
    for mss in stm.MSS_VALUES:
        for udp in (False, True):
            frames, want = hand[mss, udp]
            check_case(torch, sm.pack(frames, lead), mss, with_lead(want, lead), udp,
                       what="mss %d udp %d lead %d" % (mss, udp, lead))
        n_tcp, n_udp = int(hand[mss, False][1][2][0]), int(hand[mss, True][1][2][0])
        assert n_udp > n_tcp > len(hand[mss, False][0])


@pytest.fixture(scope="module")
def config13():
    hb = gen.make_batch(13, n=2048, seed=3)
    return hb, stm.tunnel_records(hb)


@pytest.mark.parametrize("mss,udp", [(536, False), (536, True), (100, True)])
def test_config_13(torch, config13, mss, udp):
    hb, recs = config13
    want = stm.segment(hb, *recs, mss, udp)
    kinds = stm.cut_kinds(want[1], recs[1])
    assert min(kinds[k] for k in (stm.VXLAN, stm.GTPU, stm.GRE)) >= 100, kinds
    check_case(torch, hb, mss, want, udp, what="config 13 mss %d udp %d" % (mss, udp))


def test_config_14_fuzz(torch):
    """Every tunnel status and every parse status at both levels passes through or is cut."""
    hb = gen.make_batch(14, n=4096, seed=3)
    recs = stm.tunnel_records(hb)
    assert len(np.unique(recs[1]["status"])) >= 4
    check_case(torch, hb, 100, stm.segment(hb, *recs, 100, True), True, what="config 14")


@pytest.mark.parametrize("udp", [False, True])
def test_without_tunnels_the_output_is_segment_batch_s(torch, config13, udp):
    """Every tun kind NONE: byte for byte what engine.segment_batch writes with the outer
    records."""
    # tunnel frames (cut as outer UDP datagrams with the flag) and plain TCP and UDP frames
    hb = sm.pack(sm.frames_of(config13[0])[:1024] + sm.variety(700) + um.udp_variety(700))
    db = engine.DeviceBatch.from_host(hb)
    outer, tun, inner = engine.parse_tunnel_batch(db, sm.F6)
    none = np.zeros(hb.n, dtype=as_tunnels(tun.cpu().numpy()).dtype)
    none["status"] = 1
    tun = torch.from_numpy(none.view(np.uint8).copy()).cuda()
    cap, nbytes = hb.n + hb.frames.size // 300, 2 * hb.frames.size
    a = Outputs(torch, hb.n, cap, nbytes, udp)
    b = rc.Outputs(torch, hb.n, cap, nbytes, functools.partial(engine.segment_batch, udp=udp),
                   engine.segment_workspace(hb.n), "seg_first")
    a.call(db, outer, tun, inner, 300)
    b.call(db, outer, 300)
    torch.cuda.synchronize()
    ga, gb = a.host(), b.host()
    assert int(gb[3][0]) > hb.n and int(gb[3][0]) <= cap and int(gb[3][1]) <= nbytes
    for x, y, name in zip(ga, gb, ("frames", "offsets", "seg_first", "totals")):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, config13, short):
    """Capacities below the totals: seg_first and totals exact, guards intact."""
    hb, recs = config13
    want = stm.segment(hb, *recs, 536, True)
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hb, 536, want, True, out_cap=cap, out_bytes=nbytes, what="overflow " + short)


def test_exact_capacities(torch, hand):
    frames, want = hand[17, True]
    want = with_lead(want, 5)
    check_case(torch, sm.pack(frames, 5), 17, want, True, out_cap=int(want[2][0]),
               out_bytes=int(want[2][1]), what="exact")


def test_three_plan_blocks(torch):
    """2 * kSegBlock + 5 short frames with one super-frame in each plan block: the prefix sums
    carry counts and bytes across the blocks."""
    n = 2 * K_SEG_BLOCK + 5
    short = stm.cut_frames(20)[:11] + stm.through_frames(20, 64)[:8]
    big = stm.cut_frames(700)
    frames = [short[k % len(short)] for k in range(n)]
    for at, f in ((3, big[0]), (K_SEG_BLOCK + 44, big[4]), (n - 2, big[8])):
        frames[at] = f
    hb = sm.pack(frames)
    want = model(hb, 64, False)
    cut = np.nonzero(np.diff(want[1].astype(np.int64)) > 1)[0]
    assert list(cut) == [3, K_SEG_BLOCK + 44, n - 2]
    check_case(torch, hb, 64, want, False, what="three plan blocks")


def test_records_of_another_batch_never_write_outside(torch):
    """The records of a shuffled batch: nothing is asserted about the frames; the guards and the
    0xa5 fill past out_bytes stay intact."""
    hb = gen.make_batch(13, n=1024, seed=5)
    frames = sm.frames_of(hb)
    order = np.random.default_rng(7).permutation(hb.n)
    other = engine.DeviceBatch.from_host(sm.pack([frames[k] for k in order]))
    recs = engine.parse_tunnel_batch(other, sm.F6)
    db = engine.DeviceBatch.from_host(sm.pack(frames))
    for mss, cap, nbytes in ((100, hb.n + hb.frames.size // 100, 3 * hb.frames.size),
                             (100, 3 * hb.n, hb.frames.size), (7, 4 * hb.n, hb.frames.size // 2)):
        o = Outputs(torch, hb.n, cap, nbytes, True)
        o.call(db, *recs, mss)
        torch.cuda.synchronize()
        gf, go, gs, gt = o.host()
        assert (gf[nbytes:] == 0xa5).all() and (go[cap + 1:] == 0xa5a5a5a5).all()
        assert (gs[hb.n + 1:] == 0xa5a5a5a5).all() and (gt[2:] == 0xa5a5a5a5a5a5a5a5).all()
        assert int(gs[hb.n]) == int(gt[0]) >= hb.n


def test_graph_capture(torch):
    """Tunnel parse, segment, tunnel parse of the output over out_cap slots, captured as one
    graph and replayed on two inputs: equal to the eager run's model."""
    hbs = [sm.pack(sm.frames_of(gen.make_batch(13, 512, seed=s))) for s in (5, 55)]
    wants = [model(hb, 300, True) for hb in hbs]
    assert wants[0][0] != wants[1][0] and all(int(w[2][0]) > 600 for w in wants)
    size = max(hb.frames.size for hb in hbs) + 16
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(513, dtype=torch.int32, device="cuda")
    db = engine.DeviceBatch(frames, 512, offsets)
    recs = [engine.alloc_records(512), engine._bytes(512, 16, "cuda"), engine.alloc_records(512)]
    orecs = [engine.alloc_records(out_cap), engine._bytes(out_cap, 16, "cuda"),
             engine.alloc_records(out_cap)]
    o = Outputs(torch, 512, out_cap, out_bytes, True)

    def load(hb):
        frames.zero_()
        frames[:hb.frames.size].copy_(torch.from_numpy(hb.frames.copy()))
        offsets.copy_(torch.from_numpy(hb.offsets.view(np.int32).copy()))

    def fn():
        engine.parse_tunnel_batch(db, sm.F6, *recs)
        odb, _, _ = o.call(db, *recs, 300)
        engine.parse_tunnel_batch(odb, sm.F6, *orecs)

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
        want = oracle.tunnel_batch(blob, out_cap, sm.F6, offsets=offs)
        for g, w, view in zip(orecs, want, (as_records, as_tunnels, as_records)):
            assert view(g.cpu().numpy()).tobytes() == w.tobytes()


def test_cpp_vtep_tx_through_c_abi(torch):
    """examples/vtep_tx: a C++ VTEP (C ABI only) builds four VXLAN frames around 32 KB inner TCP
    payloads, cuts them at mss 1448 and verifies all four sums of every output."""
    from rpkt_amd.build import VTEP_TX_BIN
    r = subprocess.run([VTEP_TX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "out: 92 frames" in r.stdout and "all four sums valid" in r.stdout, r.stdout
