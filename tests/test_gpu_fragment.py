"""GPU parity of rpkt_gpu_fragment_batch (IPv4 / IPv6 fragmentation): the output frames,
offsets, frag_first and totals byte for byte against tests/fragment_model.py, with every
output pre-filled with 0xa5 and followed by guard bytes that must stay 0xa5, the inputs
unchanged by the call, and the GPU's parse of the GPU's output equal to the oracle's parse of
the model's.  tests/test_fragment_model.py checks the model and the inputs without a GPU."""
import functools

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records, dispatch_ethertype

import fragment_model as fm
import reframe_check as rc
import segment_model as sm

pytestmark = pytest.mark.gpu

IDENT = 0xfffffffe                              # + i wraps at the batch's third frame


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, ignore_df, ip6_ident):
    return rc.Outputs(torch, n, out_cap, out_bytes,
                      functools.partial(engine.fragment_batch, ignore_df=ignore_df, ip6_ident=ip6_ident),
                      engine.fragment_workspace(n), "frag_first")


def check_case(torch, hb, mtu, ignore_df=False, ip6_ident=IDENT, out_cap=None, out_bytes=None,
               what="", parse_back=True, want=None):
    """One call on hb at mtu against the model.  out_cap / out_bytes default to a little more
    than the model's totals (spare slots and spare bytes to check); smaller ones overflow.
    Returns the model's (out_frames, frag_first, totals)."""
    if want is None:
        want = fm.fragment(hb, sm.oracle_records(hb), mtu, ignore_df, ip6_ident)
    out, first, totals = want
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, sm.F6)
    f0, r0 = db.frames.clone(), recs.clone()
    o = Outputs(torch, hb.n, out_cap, out_bytes, ignore_df, ip6_ident)
    odb, _, _ = o.call(db, recs, mtu)
    torch.cuda.synchronize()
    assert torch.equal(db.frames, f0) and torch.equal(recs, r0), "%s: the inputs were written" % what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back)
    return want


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_frames(torch, lead):
    """IP payloads around every slice size, IPv4 options (ihl 5, 6, 9, 15), tags, IPv6 extension
    headers (U past 128 B), padding, UDP / ICMP / TCP, DF with and without the flag, input
    fragments and pass-through frames (tests/fragment_model.py: hand_frames), at every 16-B
    phase; ip6_ident 0xfffffffe wraps inside the batch."""
    for mtu in fm.MTU_VALUES:
        hb = sm.pack(fm.hand_frames(mtu), lead)
        recs = sm.oracle_records(hb)
        for ignore_df in (False, True):
            want = fm.fragment(hb, recs, mtu, ignore_df, IDENT)
            check_case(torch, hb, mtu, ignore_df, what="mtu %d lead %d df %d" % (mtu, lead, ignore_df),
                       want=want)
            assert (int(want[2][0]) > hb.n) == (mtu < 65535)


@pytest.fixture(scope="module")
def hand68():
    hb = sm.pack(fm.hand_frames(68), 5)
    return hb, fm.fragment(hb, sm.oracle_records(hb), 68, True, IDENT)


@pytest.mark.parametrize("short", ["exact", "cap", "bytes"])
def test_exact_capacities_and_one_short(torch, hand68, short):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte.  One
    slot or one byte short: RPKT_OK, frag_first and totals exact, nothing written past the
    capacities."""
    hb, want = hand68
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"exact": (n_out, need), "cap": (n_out - 1, need), "bytes": (n_out, need - 1)}[short]
    check_case(torch, hb, 68, True, out_cap=cap, out_bytes=nbytes, what=short, want=want)


def generated(config, n, mtu, ignore_df):
    hb = gen.make_batch(config, n)
    recs = sm.oracle_records(hb)
    want = fm.fragment(hb, recs, mtu, ignore_df, IDENT)
    return hb, recs, want, np.diff(want[1].astype(np.int64)) > 1


def test_config_3_without_the_flag_is_a_copy(torch):
    hb, recs, want, cut = generated(3, 4096, 576, False)
    assert int(want[2][0]) == hb.n and want[0] == sm.frames_of(hb)
    check_case(torch, hb, 576, False, what="config 3", want=want)


def test_config_3_with_the_flag(torch):
    hb, recs, want, cut = generated(3, 4096, 576, True)
    assert cut.all()
    check_case(torch, hb, 576, True, what="config 3 ignore_df", want=want)


def holds_fragment_header(f, r):
    l3, l4 = int(r["l3_off"]), int(r["l4_off"])
    nh, x = f[l3 + 6], l3 + 40
    while x < l4:
        if nh == 44:
            return True
        nh, x = f[x], x + (4 * (2 + f[x + 1]) if nh == 51 else 8 * (1 + f[x + 1]))
    return False


@pytest.mark.parametrize("ignore_df", [False, True])
def test_config_11_dual_stack(torch, ignore_df):
    """About half the frames are IPv6.  With the flag every frame is cut but the IPv6 frames
    the generator gave an (atomic) Fragment header: those the rule passes through at any mtu."""
    hb, recs, want, cut = generated(11, 4096, 300, ignore_df)
    v6 = dispatch_ethertype(recs) == 0x86DD
    assert 0.4 <= v6.mean() <= 0.6
    if ignore_df:
        held = np.array([bool(d) and holds_fragment_header(f, r)
                         for f, r, d in zip(sm.frames_of(hb), recs, v6)])
        assert np.array_equal(cut, ~held) and held.mean() < 0.15 and (cut & v6).mean() >= 0.35
    else:
        assert not cut[~v6].any() and cut[v6].any()
    check_case(torch, hb, 300, ignore_df, what="config 11", want=want)


@pytest.mark.parametrize("ignore_df", [False, True])
def test_config_5_options(torch, ignore_df):
    hb, recs, want, cut = generated(5, 4096, 300, ignore_df)
    assert cut.mean() >= 0.75 if ignore_df else not cut.any()
    check_case(torch, hb, 300, ignore_df, what="config 5", want=want)


@pytest.mark.parametrize("ignore_df", [False, True])
def test_config_6_fuzz(torch, ignore_df):
    """Every parse status passes through or is cut."""
    hb, recs, want, cut = generated(6, 8192, 100, ignore_df)
    assert len(np.unique(recs["status"])) >= 12
    assert cut.mean() >= 0.40 if ignore_df else not cut.any()
    check_case(torch, hb, 100, ignore_df, what="config 6", want=want)


def test_scan_across_blocks(torch):
    """70,000 frames of 64..200 B at mtu 48 with the flag: the prefix sums cross the 256-frame
    blocks and the 256-block carry of the block sums' scan (274 blocks).  700 distinct frames
    (hand-built UDP over IPv4 / IPv6 of every length, and config-6 fuzz frames cut to size),
    tiled 100 times: the model's output of the 700 is tiled the same way.  ip6_ident is 0 here,
    and the IPv6 frames are too short to be cut at this mtu, so the tiles' outputs are equal."""
    fuzz = [f for f in sm.frames_of(gen.make_batch(6, 4096)) if 64 <= len(f) <= 200][:300]
    assert len(fuzz) == 300
    hand = [fm.udp4(30 + k % 117, ident=k, options=fm.OPTIONS_MIX if k % 5 == 0 else b"") if k % 3 else
            fm.udp6(10 + k % 127) for k in range(400)]
    block = [f for pair in zip(hand[:300], fuzz) for f in pair] + hand[300:]
    assert all(64 <= len(f) <= 200 for f in block) and len(set(block)) > 600
    hb1 = sm.pack(block)
    recs1 = sm.oracle_records(hb1)
    out1, first1, tot1 = fm.fragment(hb1, recs1, 48, True, 0)
    cut1 = np.diff(first1.astype(np.int64)) > 1
    assert not cut1[dispatch_ethertype(recs1) == 0x86DD].any()
    reps = 100
    hb = sm.pack(block * reps)
    assert hb.n == 70000
    first = np.concatenate([first1[:-1].astype(np.uint64) + r * int(tot1[0]) for r in range(reps)] +
                           [np.array([reps * int(tot1[0])], dtype=np.uint64)]).astype(np.uint32)
    want = (out1 * reps, first, tot1 * np.uint64(reps))
    assert int(want[2][0]) > 2 * hb.n
    check_case(torch, hb, 48, True, 0, what="70,000 frames", want=want, parse_back=False)


@pytest.mark.parametrize("stride", [1104, 1101])
def test_strided_input(torch, stride):
    """frame_len < stride, at strides that are and are not a multiple of 16."""
    frames = [fm.udp4(1000, ident=k) if k % 2 else fm.udp6(980) for k in range(75)]
    flen = len(frames[0])
    assert all(len(f) == flen for f in frames) and flen < stride
    buf = np.full(len(frames) * stride + 16, 0xee, dtype=np.uint8)
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + flen] = np.frombuffer(f, dtype=np.uint8)
    hb = gen.HostBatch(0, len(frames), 0, buf, None, stride, flen)
    out, first, totals = check_case(torch, hb, 400, what="stride %d" % stride)
    assert int(totals[0]) == 3 * hb.n
    packed = fm.fragment(sm.pack(frames), sm.oracle_records(sm.pack(frames)), 400, False, IDENT)
    assert out == packed[0]


@pytest.mark.parametrize("mtu", [68, 300, 1500])
def test_default_sizes_come_from_the_documented_bound(torch, mtu):
    """engine.fragment_batch with no outputs given sizes them from the bound: never an
    overflow for per-fragment L3 headers within its l3_header_max."""
    frames = [fm.udp4(3000), fm.udp4(3000, options=fm.OPTIONS_40, tags=2), fm.tcp4(2000, tags=1),
              fm.icmp4(1500), fm.udp4(40), fm.udp4(3000, frag=fm.DF), fm.udp6(3000),
              fm.udp6(3000, (fm.HBH,), tags=2), fm.udp6(2500, (fm.DEST,)), fm.udp6(20),
              fm.udp6(500, (fm.ext(0, 16),)), fm.udp6(900, (fm.fragment_header(17),)), b"",
              fm.ether(0, 0x0806) + bytes(28)]
    hb = sm.pack(frames * 5)
    out, first, totals = fm.fragment(hb, sm.oracle_records(hb), mtu, True, 3)
    assert int(totals[0]) > hb.n
    db = engine.DeviceBatch.from_host(hb)
    odb, gs, gt = engine.fragment_batch(db, engine.parse_batch(db, sm.F6), mtu, ignore_df=True,
                                        ip6_ident=3)
    assert odb.n == hb.n + hb.frames.size // max(8, (mtu - 68) & ~7) and odb.n >= int(totals[0])
    assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
    assert odb.frames.numel() >= int(totals[1])
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), first)
    blob, offs = sm.packed_output(out, odb.n)
    assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)


def test_graph_capture(torch):
    """Parse, fragment, parse of the output over out_cap slots, captured as one graph and
    replayed on two inputs: no host step between the three."""
    hbs = [gen.make_batch(11, 512, seed=s) for s in (5, 55)]
    wants = [fm.fragment(hb, sm.oracle_records(hb), 300, True, IDENT) for hb in hbs]
    assert wants[0][2][0] != wants[1][2][0]
    size = max(hb.frames.size for hb in hbs) + 16
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    strided = hbs[0].offsets is None
    offsets = None if strided else torch.zeros(513, dtype=torch.int32, device="cuda")
    db = engine.DeviceBatch(frames, 512, offsets, hbs[0].stride, hbs[0].frame_len)
    recs, orecs = engine.alloc_records(512), engine.alloc_records(out_cap)
    o = Outputs(torch, 512, out_cap, out_bytes, True, IDENT)

    def load(hb):
        frames.zero_()
        frames[:hb.frames.size].copy_(torch.from_numpy(hb.frames.copy()))
        if not strided:
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


def test_cpp_vtep_frag_tx_through_c_abi(torch):
    """examples/vtep_frag_tx: 1500-byte inner frames in VXLAN, fragmented at mtu 1500 and parsed
    back through the C ABI only; the example checks its own fragments."""
    import subprocess
    from rpkt_amd.build import VTEP_FRAG_TX_BIN
    r = subprocess.run([VTEP_FRAG_TX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: 2 fragments a frame" in r.stdout


def test_engine_refuses_bad_arguments(torch):
    hb = sm.pack([fm.udp4(3000)])
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, 3)
    for mtu in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.fragment_batch(db, recs, mtu, out_cap=8, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.fragment_batch(db, recs, 1500, out_cap=0, out_bytes=8192)
    odb, first, totals = engine.fragment_batch(db, recs, 1500)
    assert totals.cpu().tolist() == [3, 3000 + 3 * 34] and first.cpu().tolist() == [0, 3]
