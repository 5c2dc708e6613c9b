"""GPU parity of rpkt_gpu_reassemble_batch and rpkt_gpu_reassemble_keys (IPv4 / IPv6
reassembly): the output frames, offsets, src_first and totals byte for byte against
tests/reassemble_model.py, with every output pre-filled with 0xa5 and followed by guard bytes
that must stay 0xa5, the inputs unchanged by the call, and the GPU's parse of the GPU's output
equal to the oracle's parse of the model's.  tests/test_reassemble_model.py checks the model
without a GPU."""
import functools

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records

import fragment_model as fm
import reassemble_model as rm
import reframe_check as rc
import segment_model as sm

pytestmark = pytest.mark.gpu

IDENT = 0xfffffffe                              # + i wraps at the batch's third frame


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes):
    return rc.Outputs(torch, n, out_cap, out_bytes, engine.reassemble_batch,
                      engine.reassemble_workspace(n), "src_first")


def device_order(torch, order):
    return torch.from_numpy(np.asarray(order, dtype=np.uint32).view(np.int32).copy()).cuda()


def check_case(torch, hb, order=None, trust_sums=False, out_cap=None, out_bytes=None, what="",
               parse_back=True, want=None):
    """One call on hb against the model.  out_cap / out_bytes default to a little more than the
    model's totals (spare slots and spare bytes to check); smaller ones overflow.  Returns the
    model's (out_frames, src_first, totals)."""
    if want is None:
        want = rm.reassemble(hb, sm.oracle_records(hb), order, trust_sums)
    out, first, totals = want
    n = hb.n
    assert order is None or len(order) == n
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, sm.F6)
    dorder = None if order is None else device_order(torch, order)
    f0, r0 = db.frames.clone(), recs.clone()
    o0 = dorder.clone() if dorder is not None else None
    o = Outputs(torch, n, out_cap, out_bytes)
    odb, _, _ = o.call(db, recs, dorder, trust_sums)
    torch.cuda.synchronize()
    assert torch.equal(db.frames, f0) and torch.equal(recs, r0), "%s: the inputs were written" % what
    assert o0 is None or torch.equal(dorder, o0), "%s: the order was written" % what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back)
    return want


@functools.lru_cache(maxsize=None)
def hand_fragments(mtu):
    """fragment(hand_frames(mtu)) with ignore_df, as frames."""
    hb, _ = rm.fragmented(fm.hand_frames(mtu), mtu, True, IDENT)
    return tuple(sm.frames_of(hb))


@pytest.mark.parametrize("mtu", fm.MTU_VALUES)
def test_hand_built_frames_round_trip(torch, mtu):
    """fragment(hand_frames(mtu)) in position order: 45 frames come back at every mtu."""
    hb = sm.pack(hand_fragments(mtu))
    want = rm.reassemble(hb, sm.oracle_records(hb))
    assert int(want[2][0]) == 45
    check_case(torch, hb, what="mtu %d" % mtu, want=want)


@pytest.mark.parametrize("lead", list(range(1, 16)))
def test_hand_built_frames_at_every_phase(torch, lead):
    """Mtus 28, 68, 576 and 1500 at every 16-B phase of the input; the members' payload lengths
    put them at every destination phase."""
    for mtu in (28, 68, 576, 1500):
        hb = sm.pack(hand_fragments(mtu), lead)
        want = rm.reassemble(hb, sm.oracle_records(hb))
        assert int(want[2][0]) == 45 + 1                           # and the lead frame
        check_case(torch, hb, what="mtu %d lead %d" % (mtu, lead), want=want)


@pytest.fixture(scope="module")
def hand68():
    hb = sm.pack(hand_fragments(68), 5)
    return hb, rm.reassemble(hb, sm.oracle_records(hb))


@pytest.mark.parametrize("short", ["exact", "cap", "bytes"])
def test_exact_capacities_and_one_short(torch, hand68, short):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte.  One
    slot or one byte short: RPKT_OK, src_first and totals exact, nothing written past the
    capacities."""
    hb, want = hand68
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"exact": (n_out, need), "cap": (n_out - 1, need), "bytes": (n_out, need - 1)}[short]
    check_case(torch, hb, out_cap=cap, out_bytes=nbytes, what=short, want=want)


KINDS = 6


def datagram(k, n):
    """Datagram k of the shuffled burst: an IP payload of n bytes in one of six header kinds;
    each IPv4 datagram has its own ident (equal idents are one datagram by definition), each
    IPv6 one its own identification through ip6_ident + i."""
    kind = k % KINDS
    if kind == 0:
        return fm.udp4(n, ident=0x1000 + k)
    if kind == 1:
        return fm.udp4(n, ident=0x1000 + k, options=fm.OPTIONS_MIX, tags=1)
    if kind == 2:
        return fm.tcp4(max(n, 20), ident=0x1000 + k, tags=2)
    if kind == 3:
        return fm.udp6(n)
    if kind == 4:
        return fm.udp6(n, (fm.HBH, fm.RT0))
    return fm.udp6(n, fm.LONG_EXTS, tags=1)


@pytest.fixture(scope="module")
def shuffled():
    """300 datagrams of 8..4000 B in six header kinds fragmented at 300, permuted with a fixed
    seed: (sources, hb, recs, keys, order, the model under the order)."""
    rng = np.random.RandomState(11)
    src = [datagram(k, int(rng.randint(8, 4001))) for k in range(300)]
    hb, _ = rm.fragmented(src, 300, False, 77)
    fr = sm.frames_of(hb)
    assert len(fr) > 2500
    perm = rng.permutation(len(fr))
    hb = sm.pack([fr[k] for k in perm])
    recs = sm.oracle_records(hb)
    keys = rm.keys(hb, recs)
    order = rm.order_of(keys)
    want = rm.reassemble(hb, recs, order)
    assert int(want[2][0]) == 300
    return src, hb, recs, keys, order, want


def test_shuffled_arrival_keys_and_order(torch, shuffled):
    src, hb, recs, keys, order, want = shuffled
    db = engine.DeviceBatch.from_host(hb)
    grecs = engine.parse_batch(db, sm.F6)
    gk = engine.reassemble_keys(db, grecs)
    assert gk.dtype == torch.int64 and gk.numel() == hb.n
    assert np.array_equal(gk.cpu().numpy().view(np.uint64), keys)
    go = engine.reassemble_order(gk)
    assert go.is_cuda and go.element_size() == 4
    assert np.array_equal(go.cpu().numpy().view(np.uint32), order)
    assert np.array_equal(engine.reassemble_order(gk.cpu()).numpy().view(np.uint32), order)
    # the outputs are the 300 sources as a multiset, and the model's in order
    assert sorted(want[0]) == sorted(src)
    check_case(torch, hb, order=order, what="shuffled, key order", want=want)


def test_shuffled_arrival_without_an_order(torch, shuffled):
    src, hb, recs, keys, order, _ = shuffled
    out, first, totals = check_case(torch, hb, what="shuffled, arrival order")
    assert int(totals[0]) > 0.9 * hb.n                             # almost nothing merges


def test_keys_with_trusted_sums(torch):
    """A fragment whose header sum does not verify: a fragment's key only under trust_sums."""
    a, b = fm.ip4(fm.payload_bytes(16), frag=fm.MF), bytearray(fm.ip4(fm.payload_bytes(9), frag=2))
    b[14 + 10] ^= 0x40
    hb = sm.pack([a, bytes(b), fm.udp4(20)])
    recs = sm.oracle_records(hb)
    db = engine.DeviceBatch.from_host(hb)
    grecs = engine.parse_batch(db, sm.F6)
    for trust in (False, True):
        want = rm.keys(hb, recs, trust)
        assert (want >> np.uint64(63)).tolist() == [0, 0 if trust else 1, 1]
        got = engine.reassemble_keys(db, grecs, trust_sums=trust)
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
        check_case(torch, hb, trust_sums=trust, what="trust %d" % trust)


def test_twice_fragmented(torch):
    """Fragments of fragments (300, then 100), in position order: one call brings the IPv4
    sources back whole."""
    src = fm.hand_frames(300)
    once, _ = rm.fragmented(src, 300, True, IDENT)
    hb, _ = rm.fragmented(sm.frames_of(once), 100, True, 7)
    out, _, totals = check_case(torch, hb, what="twice")
    assert int(totals[0]) == 45 and hb.n > 2 * once.n
    for k in (0, 3, 14, 16, 21):                                   # plain, options, tags, TCP
        assert out[k] == src[k], k


@pytest.mark.parametrize("trust", [False, True])
def test_config_6_fuzz(torch, trust):
    """Every parse status passes through or merges."""
    hb, _ = rm.fragmented(sm.frames_of(gen.make_batch(6, 8192)), 100, True, IDENT)
    recs = sm.oracle_records(hb)
    assert len(np.unique(recs["status"])) >= 12
    want = rm.reassemble(hb, recs, None, trust)
    assert 8192 <= int(want[2][0]) < 0.8 * hb.n
    check_case(torch, hb, trust_sums=trust, what="config 6 trust %d" % trust, want=want)


def test_scan_across_blocks(torch):
    """72,380 positions: runs that cross the 256-position blocks (datagrams of 300 fragments: an
    IP payload of 2,400 at mtu 28) and the 256-block carry of both one-block scans (283 blocks).
    658 distinct frames tiled 110 times: the model's output of one tile is tiled the same way (a
    tile ends in a last fragment and begins with a first one, so no run crosses tiles)."""
    src = [fm.udp4(2400, ident=1), fm.udp6(40), fm.udp4(64, ident=2), fm.udp6(2400 - 1),
           fm.udp4(30, ident=3), fm.ether(0, 0x0806) + bytes(28), fm.udp4(300, ident=4, tags=1)]
    hb1, _ = rm.fragmented(src, 28, False, 9)
    hb2, _ = rm.fragmented([src[1], src[3]], 56, False, 9)          # IPv6 needs mtu >= 56
    block = sm.frames_of(hb1) + sm.frames_of(hb2)
    assert len(block) == len(set(block)) == 658
    one = sm.pack(block)
    out1, first1, tot1 = rm.reassemble(one, sm.oracle_records(one))
    assert out1 == src + [src[1], src[3]]
    runs = np.diff(first1[:len(out1) + 1].astype(np.int64))
    assert runs.max() == 300 and (runs > 256).sum() == 2
    reps = 110
    hb = sm.pack(block * reps)
    n = hb.n
    assert n == 72380 and n > 256 * 256
    first = np.full(n + 1, n, dtype=np.uint32)
    k = len(out1)
    for r in range(reps):
        first[r * k:(r + 1) * k] = first1[:k].astype(np.int64) + r * len(block)
    want = (out1 * reps, first, tot1 * np.uint64(reps))
    check_case(torch, hb, what="72,380 positions", want=want, parse_back=False)


def test_order_entries_past_n_and_repeated(torch):
    """An entry >= n is an empty position between two runs; a repeated entry is a duplicate,
    which does not link."""
    hb, _ = rm.fragmented([fm.udp4(1700, ident=1), fm.udp6(1600), fm.udp4(1200, ident=2), fm.udp4(40)], 576)
    n = hb.n
    assert n == 12
    order = [0, 1, n, 2, 3, 3, 0xffffffff, 4, 5, 0, 1, n + 7]
    want = rm.reassemble(hb, sm.oracle_records(hb), order)
    assert b"" in want[0] and int(want[2][0]) < n
    check_case(torch, hb, order=order, what="order", want=want, out_bytes=int(want[2][1]) + 9)


@pytest.mark.parametrize("stride", [1104, 1101])
def test_strided_input(torch, stride):
    """frame_len < stride, at strides that are and are not a multiple of 16: fragments of equal
    length (the middle ones of big datagrams) and their padded last ones."""
    src = [fm.udp4(4000, ident=k) if k % 2 else fm.udp6(3980) for k in range(24)]
    hb0, _ = rm.fragmented(src, 1000, False, 5)
    fr = sm.frames_of(hb0)
    flen = max(len(f) for f in fr)
    assert flen < stride
    buf = np.full(len(fr) * stride + 16, 0xee, dtype=np.uint8)
    for k, f in enumerate(fr):
        buf[k * stride:k * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    hb = gen.HostBatch(0, len(fr), 0, buf, None, stride, flen)
    out, first, totals = check_case(torch, hb, what="stride %d" % stride)
    assert int(totals[0]) == len(src) and out == src               # the padding is not carried


def test_default_sizes_come_from_the_documented_bound(torch):
    """engine.reassemble_batch with no outputs given: out_cap = n, out_bytes = frames_bytes."""
    hb = sm.pack(hand_fragments(576))
    out, first, totals = rm.reassemble(hb, sm.oracle_records(hb))
    db = engine.DeviceBatch.from_host(hb)
    odb, gs, gt = engine.reassemble_batch(db, engine.parse_batch(db, sm.F6))
    assert odb.n == hb.n and odb.frames.numel() == hb.frames.size >= int(totals[1])
    assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), first)
    blob, offs = sm.packed_output(out, odb.n)
    assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)


def test_graph_capture(torch):
    """Parse, keys, reassemble under a given order tensor, parse of the output over out_cap slots,
    captured as one graph and replayed on two inputs: no host step between the four."""
    rng = np.random.RandomState(3)
    hbs, orders, wants, keys = [], [], [], []
    for s in (0, 1):
        src = [datagram(k + s, 600 + 200 * ((k + s) % 5)) for k in range(40)]
        hb, _ = rm.fragmented(src, 300, False, 50 + s)
        fr = sm.frames_of(hb)
        hb = sm.pack([fr[k] for k in rng.permutation(len(fr))] + [b""] * (210 - len(fr)))
        assert hb.n == 210
        recs = sm.oracle_records(hb)
        keys.append(rm.keys(hb, recs))
        orders.append(rm.order_of(keys[-1]))
        wants.append(rm.reassemble(hb, recs, orders[-1]))
        hbs.append(hb)
    assert wants[0][2][1] != wants[1][2][1]
    n = 210
    size = max(hb.frames.size for hb in hbs) + 16
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    gkeys = torch.zeros(n, dtype=torch.int64, device="cuda")
    db = engine.DeviceBatch(frames, n, offsets)
    recs, orecs = engine.alloc_records(n), engine.alloc_records(out_cap)
    o = Outputs(torch, n, out_cap, out_bytes)

    def load(k):
        hb = hbs[k]
        frames.zero_()
        frames[:hb.frames.size].copy_(torch.from_numpy(hb.frames.copy()))
        offsets.copy_(torch.from_numpy(hb.offsets.view(np.int32).copy()))
        order.copy_(device_order(torch, orders[k]))

    def fn():
        engine.parse_batch(db, sm.F6, recs=recs)
        engine.reassemble_keys(db, recs, keys=gkeys)
        odb, _, _ = o.call(db, recs, order)
        engine.parse_batch(odb, sm.F6, recs=orecs)

    load(0)
    loop = graphs.CapturedLoop(fn)
    for k in (1, 0, 1):
        load(k)
        o.frames.fill_(0xa5)
        loop.replay()
        torch.cuda.synchronize()
        out, first, totals = wants[k]
        gf, go, gs, gt = o.host()
        blob, offs = sm.packed_output(out, out_cap)
        assert np.array_equal(gkeys.cpu().numpy().view(np.uint64), keys[k])
        assert list(gt[:2]) == [int(totals[0]), int(totals[1])] and np.array_equal(gs[:n + 1], first)
        assert np.array_equal(go[:out_cap + 1], offs) and np.array_equal(gf[:blob.size], blob)
        assert (gf[blob.size:] == 0xa5).all()
        w = oracle.parse_batch(blob, out_cap, sm.F6, offsets=offs)
        assert as_records(orecs.cpu().numpy()).tobytes() == w.tobytes()


def test_cpp_vtep_frag_rx_through_c_abi(torch):
    """examples/vtep_frag_rx: VXLAN around 1500-byte inner frames, fragmented at 1500, the
    fragments reversed, ordered by the keys, reassembled and decoded through the C ABI only; the
    example checks every inner record."""
    import subprocess
    from rpkt_amd.build import VTEP_FRAG_RX_BIN
    r = subprocess.run([VTEP_FRAG_RX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: 6 frames reassembled" in r.stdout


def test_engine_refuses_bad_arguments(torch):
    a, b = fm.ip4(fm.payload_bytes(16), frag=fm.MF), fm.ip4(fm.payload_bytes(9), frag=2)
    hb = sm.pack([a, b])
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, 3)
    with pytest.raises(engine.RpktError):
        engine.reassemble_batch(db, recs, out_cap=0, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.reassemble_batch(db, recs[:80])
    with pytest.raises(engine.RpktError):
        engine.reassemble_batch(db, recs, order=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(engine.RpktError):
        engine.reassemble_batch(db, recs, order=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(engine.RpktError):
        engine.reassemble_batch(db, recs, out_frames=torch.zeros(16, dtype=torch.uint8, device="cuda"),
                                out_bytes=64)
    with pytest.raises(engine.RpktError):
        engine.reassemble_keys(db, recs, keys=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(engine.RpktError):
        engine.reassemble_keys(db, recs[:80])
    odb, first, totals = engine.reassemble_batch(db, recs)
    assert totals.cpu().tolist() == [1, 34 + 25] and first.cpu().tolist() == [0, 2, 2]
