"""GPU parity of rpkt_gpu_coalesce_tunnel_batch: the output frames, offsets, src_first, out_mss
and totals byte for byte against tests/coalesce_tunnel_model.py, every output pre-filled with
0xa5 and followed by guard elements that must stay 0xa5, the inputs unchanged by the call, and
the GPU's tunnel parse of the GPU's output equal to the oracle's tunnel parse of the model's."""
import functools
import subprocess

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import F_FLOW_EV, as_records, as_tunnels

import coalesce_tunnel_model as ctm
import reframe_check as rc
import segment_model as sm
import segment_tunnel_model as stm
import tunnel_frames as tf
import udp_reframe_model as um

pytestmark = pytest.mark.gpu

K_SEG_BLOCK = 256                              # positions a plan block (rpkt_segcopy.h kSegBlock)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, fn=engine.coalesce_tunnel_batch,
            ws=engine.coalesce_tunnel_workspace, **kw):
    return rc.Outputs(torch, n, out_cap, out_bytes, functools.partial(fn, **kw), ws(n), "src_first",
                      extra=(("out_mss", n, torch.int16),))


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


def check_case(torch, hb, want=None, order=None, max_payload=65535, trust=False, udp=False,
               out_cap=None, out_bytes=None, what="", parse=True, records=None):
    """One call on hb against the model's `want` = (out_frames, src_first, totals, out_mss)
    (None: the model on the oracle's records).  out_cap / out_bytes default to a little more
    than the totals; smaller ones overflow.  Returns want."""
    if want is None:
        want = ctm.coalesce(hb, *stm.tunnel_records(hb), order, max_payload, trust, udp)
    out, first, totals, mss = want
    n = hb.n
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, sm.F6) if records is None else records
    dorder = None if order is None else torch.from_numpy(np.asarray(order, dtype=np.uint32).view(np.int32).copy()).cuda()
    ins = (db.frames,) + tuple(recs) + (() if dorder is None else (dorder,))
    before = [t.clone() for t in ins]
    o = Outputs(torch, n, out_cap, out_bytes, max_payload=max_payload, trust_sums=trust, udp=udp)
    odb, _, _ = o.call(db, *recs, dorder)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, before)), "%s: the inputs were written" % what
    fits = rc.check_outputs(o, odb, out, first, totals, what, parse_back=False)
    gm = o.host()[3]
    assert np.array_equal(gm[:n], mss), "%s: out_mss at %d" % (what, rc.first_diff(gm[:n], mss))
    assert (gm[n:] == 0xa5a5).all(), "%s: out_mss past n written" % what
    if fits and parse:
        parse_back(odb, out, out_cap, what)
    return want


def with_lead(want, lead):
    """The model's output for the same positions behind a `lead`-byte junk frame."""
    if not lead:
        return want
    out, first, totals, mss = want
    return ([b"\xee" * lead] + out, np.concatenate([[0], first + 1]).astype(np.uint32),
            totals + np.array([1, lead], dtype=np.uint64), np.concatenate([[0], mss]).astype(np.uint16))


@pytest.fixture(scope="module")
def hand():
    """(mss, udp) -> (the hand frames' segments at mss, the model's output for them)."""
    res = {}
    for mss in stm.MSS_VALUES:
        for udp in (False, True):
            hs, recs, _ = ctm.segment_then_records(stm.hand_frames(mss), mss, udp)
            res[mss, udp] = (sm.frames_of(hs), ctm.coalesce(hs, *recs, udp=udp))
    return res


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_segments(torch, hand, lead):
    """The segments of VXLAN, GTP-U and GRE frames over IPv4 and IPv6 around TCP and UDP (tags,
    options, extension headers, GTP-U extension headers, GRE with C and K, a zero outer UDP
    checksum, inner and outer padding, plain frames, undecoded tunnels) at every 16-B source
    phase, with and without RPKT_COALESCE_UDP."""
    for mss in stm.MSS_VALUES:
        for udp in (False, True):
            frames, want = hand[mss, udp]
            check_case(torch, sm.pack(frames, lead), with_lead(want, lead), udp=udp,
                       what="mss %d udp %d lead %d" % (mss, udp, lead))
        # the twelve cut shapes merge back without the flag, the inner and plain UDP with it
        merged = [int((hand[mss, u][1][3] > 0).sum()) for u in (False, True)]
        assert merged[1] > merged[0] >= stm.N_CUT_TCP, (mss, merged)


@pytest.fixture(scope="module")
def config13():
    hb = gen.make_batch(13, n=2048, seed=3)
    return hb, stm.tunnel_records(hb)


@pytest.mark.parametrize("mss,udp", [(536, False), (536, True), (100, True)])
def test_config_13(torch, config13, mss, udp):
    """gen.make_batch(13, n=2048, seed=3) cut in the tunnel and coalesced: the model merges 402 /
    383 / 139 groups of VXLAN / GTP-U / GRE at 536 without the flag and 815 / 829 / 288 with it."""
    hb, recs = config13
    hs = sm.pack(stm.segment(hb, *recs, mss, udp)[0])
    srecs = stm.tunnel_records(hs)
    want = ctm.coalesce(hs, *srecs, udp=udp)
    kinds = ctm.merged_kinds(want[1], want[2][0], srecs[1])
    assert min(kinds[k] for k in (ctm.VXLAN, ctm.GTPU, ctm.GRE)) >= 100, kinds
    check_case(torch, hs, want, udp=udp, what="config 13 mss %d udp %d" % (mss, udp))


def test_config_14_fuzz(torch):
    """Every tunnel status and every parse status at both levels is copied or merged as the
    model says: the fuzzed batch itself and its segments at 300."""
    hb = gen.make_batch(14, n=4096, seed=3)
    recs = stm.tunnel_records(hb)
    assert len(np.unique(recs[1]["status"])) >= 4
    check_case(torch, hb, udp=True, what="config 14")
    hs = sm.pack(stm.segment(hb, *recs, 300, True)[0])
    want = check_case(torch, hs, udp=True, what="config 14 cut at 300")
    assert int(want[2][0]) < hs.n


def stream(p, n_seg, **kw):
    """n_seg segments of p payload bytes each of one VXLAN-wrapped TCP stream."""
    f = tf.ether(0x0800, stm.ip4(17, tf.udp(40000, 4789, tf.vxlan(sm.tcp4(sm.payload_bytes(p * n_seg, 2), **kw)))))
    hs, _, _ = ctm.segment_then_records([f], p)
    return sm.frames_of(hs)


@pytest.mark.parametrize("max_payload", [65535, 3])
def test_a_run_across_plan_blocks(torch, max_payload):
    """2 * kSegBlock + 5 positions of one tunnelled stream with 1-byte payloads and a lone frame
    in each plan block: the heads scan's carry, the greedy cut, the copy's runs of 8 positions
    and the header's runs of 4 outputs."""
    n = 2 * K_SEG_BLOCK + 5
    frames = stream(1, n - 3)
    lone = stm.through_frames(20, 64)[0]                           # GRE with S
    for at in (100, K_SEG_BLOCK + 44, n - 3):
        frames.insert(at, lone)
    assert len(frames) == n
    want = check_case(torch, sm.pack(frames), max_payload=max_payload, what="blocks, max %d" % max_payload)
    sizes = np.diff(want[1][:int(want[2][0]) + 1].astype(np.int64))
    if max_payload == 3:
        assert sizes.max() == 3 and (sizes == 3).sum() > 160
    else:
        assert list(sizes) == [100, 1, 199, 1, 213, 1, 2]


@pytest.mark.parametrize("udp", [False, True])
def test_without_tunnels_the_output_is_coalesce_batch_s(torch, config13, udp):
    """Every tun kind NONE: byte for byte what engine.coalesce_batch writes with the outer
    records."""
    segs = stm.segment(config13[0], *config13[1], 300, True)[0][:1500]
    plain = sm.pack(sm.variety(700) + um.round_trip_frames(536))
    segs += um.segment(plain, sm.oracle_records(plain), 536, True)[0]
    hb = sm.pack(segs)
    db = engine.DeviceBatch.from_host(hb)
    outer, tun, inner = engine.parse_tunnel_batch(db, sm.F6)
    none = np.zeros(hb.n, dtype=as_tunnels(tun.cpu().numpy()).dtype)
    none["status"] = 1
    tun = torch.from_numpy(none.view(np.uint8).copy()).cuda()
    a = Outputs(torch, hb.n, hb.n, hb.frames.size, udp=udp)
    b = Outputs(torch, hb.n, hb.n, hb.frames.size, fn=engine.coalesce_batch,
                ws=engine.coalesce_workspace, udp=udp)
    a.call(db, outer, tun, inner)
    b.call(db, outer)
    torch.cuda.synchronize()
    ga, gb = a.host(), b.host()
    assert 0 < int(gb[4][0]) < hb.n - 10                            # the flat entry merged
    for x, y, name in zip(ga, gb, ("frames", "offsets", "src_first", "out_mss", "totals")):
        assert np.array_equal(x, y), name


def vni_streams():
    """Four VXLAN streams, one VNI and one inner flow each, cut at 700 into 13 segments."""
    src = []
    for s in range(4):
        inner = bytearray(sm.tcp4(sm.payload_bytes(9000 + 13 * s, s), seq=0xfffff000 + s, ident=0xfff8 + s))
        inner[34:36] = (5000 + 7 * s).to_bytes(2, "big")            # the source port, and the sum
        inner[50:52] = b"\0\0"
        pseudo = bytes(inner[26:34]) + b"\0\x06" + (len(inner) - 34).to_bytes(2, "big")
        inner[50:52] = sm.csum_field(pseudo, inner[34:]).to_bytes(2, "big")
        src.append(tf.ether(0x0800, stm.ip4(17, tf.udp(40000 + s, 4789, tf.vxlan(bytes(inner), vni=100 + s)),
                                            ident=0x100 * s)))
    per = [sm.frames_of(ctm.segment_then_records([f], 700)[0]) for f in src]
    assert all(len(p) == 13 for p in per)
    return src, per


def test_interleaved_vnis_with_flow_order(torch):
    """Four tunnelled streams interleaved round robin: nothing merges in arrival order; under
    engine.flow_order of the tunnel parse's flow events (keyed by the inner flow) every stream
    comes back whole."""
    src, per = vni_streams()
    hb = sm.pack([per[k % 4][k // 4] for k in range(52)])
    want = check_case(torch, hb, what="interleaved, arrival order")
    assert int(want[2][0]) == hb.n
    db = engine.DeviceBatch.from_host(hb)
    ev = engine.parse_tunnel_batch(db, sm.F6 | F_FLOW_EV, n_buckets=4096)[3]
    order = engine.flow_order(ev)
    assert order.is_cuda and order.element_size() == 4
    want = check_case(torch, hb, order=order.cpu().numpy().view(np.uint32), what="interleaved, flow order")
    assert sorted(want[0]) == sorted(src)


def test_order_with_empty_positions_and_repeats(torch):
    src, per = vni_streams()
    hb = sm.pack(per[0] + per[1])
    n = hb.n
    order = np.arange(n, dtype=np.uint32)
    order[3], order[7], order[20] = n, 0xffffffff, n + 5            # empty positions
    order[9] = 8                                                    # a repeat
    order[14:18] = [13, 14, 14, 15]
    want = check_case(torch, hb, order=order, out_bytes=hb.frames.size + 4096, what="order")
    assert b"" in want[0] and 3 < int(want[2][0]) < n


def corrupt(frames, at_of):
    out = []
    for f in frames:
        g = bytearray(f)
        g[at_of(f)] ^= 0x40
        out.append(bytes(g))
    return out


def test_trust_sums(torch):
    """A corrupted outer UDP checksum and a corrupted GRE checksum: copied without
    RPKT_COALESCE_TRUST_SUMS, merged with it."""
    cut = stm.cut_frames(300)
    vx = sm.frames_of(ctm.segment_then_records([cut[0]], 100)[0])
    gre = sm.frames_of(ctm.segment_then_records([cut[6]], 100)[0])  # GRE with C and K
    frames = corrupt(vx, lambda f: 14 + 20 + 6) + corrupt(gre, lambda f: 14 + 20 + 4)
    hb = sm.pack(frames)
    want = check_case(torch, hb, what="corrupt, sums required")
    assert int(want[2][0]) == hb.n == 6
    want = check_case(torch, hb, trust=True, what="corrupt, sums trusted")
    assert list(want[1][:3]) == [0, 3, 6] and int(want[2][0]) == 2


def test_exact_capacities(torch, hand):
    frames, want = hand[17, True]
    want = with_lead(want, 5)
    check_case(torch, sm.pack(frames, 5), want, udp=True, out_cap=int(want[2][0]),
               out_bytes=int(want[2][1]), what="exact")


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, hand, short):
    """Capacities below the totals: src_first, out_mss and totals exact, guards intact."""
    frames, want = hand[536, True]
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, sm.pack(frames), want, udp=True, out_cap=cap, out_bytes=nbytes,
               what="overflow " + short)


def test_records_of_another_batch_never_write_outside(torch):
    """The records of a shuffled batch: nothing is asserted about the frames; the guards and the
    0xa5 fill past out_bytes stay intact."""
    hb = gen.make_batch(13, n=1024, seed=5)
    recs0 = stm.tunnel_records(hb)
    frames = stm.segment(hb, *recs0, 300, True)[0][:2048]
    order = np.random.default_rng(7).permutation(len(frames))
    other = engine.DeviceBatch.from_host(sm.pack([frames[k] for k in order]))
    recs = engine.parse_tunnel_batch(other, sm.F6)
    hs = sm.pack(frames)
    db = engine.DeviceBatch.from_host(hs)
    n = hs.n
    for trust, cap, nbytes in ((False, n, hs.frames.size), (True, n, hs.frames.size),
                               (True, n // 2, hs.frames.size // 2)):
        o = Outputs(torch, n, cap, nbytes, trust_sums=trust, udp=True)
        o.call(db, *recs)
        torch.cuda.synchronize()
        gf, go, gs, gm, gt = o.host()
        assert (gf[nbytes:] == 0xa5).all() and (go[cap + 1:] == 0xa5a5a5a5).all()
        assert (gs[n + 1:] == 0xa5a5a5a5).all() and (gt[2:] == 0xa5a5a5a5a5a5a5a5).all()
        assert (gm[n:] == 0xa5a5).all() and 1 <= int(gt[0]) <= n


def round_trip_sources(seed):
    """Cut-eligible tunnel frames whose segments merge back: the hand shapes at two payload
    lengths, which `seed` varies."""
    return stm.cut_frames(1500 + seed) + stm.cut_frames(700 + seed)[:12]


def test_device_only_round_trip(torch):
    """parse_tunnel -> segment_tunnel -> parse_tunnel -> coalesce_tunnel, all on the device,
    gives back the input."""
    src = round_trip_sources(0)
    hb = sm.pack(src)
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, sm.F6)
    seg, _, st = engine.segment_tunnel_batch(db, *recs, 536, udp=True)
    srecs = engine.parse_tunnel_batch(seg, sm.F6)
    out, first, totals = engine.coalesce_tunnel_batch(seg, *srecs, udp=True)
    torch.cuda.synchronize()
    n_seg, need = int(st.cpu()[0]), int(hb.offsets[-1])            # the buffer is padded past it
    assert 2 * hb.n < n_seg <= seg.n
    # the segment entry's spare slots are empty frames at the end: lone, empty outputs
    assert totals.cpu().tolist() == [hb.n + seg.n - n_seg, need]
    offs = out.offsets.cpu().numpy().view(np.uint32)
    assert np.array_equal(offs[:hb.n + 1], hb.offsets)
    assert np.array_equal(out.frames.cpu().numpy()[:need], hb.frames[:need])


def test_graph_capture(torch):
    """The same chain captured as one graph and replayed on two inputs."""
    hbs = [sm.pack(round_trip_sources(s)) for s in (0, 9)]
    n = hbs[0].n
    assert hbs[1].n == n and hbs[0].frames.tobytes() != hbs[1].frames.tobytes()
    size = max(hb.frames.size for hb in hbs) + 16
    seg_cap = n + size // 536
    frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    db = engine.DeviceBatch(frames, n, offsets)
    recs = [engine.alloc_records(n), engine._bytes(n, 16, "cuda"), engine.alloc_records(n)]
    srecs = [engine.alloc_records(seg_cap), engine._bytes(seg_cap, 16, "cuda"), engine.alloc_records(seg_cap)]
    seg = rc.Outputs(torch, n, seg_cap, size + (seg_cap - n) * 272,
                     functools.partial(engine.segment_tunnel_batch, udp=True),
                     engine.segment_tunnel_workspace(n), "seg_first")
    o = Outputs(torch, seg_cap, seg_cap, size + 64, udp=True)

    def load(hb):
        frames.zero_()
        frames[:hb.frames.size].copy_(torch.from_numpy(hb.frames.copy()))
        offsets.copy_(torch.from_numpy(hb.offsets.view(np.int32).copy()))

    def fn():
        engine.parse_tunnel_batch(db, sm.F6, *recs)
        sdb, _, _ = seg.call(db, *recs, 536)
        engine.parse_tunnel_batch(sdb, sm.F6, *srecs)
        o.call(sdb, *srecs)

    load(hbs[0])
    loop = graphs.CapturedLoop(fn)
    for k in (1, 0, 1):
        hb = hbs[k]
        load(hb)
        o.frames.fill_(0xa5)
        loop.replay()
        torch.cuda.synchronize()
        gf, go, gs, gm, gt = o.host()
        # the segment entry's spare slots are empty frames at the end: lone, empty outputs
        n_seg, need = int(seg.totals.cpu()[0]), int(hb.offsets[-1])
        assert list(gt[:2]) == [n + seg_cap - n_seg, need]
        assert np.array_equal(go[:n + 1], hb.offsets) and (go[n + 1:seg_cap + 1] == need).all()
        assert np.array_equal(gf[:need], hb.frames[:need]) and (gf[need:] == 0xa5).all()


def test_cpp_vtep_gro_rx_through_c_abi(torch):
    """examples/vtep_gro_rx: a C++ VTEP (C ABI only) receives the 92 interleaved wire frames of
    vtep_tx's four VXLAN frames and coalesces them back, byte for byte."""
    from rpkt_amd.build import VTEP_GRO_RX_BIN
    r = subprocess.run([VTEP_GRO_RX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "out: 4 frames" in r.stdout and "equal to the sent frames" in r.stdout, r.stdout


def test_engine_refuses_bad_arguments(torch):
    src, per = vni_streams()
    hb = sm.pack(per[0])
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, sm.F6)
    for mp in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.coalesce_tunnel_batch(db, *recs, max_payload=mp)
    with pytest.raises(engine.RpktError):
        engine.coalesce_tunnel_batch(db, *recs, out_cap=0, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.coalesce_tunnel_batch(db, recs[0], recs[1][:16], recs[2])
    with pytest.raises(engine.RpktError):
        engine.coalesce_tunnel_batch(db, *recs, order=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(engine.RpktError):
        engine.coalesce_tunnel_batch(db, *recs, out_mss=torch.zeros(hb.n, dtype=torch.int32, device="cuda")[:1])
    odb, first, totals = engine.coalesce_tunnel_batch(db, *recs)
    assert totals.cpu().tolist() == [1, len(src[0])] and first.cpu().tolist()[:2] == [0, 13]
