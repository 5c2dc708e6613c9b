"""GPU parity of rpkt_gpu_parse_tunnel_next (nested tunnels): the next level's tunnel and
inner records, byte for byte, against tests/nested_tunnel_ref.py (a composition of
oracle.tunnel_batch), with the level-1 inputs taken from engine.parse_tunnel_batch on the
same device batch.  Every check also holds the level-k records unchanged by the call."""
import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen
from rpkt_amd.records import (F_FLOW_EV, F_IPV6, REC_DTYPE, STATUS, TUN_KIND, TUN_STATUS,
                              as_records, as_tunnels)

import nested_tunnel_ref as ref
import tunnel_frames as tf

pytestmark = pytest.mark.gpu
F6 = 3 | F_IPV6


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def same_records(g, w, what):
    if g.tobytes() == w.tobytes():
        return
    bad = np.nonzero(g.view(np.uint8).reshape(-1, 80) != w.view(np.uint8).reshape(-1, 80))[0]
    k = int(bad[0])
    fields = [f for f in REC_DTYPE.names if not np.array_equal(g[k][f], w[k][f])]
    raise AssertionError("%s: %d inner records differ; first #%d fields %s gpu=%s want=%s" % (
        what, len(np.unique(bad)), k, fields, [g[k][f] for f in fields], [w[k][f] for f in fields]))


def same_tunnels(g, w, what):
    if g.tobytes() == w.tobytes():
        return
    k = int(np.nonzero(g != w)[0][0])
    raise AssertionError("%s: %d tunnel records differ; first #%d gpu=%s want=%s" % (
        what, int((g != w).sum()), k, g[k], w[k]))


def next_on_gpu(torch, db, tun, inner, flags, **kw):
    """One next-level call into pre-filled outputs (a record the kernel did not write shows);
    the inputs must come back unchanged."""
    t0, i0 = tun.clone(), inner.clone()
    tn = torch.full((db.n * 16,), 0xa5, dtype=torch.uint8, device=tun.device)
    inn = torch.full((db.n * 80,), 0xa5, dtype=torch.uint8, device=tun.device)
    engine.parse_tunnel_next(db, tun, inner, flags, tn, inn, **kw)
    assert torch.equal(tun, t0) and torch.equal(inner, i0), "the level-k records were written"
    return tn, inn


def check_next(torch, hb, flags, depth=2, what=""):
    """Levels 2..depth of hb on the GPU against next_level on the level before's GPU records.
    Returns the last level's (tun, inner) as numpy records."""
    db = engine.DeviceBatch.from_host(hb)
    _, gt, gi = engine.parse_tunnel_batch(db, flags)
    for lv in range(2, depth + 1):
        tn, inn = next_on_gpu(torch, db, gt, gi, flags)
        wt, wi = ref.next_level(hb, flags, as_tunnels(gt.cpu().numpy()), as_records(gi.cpu().numpy()))
        same_tunnels(as_tunnels(tn.cpu().numpy()), wt, "%s flags %d level %d" % (what, flags, lv))
        same_records(as_records(inn.cpu().numpy()), wi, "%s flags %d level %d" % (what, flags, lv))
        gt, gi = tn, inn
    return wt, wi


def coverage(t2, i2, flags):
    assert set(np.unique(t2["status"])) == set(TUN_STATUS.values())
    assert len(np.unique(i2["status"])) >= 8
    if flags & F_IPV6:
        assert (t2["status"] == TUN_STATUS["OK"]).mean() >= 0.40


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_frames_and_their_cuts(torch, lead):
    """The three hand-built frames and their cuts at every byte (the innermost frame, the
    second tunnel's header and payload, the level-1 inner frame: nested_tunnel_ref.hand_cuts),
    at every 16-B phase."""
    hb = ref.pack(ref.hand_frames() + ref.hand_cuts(), lead)
    k = 1 if lead else 0
    for flags in (0, 1, 2, 3, F6):
        t2, i2 = check_next(torch, hb, flags, what="lead %d" % lead)
        assert list(t2["tun_off"][k:k + 2]) == [92, 70] and list(t2["inner_off"][k:k + 2]) == [100, 78]
    assert list(t2["kind"][k:k + 3]) == [TUN_KIND["GTPU"], TUN_KIND["VXLAN"], TUN_KIND["GRE"]]
    assert (t2["tun_off"][k + 2], t2["inner_off"][k + 2]) == (110, 118)
    assert (i2["status"][k:k + 3] == 0).all() and (i2["l4_sum"][k:k + 3] == 0xffff).all()
    assert len(np.unique(t2["status"])) >= 3 and len(np.unique(i2["status"])) >= 5


@pytest.mark.parametrize("seed", [14, 1401])
def test_nested_fuzz(torch, seed):
    hb = ref.nested_frames(14, 4096, seed)
    for flags in (3, F6, 1):
        t2, i2 = check_next(torch, hb, flags, what="seed %d" % seed)
        coverage(t2, i2, flags)


def test_ragged_and_early_exit_tiles(torch):
    """Batch sizes around the 64-frame tile, and a 192-frame batch whose middle tile holds
    only single-level frames (the wave-uniform exit) between two tiles that do not."""
    for n in (1, 63, 64, 65, 130):
        check_next(torch, ref.nested_frames(14, n, seed=n), F6, what="n %d" % n)
    fr = ref.frames_of(gen.make_batch(14, 192, seed=192))
    frames = [f if 64 <= k < 128 else ref.wrap(k % 5, f) for k, f in enumerate(fr)]
    for lead in (0, 5):
        t2, i2 = check_next(torch, ref.pack(frames, lead), F6, what="middle tile")
        mid = slice(64 + (1 if lead else 0), 128 + (1 if lead else 0))
        if not lead:
            assert (t2["kind"][mid] == TUN_KIND["NONE"]).all()
            assert (i2["status"][mid] == STATUS["NO_INNER"]).all()
        assert (t2["status"][:64] == TUN_STATUS["OK"]).any() and (t2["status"][130:] == TUN_STATUS["OK"]).any()
    t2, i2 = check_next(torch, ref.pack(fr), F6, what="single-level")   # no nested frame at all
    assert (t2["kind"] == TUN_KIND["NONE"]).all() and (i2["status"] == STATUS["NO_INNER"]).all()


PAYLOADS = [0, 1] + list(range(113, 130)) + [1400, 1401, 8900, 8901, 59981]


@pytest.mark.parametrize("lead", [0, 7])
def test_deep_inner_frames_and_long_payloads(torch, lead):
    """Second tunnels that start past the outer header window (IPv6 outer with three
    extension headers, a GTP-U chain of three: level-1 inner packet at byte 166), innermost
    payloads from 0 to 59,981 B (the stream past the innermost window, odd lengths), and
    tests/tunnel_frames.py's odd shapes (IPv6 / QinQ, long GTP-U chains, cuts and flips) as
    the second level."""
    frames = []
    for p in PAYLOADS:
        frames += [ref.deep_frame(p)] + ref.hand_frames(p)
    hb = ref.pack(frames, lead)
    for flags in (3, 1, F6):
        t2, i2 = check_next(torch, hb, flags, what="payloads, lead %d" % lead)
    k = 1 if lead else 0
    assert int(t2["tun_off"][k]) == 166 + 28 and int(t2["kind"][k]) == TUN_KIND["VXLAN"]
    assert (t2["status"][k:] == TUN_STATUS["OK"]).all() and (i2["status"][k:] == STATUS["OK"]).all()
    assert (i2["l4_sum"][k:] == 0xffff).all() and (i2["ip_sum"][k:] == 0xffff).all()
    assert int(i2["payload_len"].max()) == 59981
    # whole tiles of mid-size and of long innermost payloads (40 KB and 90 KB streamed per tile)
    mid = [ref.hand_frames(600 + 3 * k)[k % 3] for k in range(130)]
    mid += [ref.hand_frames(1200 + 5 * k)[k % 3] for k in range(70)]
    t2, i2 = check_next(torch, ref.pack(mid, lead), F6, what="mid-size tiles")
    assert (t2["status"][k:] == TUN_STATUS["OK"]).all() and (i2["l4_sum"][k:] == 0xffff).all()
    odd = [ref.wrap(k, f) for k, f in enumerate(tf.odd_frames(seed=lead, n=192))]
    for flags in (3, F6):
        t2, i2 = check_next(torch, ref.pack(odd, lead), flags, what="odd shapes")
    assert set(np.unique(t2["kind"])) == set(TUN_KIND.values())
    assert TUN_STATUS["EXT_BAD"] in t2["status"]               # the chain of 9 extension headers


@pytest.mark.parametrize("lead", [0, 3])
def test_three_levels(torch, lead):
    """VXLAN in GRE in GTP-U: the entry applied to its own output, each level against
    next_level; engine.parse_tunnel_levels gives the same, with its own tensors per level and
    ping-ponging between two."""
    hb = ref.pack(ref.three_level_frames(), lead)
    k = 1 if lead else 0
    for flags in (3, F6):
        t3, i3 = check_next(torch, hb, flags, depth=3, what="three levels")
    assert (t3["kind"][k:] == TUN_KIND["VXLAN"]).all() and (t3["status"][k:] == TUN_STATUS["OK"]).all()
    assert (i3["status"][k:] == STATUS["OK"]).all() and (i3["l4_sum"][k:] == 0xffff).all()
    t4, i4 = check_next(torch, hb, F6, depth=4)
    assert (t4["status"] == TUN_STATUS["NONE"]).all()
    db = engine.DeviceBatch.from_host(hb)
    outer, levels = engine.parse_tunnel_levels(db, F6, depth=3)
    assert len(levels) == 3
    assert as_tunnels(levels[2][0].cpu().numpy()).tobytes() == t3.tobytes()
    assert as_records(levels[2][1].cpu().numpy()).tobytes() == i3.tobytes()
    bufs = [(torch.empty(db.n * 16, dtype=torch.uint8, device="cuda"), engine.alloc_records(db.n))
            for _ in range(2)]
    outer2, last = engine.parse_tunnel_levels(db, F6, depth=3, buffers=bufs)
    assert torch.equal(outer, outer2) and last[-1][0] is bufs[0][0]
    assert as_records(last[-1][1].cpu().numpy()).tobytes() == i3.tobytes()


@pytest.mark.parametrize("n,nb", [(4096, 977), (333, 1)])
def test_flow_events(torch, n, nb):
    """RPKT_F_FLOW_EV: the level-1 call's event buffer handed on.  Events of frames whose
    second tunnel decoded are the innermost record's; all others are bit for bit what level
    1 wrote; rpkt_gpu_flow_count over them equals the oracle's counters of the expected
    events; the records are those of the call without events."""
    hb = ref.nested_frames(14, n, seed=14)
    db = engine.DeviceBatch.from_host(hb)
    go, gt, gi, ev = engine.parse_tunnel_batch(db, F6 | F_FLOW_EV, n_buckets=nb)
    ev1 = ev.cpu().numpy().view(np.uint64).copy()
    o, t, i = (as_records(go.cpu().numpy()), as_tunnels(gt.cpu().numpy()), as_records(gi.cpu().numpy()))
    assert np.array_equal(ev1, oracle.tunnel_flow_events(o, t, i, nb))
    tn, inn = next_on_gpu(torch, db, gt, gi, F6 | F_FLOW_EV, flow_ev=ev, n_buckets=nb)
    wt, wi, sub = ref.next_level(hb, F6, t, i, with_sub=True)
    same_tunnels(as_tunnels(tn.cpu().numpy()), wt, "with events")
    same_records(as_records(inn.cpu().numpy()), wi, "with events")
    want = ref.expected_events(ev1, sub, nb)
    got = ev.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
    ok = wt["status"] == TUN_STATUS["OK"]
    assert np.array_equal(got[~ok], ev1[~ok]) and ok.mean() >= 0.40
    c = engine.flow_count(ev, hb.n, nb).cpu().numpy().view(np.uint64)
    assert np.array_equal(c, oracle.flow_count(want, nb))
    tn2, inn2 = next_on_gpu(torch, db, gt, gi, F6)
    assert torch.equal(tn, tn2) and torch.equal(inn, inn2)


def test_strided_layout(torch):
    """Frames of one length at a stride (frame_len < stride, strides that are and are not a
    multiple of 16) against the packed run of the same frames."""
    a, _, _ = ref.hand_frames(272)
    _, b, _ = ref.hand_frames(280)
    _, _, c = ref.hand_frames(254)
    assert len(a) == len(b) == len(c) == 400
    frames = [(a, b, c)[k % 3] for k in range(150)]
    wt, wi = check_next(torch, ref.pack(frames), F6, what="packed")
    assert (wt["status"] == TUN_STATUS["OK"]).all()
    for stride in (432, 437):
        buf = np.full(len(frames) * stride + 16, 0xee, dtype=np.uint8)
        for k, f in enumerate(frames):
            buf[k * stride:k * stride + 400] = np.frombuffer(f, dtype=np.uint8)
        hb = gen.HostBatch(0, len(frames), 0, buf, None, stride, 400)
        st, si = check_next(torch, hb, F6, what="stride %d" % stride)
        assert st.tobytes() == wt.tobytes() and si.tobytes() == wi.tobytes()


def test_empty_batch_and_validation(torch):
    hb = ref.pack(ref.hand_frames())
    db = engine.DeviceBatch.from_host(hb)
    _, gt, gi = engine.parse_tunnel_batch(db, 3)
    with pytest.raises(engine.RpktError):
        engine.parse_tunnel_next(db, gt, gi, 3 | 16)                     # an unknown flag
    with pytest.raises(engine.RpktError):
        engine.parse_tunnel_next(db, gt, gi, 3, tun_next=gt)             # output aliases input
    with pytest.raises(engine.RpktError):
        engine.parse_tunnel_next(db, gt, gi, 3 | F_FLOW_EV, n_buckets=4)   # no event buffer
    db.n = 0
    engine.parse_tunnel_next(db, gt, gi, 3)                              # n == 0: nothing launched
