"""GPU parity of rpkt_gpu_coalesce_batch with RPKT_COALESCE_UDP: the output frames, offsets,
src_first, out_mss and totals byte for byte against tests/udp_reframe_model.py, with every
output pre-filled with 0xa5 and followed by guard elements that must stay 0xa5, the inputs
unchanged by the call, and the GPU's parse of the GPU's output equal to the oracle's parse of
the model's."""
import functools

import numpy as np
import pytest

from rpkt_amd import engine, gen
from rpkt_amd.records import F_FLOW_EV

import coalesce_model as cm
import reframe_check as rc
import segment_model as sm
import udp_reframe_model as um

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def check_case(torch, hb, order=None, max_payload=65535, trust_sums=False, udp=True, out_cap=None,
               out_bytes=None, what="", want=None):
    """One call on hb against the model; returns the model's (out_frames, src_first, totals,
    out_mss).  out_cap / out_bytes default to a little more than the totals."""
    if want is None:
        want = um.coalesce(hb, sm.oracle_records(hb), order, max_payload, trust_sums, udp)
    out, first, totals, mss = want
    n = hb.n
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, sm.F6)
    dorder = None
    if order is not None:
        dorder = torch.from_numpy(np.asarray(order, dtype=np.uint32).view(np.int32).copy()).cuda()
    f0, r0 = db.frames.clone(), recs.clone()
    o = rc.Outputs(torch, n, out_cap, out_bytes, functools.partial(engine.coalesce_batch, udp=udp),
                   engine.coalesce_workspace(n), "src_first", (("out_mss", n, torch.int16),))
    odb, _, _ = o.call(db, recs, dorder, max_payload, trust_sums)
    torch.cuda.synchronize()
    assert torch.equal(db.frames, f0) and torch.equal(recs, r0), "%s: the inputs were written" % what
    gm = o.host()[3]
    assert np.array_equal(gm[:n], mss), "%s: out_mss at %d" % (what, rc.first_diff(gm[:n], mss))
    assert (gm[n:] == 0xa5a5).all(), what
    rc.check_outputs(o, odb, out, first, totals, what)
    return want


def members(want):
    """The number of positions in each output."""
    _, first, totals, _ = want
    return np.diff(first[:int(totals[0]) + 1].astype(np.int64)).tolist()


# ---- hand positions ----------------------------------------------------------------------

def run(sizes, sport=5000, ident=100, salt=0, **kw):
    """Datagrams of one flow with the given payload sizes, idents running on."""
    return [um.udp4(sm.payload_bytes(p, salt + k), ident=(ident + k) & 0xffff, sport=sport, **kw)
            for k, p in enumerate(sizes)]


def run6(sizes, sport=5000, salt=0, **kw):
    return [um.udp6(sm.payload_bytes(p, salt + k), sport=sport, **kw) for k, p in enumerate(sizes)]


def corrupt(f):
    f = bytearray(f)
    f[-1] ^= 0x40
    return bytes(f)


def other_vlan(f):
    f = bytearray(f)
    f[15] ^= 0x01                                                  # the tag's VLAN id
    return bytes(f)


def zero_sum_run(mss=100):
    """The segments of a datagram whose own checksum computes to 0: the merged output's does."""
    f = um.zero_sum_datagram(lambda pay: um.udp4(pay, sport=7000, ident=9), 3 * mss + 20, lambda f: 34)
    hb = sm.pack([f])
    return um.segment(hb, sm.oracle_records(hb), mss, True)[0], f


def hop(b):
    return (0, bytes([0, 0, 1, 4, 0, 0, 0, b]))


# name -> (frames, arguments, the positions in each output)
def cases():
    r = sm.routing
    z, zf = zero_sum_run()
    long_flow = [um.udp4(sm.payload_bytes(1448, k), ident=k, sport=7100) for k in range(50)]
    return {
        "equal sizes ending in a shorter one": (run([500, 500, 500, 200]) + run([500, 500], 5001), {}, [4, 2]),
        "a larger one does not join": (run([500, 500, 700]), {}, [2, 1]),
        "two successive shrinking ones": (run([500, 400, 300]), {}, [2, 1]),
        "ident not running on, DF clear": (run([500], ident=1) + run([500], ident=3), {}, [1, 1]),
        "DF set: ident ignored": (run([500], ident=1, df=True) + run([500, 500], ident=7, df=True), {}, [3]),
        "ident wraps": (run([500, 500, 500], ident=0xfffe), {}, [3]),
        "a zero checksum in mid-run": (
            run([500], ident=1) + run([500], ident=2, zero_csum=True) + run([500, 500], ident=3), {}, [1, 1, 2]),
        "a zero checksum, trusted sums": (
            run([500], ident=1) + run([500], ident=2, zero_csum=True) + run([500, 500], ident=3),
            {"trust_sums": True}, [1, 1, 2]),
        "a corrupt checksum": (
            run([500], ident=1) + [corrupt(run([500], ident=2)[0])] + run([500, 500], ident=3), {}, [1, 1, 2]),
        "a corrupt checksum, trusted sums": (
            run([500], ident=1) + [corrupt(run([500], ident=2)[0])] + run([500, 500], ident=3),
            {"trust_sums": True}, [4]),
        "another port": (run([500], ident=1) + run([500], 5001, ident=2), {}, [1, 1]),
        "another TTL": (run([500], ident=1) + run([500], ident=2, ttl=63), {}, [1, 1]),
        "another tag": (run([500], ident=1, tags=1) + [other_vlan(run([500], ident=2, tags=1)[0])], {}, [1, 1]),
        "the same tag": (run([500, 500], tags=1), {}, [2]),
        "another extension header byte": (
            run6([500], exts=(hop(0),)) + run6([500], exts=(hop(1),)) + run6([500], exts=(hop(1),)), {}, [1, 2]),
        "a TCP frame between": (
            run([500], ident=1) + [sm.tcp4(sm.payload_bytes(500, 1))] + run([500], ident=2), {}, [1, 1, 1]),
        "max_payload cuts a group": (run([500] * 6), {"max_payload": 1200}, [2, 2, 2]),
        "the 65,535 limit cuts a group": (long_flow, {}, [45, 5]),
        "the checksum-zero merged output": (z, {}, [len(z)]),
        "IPv6 with a moved pseudo destination": (
            run6([300, 300, 100], exts=(sm.hop_by_hop(), r(0, 2, 1))) + run6([300, 300], 5001, exts=(r(4, 3, 2),)),
            {}, [3, 2]),
        "IPv4 and IPv6 neighbours": (run([300, 300]) + run6([300, 300]), {}, [2, 2]),
    }


CASES = sorted(cases())


@pytest.fixture(scope="module")
def hand_cases():
    return cases()


@pytest.mark.parametrize("name", CASES)
def test_hand_positions(torch, hand_cases, name):
    frames, kw, groups = hand_cases[name]
    for lead in (0, 7):
        hb = sm.pack(frames, lead)
        want = check_case(torch, hb, what="%s, lead %d" % (name, lead), **kw)
        assert members(want)[1 if lead else 0:] == groups, name
    if name == "the checksum-zero merged output":
        z, f = zero_sum_run()
        assert want[0][-1] == f and f[40:42] == b"\xff\xff"


def test_flag_clear_is_the_tcp_rule(torch, hand_cases):
    """Without the flag no UDP datagram merges: coalesce_model's output."""
    frames = [f for name in CASES for f in hand_cases[name][0]]
    frames += um.segment(sm.pack(um.hand_frames(17)), sm.oracle_records(sm.pack(um.hand_frames(17))), 17, True)[0]
    hb = sm.pack(frames, 3)
    plain = cm.coalesce(hb, sm.oracle_records(hb))
    want = check_case(torch, hb, udp=False, what="flag clear")
    assert want[0] == plain[0] and np.array_equal(want[1], plain[1]) and np.array_equal(want[3], plain[3])
    assert int(check_case(torch, hb, what="flag set")[2][0]) < int(plain[2][0])


# ---- order -------------------------------------------------------------------------------

def interleaved():
    """Three UDP streams and a TCP one cut at 700 and interleaved round robin."""
    src = [um.udp4(sm.payload_bytes(9000 + 13 * s, s), sport=5000 + 7 * s, ident=0xfff8 + s) for s in range(3)]
    src.append(sm.tcp4(sm.payload_bytes(9039, 3), seq=0xfffff003, ident=0xfffb, flags=sm.ACK))
    per = []
    for f in src:
        hb = sm.pack([f])
        per.append(um.segment(hb, sm.oracle_records(hb), 700, True)[0])
    assert all(len(p) == 13 for p in per)
    return src, sm.pack([per[k % 4][k // 4] for k in range(52)])


def test_interleaved_flows_with_flow_order(torch):
    """Nothing merges in arrival order; under engine.flow_order of the GPU's flow events every
    stream, UDP and TCP, comes back whole."""
    src, hb = interleaved()
    want = check_case(torch, hb, what="interleaved, arrival order")
    assert int(want[2][0]) == hb.n
    db = engine.DeviceBatch.from_host(hb)
    _, ev = engine.parse_batch(db, sm.F6 | F_FLOW_EV, n_buckets=4096)
    order = engine.flow_order(ev).cpu().numpy().view(np.uint32)
    assert np.array_equal(order, cm.flow_order_host(hb))
    want = check_case(torch, hb, order=order, what="interleaved, flow order")
    assert sorted(want[0]) == sorted(src)


def test_order_with_entries_past_n_and_repeats(torch):
    """An entry >= n is an empty frame that ends a run; a frame named twice is read twice."""
    frames = run([400, 400, 400, 100]) + run([300, 300], 5001) + run([200, 200], 5002)
    hb = sm.pack(frames, 5)                                        # frame 0 is the junk frame
    n = hb.n
    assert n == 9
    want = check_case(torch, hb, order=[1, 2, n, 3, 4, 0xffffffff, 5, 6, 0], what="entries >= n")
    assert members(want) == [2, 1, 2, 1, 2, 1] and want[0][1] == want[0][3] == b""
    want = check_case(torch, hb, order=[1, 2, 2, 3, 4, 1, 5, 6, 6], what="a non-permutation")
    assert members(want) == [2, 3, 1, 2, 1]


# ---- round trip, capacities ----------------------------------------------------------------

@pytest.mark.parametrize("mss", [7, 536, 1448])
def test_round_trip_on_the_device(torch, mss):
    """coalesce_batch(segment_batch(F, udp), udp) returns F's bytes; out_mss is the mss, and a
    second segment_batch at that value reproduces the segments."""
    F = um.round_trip_frames(mss)
    hb = sm.pack(F)
    db = engine.DeviceBatch.from_host(hb)
    n_seg = sum(-(-(len(f) - 42) // mss) for f in F) + 64         # at least the segments of all
    sdb, seg_first, stot = engine.segment_batch(db, engine.parse_batch(db, sm.F6), mss, udp=True,
                                                out_cap=n_seg, out_bytes=hb.frames.size + n_seg * 134)
    out_mss = torch.zeros(sdb.n, dtype=torch.int16, device="cuda")
    cdb, src_first, ctot = engine.coalesce_batch(sdb, engine.parse_batch(sdb, sm.F6), udp=True,
                                                 out_mss=out_mss)
    torch.cuda.synchronize()
    n_out = int(stot[0])
    assert n_out <= sdb.n and int(stot[1]) <= sdb.frames.numel()
    spare = sdb.n - n_out
    want = F + [b""] * spare
    assert ctot.cpu().tolist() == [len(want), sum(len(f) for f in want)]
    blob, offs = sm.packed_output(want, cdb.n)
    assert np.array_equal(cdb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(cdb.frames.cpu().numpy()[:blob.size], blob)
    assert torch.equal(src_first[:len(F) + 1], seg_first)
    assert out_mss[:len(F)].cpu().tolist() == [mss] * len(F)
    # again at out_mss's value: the same segments
    back = engine.DeviceBatch(cdb.frames, len(F), cdb.offsets[:len(F) + 1].clone())
    sdb2, _, stot2 = engine.segment_batch(back, engine.parse_batch(back, sm.F6), int(out_mss[0]), udp=True,
                                          out_cap=n_seg, out_bytes=hb.frames.size + n_seg * 134)
    torch.cuda.synchronize()
    assert torch.equal(stot2, stot)
    assert torch.equal(sdb2.offsets[:n_out + 1], sdb.offsets[:n_out + 1])
    assert torch.equal(sdb2.frames[:int(stot[1])], sdb.frames[:int(stot[1])])


@pytest.fixture(scope="module")
def config11():
    hb0 = gen.make_batch(11, 4096)
    hb = sm.pack(um.segment(hb0, sm.oracle_records(hb0), 300, True)[0])
    want = um.coalesce(hb, sm.oracle_records(hb), udp=True)
    assert int((want[3] != 0).sum()) >= 3000
    return hb, want


def test_config_11_segments(torch, config11):
    hb, want = config11
    check_case(torch, hb, what="config 11", want=want)


def test_exact_capacities(torch, config11):
    hb, want = config11
    check_case(torch, hb, out_cap=int(want[2][0]), out_bytes=int(want[2][1]), what="exact", want=want)


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, config11, short):
    """Capacities below the totals: src_first, out_mss and totals exact, nothing written."""
    hb, want = config11
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hb, out_cap=cap, out_bytes=nbytes, what="overflow " + short, want=want)
