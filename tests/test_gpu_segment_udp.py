"""GPU parity of rpkt_gpu_segment_batch and rpkt_gpu_segment_chains with RPKT_SEGMENT_UDP:
the output frames, offsets, seg_first and totals byte for byte against
tests/udp_reframe_model.py, with every output pre-filled with 0xa5 and followed by guard
elements that must stay 0xa5, the inputs unchanged by the call, and the GPU's parse of the
GPU's output equal to the oracle's parse of the model's."""
import functools

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records

import reframe_check as rc
import segment_chains_model as scm
import segment_model as sm
import udp_reframe_model as um

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, udp=True):
    return rc.Outputs(torch, n, out_cap, out_bytes, functools.partial(engine.segment_batch, udp=udp),
                      engine.segment_workspace(n), "seg_first")


def check_case(torch, hb, mss, want, udp=True, out_cap=None, out_bytes=None, what="", parse_back=True):
    """One call on hb at mss against the model's `want` = (out_frames, seg_first, totals).
    out_cap / out_bytes default to a little more than the totals; smaller ones overflow."""
    out, first, totals = want
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_batch(db, sm.F6)
    f0, r0 = db.frames.clone(), recs.clone()
    o = Outputs(torch, hb.n, out_cap, out_bytes, udp)
    odb, _, _ = o.call(db, recs, mss)
    torch.cuda.synchronize()
    assert torch.equal(db.frames, f0) and torch.equal(recs, r0), "%s: the inputs were written" % what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back)


def with_lead(want, lead):
    """The model's output for the same frames behind a `lead`-byte junk frame (segment_model.pack):
    the junk frame passes through, everything else moves by one output."""
    if not lead:
        return want
    out, first, totals = want
    return ([b"\xee" * lead] + out, np.concatenate([[0], first + 1]).astype(np.uint32),
            totals + np.array([1, lead], dtype=np.uint64))


@pytest.fixture(scope="module")
def hand():
    """mss -> (frames, the model's output with the flag, the TCP model's output)."""
    res = {}
    for mss in um.MSS_VALUES:
        frames = um.hand_frames(mss)
        hb = sm.pack(frames)
        recs = sm.oracle_records(hb)
        res[mss] = (frames, um.segment(hb, recs, mss, True), sm.segment(hb, recs, mss))
    return res


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_frames(torch, hand, lead):
    """UDP payload lengths around every mss, tags, IPv4 options, IPv6 with extension headers (a
    moved pseudo destination, the UDP header past 128 B), ident wrap-around, padding, a
    zero-checksum datagram, the segment whose checksum computes to 0, fragments and a truncated
    header (pass through), TCP frames mixed in, at every 16-B phase."""
    for mss in um.MSS_VALUES:
        frames, want, plain = hand[mss]
        check_case(torch, sm.pack(frames, lead), mss, with_lead(want, lead),
                   what="mss %d lead %d" % (mss, lead))
        assert (int(want[2][0]) > int(plain[2][0])) == (mss < 65535)
        if lead == 0 and 1 < mss < 65535:                          # the checksum-zero segments
            out = want[0]
            assert um.zero_sum_segments(out, sm.oracle_records(sm.pack(out))) >= 2


@pytest.mark.parametrize("lead", [0, 5])
def test_flag_clear_passes_udp_through(torch, hand, lead):
    """The same batches with flags 0: segment_model's output, every UDP frame a copy."""
    for mss in um.MSS_VALUES:
        frames, want, plain = hand[mss]
        check_case(torch, sm.pack(frames, lead), mss, with_lead(plain, lead), udp=False,
                   what="flag clear mss %d lead %d" % (mss, lead))


@pytest.fixture(scope="module")
def config11():
    hb = gen.make_batch(11, 4096)
    recs = sm.oracle_records(hb)
    assert min(um.cut_counts(recs, 300)) >= 1000
    return hb, um.segment(hb, recs, 300, True)


def test_config_11_dual_stack(torch, config11):
    hb, want = config11
    check_case(torch, hb, 300, want, what="config 11")


def test_config_4(torch):
    hb = gen.make_batch(4, 4096)
    recs = sm.oracle_records(hb)
    assert min(um.cut_counts(recs, 300)) >= 430
    check_case(torch, hb, 300, um.segment(hb, recs, 300, True), what="config 4")


def test_config_6_fuzz(torch):
    """Every parse status passes through or segments; zero-checksum datagrams are cut too."""
    hb = gen.make_batch(6, 8192)
    recs = sm.oracle_records(hb)
    assert len(np.unique(recs["status"])) >= 12 and um.cut_counts(recs, 100)[0] >= 849
    check_case(torch, hb, 100, um.segment(hb, recs, 100, True), what="config 6")


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, config11, short):
    """Capacities below the totals: seg_first and totals exact, nothing written."""
    hb, want = config11
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hb, 300, want, out_cap=cap, out_bytes=nbytes, what="overflow " + short)


def test_exact_capacities(torch, hand):
    frames, want, _ = hand[17]
    want = with_lead(want, 5)
    check_case(torch, sm.pack(frames, 5), 17, want, out_cap=int(want[2][0]), out_bytes=int(want[2][1]),
               what="exact")


def test_scan_across_blocks(torch):
    """70,000 frames of 64..200 B at mss 32, as test_gpu_segment.py builds them, with every
    third hand frame a UDP one: the prefix sums cross the 256-frame blocks and the 256-block
    carry.  700 distinct frames tiled 100 times: the model's output is tiled the same way."""
    fuzz = [f for f in sm.frames_of(gen.make_batch(6, 4096)) if 64 <= len(f) <= 200][:300]
    assert len(fuzz) == 300

    def hand_frame(k):
        if k % 3 == 2:
            pay = sm.payload_bytes(22 + k % 137, k)
            return um.udp4(pay, ident=k, sport=5000 + k) if k % 2 else um.udp6(pay[:118], sport=5000 + k)
        return sm.tcp4(sm.payload_bytes(10 + k % 137, k), seq=k * 977, ident=k) if k % 3 else \
            sm.tcp6(sm.payload_bytes(k % 127, k))
    hand = [hand_frame(k) for k in range(400)]
    block = [f for pair in zip(hand[:300], fuzz) for f in pair] + hand[300:]
    assert all(64 <= len(f) <= 200 for f in block) and len(set(block)) > 600
    hb1 = sm.pack(block)
    recs1 = sm.oracle_records(hb1)
    assert um.cut_counts(recs1, 32)[0] >= 100
    out1, first1, tot1 = um.segment(hb1, recs1, 32, True)
    reps = 100
    hb = sm.pack(block * reps)
    assert hb.n == 70000
    first = np.concatenate([first1[:-1].astype(np.uint64) + r * int(tot1[0]) for r in range(reps)] +
                           [np.array([reps * int(tot1[0])], dtype=np.uint64)]).astype(np.uint32)
    want = (out1 * reps, first, tot1 * np.uint64(reps))
    assert int(want[2][0]) > 2 * hb.n
    check_case(torch, hb, 32, want, what="70,000 frames", parse_back=False)


# ---- chains ------------------------------------------------------------------------------

def check_chains(torch, hc, recs, mss, what):
    """rpkt_gpu_segment_chains with the flag on hc with the host records: what the flat entry
    writes for the flattened bytes (the model's output for them)."""
    want = um.segment(scm.flatten(hc), recs, mss, True)
    out, first, totals = want
    out_cap, out_bytes = int(totals[0]) + 5, int(totals[1]) + 7
    dc = engine.DeviceChains.from_host(hc)
    drecs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).cuda()
    inputs = (dc.buf, dc.segs, dc.chain_first, drecs)
    before = [t.clone() for t in inputs]
    o = rc.Outputs(torch, hc.n, out_cap, out_bytes, functools.partial(engine.segment_chains, udp=True),
                   engine.segment_chains_workspace(hc.n), "seg_first")
    odb, _, _ = o.call(dc, drecs, mss)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "%s: the inputs were written" % what
    rc.check_outputs(o, odb, out, first, totals, what,
                     where=lambda j: "; chain %d" % (int(np.searchsorted(first, j, side="right")) - 1))
    return want


@pytest.mark.parametrize("room", [2048, 64])
def test_chains_in_data_rooms(torch, room):
    """The hand-built set as mbuf chains with the chain parse's records: with 2048-byte rooms
    every header lies in the first segment and UDP datagrams are cut; with 64-byte rooms the
    payload slices cross many segments."""
    for mss in (17, 536):
        frames = [f for f in um.hand_frames(mss) if len(f) < 20000]
        hc = scm.chains_of(frames, [scm.room_cuts(f, room) for f in frames], lead=3, seed=mss)
        recs = scm.chain_records(hc)
        assert um.cut_counts(recs, mss)[0] >= 5
        check_chains(torch, hc, recs, mss, "rooms of %d, mss %d" % (room, mss))


@pytest.mark.parametrize("lead", [0, 5])
def test_chains_cut_at_every_byte_of_the_headers(torch, lead):
    """Flat records over chains cut at every position through the first 90 bytes: inside the
    UDP header, inside the IPv6 addresses and inside a routing header's final address, the
    moved pseudo destination.  The header bytes are gathered across the cut."""
    pay = sm.payload_bytes(40, 5)
    base = [um.udp4(pay, tags=1), um.udp6(pay), um.udp6(pay, exts=(sm.routing(0, 1, 1),)), sm.tcp4(pay)]
    frames, cuts = [], []
    for f in base:
        n = min(len(f), 90) + 1
        frames += [f] * n
        cuts += [[c] for c in range(n)]
    for mss in (7, 16, 17):
        hc = scm.chains_of(frames, cuts, lead=lead, seed=11)
        _, first, _ = check_chains(torch, hc, scm.flat_records(hc), mss, "every cut, mss %d lead %d" % (mss, lead))
        assert (np.diff(first.astype(np.int64)) > 1).all()


def test_graph_capture(torch):
    """Parse, segment with the flag, parse of the output over out_cap slots, captured as one
    graph and replayed on two inputs."""
    hbs = [sm.pack(sm.frames_of(gen.make_batch(11, 512, seed=s))) for s in (5, 55)]
    wants = [um.segment(hb, sm.oracle_records(hb), 300, True) for hb in hbs]
    plain = [sm.segment(hb, sm.oracle_records(hb), 300) for hb in hbs]
    assert wants[0][0] != wants[1][0] and all(w[2][0] > p[2][0] for w, p in zip(wants, plain))
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
