"""GPU parity of rpkt_gpu_segment_chains (TCP segmentation of mbuf chains): the output
frames, offsets, seg_first and totals byte for byte against tests/segment_chains_model.py
(the flat model on the flattened chains), with every output pre-filled with 0xa5 and
followed by guard elements that must stay 0xa5, and the inputs unchanged by the call.

Two kinds of records drive it: oracle.parse_chains' (what a caller has: a header cut by a
segment boundary is a parse error there, so the chain passes through) and the flat oracle's
records of the flattened bytes (they say "segment this" wherever the cuts fall, which is
the only way to drive header bytes across arbitrary cuts)."""
import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records

import reframe_check as rc
import segment_chains_model as scm
import segment_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes):
    return rc.Outputs(torch, n, out_cap, out_bytes, engine.segment_chains,
                      engine.segment_chains_workspace(n), "seg_first")


def device_records(torch, recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).cuda()


def check_case(torch, hc, recs, mss, out_cap=None, out_bytes=None, what="", parse_back=True,
               want=None):
    """One call on the chains hc with the host records `recs` at mss against the model.
    out_cap / out_bytes default to a little more than the model's totals (spare slots and
    spare bytes to check); smaller ones overflow.  Returns the model's (out_frames,
    seg_first, totals)."""
    out, first, totals = want if want is not None else scm.segment_chains(hc, recs, mss)
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    dc = engine.DeviceChains.from_host(hc)
    drecs = device_records(torch, recs)
    inputs = (dc.buf, dc.segs, dc.chain_first, drecs)
    before = [t.clone() for t in inputs]
    o = Outputs(torch, hc.n, out_cap, out_bytes)
    odb, _, _ = o.call(dc, drecs, mss)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "%s: the inputs were written" % what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back,
                     where=lambda j: "; chain %d" % (int(np.searchsorted(first, j, side="right")) - 1))
    return out, first, totals


def segmented(first):
    return np.diff(first.astype(np.int64)) > 1


RECORDS = {"chain": scm.chain_records, "flat": scm.flat_records}


# ---- every cut ---------------------------------------------------------------------------

def cut_frames():
    pay = sm.payload_bytes(40, 5)
    return [sm.tcp4(pay), sm.tcp4(pay, tags=2, ihl=6, doff=8),
            sm.tcp6(pay, exts=(sm.hop_by_hop(), sm.routing(0, 2, 1))), sm.udp4(pay)]


_every_cut = {}


def every_cut(lead, kind, mss):
    """All two-segment cuts c in 0..len of the four frames as one batch, and the model's
    output for it (the same for every lead: computed once)."""
    frames, cuts = [], []
    for f in cut_frames():
        frames += [f] * (len(f) + 1)
        cuts += [[c] for c in range(len(f) + 1)]
    hc = scm.chains_of(frames, cuts, lead=lead, seed=7)
    key = (kind, mss)
    if key not in _every_cut:
        recs = RECORDS[kind](hc)
        _every_cut[key] = (recs, scm.segment_chains(hc, recs, mss))
    return (hc,) + _every_cut[key]


@pytest.mark.parametrize("lead", list(range(16)))
def test_every_two_segment_cut(torch, lead):
    """Every cut of a plain TCP/IPv4 frame, one with two tags and IPv4 / TCP options, a
    TCP/IPv6 frame behind hop-by-hop and routing headers, and a UDP frame, at mss 7, 16 and
    17 and every 16-B arena phase.  With the chain parse's records a cut inside a header
    passes through; with the flat records the header bytes are gathered across the cut."""
    for kind in ("chain", "flat"):
        for mss in (7, 16, 17):
            hc, recs, want = every_cut(lead, kind, mss)
            check_case(torch, hc, recs, mss, what="%s records mss %d lead %d" % (kind, mss, lead),
                       want=want, parse_back=lead == 0)
            seg = segmented(want[1])
            n4 = len(cut_frames()[0]) + 1                          # the plain frame's cuts
            if kind == "flat":
                assert seg[:-(len(cut_frames()[3]) + 1)].all() and not seg[-1]
            else:
                # a header may start where a segment ends, but not straddle its end
                assert np.nonzero(seg[:n4])[0].tolist() == [14, 34] + list(range(54, n4))


def test_three_and_four_segments(torch):
    """An empty first segment, an empty middle one, a 1-byte segment inside the payload (the
    next piece starts at the other checksum phase), cuts exactly at payload_off and at
    payload_off + k * mss, alone and together."""
    pay = sm.payload_bytes(40, 9)
    f4, f6 = sm.tcp4(pay), sm.tcp6(pay, exts=(sm.hop_by_hop(),))
    for f, po in ((f4, 54), (f6, 82)):
        assert len(f) == po + 40
        cuts = [[0, 60], [0, 0, po], [30, 30, 70], [po, po, po + 1], [po + 6, po + 7],
                [po + 7, po + 8, po + 9], [po + 15, po + 16, po + 17], [po], [po, po + 16],
                [po + 16, po + 32], [po, po + 16, po + 32], [po + 32, po + 39, po + 40],
                [10, po - 1, po + 1], [po - 20, po - 19, po - 18]]
        for mss in (7, 16, 17):
            for lead in (0, 5):
                hc = scm.chains_of([f] * len(cuts), cuts, lead=lead, seed=po + mss)
                for kind in ("chain", "flat"):
                    _, first, _ = check_case(torch, hc, RECORDS[kind](hc), mss,
                                             what="%s records po %d mss %d lead %d" % (kind, po, mss, lead))
                    assert segmented(first).all() if kind == "flat" else segmented(first)[7:12].all()


@pytest.mark.parametrize("room", [61, 64, 2048])
def test_hand_built_frames_in_data_rooms(torch, room):
    """tests/segment_model.py's hand-built set for every mss, each frame laid out as an mbuf
    chain with data rooms of 61, 64 and 2048 bytes: payload slices cross several segments at
    odd and even phases, and at the small rooms most headers cross them too."""
    for mss in sm.MSS_VALUES:
        frames = sm.hand_frames(mss)
        hc = scm.chains_of(frames, [scm.room_cuts(f, room) for f in frames], lead=room & 15, seed=mss)
        for kind in ("chain", "flat"):
            out, first, totals = check_case(torch, hc, RECORDS[kind](hc), mss,
                                            what="%s records room %d mss %d" % (kind, room, mss))
            assert (int(totals[0]) > hc.n) == (mss < 65535)


# ---- the generator's configs ------------------------------------------------------------

@pytest.fixture(scope="module")
def config7():
    hc = gen.make_chains(7, 1024, layout="mbuf")
    recs = scm.chain_records(hc)
    return hc, recs, scm.segment_chains(hc, recs, 1448)


def test_config_7_jumbo_frames_in_mbufs(torch, config7):
    """jumboframe_tx.rs: 8000-byte frames in 2048-byte data rooms, half of them TCP."""
    hc, recs, want = config7
    assert segmented(want[1]).mean() >= 0.40
    check_case(torch, hc, recs, 1448, what="config 7", want=want)


def header_past_first_segment(hc, recs, first):
    """The segmented chains whose [0, payload_off) extends past the first non-empty segment."""
    n = 0
    for p in np.nonzero(segmented(first))[0]:
        lens = hc.segs[int(hc.chain_first[p]):int(hc.chain_first[p + 1]), 1]
        n += int(lens[lens > 0][0]) < int(recs["payload_off"][p])
    return n


@pytest.mark.parametrize("config", [5, 11])
def test_configs_with_options_and_dual_stack(torch, config):
    """Fuzz layout: up to six segments cut anywhere.  The chain parse's own records reach the
    gathered header: a header may start exactly where a segment ends."""
    hc = gen.make_chains(config, 2048, layout="fuzz")
    recs = scm.chain_records(hc)
    want = scm.segment_chains(hc, recs, 300)
    assert segmented(want[1]).mean() >= 0.30
    assert header_past_first_segment(hc, recs, want[1]) >= 1
    check_case(torch, hc, recs, 300, what="config %d" % config, want=want)


def test_config_6_fuzz(torch):
    """Every parse status passes through or segments."""
    hc = gen.make_chains(6, 4096, layout="fuzz")
    recs = scm.chain_records(hc)
    assert len(np.unique(recs["status"])) >= 15
    want = scm.segment_chains(hc, recs, 100)
    assert segmented(want[1]).any()
    check_case(torch, hc, recs, 100, what="config 6", want=want)


# ---- against the flat entry, capacities, the scan ------------------------------------------

def test_single_segment_chains_equal_segment_batch(torch):
    """One segment per chain: every output equals rpkt_gpu_segment_batch's on the same bytes
    and the same records, GPU against GPU, guards included."""
    for mss, lead in ((17, 5), (536, 0)):
        hb = sm.pack(sm.hand_frames(mss), lead)
        segs = np.stack([hb.offsets[:-1], np.diff(hb.offsets.astype(np.int64)).astype(np.uint32)], axis=1)
        hc = gen.HostChains(0, hb.n, 0, hb.frames, np.ascontiguousarray(segs, dtype=np.uint32),
                            np.arange(hb.n + 1, dtype=np.uint32), hb.lens().astype(np.uint32))
        db, dc = engine.DeviceBatch.from_host(hb), engine.DeviceChains.from_host(hc)
        recs = engine.parse_batch(db, sm.F6)
        _, _, totals = sm.segment(hb, sm.oracle_records(hb), mss)
        a = Outputs(torch, hb.n, int(totals[0]) + 3, int(totals[1]) + 9)
        b = Outputs(torch, hb.n, int(totals[0]) + 3, int(totals[1]) + 9)
        a.call(db, recs, mss, fn=engine.segment_batch)
        b.call(dc, recs, mss)
        torch.cuda.synchronize()
        for x, y, name in zip(a.host(), b.host(), ("frames", "offsets", "seg_first", "totals")):
            assert np.array_equal(x, y), "mss %d: %s differ" % (mss, name)
        assert b.host()[3][:2].tolist() == [int(totals[0]), int(totals[1])]


@pytest.fixture(scope="module")
def rooms64():
    frames = sm.hand_frames(17)
    hc = scm.chains_of(frames, [scm.room_cuts(f, 64) for f in frames], lead=3, seed=64)
    recs = scm.flat_records(hc)
    return hc, recs, scm.segment_chains(hc, recs, 17)


def test_exact_capacities(torch, rooms64):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte."""
    hc, recs, want = rooms64
    check_case(torch, hc, recs, 17, out_cap=int(want[2][0]), out_bytes=int(want[2][1]), what="exact",
               want=want)


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, rooms64, short):
    """Capacities below the totals: RPKT_OK, seg_first and totals exact, nothing written past
    out_bytes or out_cap + 1 offsets."""
    hc, recs, want = rooms64
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hc, recs, 17, out_cap=cap, out_bytes=nbytes, what="overflow " + short, want=want)


def test_scan_across_blocks(torch):
    """70,000 chains of 64..200 B in two or three segments at mss 32: the prefix sums cross the
    256-chain blocks and the 256-block carry of the block sums' scan.  700 distinct chains
    (hand-built TCP over IPv4 / IPv6 with every payload length, and config-6 fuzz frames cut
    to size), their arena, segments and records tiled 100 times: the model's output of the
    700 is tiled the same way."""
    fuzz = [f for f in sm.frames_of(gen.make_batch(6, 4096)) if 64 <= len(f) <= 200][:300]
    assert len(fuzz) == 300
    hand = [sm.tcp4(sm.payload_bytes(10 + k % 137, k), seq=k * 977, ident=k) if k % 3 else
            sm.tcp6(sm.payload_bytes(k % 127, k)) for k in range(400)]
    block = [f for pair in zip(hand[:300], fuzz) for f in pair] + hand[300:]
    assert all(64 <= len(f) <= 200 for f in block) and len(set(block)) > 600
    rng = np.random.default_rng(32)
    cuts = [sorted(rng.integers(1, len(f), size=1 + k % 2).tolist()) for k, f in enumerate(block)]
    hc1 = scm.chains_of(block, cuts, lead=9, seed=32)
    recs1 = scm.flat_records(hc1)
    out1, first1, tot1 = scm.segment_chains(hc1, recs1, 32)
    reps, nb, ns = 100, hc1.buf.size, hc1.n_segs
    segs = np.concatenate([hc1.segs + np.array([r * nb, 0], dtype=np.uint32) for r in range(reps)])
    chain_first = np.concatenate([hc1.chain_first[:-1] + np.uint32(r * ns) for r in range(reps)] +
                                 [np.array([reps * ns], dtype=np.uint32)])
    hc = gen.HostChains(0, reps * hc1.n, 0, np.tile(hc1.buf, reps), segs, chain_first,
                        np.tile(hc1.pkt_lens, reps))
    assert hc.n == 70000 and 2 * hc.n <= hc.n_segs <= 3 * hc.n
    first = np.concatenate([first1[:-1].astype(np.uint64) + r * int(tot1[0]) for r in range(reps)] +
                           [np.array([reps * int(tot1[0])], dtype=np.uint64)]).astype(np.uint32)
    want = (out1 * reps, first, tot1 * np.uint64(reps))
    assert int(want[2][0]) > 2 * hc.n
    check_case(torch, hc, np.tile(recs1, reps), 32, what="70,000 chains", want=want, parse_back=False)


# ---- descriptors --------------------------------------------------------------------------

def test_descriptor_edge_cases(torch):
    """chain_first entries past n_segs and decreasing, segment offsets and lengths past
    buf_bytes, two chains sharing a segment: the documented clamps; the model flattens under
    the same ones (tests/test_segment_chains_model.py)."""
    frames = [sm.tcp4(sm.payload_bytes(40 + 30 * k, k)) for k in range(4)]
    hc = scm.chains_of(frames, [[30], [], [10, 60], [54]], lead=2, seed=3)
    fb = hc.buf.size
    segs = hc.segs.copy()
    segs[7] = (segs[7][0], 0xffffffff)                          # a length past the arena
    segs[6] = (fb + 5, 7)                                       # an offset past the arena
    hc.segs = segs
    # chains: [0, 2), none (decreasing), [1, 6) sharing segments with its neighbours, [6, 8)
    # clamped from 1000, none (past n_segs), [2, 3) shared again
    hc.chain_first = np.array([0, 2, 1, 6, 1000, 2, 3], dtype=np.uint32)
    hc.n = 6
    got = scm.chain_bytes(hc)
    assert [len(g) for g in got][:2] == [len(frames[0]), 0] and got[4] == b"" and got[5] == frames[1]
    assert got[2] == frames[0][30:] + frames[1] + frames[2] and len(got[3]) == fb - int(segs[7][0])
    for mss in (16, 33):
        for kind in ("chain", "flat"):
            _, first, _ = check_case(torch, hc, RECORDS[kind](hc), mss, what="descriptors, %s records" % kind)
            # chain 0 is cut inside its IPv4 header: segmented only with the flat records
            assert segmented(first)[[0, 5]].tolist() == [kind == "flat", True]


def test_no_segments_at_all(torch):
    """n_segs == 0 with n_chains > 0 (no arena, no segment table): every chain is empty, every
    output an empty frame."""
    n = 300
    hc = gen.HostChains(0, n, 0, np.zeros(0, dtype=np.uint8), np.zeros((0, 2), dtype=np.uint32),
                        np.arange(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
    _, first, totals = check_case(torch, hc, scm.flat_records(hc), 100, what="no segments")
    assert totals.tolist() == [n, 0] and np.array_equal(first, np.arange(n + 1))


# ---- graph, example, engine ------------------------------------------------------------------

def test_graph_capture(torch):
    """Chain parse, segmentation, parse of the flat output over out_cap slots, captured as one
    graph and replayed on two inputs with different totals: no host step between the three."""
    hcs = [gen.make_chains(5, 512, seed=s, layout="fuzz") for s in (5, 55)]
    wants = [scm.segment_chains(hc, scm.chain_records(hc), 300) for hc in hcs]
    assert wants[0][2][0] != wants[1][2][0]
    size = max(hc.buf.size for hc in hcs) + 16
    n_segs = max(hc.n_segs for hc in hcs)
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    segs = torch.zeros(2 * n_segs, dtype=torch.int32, device="cuda")
    chain_first = torch.zeros(513, dtype=torch.int32, device="cuda")
    dc = engine.DeviceChains(buf, segs, chain_first, 512)
    recs, orecs = engine.alloc_records(512), engine.alloc_records(out_cap)
    o = Outputs(torch, 512, out_cap, out_bytes)

    def load(hc):
        buf.zero_()
        segs.zero_()                                   # the table's tail: segments of no chain
        buf[:hc.buf.size].copy_(torch.from_numpy(hc.buf.copy()))
        segs[:2 * hc.n_segs].copy_(torch.from_numpy(hc.segs.view(np.int32).reshape(-1).copy()))
        chain_first.copy_(torch.from_numpy(hc.chain_first.view(np.int32).copy()))

    def fn():
        engine.parse_chains(dc, sm.F6, recs=recs)
        odb, _, _ = o.call(dc, recs, 300)
        engine.parse_batch(odb, sm.F6, recs=orecs)

    load(hcs[0])
    loop = graphs.CapturedLoop(fn)
    for k in (1, 0, 1):
        load(hcs[k])
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


def test_cpp_tso_tx_chains_through_c_abi(torch):
    """examples/tso_tx_chains: the reference's tso_tx.rs frame as the two-segment mbuf chain
    from_slice + extend_front make of it, parsed, segmented at 1024 and parsed back through
    the C ABI only; the example checks its own four segments."""
    import subprocess
    from rpkt_amd.build import TSO_TX_CHAINS_BIN
    r = subprocess.run([TSO_TX_CHAINS_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: 4 segments from a 2-segment chain, sums valid" in r.stdout
    assert r.stdout.count("l4_sum=0xffff") == 4 and "segments of 2102 + 1952" in r.stdout


def test_engine_refuses_bad_arguments(torch):
    f = sm.tso_tx_frame()
    hc = scm.chains_of([f], [[54 + 2048]], shuffle=False)
    dc = engine.DeviceChains.from_host(hc)
    recs = engine.parse_chains(dc, 3)
    for mss in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.segment_chains(dc, recs, mss, out_cap=8, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.segment_chains(dc, recs, 1024, out_cap=0, out_bytes=8192)
    odb, first, totals = engine.segment_chains(dc, recs, 1024)
    assert totals.cpu().tolist() == [4, 4000 + 4 * 54] and first.cpu().tolist() == [0, 4]


def test_default_sizes_come_from_the_documented_bound(torch, config7):
    """engine.segment_chains with no outputs given sizes them from the bound with the arena's
    size for frames_bytes (the mbuf layout's segments do not overlap): never an overflow."""
    hc, recs, (out, first, totals) = config7
    dc = engine.DeviceChains.from_host(hc)
    odb, gs, gt = engine.segment_chains(dc, engine.parse_chains(dc, sm.F6), 1448)
    assert odb.n == hc.n + hc.buf.size // 1448 and odb.n >= int(totals[0])
    assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
    assert odb.frames.numel() >= int(totals[1])
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), first)
    blob, offs = sm.packed_output(out, odb.n)
    assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)
