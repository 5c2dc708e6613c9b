"""GPU parity of rpkt_gpu_segment_tunnel_chains (segmentation of the inner TCP / UDP of tunnels
over mbuf chains): the output frames, offsets, seg_first and totals byte for byte against
tests/segment_tunnel_chains_model.py (the flat tunnel model on the flattened chains), every
output pre-filled with 0xa5 and followed by guard elements that must stay 0xa5, the inputs
unchanged by the call, and the GPU's tunnel parse of the GPU's output equal to the oracle's
tunnel parse of the model's.

Two kinds of records drive it, as for rpkt_gpu_segment_chains: the chain tunnel parse's (what a
caller has: a header cut by a segment end is a parse error or RPKT_T_BAD there, so the chain
passes through) and the flat tunnel parse's records of the flattened bytes (they say "cut"
wherever the segment ends fall: the only way to drive header bytes across arbitrary cuts).
tests/test_segment_tunnel_chains_model.py checks the inputs' conditions without a GPU."""
import functools
import subprocess

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records, as_tunnels

import reframe_check as rc
import segment_chains_model as scm
import segment_model as sm
import segment_tunnel_chains_model as stcm
import segment_tunnel_model as stm
import test_segment_tunnel_model as flat_tests

pytestmark = pytest.mark.gpu

K_SEG_BLOCK = 256                              # chains a plan block (rpkt_segcopy.h kSegBlock)
TUNNELS = (stm.VXLAN, stm.GTPU, stm.GRE)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, udp, fn=None, ws=None):
    return rc.Outputs(torch, n, out_cap, out_bytes,
                      functools.partial(fn or engine.segment_tunnel_chains, udp=udp),
                      engine.segment_tunnel_chains_workspace(n) if ws is None else ws, "seg_first")


def device_records(torch, recs):
    return tuple(torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).copy()).cuda() for r in recs)


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


def check_case(torch, hc, recs, mss, udp, want=None, out_cap=None, out_bytes=None, what="",
               parse=True):
    """One call on the chains hc with the host records `recs` = (outer, tun, inner) at mss
    against the model's `want` = (out_frames, seg_first, totals).  out_cap / out_bytes default
    to a little more than the totals; smaller ones overflow.  Returns `want`."""
    want = stcm.segment(hc, *recs, mss, udp) if want is None else want
    out, first, totals = want
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    dc = engine.DeviceChains.from_host(hc)
    inputs = (dc.buf, dc.segs, dc.chain_first) + device_records(torch, recs)
    before = [t.clone() for t in inputs]
    o = Outputs(torch, hc.n, out_cap, out_bytes, udp)
    odb, _, _ = o.call(dc, *inputs[3:], mss)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "%s: the inputs were written" % what
    where = lambda j: "; chain %d" % (int(np.searchsorted(first, j, side="right")) - 1)
    if rc.check_outputs(o, odb, out, first, totals, what, parse_back=False, where=where) and parse:
        parse_back(odb, out, out_cap, what)
    return want


def segmented(first):
    return np.diff(first.astype(np.int64)) > 1


# ---- every cut ---------------------------------------------------------------------------

def cut_frames():
    """VXLAN / IPv4 around TCP; GTP-U with extension headers and a sequence number around
    TCP / IPv6; GRE with C and K around TCP; VXLAN around UDP."""
    f = stm.cut_frames(40)
    return [f[0], f[4], f[6], f[11]]


def header_offsets(f):
    """(O.l3, O.l4, tun_off, inner_off, I.l3, I.l4, I.payload_off) of one frame."""
    O, T, I = (r[0] for r in stm.tunnel_records(sm.pack([f])))
    return [int(x) for x in (O["l3_off"], O["l4_off"], T["tun_off"], T["inner_off"], I["l3_off"],
                             I["l4_off"], I["payload_off"])]


_every_cut = {}


def every_cut(lead, kind, mss, udp):
    """All two-segment cuts c in 0..len of the four frames as one set of chains, its records
    (the same for every lead: where the segments lie in the arena does not enter them) and the
    model's output, computed once per (records, mss, flag)."""
    frames, cuts = [], []
    for f in cut_frames():
        frames += [f] * (len(f) + 1)
        cuts += [[c] for c in range(len(f) + 1)]
    hc = scm.chains_of(frames, cuts, lead=lead, seed=7)
    if kind not in _every_cut:
        _every_cut[kind] = stcm.RECORDS[kind](hc)
    recs = _every_cut[kind]
    key = (kind, mss, udp)
    if key not in _every_cut:
        _every_cut[key] = stcm.segment(hc, *recs, mss, udp)
    return hc, recs, _every_cut[key]


def check_every_cut_conditions(kind, udp, want):
    """Which of the two-segment chains the model cuts."""
    seg = segmented(want[1])
    fr = cut_frames()
    n_udp = len(fr[3]) + 1
    if kind == "flat":
        # every TCP-carrying chain wherever its cut falls; the UDP-carrying one with the flag
        assert seg[:-n_udp].all() and seg[-n_udp:].all() == udp and seg[-n_udp:].any() == udp
        return
    # the chain parse: a header may start where a segment ends but not straddle an end
    n0 = len(fr[0]) + 1
    ol3, ol4, toff, ioff, il3, il4, po = header_offsets(fr[0])
    assert (ol3, ol4, toff, ioff, il3, il4, po) == (14, 34, 42, 50, 64, 84, 104)
    cut = set(np.nonzero(seg[:n0])[0].tolist())
    assert cut >= {ol3, ol4, toff, ioff, il3, il4} | set(range(po, n0))
    inside = {ol3 + 7, ol4 + 3, toff + 5, il3 + 9, il4 + 11}
    assert not (cut & inside)
    for c in range(1, po):                          # strictly inside one of those headers
        if any(a < c < b for a, b in ((ol3, ol4), (ol4, toff), (toff, ioff), (il3, il4), (il4, po))):
            assert c not in cut, c


@pytest.mark.parametrize("lead", list(range(16)))
def test_every_two_segment_cut(torch, lead):
    """Every cut of four tunnel frames at mss 7, 16 and 17 and every 16-B arena phase, with and
    without RPKT_SEGMENT_UDP.  With the chain parse's records a cut inside a header passes
    through; with the flat records the outer, tunnel and inner header bytes are gathered across
    the cut."""
    for kind in ("chain", "flat"):
        for mss in (7, 16, 17):
            for udp in (False, True):
                hc, recs, want = every_cut(lead, kind, mss, udp)
                check_case(torch, hc, recs, mss, udp, want=want, parse=lead == 0,
                           what="%s records mss %d udp %d lead %d" % (kind, mss, udp, lead))
                check_every_cut_conditions(kind, udp, want)


def multi_cuts(f):
    """Three- and four-segment cuts of a tunnel frame around its own header offsets, and the
    indices of the ones the chain parse's records cut too (no header straddles an end)."""
    _, _, toff, ioff, _, _, po = header_offsets(f)
    assert len(f) == po + 40
    cuts = [[0, po + 6], [0, 0, po], [30, 30, po + 16], [po, po, po + 1], [po + 6, po + 7],
            [po + 7, po + 8, po + 9], [po + 15, po + 16, po + 17], [toff], [ioff], [toff, ioff, po],
            [po], [po, po + 16], [po + 16, po + 32], [po, po + 7, po + 14], [po, po + 17, po + 34],
            [po + 32, po + 39, po + 40], [10, po - 1, po + 1], [po - 20, po - 19, po - 18]]
    # (to the chain parse an empty first segment is a frame too short for its first header)
    return cuts, list(range(3, 16))


def test_three_and_four_segments(torch):
    """An empty first segment, an empty middle one, a 1-byte segment inside the payload (the next
    piece starts at the other checksum phase), cuts exactly at tun_off, at inner_off, at the
    inner payload_off and at payload_off + k * mss, alone and together."""
    for f in cut_frames()[:3]:
        cuts, by_chain = multi_cuts(f)
        for mss in (7, 16, 17):
            for lead in (0, 5):
                hc = scm.chains_of([f] * len(cuts), cuts, lead=lead, seed=len(f) + mss)
                for kind in ("chain", "flat"):
                    _, first, _ = check_case(torch, hc, stcm.RECORDS[kind](hc), mss, False,
                                             what="%s records len %d mss %d lead %d" % (kind, len(f), mss, lead))
                    seg = segmented(first)
                    assert seg.all() if kind == "flat" else seg[by_chain].all() and not seg[[0, 1, 2, 16, 17]].any()


@pytest.mark.parametrize("room", [61, 64, 2048])
def test_hand_built_frames_in_data_rooms(torch, room):
    """tests/segment_tunnel_model.py's hand-built set for every mss, with and without the flag,
    each frame laid out as an mbuf chain with data rooms of 61, 64 and 2048 bytes: at the small
    rooms most inner headers lie past the first segment and payload slices cross several."""
    for mss in stm.MSS_VALUES:
        frames = stm.hand_frames(mss)
        hc = scm.chains_of(frames, [scm.room_cuts(f, room) for f in frames], lead=room & 15, seed=mss)
        for kind in ("chain", "flat"):
            recs = stcm.RECORDS[kind](hc)
            for udp in (False, True):
                _, first, totals = check_case(torch, hc, recs, mss, udp,
                                              what="%s records room %d mss %d udp %d" % (kind, room, mss, udp))
                if kind == "flat" or room == 2048:
                    assert int(totals[0]) > hc.n + 10


@pytest.mark.parametrize("mss", [1448, 536])
def test_super_frames_in_2048_byte_rooms(torch, mss):
    """5000-byte inner payloads in 2048-byte data rooms: every header lies in the first room, so
    the chain parse's records are the flat ones; every tunnel kind is cut, and every output
    parses back with all four sums valid."""
    frames = stm.cut_frames(5000)
    hc = scm.chains_of(frames, [scm.room_cuts(f, 2048) for f in frames], lead=8, seed=mss)
    recs = stcm.chain_records(hc)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(recs, stcm.flat_records(hc)))
    want = check_case(torch, hc, recs, mss, True, what="super-frames mss %d" % mss)
    kinds = stm.cut_kinds(want[1], recs[1])
    assert kinds[stm.VXLAN] >= 4 and kinds[stm.GTPU] == 3 and kinds[stm.GRE] == 4
    assert segmented(want[1]).all()
    # the outputs equal the model's, whose outputs verify under the oracle: all four sums
    flat_tests.check_cut(scm.flatten(hc), recs, mss, True, "super-frames mss %d" % mss)


# ---- the generator's configs ------------------------------------------------------------

@pytest.fixture(scope="module")
def config13():
    hc = gen.make_chains(13, 2048, layout="fuzz")
    return hc, stcm.chain_records(hc)


@pytest.mark.parametrize("udp,floor,past", [(True, 150, 40), (False, 80, 20)])
def test_config_13_fuzz(torch, config13, udp, floor, past):
    """Up to six segments cut anywhere.  The chain parse's own records reach the gathered header:
    the inner headers may lie anywhere behind the first segment as long as none straddles an
    end."""
    hc, recs = config13
    want = stcm.segment(hc, *recs, 300, udp)
    kinds = stm.cut_kinds(want[1], recs[1])
    assert min(kinds[k] for k in TUNNELS) >= floor, kinds
    assert stcm.header_past_first_segment(hc, *recs, want[1]) >= past
    check_case(torch, hc, recs, 300, udp, want=want, what="config 13 udp %d" % udp)


def test_config_14_fuzz(torch):
    """Every tunnel status and every parse status at both levels passes through or is cut."""
    hc = gen.make_chains(14, 4096, layout="fuzz")
    recs = stcm.chain_records(hc)
    assert len(np.unique(recs[1]["status"])) == 6
    want = stcm.segment(hc, *recs, 100, True)
    kinds = stm.cut_kinds(want[1], recs[1])
    assert min(kinds[k] for k in TUNNELS) >= 100, kinds
    check_case(torch, hc, recs, 100, True, want=want, what="config 14")


# ---- GPU against GPU -----------------------------------------------------------------------

def test_single_segment_chains_equal_segment_tunnel_batch(torch):
    """One segment per chain: every output equals rpkt_gpu_segment_tunnel_batch's on the same
    bytes and the same records, GPU against GPU, guards included."""
    for mss, lead, udp in ((17, 5, True), (536, 0, False)):
        hb = sm.pack(stm.hand_frames(mss), lead)
        hc = stcm.single_segment_chains(hb)
        db, dc = engine.DeviceBatch.from_host(hb), engine.DeviceChains.from_host(hc)
        recs = engine.parse_tunnel_batch(db, sm.F6)
        _, _, totals = stm.segment(hb, *stm.tunnel_records(hb), mss, udp)
        cap, nbytes = int(totals[0]) + 3, int(totals[1]) + 9
        a = Outputs(torch, hb.n, cap, nbytes, udp, engine.segment_tunnel_batch,
                    engine.segment_tunnel_workspace(hb.n))
        b = Outputs(torch, hb.n, cap, nbytes, udp)
        a.call(db, *recs, mss)
        b.call(dc, *recs, mss)
        torch.cuda.synchronize()
        for x, y, name in zip(a.host(), b.host(), ("frames", "offsets", "seg_first", "totals")):
            assert np.array_equal(x, y), "mss %d: %s differ" % (mss, name)
        assert b.host()[3][:2].tolist() == [int(totals[0]), int(totals[1])] and int(totals[0]) > hb.n


@pytest.mark.parametrize("udp", [False, True])
def test_without_tunnels_the_output_is_segment_chains_s(torch, config13, udp):
    """Every tun kind NONE: byte for byte what engine.segment_chains writes with the outer
    records (with the flag the outer datagrams are cut, as that entry would)."""
    hc = config13[0]
    dc = engine.DeviceChains.from_host(hc)
    outer, tun, inner = engine.parse_tunnel_chains(dc, sm.F6)
    none = np.zeros(hc.n, dtype=as_tunnels(tun.cpu().numpy()).dtype)
    none["status"] = 1
    tun = torch.from_numpy(none.view(np.uint8).copy()).cuda()
    cap, nbytes = hc.n + hc.buf.size // 300, 2 * hc.buf.size
    a = Outputs(torch, hc.n, cap, nbytes, udp)
    b = rc.Outputs(torch, hc.n, cap, nbytes, functools.partial(engine.segment_chains, udp=udp),
                   engine.segment_chains_workspace(hc.n), "seg_first")
    a.call(dc, outer, tun, inner, 300)
    b.call(dc, outer, 300)
    torch.cuda.synchronize()
    ga, gb = a.host(), b.host()
    assert int(gb[3][0]) <= cap and int(gb[3][1]) <= nbytes and (int(gb[3][0]) > hc.n) == udp
    for x, y, name in zip(ga, gb, ("frames", "offsets", "seg_first", "totals")):
        assert np.array_equal(x, y), name


# ---- capacities and the scan ----------------------------------------------------------------

@pytest.fixture(scope="module")
def rooms64():
    frames = stm.hand_frames(17)
    hc = scm.chains_of(frames, [scm.room_cuts(f, 64) for f in frames], lead=3, seed=64)
    recs = stcm.flat_records(hc)
    return hc, recs, stcm.segment(hc, *recs, 17, True)


def test_exact_capacities(torch, rooms64):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte."""
    hc, recs, want = rooms64
    check_case(torch, hc, recs, 17, True, want=want, out_cap=int(want[2][0]),
               out_bytes=int(want[2][1]), what="exact")


@pytest.mark.parametrize("short", ["cap", "bytes", "both"])
def test_overflow(torch, rooms64, short):
    """Capacities below the totals: RPKT_OK, seg_first and totals exact, nothing written past
    out_bytes or out_cap + 1 offsets."""
    hc, recs, want = rooms64
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"cap": (n_out - 1, need), "bytes": (n_out, need - 1), "both": (1, 16)}[short]
    check_case(torch, hc, recs, 17, True, want=want, out_cap=cap, out_bytes=nbytes,
               what="overflow " + short)


def three_block_chains():
    """2 * kSegBlock + 5 short chains in 64-byte rooms with one super-frame chain in each plan
    block."""
    n = 2 * K_SEG_BLOCK + 5
    short = stm.cut_frames(20)[:11] + stm.through_frames(20, 64)[:8]
    big = stm.cut_frames(700)
    frames = [short[k % len(short)] for k in range(n)]
    at = (3, K_SEG_BLOCK + 44, n - 2)
    for a, f in zip(at, (big[0], big[4], big[8])):
        frames[a] = f
    return scm.chains_of(frames, [scm.room_cuts(f, 64) for f in frames], lead=1, seed=3), list(at)


def test_three_plan_blocks(torch):
    """The prefix sums carry counts and bytes across the plan blocks."""
    hc, at = three_block_chains()
    recs = stcm.flat_records(hc)
    want = stcm.segment(hc, *recs, 64, False)
    assert np.nonzero(segmented(want[1]))[0].tolist() == at
    check_case(torch, hc, recs, 64, False, want=want, what="three plan blocks")


# ---- descriptors and robustness --------------------------------------------------------------

def descriptor_chains():
    """tests/test_gpu_segment_chains.py's descriptor edge cases with tunnel frames among the
    chains: chain_first entries past n_segs and decreasing, a segment offset and a length past
    buf_bytes, chains sharing segments."""
    big = stm.cut_frames(70)
    frames = [big[0], big[6], sm.tcp4(sm.payload_bytes(100, 2)), sm.tcp4(sm.payload_bytes(130, 3))]
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
    return hc


def test_descriptor_edge_cases(torch):
    """The documented clamps; the model flattens under the same ones."""
    hc = descriptor_chains()
    for mss in (16, 33):
        for kind in ("chain", "flat"):
            recs = stcm.RECORDS[kind](hc)
            _, first, _ = check_case(torch, hc, recs, mss, False, what="descriptors, %s records" % kind)
            # chain 0 (VXLAN) is cut inside its outer IPv4 header: segmented only with the flat
            # records; chain 5 (GRE with C) is one shared segment
            assert segmented(first)[[0, 5]].tolist() == [kind == "flat", True]
            assert recs[1]["kind"][5] == stm.GRE


def test_no_segments_at_all(torch):
    """n_segs == 0 with n_chains > 0 (no arena, no segment table): every chain is empty, every
    output an empty frame."""
    n = 300
    hc = gen.HostChains(0, n, 0, np.zeros(0, dtype=np.uint8), np.zeros((0, 2), dtype=np.uint32),
                        np.arange(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
    _, first, totals = check_case(torch, hc, stcm.flat_records(hc), 100, True, what="no segments")
    assert totals.tolist() == [n, 0] and np.array_equal(first, np.arange(n + 1))


def test_records_of_other_chains_never_write_outside(torch):
    """The records of the same chains in a shuffled order: nothing is asserted about the frames;
    the guards and the 0xa5 fill past out_bytes stay intact."""
    hc = gen.make_chains(13, 1024, seed=5, layout="fuzz")
    dc = engine.DeviceChains.from_host(hc)
    order = torch.from_numpy(np.random.default_rng(7).permutation(hc.n)).cuda()
    recs = [r.view(hc.n, -1)[order].contiguous().view(-1) for r in engine.parse_tunnel_chains(dc, sm.F6)]
    size = hc.buf.size
    for mss, cap, nbytes in ((100, hc.n + size // 100, 3 * size), (100, 3 * hc.n, size),
                             (7, 4 * hc.n, size // 2)):
        o = Outputs(torch, hc.n, cap, nbytes, True)
        o.call(dc, *recs, mss)
        torch.cuda.synchronize()
        gf, go, gs, gt = o.host()
        assert (gf[nbytes:] == 0xa5).all() and (go[cap + 1:] == 0xa5a5a5a5).all()
        assert (gs[hc.n + 1:] == 0xa5a5a5a5).all() and (gt[2:] == 0xa5a5a5a5a5a5a5a5).all()
        assert int(gs[hc.n]) == int(gt[0]) >= hc.n


# ---- graph, example, engine ------------------------------------------------------------------

def test_graph_capture(torch):
    """Chain tunnel parse, segmentation, tunnel parse of the flat output over out_cap slots,
    captured as one graph and replayed on two inputs with different totals: no host step between
    the three."""
    hcs = [gen.make_chains(13, 512, seed=s, layout="fuzz") for s in (5, 55)]
    wants = [stcm.segment(hc, *stcm.chain_records(hc), 300, True) for hc in hcs]
    assert wants[0][2][0] != wants[1][2][0] and all(int(w[2][0]) > 600 for w in wants)
    size = max(hc.buf.size for hc in hcs) + 16
    n_segs = max(hc.n_segs for hc in hcs)
    out_cap = max(int(w[2][0]) for w in wants) + 3
    out_bytes = max(int(w[2][1]) for w in wants) + 5
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    segs = torch.zeros(2 * n_segs, dtype=torch.int32, device="cuda")
    chain_first = torch.zeros(513, dtype=torch.int32, device="cuda")
    dc = engine.DeviceChains(buf, segs, chain_first, 512)
    recs = [engine.alloc_records(512), engine._bytes(512, 16, "cuda"), engine.alloc_records(512)]
    orecs = [engine.alloc_records(out_cap), engine._bytes(out_cap, 16, "cuda"),
             engine.alloc_records(out_cap)]
    o = Outputs(torch, 512, out_cap, out_bytes, True)

    def load(hc):
        buf.zero_()
        segs.zero_()                                   # the table's tail: segments of no chain
        buf[:hc.buf.size].copy_(torch.from_numpy(hc.buf.copy()))
        segs[:2 * hc.n_segs].copy_(torch.from_numpy(hc.segs.view(np.int32).reshape(-1).copy()))
        chain_first.copy_(torch.from_numpy(hc.chain_first.view(np.int32).copy()))

    def fn():
        engine.parse_tunnel_chains(dc, sm.F6, *recs)
        odb, _, _ = o.call(dc, *recs, 300)
        engine.parse_tunnel_batch(odb, sm.F6, *orecs)

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
        want = oracle.tunnel_batch(blob, out_cap, sm.F6, offsets=offs)
        for g, w, view in zip(orecs, want, (as_records, as_tunnels, as_records)):
            assert view(g.cpu().numpy()).tobytes() == w.tobytes()


def test_cpp_vtep_tx_chains_through_c_abi(torch):
    """examples/vtep_tx_chains: a C++ VTEP (C ABI only) lays four VXLAN frames around 32 KB inner
    TCP payloads out as chains of sixteen 2048-B data rooms, cuts them at mss 1448 and verifies
    all four sums of every output."""
    from rpkt_amd.build import VTEP_TX_CHAINS_BIN
    r = subprocess.run([VTEP_TX_CHAINS_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "out: 92 frames" in r.stdout and "all four sums valid" in r.stdout, r.stdout
    assert r.stdout.count("in 16 mbufs") == 4


def super_chain():
    f = stm.cut_frames(4000)[0]
    return f, scm.chains_of([f], [scm.room_cuts(f, 2048)], shuffle=False)


def test_engine_refuses_bad_arguments(torch):
    f, hc = super_chain()
    dc = engine.DeviceChains.from_host(hc)
    recs = engine.parse_tunnel_chains(dc, 3)
    for mss in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.segment_tunnel_chains(dc, *recs, mss, out_cap=8, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.segment_tunnel_chains(dc, *recs, 1024, out_cap=0, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.segment_tunnel_chains(dc, recs[0], recs[1][:8], recs[2], 1024)
    odb, first, totals = engine.segment_tunnel_chains(dc, *recs, 1024)
    assert totals.cpu().tolist() == [4, 4000 + 4 * 104] and first.cpu().tolist() == [0, 4]


def test_default_sizes_come_from_the_documented_bound(torch):
    """engine.segment_tunnel_chains with no outputs given sizes them from the bound with the
    arena's size for frames_bytes (the mbuf layout's segments do not overlap): never an
    overflow."""
    hc = gen.make_chains(13, 512, layout="mbuf")
    out, first, totals = stcm.segment(hc, *stcm.chain_records(hc), 300, True)
    dc = engine.DeviceChains.from_host(hc)
    odb, gs, gt = engine.segment_tunnel_chains(dc, *engine.parse_tunnel_chains(dc, sm.F6), 300, udp=True)
    assert odb.n == hc.n + hc.buf.size // 300 and odb.n >= int(totals[0]) > hc.n
    assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
    assert odb.frames.numel() >= int(totals[1])
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), first)
    blob, offs = sm.packed_output(out, odb.n)
    assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)
