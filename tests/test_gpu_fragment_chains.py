"""GPU parity of rpkt_gpu_fragment_chains (IPv4 / IPv6 fragmentation of mbuf chains): the
output frames, offsets, frag_first and totals byte for byte against
tests/fragment_chains_model.py (tests/fragment_model.py on the flattened chains), with every
output pre-filled with 0xa5 and followed by guard elements that must stay 0xa5, and the
inputs unchanged by the call.  tests/test_fragment_chains_model.py checks on the CPU that each
batch here reaches what it was built to reach.

Two kinds of records drive it: oracle.parse_chains' (what a caller has: a header cut by a
segment boundary is a parse error there, so the chain passes through) and the flat oracle's
records of the flattened bytes (they say "cut" wherever the segment cuts fall, which is the
only way to drive header bytes across arbitrary cuts)."""
import functools

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records

import fragment_chains_model as fcm
import fragment_model as fm
import reframe_check as rc
import segment_model as sm

pytestmark = pytest.mark.gpu

IDENT = fcm.IDENT
RECORDS = fcm.RECORDS


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, ignore_df, ip6_ident):
    return rc.Outputs(torch, n, out_cap, out_bytes,
                      functools.partial(engine.fragment_chains, ignore_df=ignore_df, ip6_ident=ip6_ident),
                      engine.fragment_chains_workspace(n), "frag_first")


def device_records(torch, recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).cuda()


def check_case(torch, hc, recs, mtu, ignore_df=True, ip6_ident=IDENT, out_cap=None, out_bytes=None,
               what="", parse_back=True, want=None):
    """One call on the chains hc with the host records `recs` at mtu against the model.
    out_cap / out_bytes default to a little more than the model's totals (spare slots and
    spare bytes to check); smaller ones overflow.  Returns the model's (out_frames,
    frag_first, totals)."""
    if want is None:
        want = fcm.fragment_chains(hc, recs, mtu, ignore_df, ip6_ident)
    out, first, totals = want
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    dc = engine.DeviceChains.from_host(hc)
    drecs = device_records(torch, recs)
    inputs = (dc.buf, dc.segs, dc.chain_first, drecs)
    before = [t.clone() for t in inputs]
    o = Outputs(torch, hc.n, out_cap, out_bytes, ignore_df, ip6_ident)
    odb, _, _ = o.call(dc, drecs, mtu)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "%s: the inputs were written" % what
    rc.check_outputs(o, odb, out, first, totals, what, parse_back,
                     where=lambda j: "; chain %d" % (int(np.searchsorted(first, j, side="right")) - 1))
    return want


# ---- every cut ---------------------------------------------------------------------------

# which of fcm.cut_frames() each mtu cuts (tests/test_fragment_chains_model.py has the counts)
EVERY_CUT = {36: (0, 1), 68: (1, 2, 3, 4, 5), 120: (6,), 208: (7,)}


@pytest.mark.parametrize("lead", list(range(16)))
def test_every_two_segment_cut(torch, lead):
    """Every cut of eight frames (plain IPv4, ihl 60 behind two tags, an input fragment with MF
    and padding, IPv6 with per-fragment headers of 40, 48 and 184 bytes and an extension walk
    past them) at mtu 36, 68, 120 and 208 and every 16-B arena phase, ip6_ident wrapping inside
    the batch.  With the chain parse's records a cut inside a header passes through; with the
    flat records the header bytes, the option walk, the extension walk and the patched fields
    are gathered across the cut."""
    ranges = fcm.cut_ranges()
    for kind in ("chain", "flat"):
        for mtu in fcm.CUT_MTUS:
            hc, recs, want = fcm.every_cut(lead, kind, mtu)
            check_case(torch, hc, recs, mtu, what="%s records mtu %d lead %d" % (kind, mtu, lead),
                       want=want, parse_back=lead == 0)
            cut = fcm.cut(want[1])
            for k, (lo, hi) in enumerate(ranges):
                share = cut[lo:hi].mean()
                if k not in EVERY_CUT[mtu]:
                    assert share == 0
                else:
                    assert share == 1 if kind == "flat" else 0 < share < 1


def test_three_and_four_segments(torch):
    """An empty first segment, an empty middle one, a 1-byte segment inside a slice, cuts
    exactly at the header's end and at slice ends, alone and together: an IPv4 frame with
    options at mtu 68 and 76, an IPv6 frame behind hop-by-hop and routing headers at 68 and 76
    (its per-fragment headers leave no room there: every chain passes through) and at 104,
    where it is cut."""
    for f, hs, mtu, c in fcm.multi_cases():
        cuts = fcm.multi_cuts(hs, c)
        is_cut = not (hs == 86 and mtu < 104)
        for lead in (0, 5):
            hc = fcm.chains_of([f] * len(cuts), cuts, lead=lead, seed=hs + mtu)
            for kind in ("chain", "flat"):
                _, first, _ = check_case(torch, hc, RECORDS[kind](hc), mtu,
                                         what="%s records hs %d mtu %d lead %d" % (kind, hs, mtu, lead))
                got = fcm.cut(first)
                assert (got.all() if kind == "flat" else got[7:12].all()) == is_cut


@pytest.mark.parametrize("room", [61, 64, 2048])
def test_hand_built_frames_in_data_rooms(torch, room):
    """tests/fragment_model.py's hand-built set for every mtu, each frame laid out as an mbuf
    chain with data rooms of 61, 64 and 2048 bytes, with and without ignore_df: slices cross
    several segments, and at the small rooms most headers cross them too."""
    for mtu in fm.MTU_VALUES:
        frames = fm.hand_frames(mtu)
        hc = fcm.chains_of(frames, [fcm.room_cuts(f, room) for f in frames], lead=room & 15, seed=mtu)
        for kind in ("chain", "flat"):
            recs = RECORDS[kind](hc)
            for ignore_df in (False, True):
                _, _, totals = check_case(torch, hc, recs, mtu, ignore_df,
                                          what="%s records room %d mtu %d df %d" % (kind, room, mtu, ignore_df))
                assert (int(totals[0]) > hc.n) == (mtu < 65535)


# ---- the generator's configs ------------------------------------------------------------

@pytest.fixture(scope="module")
def config7():
    hc = gen.make_chains(7, 1024, layout="mbuf")
    recs = fcm.chain_records(hc)
    return hc, recs, fcm.fragment_chains(hc, recs, 1500, True, IDENT)


def test_config_7_jumbo_frames_in_mbufs(torch, config7):
    """jumboframe_tx.rs: 8000-byte frames in 2048-byte data rooms.  With the flag every chain is
    cut at 1500; without it none is, and the output is the flattened input."""
    hc, recs, want = config7
    assert fcm.cut(want[1]).all() and int(want[2][0]) == 6144
    check_case(torch, hc, recs, 1500, what="config 7", want=want)
    copy = fcm.fragment_chains(hc, recs, 1500, False, IDENT)
    assert not fcm.cut(copy[1]).any() and copy[0] == fcm.chain_bytes(hc)
    check_case(torch, hc, recs, 1500, False, what="config 7 without the flag", want=copy)


@pytest.mark.parametrize("config,share", [(11, 0.5), (5, 0.4)])
def test_configs_with_options_and_dual_stack(torch, config, share):
    """Fuzz layout: up to six segments cut anywhere.  The chain parse's own records reach the
    gathered header: a header may start exactly where a segment ends."""
    hc = gen.make_chains(config, 2048, layout="fuzz")
    recs = fcm.chain_records(hc)
    want = fcm.fragment_chains(hc, recs, 300, True, IDENT)
    assert fcm.cut(want[1]).mean() >= share
    assert fcm.header_past_first_segment(hc, recs, want[1]) >= 1
    check_case(torch, hc, recs, 300, what="config %d" % config, want=want)


def test_config_6_fuzz(torch):
    """Every parse status passes through or is cut."""
    hc = gen.make_chains(6, 4096, layout="fuzz")
    recs = fcm.chain_records(hc)
    assert len(np.unique(recs["status"])) >= 15
    want = fcm.fragment_chains(hc, recs, 100, True, IDENT)
    assert fcm.cut(want[1]).any()
    check_case(torch, hc, recs, 100, what="config 6", want=want)


# ---- against the flat entry, capacities, the scan ------------------------------------------

def test_single_segment_chains_equal_fragment_batch(torch):
    """One segment per chain: every output equals rpkt_gpu_fragment_batch's on the same bytes
    and the same device records, GPU against GPU, guards included."""
    for mtu, lead in ((68, 5), (1500, 0)):
        hb = sm.pack(fm.hand_frames(mtu), lead)
        hc = fcm.single_segment_chains(hb)
        db, dc = engine.DeviceBatch.from_host(hb), engine.DeviceChains.from_host(hc)
        recs = engine.parse_batch(db, sm.F6)
        _, _, totals = fm.fragment(hb, sm.oracle_records(hb), mtu, True, IDENT)
        a = Outputs(torch, hb.n, int(totals[0]) + 3, int(totals[1]) + 9, True, IDENT)
        b = Outputs(torch, hb.n, int(totals[0]) + 3, int(totals[1]) + 9, True, IDENT)
        a.call(db, recs, mtu, fn=functools.partial(engine.fragment_batch, ignore_df=True, ip6_ident=IDENT))
        b.call(dc, recs, mtu)
        torch.cuda.synchronize()
        for x, y, name in zip(a.host(), b.host(), ("frames", "offsets", "frag_first", "totals")):
            assert np.array_equal(x, y), "mtu %d: %s differ" % (mtu, name)
        assert b.host()[3][:2].tolist() == [int(totals[0]), int(totals[1])]


@pytest.fixture(scope="module")
def rooms64():
    frames = fm.hand_frames(68)
    hc = fcm.chains_of(frames, [fcm.room_cuts(f, 64) for f in frames], lead=3, seed=64)
    recs = fcm.flat_records(hc)
    return hc, recs, fcm.fragment_chains(hc, recs, 68, True, IDENT)


@pytest.mark.parametrize("short", ["exact", "cap", "bytes", "both"])
def test_capacities(torch, rooms64, short):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte.  One
    slot short, one byte short, (1, 16): RPKT_OK, frag_first and totals exact, nothing written
    past the capacities."""
    hc, recs, want = rooms64
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"exact": (n_out, need), "cap": (n_out - 1, need), "bytes": (n_out, need - 1),
                   "both": (1, 16)}[short]
    check_case(torch, hc, recs, 68, out_cap=cap, out_bytes=nbytes, what=short, want=want)


def test_scan_across_blocks(torch):
    """70,000 chains of 64..200 B in two or three segments at mtu 68 with the flag: the prefix
    sums cross the 256-chain blocks and the 256-block carry of the block sums' scan.  700
    distinct chains (UDP over IPv4 / IPv6 of every length, and config-6 fuzz frames cut to
    size), their arena, segments and records tiled 100 times: the model's output of the 700 is
    tiled the same way, with each tile's own Fragment header identifications."""
    hc1, recs1, want1 = fcm.scan_block()
    hc, recs, want = fcm.tiled(hc1, recs1, want1, 100)
    assert hc.n == 70000 and 2 * hc.n <= hc.n_segs <= 3 * hc.n
    assert int(want[2][0]) > 2 * hc.n
    check_case(torch, hc, recs, 68, True, 0, what="70,000 chains", want=want, parse_back=False)


# ---- descriptors --------------------------------------------------------------------------

def test_descriptor_edge_cases(torch):
    """chain_first entries past n_segs and decreasing, segment offsets and lengths past
    buf_bytes, two chains sharing a segment: the documented clamps; the model flattens under
    the same ones (tests/test_fragment_chains_model.py)."""
    hc, frames = fcm.descriptor_edge_chains()
    for mtu in (36, 68):
        for kind in ("chain", "flat"):
            _, first, _ = check_case(torch, hc, RECORDS[kind](hc), mtu, what="descriptors, %s records" % kind)
            # chain 0 is cut inside its IPv4 header: fragmented only with the flat records
            assert fcm.cut(first)[[0, 5]].tolist() == [kind == "flat", True]


def test_no_segments_at_all(torch):
    """n_segs == 0 with n_chains > 0 (no arena, no segment table): every chain is empty, every
    output an empty frame."""
    hc = fcm.no_segments(300)
    _, first, totals = check_case(torch, hc, fcm.flat_records(hc), 100, what="no segments")
    assert totals.tolist() == [300, 0] and np.array_equal(first, np.arange(301))


# ---- the inverse ---------------------------------------------------------------------------

def test_reassembly_gives_back_the_chains(torch):
    """engine.reassemble_batch on the fragments gives back the flattened chains byte for byte:
    every frame of hand_frames(576) whose IP packet ends at the frame's end and has neither DF
    nor the reserved bit, in 64-byte rooms.  In arrival order all of them come back, in place.
    engine.reassemble_order tells datagrams apart by (source, destination, identification,
    protocol), and hand_frames' IPv4 datagrams share one identification, so in its order the
    output is checked against tests/reassemble_model.py under that order, and the IPv6 chains
    (identification ip6_ident + p) and the chains that were not cut come back whole."""
    import reassemble_model as rm
    frames = fcm.inverse_frames(576)
    hc = fcm.chains_of(frames, [fcm.room_cuts(f, 64) for f in frames], lead=3, seed=576)
    dc = engine.DeviceChains.from_host(hc)
    assert fcm.chain_bytes(hc) == frames
    for kind in ("chain", "flat"):
        recs = RECORDS[kind](hc)
        out, first, totals = fcm.fragment_chains(hc, recs, 576, False, IDENT)
        assert fcm.cut(first).sum() >= 17
        odb, _, gt = engine.fragment_chains(dc, device_records(torch, recs), 576, ip6_ident=IDENT,
                                            out_cap=int(totals[0]), out_bytes=int(totals[1]))
        assert gt.cpu().tolist() == [int(totals[0]), int(totals[1])]
        orecs = engine.parse_batch(odb, sm.F6)
        hb = sm.pack(out)
        hrecs = sm.oracle_records(hb)

        def reassembled(order):
            rdb, _, rt = engine.reassemble_batch(odb, orecs, order=order)
            n, nbytes = rt.cpu().tolist()
            offs = rdb.offsets.cpu().numpy().view(np.uint32)[:n + 1]
            blob = rdb.frames.cpu().numpy()[:nbytes].tobytes()
            return [blob[int(offs[k]):int(offs[k + 1])] for k in range(n)]

        assert reassembled(None) == frames, kind
        order = engine.reassemble_order(engine.reassemble_keys(odb, orecs))
        keyed = reassembled(order)
        assert keyed == rm.reassemble(hb, hrecs, order.cpu().numpy().view(np.uint32))[0]
        sure = [f for f, c in zip(frames, fcm.cut(first)) if not c or f[12:14] == b"\x86\xdd"]
        assert len(sure) >= 20 and all(f in keyed for f in sure)


# ---- graph, example, engine ------------------------------------------------------------------

def test_graph_capture(torch):
    """Chain parse, fragmentation, parse of the flat output over out_cap slots, captured as one
    graph and replayed on two inputs with different totals: no host step between the three."""
    hcs = [gen.make_chains(5, 512, seed=s, layout="fuzz") for s in (5, 55)]
    wants = [fcm.fragment_chains(hc, fcm.chain_records(hc), 300, True, IDENT) for hc in hcs]
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
    o = Outputs(torch, 512, out_cap, out_bytes, True, IDENT)

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


def test_cpp_frag_tx_chains_through_c_abi(torch):
    """examples/frag_tx_chains: an 8000-byte UDP/IPv4 datagram in 2048-byte data rooms, parsed as
    a chain, fragmented at 1500, parsed back and reassembled through the C ABI only; the example
    checks its own fragments and the reassembled frame."""
    import subprocess
    from rpkt_amd.build import FRAG_TX_CHAINS_BIN
    r = subprocess.run([FRAG_TX_CHAINS_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: 6 fragments from a 4-segment chain, header sums valid, reassembled" in r.stdout


def test_engine_refuses_bad_arguments(torch):
    f = fm.udp4(3000)
    hc = fcm.chains_of([f], [[2048]], shuffle=False)
    dc = engine.DeviceChains.from_host(hc)
    recs = engine.parse_chains(dc, 3)
    for mtu in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.fragment_chains(dc, recs, mtu, out_cap=8, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.fragment_chains(dc, recs, 1500, out_cap=0, out_bytes=8192)
    odb, first, totals = engine.fragment_chains(dc, recs, 1500)
    assert totals.cpu().tolist() == [3, 3000 + 3 * 34] and first.cpu().tolist() == [0, 3]


def test_default_sizes_come_from_the_documented_bound(torch, config7):
    """engine.fragment_chains with no outputs given sizes them from the bound with the arena's
    size for frames_bytes (the mbuf layout's segments do not overlap): never an overflow."""
    hc, recs, (out, first, totals) = config7
    dc = engine.DeviceChains.from_host(hc)
    odb, gs, gt = engine.fragment_chains(dc, engine.parse_chains(dc, sm.F6), 1500, ignore_df=True,
                                         ip6_ident=IDENT)
    assert odb.n == hc.n + hc.buf.size // ((1500 - 68) & ~7) and odb.n >= int(totals[0])
    assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
    assert odb.frames.numel() >= int(totals[1])
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), first)
    blob, offs = sm.packed_output(out, odb.n)
    assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)
