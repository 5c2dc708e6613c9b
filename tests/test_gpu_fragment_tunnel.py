"""GPU parity of rpkt_gpu_fragment_tunnel_batch: the output frames, offsets, frag_first and totals
byte for byte against tests/fragment_tunnel_model.py, every output pre-filled with 0xa5 and
followed by guard elements that must stay 0xa5, the inputs unchanged by the call, and the GPU's
tunnel parse of the GPU's output equal to the oracle's tunnel parse of the model's."""
import functools
import subprocess

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen, graphs
from rpkt_amd.records import as_records, as_tunnels, dispatch_ethertype

import fragment_model as fm
import fragment_tunnel_model as ftm
import reassemble_model as rm
import reframe_check as rc
import segment_model as sm

pytestmark = pytest.mark.gpu

K_SEG_BLOCK = 256                              # frames a plan block (rpkt_segcopy.h kSegBlock)
IDENT = 0xfffffff0                             # wraps inside a batch
FLAGS = [(False, False), (True, False), (False, True), (True, True)]    # (ignore_df, outer_fallback)
ETHER = bytes.fromhex("02000000000a02000000000b0800")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def Outputs(torch, n, out_cap, out_bytes, ignore_df, fallback, ip6_ident=IDENT):
    return rc.Outputs(torch, n, out_cap, out_bytes,
                      functools.partial(engine.fragment_tunnel_batch, ignore_df=ignore_df,
                                        outer_fallback=fallback, ip6_ident=ip6_ident),
                      engine.fragment_tunnel_workspace(n), "frag_first")


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


def check_case(torch, hb, mtu, want, ignore_df, fallback, out_cap=None, out_bytes=None, what="",
               parse=True, records=None, ip6_ident=IDENT):
    """One call on hb at mtu against the model's `want` = (out_frames, frag_first, totals).
    out_cap / out_bytes default to a little more than the totals; smaller ones overflow."""
    out, first, totals = want
    out_cap = int(totals[0]) + 5 if out_cap is None else out_cap
    out_bytes = int(totals[1]) + 7 if out_bytes is None else out_bytes
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, sm.F6) if records is None else records
    before = [t.clone() for t in (db.frames,) + tuple(recs)]
    o = Outputs(torch, hb.n, out_cap, out_bytes, ignore_df, fallback, ip6_ident)
    odb, _, _ = o.call(db, *recs, mtu)
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
    """(mtu, ignore_df, fallback) -> (frames, the model's output with ip6_ident IDENT + 1: the
    frames' indices behind a lead frame)."""
    res = {}
    for mtu in ftm.MTU_VALUES:
        frames = ftm.hand_frames(mtu)
        hb = sm.pack(frames)
        recs = ftm.tunnel_records(hb)
        for df, fb in FLAGS:
            res[mtu, df, fb] = (frames, {lead: ftm.fragment(hb, *recs, mtu, df, fb, IDENT + lead)
                                         for lead in (0, 1)})
    return res


@pytest.mark.parametrize("lead", list(range(16)))
def test_hand_built_frames(torch, hand, lead):
    """VXLAN, GTP-U and GRE over IPv4 and IPv6 around IPv4 with and without options, tags, GTP-U
    extension headers, GRE with C and K, a zero outer UDP checksum, padding, inner DF, inner
    fragments, the frames that are not inner-cut and plain frames, at every 16-B source phase,
    every mtu and the four flag combinations."""
    for mtu in ftm.MTU_VALUES:
        for df, fb in FLAGS:
            frames, wants = hand[mtu, df, fb]
            # behind a lead frame every index, and with it ip6_ident + i, moves by one
            want = with_lead(wants[1 if lead else 0], lead)
            check_case(torch, sm.pack(frames, lead), mtu, want, df, fb,
                       what="mtu %d df %d outer %d lead %d" % (mtu, df, fb, lead))


@pytest.fixture(scope="module")
def config13():
    hb = gen.make_batch(13, n=2048, seed=3)
    return hb, ftm.tunnel_records(hb)


@pytest.mark.parametrize("mtu,fallback", [(576, False), (576, True), (120, False), (120, True)])
def test_config_13(torch, config13, mtu, fallback):
    hb, recs = config13
    want = ftm.fragment(hb, *recs, mtu, True, fallback, IDENT)
    kinds, outer_cuts = ftm.cut_kinds(want[1], recs[1], ftm.inner_cuts(hb, *recs, mtu, True))
    assert min(kinds.values()) >= 100 and (outer_cuts > 0) == fallback, kinds
    check_case(torch, hb, mtu, want, True, fallback, what="config 13 mtu %d outer %d" % (mtu, fallback))


def test_config_13_without_ignore_df_is_a_copy(torch, config13):
    hb, recs = config13
    want = ftm.fragment(hb, *recs, 576, False, True, IDENT)
    assert want[0] == sm.frames_of(hb)
    check_case(torch, hb, 576, want, False, True, what="config 13 copy")


def test_config_14_fuzz(torch):
    """Every tunnel status and every parse status at both levels passes through or is cut."""
    hb = gen.make_batch(14, n=4096, seed=3)
    recs = ftm.tunnel_records(hb)
    assert len(np.unique(recs[1]["status"])) >= 4
    want = ftm.fragment(hb, *recs, 120, True, True, IDENT)
    kinds, outer_cuts = ftm.cut_kinds(want[1], recs[1], ftm.inner_cuts(hb, *recs, 120, True))
    assert min(kinds.values()) >= 100 and outer_cuts >= 100
    check_case(torch, hb, 120, want, True, True, what="config 14")


@pytest.mark.parametrize("ident", [0, 0xfffffff0])
def test_without_tunnels_the_output_is_fragment_batch_s(torch, config13, ident):
    """Every tun kind NONE: byte for byte what engine.fragment_batch writes with the outer
    records."""
    hb = sm.pack(sm.frames_of(config13[0])[:1024] + list(fm.hand_frames(300)) * 3)
    db = engine.DeviceBatch.from_host(hb)
    outer, tun, inner = engine.parse_tunnel_batch(db, sm.F6)
    none = np.zeros(hb.n, dtype=as_tunnels(tun.cpu().numpy()).dtype)
    none["status"] = 1
    tun = torch.from_numpy(none.view(np.uint8).copy()).cuda()
    cap, nbytes = hb.n + hb.frames.size // 200, 2 * hb.frames.size
    a = Outputs(torch, hb.n, cap, nbytes, True, False, ident)
    b = rc.Outputs(torch, hb.n, cap, nbytes,
                   functools.partial(engine.fragment_batch, ignore_df=True, ip6_ident=ident),
                   engine.fragment_workspace(hb.n), "frag_first")
    a.call(db, outer, tun, inner, 300)
    b.call(db, outer, 300)
    torch.cuda.synchronize()
    ga, gb = a.host(), b.host()
    assert int(gb[3][0]) > hb.n + 1000 and int(gb[3][0]) <= cap and int(gb[3][1]) <= nbytes
    for x, y, name in zip(ga, gb, ("frames", "offsets", "frag_first", "totals")):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("short", ["exact", "cap", "bytes"])
def test_exact_capacities_and_one_short(torch, hand, short):
    """out_cap == n_out and out_bytes == out_bytes_needed: no spare slot, no spare byte.  One
    slot or one byte short: RPKT_OK, frag_first and totals exact, guards intact."""
    frames, wants = hand[120, True, True]
    want = with_lead(wants[1], 5)
    n_out, need = int(want[2][0]), int(want[2][1])
    cap, nbytes = {"exact": (n_out, need), "cap": (n_out - 1, need), "bytes": (n_out, need - 1)}[short]
    check_case(torch, sm.pack(frames, 5), 120, want, True, True, out_cap=cap, out_bytes=nbytes,
               what=short)


def test_three_plan_blocks(torch):
    """600 distinct frames that are cut, inner or outer: three plan blocks of 256, several write
    runs a frame."""
    wraps = [w for _, _, w in ftm.BASE]
    frames = [wraps[k % 3](fm.udp4(700 + k, ident=k, options=fm.OPTIONS_MIX if k % 5 == 0 else b""))
              if k % 7 else fm.udp4(900 + k, ident=k) for k in range(600)]
    assert len(set(frames)) == 600 and len(frames) > 2 * K_SEG_BLOCK
    hb = sm.pack(frames)
    recs = ftm.tunnel_records(hb)
    want = ftm.fragment(hb, *recs, 120, False, False, IDENT)
    per = np.diff(want[1].astype(np.int64))
    assert (per > 8).all() and ftm.inner_cuts(hb, *recs, 120, False).sum() == 600 - 86
    check_case(torch, hb, 120, want, False, False, what="three plan blocks")


def test_strided_input(torch):
    """frame_len < stride, at a stride that is no multiple of 16."""
    stride = 1101
    wraps = [w for _, _, w in ftm.BASE]
    frames = [wraps[0](fm.udp4(1000, ident=k)) if k % 2 else wraps[1](fm.udp4(1014, ident=k))
              for k in range(75)]
    flen = len(frames[0])
    assert all(len(f) == flen for f in frames) and flen < stride
    buf = np.full(len(frames) * stride + 16, 0xee, dtype=np.uint8)
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + flen] = np.frombuffer(f, dtype=np.uint8)
    hb = gen.HostBatch(0, len(frames), 0, buf, None, stride, flen)
    want = ftm.fragment(hb, *ftm.tunnel_records(hb), 400, False, False, IDENT)
    assert int(want[2][0]) >= 3 * hb.n
    check_case(torch, hb, 400, want, False, False, what="stride %d" % stride)
    packed = sm.pack(frames)
    assert want[0] == ftm.fragment(packed, *ftm.tunnel_records(packed), 400, False, False, IDENT)[0]


@pytest.mark.parametrize("fallback", [False, True])
def test_records_of_another_batch(torch, hand, fallback):
    """The three record arrays rolled by one frame: RPKT_OK, nothing written outside the
    buffers, and the bytes the model gives for the same wrong records."""
    frames, _ = hand[120, True, fallback]
    hb = sm.pack(frames)
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, sm.F6)
    rolled = [t.view(hb.n, -1).roll(1, 0).contiguous().view(-1) for t in recs]
    host = [view(t.cpu().numpy()) for t, view in zip(rolled, (as_records, as_tunnels, as_records))]
    want = ftm.fragment(hb, *host, 120, True, fallback, IDENT)
    check_case(torch, hb, 120, want, True, fallback, what="rolled records", parse=False,
               records=rolled)


def test_graph_capture(torch):
    """Tunnel parse, fragment, tunnel parse of the output over out_cap slots, captured as one
    graph and replayed on two inputs."""
    hbs = [sm.pack(sm.frames_of(gen.make_batch(13, 512, seed=s))) for s in (5, 55)]
    wants = [ftm.fragment(hb, *ftm.tunnel_records(hb), 300, True, True, IDENT) for hb in hbs]
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
    o = Outputs(torch, 512, out_cap, out_bytes, True, True)

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


def test_inverse_on_the_device(torch, hand):
    """The DF-clear hand frames that are inner-cut: the inner packets of the GPU's outputs,
    sliced on the host and put behind an Ethernet header, go through engine.parse_batch ->
    engine.reassemble_batch in arrival order and come out as the original inner packets."""
    mtu = 120
    frames, _ = hand[mtu, False, False]
    hb = sm.pack(frames)
    outer, tun, inner = ftm.tunnel_records(hb)
    mask = ftm.inner_cuts(hb, outer, tun, inner, mtu, False)
    assert mask.sum() >= 20
    db = engine.DeviceBatch.from_host(hb)
    odb, gfirst, gtot = engine.fragment_tunnel_batch(db, *engine.parse_tunnel_batch(db, sm.F6), mtu)
    torch.cuda.synchronize()
    first = gfirst.cpu().numpy().view(np.uint32)
    offs = odb.offsets.cpu().numpy().view(np.uint32)
    blob = odb.frames.cpu().numpy().tobytes()
    pieces, originals = [], []
    for i in np.nonzero(mask)[0]:
        il3 = int(inner[i]["l3_off"])
        L = int.from_bytes(frames[i][il3 + 2:il3 + 4], "big")
        assert ftm.df_clear(frames[i], inner[i])
        originals.append(ETHER + frames[i][il3:il3 + L])
        pieces += [ETHER + blob[int(offs[j]) + il3:int(offs[j + 1])]
                   for j in range(int(first[i]), int(first[i + 1]))]
    assert len(pieces) > 3 * len(originals)
    pb = sm.pack(pieces)
    pdb = engine.DeviceBatch.from_host(pb)
    rdb, _, rtot = engine.reassemble_batch(pdb, engine.parse_batch(pdb, sm.F6))
    torch.cuda.synchronize()
    n_out, need = (int(x) for x in rtot.cpu().numpy().view(np.uint64)[:2])
    assert n_out == len(originals)
    want_blob, want_offs = sm.packed_output(originals, rdb.n)
    assert np.array_equal(rdb.offsets.cpu().numpy().view(np.uint32), want_offs)
    assert np.array_equal(rdb.frames.cpu().numpy()[:need], want_blob)
    # the model's reassembly agrees
    assert rm.reassemble(pb, sm.oracle_records(pb))[0] == originals


def test_default_sizes_come_from_the_documented_bound(torch, hand):
    """engine.fragment_tunnel_batch with no outputs given never overflows on the hand frames."""
    for mtu in (78, 120, 1500):
        frames, wants = hand[mtu, True, True]
        out, first, totals = wants[0]
        db = engine.DeviceBatch.from_host(sm.pack(frames))
        odb, gs, gt = engine.fragment_tunnel_batch(db, *engine.parse_tunnel_batch(db, sm.F6), mtu,
                                                   ignore_df=True, outer_fallback=True, ip6_ident=IDENT)
        assert gt.cpu().numpy().view(np.uint64).tolist() == [int(totals[0]), int(totals[1])]
        assert odb.n >= int(totals[0]) and odb.frames.numel() >= int(totals[1])
        blob, offs = sm.packed_output(out, odb.n)
        assert np.array_equal(odb.offsets.cpu().numpy().view(np.uint32), offs)
        assert np.array_equal(odb.frames.cpu().numpy()[:int(totals[1])], blob)


def test_cpp_vtep_prefrag_tx_through_c_abi(torch):
    """examples/vtep_prefrag_tx: 1500-byte inner IPv4/UDP frames behind VXLAN and GTP-U,
    pre-fragmented at mtu 1500 and parsed back through the C ABI only; the example checks its
    own outputs."""
    from rpkt_amd.build import VTEP_PREFRAG_TX_BIN
    r = subprocess.run([VTEP_PREFRAG_TX_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: 2 tunnel packets a frame" in r.stdout, r.stdout


def test_engine_refuses_bad_arguments(torch):
    hb = sm.pack([ftm.BASE[0][2](fm.udp4(3000))])
    db = engine.DeviceBatch.from_host(hb)
    recs = engine.parse_tunnel_batch(db, 3)
    for mtu in (0, 65536):
        with pytest.raises(engine.RpktError):
            engine.fragment_tunnel_batch(db, *recs, mtu, out_cap=8, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.fragment_tunnel_batch(db, *recs, 1500, out_cap=0, out_bytes=8192)
    with pytest.raises(engine.RpktError):
        engine.fragment_tunnel_batch(db, recs[0], recs[1][:8], recs[2], 1500)
    odb, first, totals = engine.fragment_tunnel_batch(db, *recs, 1500)
    # mtu' 1450, c 1424: 3000 bytes of inner IP payload in three slices behind 84 header bytes
    assert totals.cpu().tolist() == [3, 3000 + 3 * 84] and first.cpu().tolist() == [0, 3]
