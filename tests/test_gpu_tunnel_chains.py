"""GPU parity of rpkt_gpu_parse_tunnel_chains against tests/tunnel_chain_model.py (the two
committed oracles composed over the Pbuf rules): the outer record, the rpkt_tun_t and the
inner record of every chain, and the flow events, byte for byte."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine, gen
from rpkt_amd.records import F_IPV6, TUN_STATUS, as_records, as_tunnels

import tunnel_chain_model as model
import tunnel_frames as tf

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKTS = os.path.join(HERE, "golden", "packets")
F6 = 3 | F_IPV6
TUNNEL_CAPS = ("Vxlan1.dat", "Vxlan2.dat", "gtp-u-1ext.dat", "gtp-u-2ext.dat",
               "gtp_nr_container.dat", "gtp_pdu_session_container.dat", "gtp-c1.dat",
               "GREv0_1.dat", "GREv0_2.dat", "GREv0_3.dat", "GREv0_4.dat", "GREv1_1.dat",
               "GREv1_2.dat", "GREv1_3.dat")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def caps():
    return [oracle.load_dat(os.path.join(PKTS, n)) for n in TUNNEL_CAPS]


def gpu(hc, flags, **kw):
    dc = engine.DeviceChains.from_host(hc)
    out = engine.parse_tunnel_chains(dc, flags, **kw)
    o, t, i = (x.cpu().numpy() for x in out[:3])
    return (as_records(o), as_tunnels(t), as_records(i)) + tuple(out[3:])


def same(got, want, what="model"):
    for name, g, w in zip(("outer", "tun", "inner"), got, want):
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g != w)[0]
            k = int(bad[0])
            raise AssertionError("%d %s records differ from the %s; first #%d gpu=%s want=%s" % (
                bad.size, name, what, k, g[k], w[k]))


def check(hc, flags):
    want = model.tunnel_chains(hc.buf, hc.segs, hc.chain_first, flags)
    same(gpu(hc, flags)[:3], want)
    return want


def flat(frames, flags):
    offs = np.zeros(len(frames) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(f) for f in frames])
    buf = np.frombuffer(b"".join(frames) + bytes(16), dtype=np.uint8)
    return oracle.tunnel_batch(buf, len(frames), flags, offsets=offs)


@functools.lru_cache(maxsize=None)
def fuzz_chains(seed):
    return gen.make_chains(14, n=4096, seed=seed, layout="fuzz")


@pytest.mark.parametrize("flags", [3, 11, 1])
@pytest.mark.parametrize("seed", [14, 141, 142])
def test_tunnel_fuzz_chains(torch, seed, flags):
    """Config 14 cut at random and header-boundary positions: cuts inside the tunnel header
    and inside the inner headers, empty segments, odd slot alignments; every tunnel status."""
    o, t, i = check(fuzz_chains(seed), flags)
    assert len(np.unique(t["status"])) == 6


def test_mbuf_layout_equals_the_flat_oracle(torch):
    """Config 13 in 2048-B mbufs: every header in segment 0, so the records are the flat
    frames' (the committed C oracle) as well as the model's."""
    hc = gen.make_chains(13, n=4096, layout="mbuf")
    frames = [hc.frame(p) for p in range(hc.n)]
    got = gpu(hc, 11)[:3]
    same(got, flat(frames, 11), "flat oracle")
    same(got, model.tunnel_chains(hc.buf, hc.segs, hc.chain_first, 11))
    assert (got[1]["status"] == TUN_STATUS["OK"]).all()


@pytest.mark.parametrize("odd", [False, True])
def test_jumbo_tunnels_in_mbuf_segments(torch, odd):
    """Tunnelled jumbo frames (up to 60 KB) in 2048-B segments, 2-30 per chain: the long
    stream; with odd segment lengths the odd-byte pairing across every boundary."""
    rng = np.random.default_rng(3)
    frames = tf.jumbo_frames(n=48)
    lens = []
    for f in frames:
        cuts, c = [], 0
        while c < len(f):
            c += int(rng.integers(500, 1024)) * 2 + 1 if odd else 2048
            cuts.append(c)
        lens.append(model.cut_at(len(f), cuts[:-1]))
    hc = model.lay_out(frames, lens, gap=128 - (1 if odd else 0), lead=128)
    assert max(len(x) for x in lens) >= 29
    o, t, i = check(hc, F6)
    assert (t["status"] == TUN_STATUS["OK"]).sum() >= 20


def test_captures_cut_at_every_position(torch):
    """The 14 tunnel captures as two-segment chains cut at every position 1..len-1 (about
    2,000 chains in one launch)."""
    frames, lens = [], []
    for f in caps():
        for c in range(1, len(f)):
            frames.append(f)
            lens.append([c, len(f) - c])
    o, t, i = check(model.lay_out(frames, lens), F6)
    assert len(np.unique(t["status"])) >= 5


def test_inner_ip6_extension_headers_cut_at_every_position(torch):
    """VXLAN, GTP-U and GRE around an inner IPv6/UDP packet with a hop-by-hop header, a
    routing header (the pseudo header's final destination) and destination options plus a
    fragment header, as two-segment chains cut at every position 1..len-1 (about 1,800 chains
    in one launch): the IPv6 extension walk on an inner packet, every header in or past
    segment 0's window, whole or cut.  test_tunnel_chain_model.py pins the uncut frames."""
    frames, lens = [], []
    for f in tf.inner_ip6_ext_frames():
        for c in range(1, len(f)):
            frames.append(f)
            lens.append([c, len(f) - c])
    o, t, i = check(model.lay_out(frames, lens), F6)
    assert (i["status"] == 0).sum() >= 9 * 62     # at least the cuts in the 62 data bytes


def test_captures_in_tiny_segments(torch):
    """[2] * k and [1] * len chains: the many-items path of the chain stream."""
    frames, lens = [], []
    for f in caps():
        frames += [f, f]
        lens += [[2] * (len(f) // 2) + [len(f) % 2], [1] * len(f)]
    check(model.lay_out(frames, lens, gap=1), F6)


def test_odd_outers_with_fuzz_cuts(torch):
    """IPv6 outers with extension headers, QinQ, GTP extension chains past the window."""
    rng = np.random.default_rng(9)
    frames = tf.odd_frames(n=256)
    lens = []
    for f in frames:
        k = int(rng.integers(0, 6))
        cuts = rng.integers(0, len(f) + 1, size=k).tolist()
        if k and rng.integers(2):
            cuts[0] = min(int(rng.choice(gen.FUZZ_CUTS6)), len(f))
        lens.append(model.cut_at(len(f), cuts))
    for flags in (F6, 3):
        check(model.lay_out(frames, lens, gap=5), flags)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_ragged_sizes(torch, n):
    check(gen.make_chains(14, n=n, seed=1400 + n, layout="fuzz"), 11)


def test_descriptor_edge_cases(torch):
    """An empty chain, decreasing chain_first, an index past n_segs, a segment clamped at
    the arena end (as test_gpu_chains.py::test_chain_descriptor_edge_cases)."""
    f, g = caps()[0], caps()[2]
    hc = model.lay_out([f, g, f], [[50, len(f) - 50], [len(g)], [34, len(f) - 34]])
    weird = np.array([0, 0, 2, 1, 99, 3, 4, 5], np.uint32)
    w = gen.HostChains(None, weird.size - 1, None, hc.buf, hc.segs, weird, None)
    check(w, F6)
    segs2 = hc.segs.copy()
    segs2[-1, 1] = 100000
    check(gen.HostChains(None, hc.n, None, hc.buf, segs2, hc.chain_first, None), F6)


@pytest.mark.parametrize("nb", [977, 1])
def test_flow_events(torch, nb):
    hc = fuzz_chains(14)
    o, t, i, ev = gpu(hc, 11 | 4, n_buckets=nb)
    want = model.tunnel_chains(hc.buf, hc.segs, hc.chain_first, 11)
    same((o, t, i), want)
    wev = model.flow_events(*want, nb)
    got = ev.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, wev), int(np.nonzero(got != wev)[0][0])
    c = engine.flow_count(ev, hc.n, nb).cpu().numpy().view(np.uint64)
    assert np.array_equal(c, oracle.flow_count(wev, nb))


def test_single_segment_chains_equal_parse_tunnel_batch(torch):
    hb = gen.make_batch(14, n=5000, seed=77)
    frames = [hb.frames[hb.offsets[k]:hb.offsets[k + 1]].tobytes() for k in range(hb.n)]
    got = gpu(model.lay_out(frames, [[len(x)] for x in frames]), 11)[:3]
    fo, ft, fi = engine.parse_tunnel_batch(engine.DeviceBatch.from_host(hb), 11)
    same(got, (as_records(fo.cpu().numpy()), as_tunnels(ft.cpu().numpy()),
               as_records(fi.cpu().numpy())), "flat entry")


def test_tunnel_views_over_chain_records(torch):
    """rpkt_amd.tunviews over the device records of Vxlan1.dat cut as [42, 8, rest], with the
    chain's bytes concatenated, reads as over the flat frame (test_gpu_tunnel.py)."""
    from rpkt_amd.tunviews import TunnelPacket, Vxlan
    from rpkt_amd.views import EtherFrame, Ipv4, Udp
    f = caps()[0]
    hc = model.lay_out([f], [[42, 8, len(f) - 50]])
    o, t, i = gpu(hc, F6)[:3]
    pk = TunnelPacket(o[0], t[0], i[0], hc.frame(0))
    ip = Ipv4.parse(EtherFrame.parse(pk).unwrap().payload()).unwrap()
    vx = Vxlan.parse(Udp.parse(ip.payload()).unwrap().payload()).unwrap()
    assert vx.vni() == 3000001 and vx.group_id() == 100
    assert Ipv4.parse(EtherFrame.parse(vx.payload()).unwrap().payload()).unwrap().verify_checksum()
