"""tests/tunnel_chain_model.py (the reference model of rpkt_gpu_parse_tunnel_chains) pinned
to the committed oracles, all three record arrays byte for byte: single-segment chains and
chains cut only where the Pbuf rules change nothing equal oracle.tunnel_batch on the flat
frames; a cut inside a tunnel header or a GTP-U extension header is T_BAD / T_EXT_BAD, as
the reference's parses return Err over a Pbuf whose chunk ends inside the header."""
import os

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import gen
from rpkt_amd.records import F_IPV6, STATUS, TUN_KIND, TUN_STATUS, ip6_block

import tunnel_chain_model as model
import tunnel_frames as tf

HERE = os.path.dirname(os.path.abspath(__file__))
PKTS = os.path.join(HERE, "golden", "packets")
F6 = 3 | F_IPV6
TUNNEL_CAPS = ("Vxlan1.dat", "Vxlan2.dat", "gtp-u-1ext.dat", "gtp-u-2ext.dat",
               "gtp_nr_container.dat", "gtp_pdu_session_container.dat", "gtp-c1.dat",
               "GREv0_1.dat", "GREv0_2.dat", "GREv0_3.dat", "GREv0_4.dat", "GREv1_1.dat",
               "GREv1_2.dat", "GREv1_3.dat")


def caps():
    return [oracle.load_dat(os.path.join(PKTS, n)) for n in TUNNEL_CAPS]


def cap(name):
    return oracle.load_dat(os.path.join(PKTS, name))


def flat(frames, flags):
    """oracle.tunnel_batch on the frames, packed."""
    offs = np.zeros(len(frames) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(f) for f in frames])
    buf = np.frombuffer(b"".join(frames) + bytes(16), dtype=np.uint8)
    return oracle.tunnel_batch(buf, len(frames), flags, offsets=offs)


def same(got, want, what=""):
    for name, g, w in zip(("outer", "tun", "inner"), got, want):
        if g.tobytes() != w.tobytes():
            k = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s %s record #%d: model=%s oracle=%s" % (what, name, k, g[k], w[k]))


def run(hc, flags):
    return model.tunnel_chains(hc.buf, hc.segs, hc.chain_first, flags)


def frames_of(hb):
    return [hb.frames[hb.offsets[i]:hb.offsets[i + 1]].tobytes() for i in range(hb.n)]


@pytest.mark.parametrize("flags", [3, 11, 1])
def test_single_segment_chains_equal_the_flat_oracle(flags):
    for frames in (frames_of(gen.make_batch(14, 4000)), tf.odd_frames(n=64), caps()):
        hc = model.lay_out(frames, [[len(f)] for f in frames])
        same(run(hc, flags), flat(frames, flags), "flags %d" % flags)


def header_starts(f, flags):
    """14, the outer l4_off, tun_off, inner_off, each GTP extension header's start and the
    inner l3_off / l4_off / payload_off of a capture: the cuts that change no chunk test."""
    o, t, i = (x[0] for x in flat([f], flags))
    cuts = {14, int(o["l4_off"]), int(t["tun_off"]), int(t["inner_off"]), int(i["l3_off"]),
            int(i["l4_off"]), int(i["payload_off"])}
    if t["kind"] == TUN_KIND["GTPU"] and (f[t["tun_off"]] & 4):
        c, nxt = int(t["tun_off"]) + 12, f[int(t["tun_off"]) + 11]
        while nxt and c < int(t["inner_off"]):
            cuts.add(c)
            hl = 4 if nxt in (0x40, 0xc0, 0x20) else (8 if nxt in (0x03, 0x82) else f[c] * 4)
            nxt = f[c + hl - 1]
            c += hl
    return sorted(c for c in cuts if 0 < c < len(f))


@pytest.mark.parametrize("flags", [3, F6])
def test_cuts_at_header_starts_and_in_the_payload_change_nothing(flags):
    rng = np.random.default_rng(5)
    frames, lens = [], []
    for f in caps():
        hs = header_starts(f, flags)
        pay = int(flat([f], flags)[2][0]["payload_off"])      # 0: no inner payload to cut
        for k in range(8):
            pick = [c for c in hs if rng.integers(2)]
            if pay:
                pick += rng.integers(pay, len(f) + 1, size=int(rng.integers(0, 3))).tolist()
            frames.append(f)
            lens.append(model.cut_at(len(f), pick))
        frames.append(f)
        lens.append(model.cut_at(len(f), hs))         # every header in a segment of its own
    same(run(model.lay_out(frames, lens), flags), flat(frames, flags))


@pytest.mark.parametrize("name,inside", [("Vxlan1.dat", 7), ("gtp-u-1ext.dat", 11),
                                         ("GREv0_1.dat", 3)])
def test_a_cut_inside_the_tunnel_header_is_t_bad(name, inside):
    f = cap(name)
    ts = int(flat([f], 3)[1][0]["tun_off"])
    c = ts + inside
    # one cut, empty segments at the cut, the header's start in a segment of its own
    hc = model.lay_out([f] * 3, [model.cut_at(len(f), x) for x in ([c], [c, c, c], [ts, c])])
    o, t, i = run(hc, 3)
    assert (t["status"] == TUN_STATUS["BAD"]).all() and (t["tun_off"] == ts).all()
    assert (i["status"] == STATUS["NO_INNER"]).all()
    assert not i.view(np.uint8).reshape(3, 80)[:, 1:].any()
    assert o.tobytes() == oracle.parse_chains(hc.buf, hc.segs, hc.chain_first, 3).tobytes()


def test_a_cut_inside_a_gtp_extension_header_is_t_ext_bad():
    f = cap("gtp-u-1ext.dat")
    ts = int(flat([f], 3)[1][0]["tun_off"])
    ext = ts + 12                                     # the 4-byte ExtPduNumber
    cuts = [[ext + 1], [ext + 3], [ext + 2, ext + 2], [ts, ext + 1]]
    o, t, i = run(model.lay_out([f] * 4, [model.cut_at(len(f), c) for c in cuts]), 3)
    assert (t["status"] == TUN_STATUS["EXT_BAD"]).all() and (t["inner_off"] == ext).all()
    assert (i["status"] == STATUS["NO_INNER"]).all()
    # the cut at the extension header's start and at its end decode
    o, t, i = run(model.lay_out([f], [model.cut_at(len(f), [ext, ext + 4])]), 3)
    same((o, t, i), flat([f], 3))


def test_gtp_packet_len_is_tested_against_remaining_not_chunk():
    """Gtpv1::parse: packet_len <= remaining (gtpv1/generated.rs:33-49) -- a chunk that ends
    after the 12-byte header but before packet_len decodes."""
    f = cap("gtp-u-1ext.dat")
    _, t, i = (x[0] for x in flat([f], 3))
    ts = int(t["tun_off"])
    plen = ((f[ts + 2] << 8) | f[ts + 3]) + 8
    hc = model.lay_out([f, f], [model.cut_at(len(f), [ts + 12]),
                                model.cut_at(len(f), [ts, int(t["inner_off"])])])
    pb = model.Pbuf(hc.buf, hc.segs, hc.chain_first, 0)
    assert pb.chunk_len(ts, ts + plen) == 12 < plen
    same(run(hc, 3), flat([f, f], 3))


def test_inner_ip6_extension_headers_equal_the_flat_oracle():
    """The frames of test_gpu_tunnel_chains.py's every-cut sweep, uncut: the model is the
    flat oracle, every tunnel decodes, and every inner record is an IPv6 one whose parse
    went through the extension walk."""
    frames = tf.inner_ip6_ext_frames()
    assert len(frames) == 9
    got = run(model.lay_out(frames, [[len(f)] for f in frames]), F6)
    same(got, flat(frames, F6))
    o, t, i = got
    assert (t["status"] == TUN_STATUS["OK"]).all()
    assert sorted(t["kind"]) == sorted([TUN_KIND["VXLAN"], TUN_KIND["GTPU"], TUN_KIND["GRE"]] * 3)
    assert (i["status"] == STATUS["OK"]).all()
    assert (ip6_block(i)["ip6_n_ext"] >= 1).all() and (ip6_block(i)["ip_protocol"] == 17).all()
    assert (i["l4_sum"] == 0xffff).all()          # the routing header's final destination too
