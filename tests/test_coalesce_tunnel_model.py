"""tests/coalesce_tunnel_model.py against tests/segment_tunnel_model.py and the oracle's tunnel
parse: coalesce_tunnel(segment_tunnel(F)) == F, every merged output verifies (all four sums),
and the hand cases of the rule, each with its expected grouping.  CPU only."""
import os
import re

import numpy as np
import pytest

from rpkt_amd import engine, gen
from rpkt_amd.records import dispatch_ethertype

import coalesce_tunnel_model as ctm
import segment_model as sm
import segment_tunnel_model as stm
import tunnel_frames as tf
import udp_reframe_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(frames, **kw):
    """(out_frames, src_first[:n_out + 1] as a list, the records) of the model on `frames`."""
    hb = sm.pack(frames)
    recs = stm.tunnel_records(hb)
    out, first, totals, mss = ctm.coalesce(hb, *recs, **kw)
    assert int(totals[0]) == len(out) and int(totals[1]) == sum(len(o) for o in out)
    assert all((int(mss[j]) > 0) == (int(first[j + 1]) - int(first[j]) > 1) for j in range(len(out)))
    return out, [int(x) for x in first[:len(out) + 1]], recs


def segments(frame, mss, udp=False):
    return sm.frames_of(ctm.segment_then_records([frame], mss, udp)[0])


def verify(out, first):
    """Every merged output (first: src_first) decodes and carries valid inner and outer sums."""
    O, T, I = stm.tunnel_records(sm.pack(out))
    o_et, i_et = dispatch_ethertype(O), dispatch_ethertype(I)
    merged = [j for j in range(len(out)) if int(first[j + 1]) - int(first[j]) > 1]
    assert merged
    for j in merged:
        f = out[j]
        if T[j]["kind"] == stm.NONE:
            assert int(O[j]["l4_sum"]) == 0xffff and (o_et[j] == 0x86DD or int(O[j]["ip_sum"]) == 0xffff), j
            continue
        assert T[j]["status"] == 0 and I[j]["status"] == 0, j
        assert int(I[j]["l4_sum"]) == 0xffff and (i_et[j] == 0x86DD or int(I[j]["ip_sum"]) == 0xffff), j
        assert o_et[j] == 0x86DD or int(O[j]["ip_sum"]) == 0xffff, j
        ol4, toff = int(O[j]["l4_off"]), int(T[j]["tun_off"])
        if T[j]["kind"] != stm.GRE and f[ol4 + 6:ol4 + 8] == b"\0\0":
            continue                                        # "no checksum" kept
        if T[j]["kind"] != stm.GRE or f[toff] & 0x80:
            assert int(O[j]["l4_sum"]) == 0xffff, j


@pytest.mark.parametrize("udp", [False, True])
@pytest.mark.parametrize("mss", stm.MSS_VALUES)
def test_coalesce_of_segment_is_the_identity(mss, udp):
    """The cut shapes (the inner and plain UDP ones are cut with the flag only: without it they
    pass through both ways) come back byte for byte, and every output verifies."""
    src = stm.cut_frames(min(2 * mss + 1, 2000))
    hs, recs, first = ctm.segment_then_records(src, mss, udp)
    assert hs.n > 2 * stm.N_CUT_TCP
    out, got_first, totals, out_mss = ctm.coalesce(hs, *recs, udp=udp)
    assert out == src
    assert np.array_equal(got_first[:len(src) + 1], first)          # the groups are the cuts
    cut = np.diff(first.astype(np.int64)) > 1
    assert np.array_equal(out_mss[:len(src)] > 0, cut) and (out_mss[:len(src)][cut] == mss).all()
    verify(out, got_first)


def test_config_13_round_trip():
    hb = gen.make_batch(13, n=2048, seed=3)
    recs = stm.tunnel_records(hb)
    segs, first, _ = stm.segment(hb, *recs, 536, True)
    hs = sm.pack(segs)
    srecs = stm.tunnel_records(hs)
    out, got_first, totals, _ = ctm.coalesce(hs, *srecs, udp=True)
    kinds = ctm.merged_kinds(got_first, totals[0], srecs[1])
    assert [kinds[k] for k in (1, 2, 3)] == [815, 829, 288]
    verify(out, got_first)
    # a cut frame with padding loses it; every other one comes back
    src = sm.frames_of(hb)
    assert len(out) == len(src) and sum(a == b for a, b in zip(out, src)) > 2000
    assert all(len(a) <= len(b) and a[:40] != b"" for a, b in zip(out, src))


VX = lambda inner, **kw: tf.ether(0x0800, stm.ip4(17, tf.udp(40000, 4789, tf.vxlan(inner)), **kw))


def test_a_zero_outer_udp_checksum_stays_zero():
    f = VX(sm.tcp4(sm.payload_bytes(300, 1)), zero_udp_csum=True)
    segs = segments(f, 100)
    assert len(segs) == 3 and all(s[40:42] == b"\0\0" for s in segs)
    out, first, _ = run(segs)
    assert first == [0, 3] and out == [f] and out[0][40:42] == b"\0\0"
    out, first, _ = run(segs, trust_sums=True)
    assert out == [f]


def test_zero_next_to_non_zero_does_not_link():
    f = VX(sm.tcp4(sm.payload_bytes(400, 1)))
    segs = segments(f, 100)
    z = bytearray(segs[2])
    z[40:42] = b"\0\0"                                              # "not computed": still valid
    out, first, _ = run(segs[:2] + [bytes(z)] + segs[3:])
    assert first == [0, 2, 3, 4]
    assert out[1] == bytes(z) and out[2] == segs[3]


def test_outer_ident_gap():
    """DF clear: ident_i == ident_{i-1} + 1 or no link; DF set: the outer ident is ignored."""
    def reident(seg, ident, df):
        g = bytearray(seg)
        g[18:20] = ident.to_bytes(2, "big")
        g[20:22] = (0x4000 if df else 0).to_bytes(2, "big")
        g[24:26] = b"\0\0"
        g[24:26] = sm.csum_field(g[14:34]).to_bytes(2, "big")
        return bytes(g)
    segs = segments(VX(sm.tcp4(sm.payload_bytes(400, 1)), ident=0xfffe), 100)
    assert [int.from_bytes(s[18:20], "big") for s in segs] == [0xfffe, 0xffff, 0, 1]
    for df, want in ((False, [0, 2, 4]), (True, [0, 4])):
        gap = [reident(s, int.from_bytes(s[18:20], "big") + (5 if k >= 2 else 0), df)
               for k, s in enumerate(segs)]
        out, first, _ = run(gap)
        assert first == want, df
        verify(out, first + [first[-1]])
        assert out[0][18:20] == b"\xff\xfe"                        # the head's ident


def test_differing_vni_teid_and_gre_key_do_not_link():
    pay = sm.payload_bytes(300, 2)
    ip = stm.ip_only(sm.tcp4(pay))
    e4 = lambda x: tf.ether(0x0800, x)
    pairs = [
        [e4(stm.ip4(17, tf.udp(40000, 4789, tf.vxlan(sm.tcp4(pay), vni=v)))) for v in (7, 8)],
        [e4(stm.ip4(17, tf.udp(2152, 2152, tf.gtpu(ip, teid=t)))) for t in (7, 8)],
        [e4(stm.ip4(47, tf.gre(ip, key=k))) for k in (7, 8)],
        [e4(stm.ip4(47, tf.gre(ip, checksum=True, key=k))) for k in (7, 8)],
    ]
    for a, b in pairs:
        sa, sb = segments(a, 100), segments(b, 100)
        assert len(sa) == len(sb) == 3
        # the first two segments of one, then the third of the other: in sequence, another id
        out, first, _ = run(sa[:2] + [sb[2]])
        assert first == [0, 2, 3] and out[1] == sb[2]
        out, first, _ = run(sa)
        assert first == [0, 3] and out == [a]


def test_gre_with_s_does_not_merge():
    pay = sm.payload_bytes(100, 3)
    def seg(k, s_bit):
        ip = stm.ip_only(sm.tcp4(pay, seq=0x1000 + 100 * k, ident=0x10 + k, flags=sm.ACK))
        body = stm.gre_seq(ip, seq=7) if s_bit else tf.gre(ip)
        return tf.ether(0x0800, stm.ip4(47, body, ident=0x20 + k))
    out, first, _ = run([seg(k, False) for k in range(3)])
    assert first == [0, 3]
    frames = [seg(k, True) for k in range(3)]
    out, first, _ = run(frames)
    assert first == [0, 1, 2, 3] and out == frames


def test_inner_ethernet_padding_is_copied():
    """Bytes between the inner packet's end and the outer packet's end: the lengths disagree."""
    def seg(k, pad):
        inner = sm.tcp4(sm.payload_bytes(100, 4), seq=0x1000 + 100 * k, ident=0x10 + k, flags=sm.ACK,
                        pad=pad)
        return VX(inner, ident=0x20 + k)
    out, first, _ = run([seg(k, 0) for k in range(3)])
    assert first == [0, 3]
    frames = [seg(k, 6) for k in range(3)]
    out, first, recs = run(frames)
    assert first == [0, 1, 2, 3] and out == frames
    assert all(I["status"] == 0 and int(I["l4_sum"]) == 0xffff for I in recs[2])
    # outer Ethernet padding (past tot) is allowed and not carried
    out, first, _ = run([seg(k, 0) + b"\x5a" * 5 for k in range(3)])
    assert first == [0, 3] and out[0][-5:] != b"\x5a" * 5 and len(out[0]) == len(seg(0, 0)) + 200


def test_an_undecoded_tunnel_is_copied_even_with_the_udp_flag():
    """T.status BAD on outer UDP datagrams that the flat UDP rule would merge."""
    frames = [tf.ether(0x0800, stm.ip4(17, tf.udp(40000, 4789, b"\x08\0\0"), ident=0x30 + k))
              for k in range(3)]                                    # a 3-byte VXLAN header
    hb = sm.pack(frames)
    O, T, I = stm.tunnel_records(hb)
    assert (T["kind"] == stm.VXLAN).all() and (T["status"] != 0).all()
    for udp in (False, True):
        out, first, _, _ = ctm.coalesce(hb, O, T, I, udp=udp)
        assert out == frames
    # the same datagrams under the flat rule merge
    assert len(um.coalesce(hb, sm.oracle_records(hb), udp=True)[0]) == 1


@pytest.mark.parametrize("udp", [False, True])
def test_without_tunnels_the_model_is_the_flat_one(udp):
    """Every tun kind NONE: udp_reframe_model.coalesce on the outer records."""
    hb = gen.make_batch(13, n=512, seed=3)
    segs = stm.segment(hb, *stm.tunnel_records(hb), 300, True)[0]
    plain = sm.pack(um.round_trip_frames(536))
    segs += um.segment(plain, sm.oracle_records(plain), 536, True)[0]
    hs = sm.pack(segs)
    O, T, I = stm.tunnel_records(hs)
    none = np.zeros_like(T)
    none["status"] = 1
    for kw in ({}, {"max_payload": 1000}, {"trust_sums": True}):
        got = ctm.coalesce(hs, O, none, I, udp=udp, **kw)
        want = um.coalesce(hs, O, udp=udp, **kw)
        assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    assert len(want[0]) < hs.n


def test_the_limit_is_the_outer_ip_s():
    """48 segments of 1400 bytes of one stream: a group's payload stays within what the outer
    IPv4 packet_len can say."""
    n = 48
    segs = []
    for k in range(n):
        inner = sm.tcp4(sm.payload_bytes(1400, 6), seq=(0x1000 + 1400 * k) & 0xffffffff, ident=k,
                        flags=sm.ACK)
        segs.append(VX(inner, ident=0x100 + k))
    out, first, _ = run(segs)
    ipo, ol3 = 50 + 54, 14
    k = (65535 - (ipo - ol3)) // 1400
    assert first == [0, k, n] and k == 46
    assert int.from_bytes(out[0][16:18], "big") == ipo - ol3 + k * 1400
    verify(out, first)


def test_the_entry_in_the_header_the_wrapper_and_the_rust_binding():
    hdr = open(os.path.join(ROOT, "include", "rpkt_gpu.h")).read()
    for name in ("rpkt_gpu_coalesce_tunnel_batch", "rpkt_gpu_coalesce_tunnel_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, hdr) and name in engine.EXPORTS
    assert callable(engine.coalesce_tunnel_batch) and callable(engine.coalesce_tunnel_workspace)
    # the neighbours point to it
    assert hdr.count("rpkt_gpu_coalesce_tunnel_batch") >= 4
    assert "Not covered: coalescing of tunnelled frames" not in hdr
    ffi = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "ffi.rs")).read()
    assert "pub fn rpkt_gpu_coalesce_tunnel_batch(" in ffi
    assert "pub fn rpkt_gpu_coalesce_tunnel_workspace_bytes(" in ffi
    lib_rs = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "lib.rs")).read()
    for name in ("coalesce_tunnel_batch", "coalesce_tunnel_workspace_bytes"):
        assert re.search(r"pub (unsafe )?fn %s\(" % name, lib_rs)
