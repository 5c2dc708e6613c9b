"""tests/segment_tunnel_model.py against the oracle's tunnel parse: every output of a cut frame
decodes, carries valid inner and outer sums, and the outputs of one frame carry its payload in
order with seq / ident running on.  CPU only."""
import os
import re

import numpy as np
import pytest

from rpkt_amd import engine, gen
from rpkt_amd.records import dispatch_ethertype

import segment_model as sm
import segment_tunnel_model as stm
import udp_reframe_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSS = (1, 7, 536, 1448, 3000, 3001)


def check_cut(hb, recs, mss, udp, what):
    """The model's output for hb: every cut tunnel frame's outputs verify under the oracle.
    Returns (seg_first, the records of the output)."""
    outer, tun, inner = recs
    out, first, totals = stm.segment(hb, outer, tun, inner, mss, udp)
    assert int(totals[0]) == len(out) == int(first[-1])
    assert int(totals[1]) == sum(len(o) for o in out)
    ohb = sm.pack(out)
    oo, ot, oi = stm.tunnel_records(ohb)
    o_et, i_et = dispatch_ethertype(oo), dispatch_ethertype(oi)
    frames = sm.frames_of(hb)
    for i, f in enumerate(frames):
        a, b = int(first[i]), int(first[i + 1])
        if b - a == 1:
            assert out[a] == f, "%s: frame %d is not a copy" % (what, i)
            continue
        if tun[i]["kind"] == stm.NONE:
            continue                                    # rule 1: udp_reframe_model's own tests
        w = "%s: frame %d" % (what, i)
        ipo, ipl = int(inner[i]["payload_off"]), int(inner[i]["payload_len"])
        assert b - a == -(-ipl // mss), w
        assert b"".join(out[j][ipo:] for j in range(a, b)) == f[ipo:ipo + ipl], w
        for k, j in enumerate(range(a, b)):
            O, T, I = oo[j], ot[j], oi[j]
            assert len(out[j]) == ipo + min(mss, ipl - k * mss), w
            assert T["status"] == 0 and T["kind"] == tun[i]["kind"] and I["status"] == 0, (w, k)
            assert all(int(T[x]) == int(tun[i][x]) for x in ("tun_off", "inner_off", "id")), (w, k)
            assert int(I["payload_off"]) == ipo and int(I["payload_len"]) == len(out[j]) - ipo, (w, k)
            assert int(I["l4_sum"]) == 0xffff and (i_et[j] == 0x86DD or int(I["ip_sum"]) == 0xffff), (w, k)
            assert o_et[j] == 0x86DD or int(O["ip_sum"]) == 0xffff, (w, k)
            ol4 = int(O["l4_off"])
            zero = T["kind"] != stm.GRE and f[ol4 + 6:ol4 + 8] == b"\0\0"
            if zero:
                assert out[j][ol4 + 6:ol4 + 8] == b"\0\0", (w, k)
            elif T["kind"] != stm.GRE or f[int(T["tun_off"])] & 0x80:
                assert int(O["l4_sum"]) == 0xffff, (w, k)
            if o_et[j] == 0x0800:
                assert int(O["ip_ident"]) == (int(outer[i]["ip_ident"]) + k) & 0xffff, (w, k)
            if i_et[j] == 0x0800:
                assert int(I["ip_ident"]) == (int(inner[i]["ip_ident"]) + k) & 0xffff, (w, k)
            if I["ip_protocol"] == 6:
                assert int(I["tcp_seq"]) == (int(inner[i]["tcp_seq"]) + k * mss) & 0xffffffff, (w, k)
    return first, (oo, ot, oi)


@pytest.mark.parametrize("udp", [False, True])
@pytest.mark.parametrize("mss", MSS)
def test_hand_shapes_verify_under_the_oracle(mss, udp):
    frames = stm.hand_frames(mss)
    hb = sm.pack(frames)
    recs = stm.tunnel_records(hb)
    first, _ = check_cut(hb, recs, mss, udp, "mss %d udp %d" % (mss, udp))
    n = np.diff(first.astype(np.int64))
    cut = len(stm.cut_frames(1))
    # every cut shape is cut (inner UDP and the plain UDP frame with the flag only), the padded
    # ones too, and nothing else; at mss 3000 and 3001 the 2000-byte payloads fit: nothing is
    want = [k < stm.N_CUT_TCP - 1 or k == stm.N_CUT_TCP or udp for k in range(cut)] + [True] * 3
    if mss >= 2000:
        want = [False] * (cut + 3)
    assert [x > 1 for x in n[:cut + 3]] == want
    assert (n[cut + 3:] == 1).all()
    outer, tun, inner = recs
    assert {int(t["status"]) for t in tun[cut + 3:]} >= {0, 2, 3, 5}


def test_padding_is_dropped_and_outer_lengths_recomputed():
    mss = 100
    frames = stm.padded_frames(250)
    hb = sm.pack(frames)
    outer, tun, inner = stm.tunnel_records(hb)
    out, first, _ = stm.segment(hb, outer, tun, inner, mss)
    assert list(first) == [0, 3, 6, 9]
    for i in range(3):
        ipo = int(inner[i]["payload_off"])
        ol3, ol4 = int(outer[i]["l3_off"]), int(outer[i]["l4_off"])
        for k, p in enumerate((100, 100, 50)):
            o = out[3 * i + k]
            assert len(o) == ipo + p and b"\x5a" * 2 not in o[ipo - 20:]
            assert int.from_bytes(o[ol3 + 2:ol3 + 4], "big") == len(o) - ol3
            if tun[i]["kind"] != stm.GRE:
                assert int.from_bytes(o[ol4 + 4:ol4 + 6], "big") == len(o) - ol4
    check_cut(hb, (outer, tun, inner), mss, False, "padding")


def test_zero_outer_udp_checksum_is_kept_and_gtp_length_is_set():
    frames = stm.cut_frames(300)
    hb = sm.pack(frames)
    outer, tun, inner = stm.tunnel_records(hb)
    out, first, _ = stm.segment(hb, outer, tun, inner, 128)
    for j in range(int(first[10]), int(first[11])):                # VXLAN, outer checksum 0
        assert out[j][40:42] == b"\0\0"
    for j in range(int(first[0]), int(first[1])):
        assert out[j][40:42] != b"\0\0"
    for i in (3, 4, 5):                                            # GTP-U
        toff = int(tun[i]["tun_off"])
        for j in range(int(first[i]), int(first[i + 1])):
            assert int.from_bytes(out[j][toff + 2:toff + 4], "big") == len(out[j]) - toff - 8
            assert out[j][toff + 8:int(tun[i]["inner_off"])] == \
                frames[i][toff + 8:int(tun[i]["inner_off"])]       # sequence, extensions copied


@pytest.fixture(scope="module")
def config13():
    hb = gen.make_batch(13, n=2048, seed=3)
    return hb, stm.tunnel_records(hb)


@pytest.mark.parametrize("mss,udp", [(536, False), (536, True), (100, True)])
def test_config_13(config13, mss, udp):
    hb, recs = config13
    first, _ = check_cut(hb, recs, mss, udp, "config 13 mss %d" % mss)
    kinds = stm.cut_kinds(first, recs[1])
    assert min(kinds[k] for k in (stm.VXLAN, stm.GTPU, stm.GRE)) >= 100, kinds
    if mss == 536:
        assert [kinds[k] for k in (1, 2, 3)] == ([815, 829, 288] if udp else [402, 383, 139])


def test_config_14_fuzz():
    hb = gen.make_batch(14, n=4096, seed=3)
    recs = stm.tunnel_records(hb)
    first, _ = check_cut(hb, recs, 100, True, "config 14")
    assert sum(stm.cut_kinds(first, recs[1]).values()) > 0


@pytest.mark.parametrize("udp", [False, True])
def test_without_tunnels_the_model_is_the_flat_one(config13, udp):
    """Every tun kind NONE: udp_reframe_model.segment on the outer records."""
    hb, (outer, tun, inner) = config13
    none = np.zeros_like(tun)
    none["status"] = 1
    got = stm.segment(hb, outer, none, inner, 300, udp)
    want = um.segment(hb, outer, 300, udp)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    hand = sm.pack(um.hand_frames(17))
    o, t, i = stm.tunnel_records(hand)
    assert (t["kind"] == 0).all()
    got, want = stm.segment(hand, o, t, i, 17, udp), um.segment(hand, sm.oracle_records(hand), 17, udp)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


def test_the_entry_in_the_header_the_wrapper_and_the_rust_binding():
    hdr = open(os.path.join(ROOT, "include", "rpkt_gpu.h")).read()
    for name in ("rpkt_gpu_segment_tunnel_batch", "rpkt_gpu_segment_tunnel_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, hdr) and name in engine.EXPORTS
    # the entry takes the segment entries' flag; the flat entries point to it
    assert hdr.count("rpkt_gpu_segment_tunnel_batch") >= 4
    assert hdr.count("Not covered: the inner TCP or UDP of tunnelled frames") == 0
    assert "mbuf chains, the inner TCP or UDP of tunnelled frames" in hdr      # coalescing keeps it
    ffi = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "ffi.rs")).read()
    assert "pub fn rpkt_gpu_segment_tunnel_batch(" in ffi
    assert "pub fn rpkt_gpu_segment_tunnel_workspace_bytes(" in ffi
    lib_rs = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "lib.rs")).read()
    for name in ("segment_tunnel_batch", "segment_tunnel_workspace_bytes"):
        assert re.search(r"pub (unsafe )?fn %s\(" % name, lib_rs)
