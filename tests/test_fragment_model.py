"""tests/fragment_model.py checked against things that are not itself: known answers written
out as bytes, the oracle's parse of its output, a reassembly by offset, and every way a frame
passes through.  Also the input conditions the GPU tests of rpkt_gpu_fragment_batch rely on
(tests/test_gpu_fragment.py), so that they are checked where no GPU is."""
import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import gen
from rpkt_amd.records import STATUS, dispatch_ethertype

import fragment_model as fm
import segment_model as sm

ETH = "020000000001020000000002"


def run(frames, mtu, **kw):
    hb = sm.pack(frames)
    return fm.fragment(hb, sm.oracle_records(hb), mtu, **kw)


def test_known_answer_three_ipv4_fragments():
    """20 bytes of protocol 253 at mtu 28: c = 8, fragments of 8, 8 and 4 bytes."""
    f = bytes.fromhex(ETH + "0800" "450000281234000040fd763dc0a8380bc0a8380c"
                      "a0a1a2a3a4a5a6a7a8a9aaabacadaeafb0b1b2b3")
    assert f == fm.ip4(bytes(range(0xa0, 0xb4)), 253)
    out, first, totals = run([f], 28)
    assert [o.hex() for o in out] == [
        ETH + "0800" "4500001c1234200040fd5649c0a8380bc0a8380c" "a0a1a2a3a4a5a6a7",
        ETH + "0800" "4500001c1234200140fd5648c0a8380bc0a8380c" "a8a9aaabacadaeaf",
        ETH + "0800" "450000181234000240fd764bc0a8380bc0a8380c" "b0b1b2b3"]
    assert first.tolist() == [0, 3] and totals.tolist() == [3, 3 * 34 + 20]


def test_known_answer_ipv4_options():
    """NOOP, Record Route (7: not copied), LSRR (0x83: copied), EOL at mtu 44 (ihl 36, c = 8):
    fragment 0 keeps the options, the others carry NOOPs where the Record Route was."""
    opts = "01" "0707040a0b0c0d" "83070421222324" "00"
    f = bytes.fromhex(ETH + "0800" "490000351234000040fd86c1c0a8380bc0a8380c" + opts +
                      "c0c1c2c3c4c5c6c7c8c9cacbcccdcecfd0")
    assert bytes.fromhex(opts) == fm.OPTIONS_MIX
    noop = "01" "01010101010101" "83070421222324" "00"
    out, _, _ = run([f], 44)
    assert [o.hex() for o in out] == [
        ETH + "0800" "4900002c1234200040fd66cac0a8380bc0a8380c" + opts + "c0c1c2c3c4c5c6c7",
        ETH + "0800" "4900002c1234200140fd80e8c0a8380bc0a8380c" + noop + "c8c9cacbcccdcecf",
        ETH + "0800" "490000251234000240fda0eec0a8380bc0a8380c" + noop + "d0"]


def test_known_answer_ipv6_hop_by_hop_routing_tcp():
    """Hop-by-Hop + Routing + 28 bytes of TCP at mtu 96: U = l3 + 72, c = 16; the 44 goes into
    the routing header's next-header byte, the TCP's 6 into the Fragment header."""
    ip = "202122232425262728292a2b2c2d2e2f" "404142434445464748494a4b4c4d4e4f"
    hbh, rt = "2b00010400000000", "%s02000000000000" + "a0" * 16
    tcp = "138801bb010203040a0b0c0d501820009b4b0000" "2132435465768798"
    f = bytes.fromhex(ETH + "86dd" "60000000003c0040" + ip + hbh + rt % "06" + tcp)
    assert f == fm.tcp6(28, (fm.HBH, fm.RT0))
    out, _, _ = run([f], 96, ip6_ident=0xfffffffe)
    assert [o.hex() for o in out] == [
        ETH + "86dd" "6000000000380040" + ip + hbh + rt % "2c" + "06000001fffffffe" + tcp[:32],
        ETH + "86dd" "6000000000340040" + ip + hbh + rt % "2c" + "06000010fffffffe" + tcp[32:]]
    # the identification is ip6_ident + i, mod 2^32
    out, _, _ = run([b"", b"", f, f], 96, ip6_ident=0xfffffffe)
    assert [o[90:94].hex() for o in out[2:]] == ["00000000"] * 2 + ["00000001"] * 2


def reassemble_ip4(frags, l3):
    """(header of the first fragment, payload by offset, offset of the first, MF of the last)."""
    pay = {}
    for o in frags:
        ihl = (o[l3] & 0xf) * 4
        fw = int.from_bytes(o[l3 + 6:l3 + 8], "big")
        assert len(o) == l3 + int.from_bytes(o[l3 + 2:l3 + 4], "big")
        pay[(fw & 0x1fff) * 8] = (o[l3 + ihl:], fw)
    offs = sorted(pay)
    blob = b""
    for k, off in enumerate(offs):
        assert off == offs[0] + len(blob)
        assert bool(pay[off][1] & fm.MF) or k == len(offs) - 1
        assert not pay[off][1] & 0xc000
        blob += pay[off][0]
    return blob, offs[0] // 8, bool(pay[offs[-1]][1] & fm.MF)


def check_cut_outputs(frames, recs, mtu, out, first, ident=0):
    """Every property of the cut frames' fragments that something other than the model says."""
    blob, offs = sm.packed_output(out, len(out))
    orec = oracle.parse_batch(blob, len(out), sm.F6, offsets=offs)
    det = dispatch_ethertype(recs)
    n_cut = 0
    for i, f in enumerate(frames):
        a, b = int(first[i]), int(first[i + 1])
        if b - a == 1:
            assert out[a] == f
            continue
        n_cut += 1
        l3, l4 = int(recs[i]["l3_off"]), int(recs[i]["l4_off"])
        frs = out[a:b]
        for k, o in enumerate(frs):
            r = orec[a + k]
            assert int(r["l3_off"]) == l3 and len(o) - l3 <= mtu
            assert o[:l3] == f[:l3]
        if det[i] == 0x0800:
            ihl = l4 - l3
            L = int.from_bytes(f[l3 + 2:l3 + 4], "big")
            fw = int.from_bytes(f[l3 + 6:l3 + 8], "big")
            for k, o in enumerate(frs):
                assert int(orec[a + k]["ip_sum"]) == 0xffff
                assert (len(o) - l4) % 8 == 0 or k == len(frs) - 1
                assert int(orec[a + k]["ip_packet_len"]) == len(o) - l3
                # the header apart from the length, the frag word and the checksum; options of
                # the first fragment are the input's
                for lo, hi in ((0, 2), (4, 6), (8, 10), (12, 20)):
                    assert o[l3 + lo:l3 + hi] == f[l3 + lo:l3 + hi]
                if k == 0:
                    assert o[l3 + 20:l4] == f[l3 + 20:l4]
            pay, o0, mf = reassemble_ip4(frs, l3)
            assert pay == f[l4:l3 + L] and o0 == fw & 0x1fff and mf == bool(fw & fm.MF)
        else:
            plen = int.from_bytes(f[l3 + 4:l3 + 6], "big")
            parts = {}
            for k, o in enumerate(frs):
                r = orec[a + k]
                assert int(r["status"]) == STATUS["IP6_FRAGMENT"]
                fo = int(r["l4_off"]) - 8                       # the Fragment header
                assert o[fo + 1] == 0 and int.from_bytes(o[fo + 4:fo + 8], "big") == (ident + i) % 2 ** 32
                w = int.from_bytes(o[fo + 2:fo + 4], "big")
                assert (w & 1) == (k != len(frs) - 1) and not w & 6
                assert (len(o) - fo - 8) % 8 == 0 or k == len(frs) - 1
                assert int.from_bytes(o[l3 + 4:l3 + 6], "big") == len(o) - l3 - 40
                parts[w & ~7] = (o[:fo], o[fo], o[fo + 8:])
            # the original headers with the 44 undone, the fragmentable part by offset
            U = len(parts[0][0])
            whole = b"".join(parts[k][2] for k in sorted(parts))
            assert sorted(parts)[-1] + len(parts[sorted(parts)[-1]][2]) == len(whole)
            for head, nh, _ in parts.values():
                h = bytearray(head)
                at = [x for x in range(l3, U) if h[x] == 44 and f[x] == nh and f[x] != 44]
                h[l3 + 4:l3 + 6] = f[l3 + 4:l3 + 6]
                assert len(at) >= 1
                h[at[-1]] = nh
                assert bytes(h) == f[:U]
            assert whole == f[U:l3 + 40 + plen]
    return n_cut


@pytest.mark.parametrize("mtu", fm.MTU_VALUES)
def test_hand_frames_against_oracle_and_reassembly(mtu):
    frames = list(fm.hand_frames(mtu))
    hb = sm.pack(frames)
    recs = sm.oracle_records(hb)
    for ignore_df in (False, True):
        out, first, totals = fm.fragment(hb, recs, mtu, ignore_df, 0xfffffffe)
        n_cut = check_cut_outputs(frames, recs, mtu, out, first, 0xfffffffe)
        assert (n_cut > 0) == (mtu < 65535)
        assert int(totals[0]) == len(out) == int(first[-1])


def test_hand_frames_cover_both_families_and_every_header_shape():
    frames = list(fm.hand_frames(1500))
    hb = sm.pack(frames)
    recs = sm.oracle_records(hb)
    out, first, _ = fm.fragment(hb, recs, 1500)
    cut = np.diff(first.astype(np.int64)) > 1
    det = dispatch_ethertype(recs)
    assert (cut & (det == 0x0800)).sum() >= 10 and (cut & (det == 0x86DD)).sum() >= 10
    assert {20, 24, 36, 60} <= {int(r["l4_off"]) - int(r["l3_off"]) for r in recs[cut & (det == 0x0800)]}
    assert {0, 1, 2} <= set(recs["n_vlan"][cut].tolist())
    assert max(int(r["l4_off"]) - int(r["l3_off"]) for r in recs[cut & (det == 0x86DD)]) > 128
    assert {1, 6, 17} <= set(recs["ip_protocol"][cut & (det == 0x0800)].tolist())


def one(frame, mtu, **kw):
    out, first, _ = run([frame], mtu, **kw)
    return out


def test_pass_through_cases():
    f = fm.udp4(100)
    assert len(one(f, 68)) == 3
    assert one(fm.udp4(100, frag=fm.DF), 68) == [fm.udp4(100, frag=fm.DF)]          # DF
    assert len(one(fm.udp4(100, frag=fm.DF), 68, ignore_df=True)) == 3
    assert one(f, 120) == [f] and len(one(f, 119)) == 2                            # L <= mtu
    assert one(f, 27) == [f] and len(one(f, 28)) == 13                             # c < 8
    g = fm.udp4(100, options=fm.OPTIONS_40)
    assert one(g, 67) == [g] and len(one(g, 68)) == 13
    h = fm.udp4(200, frag=0x1ff0)                                                  # offset overflow
    assert one(h, 28) == [h] and one(h, 68) == [h]
    assert len(one(fm.udp4(100, frag=0x1ff0), 116)) == 2                           # 0x1ff0 + 12 fits
    assert one(fm.udp4(100, frag=0x1ff4), 116) == [fm.udp4(100, frag=0x1ff4)]
    # IPv6: a Fragment header anywhere, atomic or not; c < 8
    for exts in ((fm.fragment_header(17),), (fm.HBH, fm.fragment_header(17)),
                 (fm.HBH, fm.RT0, fm.fragment_header(17, 16, 1))):
        v = fm.udp6(200, exts)
        assert one(v, 100) == [v]
    v = fm.udp6(200)
    assert one(v, 55) == [v] and len(one(v, 56)) == 25
    assert one(v, 240) == [v] and len(one(v, 239)) == 2
    # a truncated IPv4 packet (l3 + L > frame_len), Ethernet padding (not carried)
    assert one(f[:-1], 68) == [f[:-1]]
    assert b"".join(o[34:] for o in one(f + b"\x5a" * 7, 68)) == f[34:]


def test_refragmenting_a_fragment_keeps_mf_and_adds_the_offset():
    f = fm.udp4(100, frag=fm.MF | 0x0100)
    out = one(f, 68)
    assert [int.from_bytes(o[20:22], "big") for o in out] == [0x2100, 0x2106, 0x210c]
    f = fm.udp4(100, frag=0x0100)
    assert [int.from_bytes(o[20:22], "big") for o in one(f, 68)] == [0x2100, 0x2106, 0x010c]
    # and the fragments of fragments reassemble to the first packet's payload
    first = one(fm.udp4(1000), 576)
    again, _, _ = run(first, 68)
    pay, o0, mf = reassemble_ip4(again, 14)
    assert pay == fm.udp4(1000)[34:] and o0 == 0 and not mf


def test_every_status_that_is_not_eligible_passes_through():
    """Config 6 (every parse status) at mtu 100 with the flag: a frame is cut only under the
    documented statuses, and what is cut passes every check above."""
    hb = gen.make_batch(6, 4096)
    recs = sm.oracle_records(hb)
    frames = sm.frames_of(hb)
    out, first, _ = fm.fragment(hb, recs, 100, True)
    cut = np.diff(first.astype(np.int64)) > 1
    ok = np.isin(recs["status"], fm.IP4_STATUSES)
    assert cut.any() and not (cut & ~ok).any()
    assert len(set(recs["status"][~cut].tolist()) - set(fm.IP4_STATUSES)) >= 6
    assert check_cut_outputs(frames, recs, 100, out, first) == cut.sum()


def test_generated_frames_carry_df():
    """gen's IPv4 frames all carry DF: the generated configs of the GPU test run twice."""
    for config in (3, 5, 6, 11):
        hb = gen.make_batch(config, 2048)
        recs = sm.oracle_records(hb)
        v4 = (dispatch_ethertype(recs) == 0x0800) & np.isin(recs["status"], fm.IP4_STATUSES)
        assert v4.any() and (recs["ip_frag"][v4] & fm.DF).all(), config


def test_engine_has_the_entry():
    from rpkt_amd import engine
    assert {"rpkt_gpu_fragment_batch", "rpkt_gpu_fragment_workspace_bytes"} <= set(engine.EXPORTS)
    assert engine.FRAGMENT_IGNORE_DF == 1 and callable(engine.fragment_batch)
