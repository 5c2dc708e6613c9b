"""tests/udp_reframe_model.py anchored to the oracle, the model's own round trip, and what
needs no GPU of RPKT_SEGMENT_UDP / RPKT_COALESCE_UDP: the flags the three entries accept (with
n == 0 their checks return before any launch), the wrappers' and the Rust binding's constants."""
import ctypes
import os
import re

import numpy as np
import pytest

from rpkt_amd import engine, gen
from rpkt_amd.build import build_gpu
from rpkt_amd.records import dispatch_ethertype

import coalesce_model as cm
import segment_model as sm
import udp_reframe_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_against_oracle(hb, recs, mss):
    """Every output of a UDP-segmented frame of hb parses OK with valid sums, has UDP length
    8 + payload, idents that run on, and the payloads concatenate to the input's.  Returns the
    number of UDP frames cut and of output segments whose checksum field is 0xffff."""
    out, first, totals = um.segment(hb, recs, mss, True)
    assert int(totals[0]) == len(out) == int(first[-1])
    ohb = sm.pack(out)
    orecs = sm.oracle_records(ohb)
    v6 = dispatch_ethertype(recs) == 0x86DD
    frames = sm.frames_of(hb)
    n_cut = 0
    for i, (f, r) in enumerate(zip(frames, recs)):
        a, b = int(first[i]), int(first[i + 1])
        if not um.is_udp_segmented(r, bool(v6[i]), mss):
            continue
        n_cut += 1
        l3, l4, po, pl = (int(r[k]) for k in ("l3_off", "l4_off", "payload_off", "payload_len"))
        assert b - a == -(-pl // mss)
        ident = int.from_bytes(f[l3 + 4:l3 + 6], "big")
        pays = []
        for k in range(a, b):
            o, q = out[k], orecs[k]
            assert q["status"] == 0 and q["ip_protocol"] == 17, (i, k)
            assert int(q["l4_sum"]) == 0xffff and (v6[i] or int(q["ip_sum"]) == 0xffff), (i, k)
            assert (int(q["l3_off"]), int(q["l4_off"]), int(q["payload_off"])) == (l3, l4, po)
            p = int(q["payload_len"])
            assert p == (mss if k < b - 1 else pl - (b - a - 1) * mss) and len(o) == po + p
            assert int.from_bytes(o[l4 + 4:l4 + 6], "big") == 8 + p
            assert o[l4 + 6:l4 + 8] != b"\0\0"
            if not v6[i]:
                assert int.from_bytes(o[l3 + 4:l3 + 6], "big") == (ident + k - a) & 0xffff
            pays.append(o[po:])
        assert b"".join(pays) == f[po:po + pl], i
    return n_cut, um.zero_sum_segments(out, orecs)


@pytest.mark.parametrize("mss", [100, 300, 536])
def test_hand_frames_against_the_oracle(mss):
    frames = um.hand_frames(mss) + um.hand_frames(1448) + [um.udp4(sm.payload_bytes(um.TOP, 1), zero_csum=True)]
    hb = sm.pack(frames)
    n_cut, n_zero = check_against_oracle(hb, sm.oracle_records(hb), mss)
    assert n_cut >= 20 and n_zero >= 2


# UDP frames cut, TCP frames cut (None: not counted), UDP frames cut with a zero checksum
# field: what the generator gives today; half of each must remain
SHAPES = {(11, 4096, 300): (2037, 2059, None), (4, 4096, 300): (861, 864, None),
          (6, 8192, 100): (1698, None, 86)}


@pytest.mark.parametrize("config,n,mss", list(SHAPES))
def test_generated_configs_against_the_oracle(config, n, mss):
    hb = gen.make_batch(config, n)
    recs = sm.oracle_records(hb)
    n_udp, n_tcp = um.cut_counts(recs, mss)
    want_udp, want_tcp, want_zero = SHAPES[(config, n, mss)]
    assert n_udp >= want_udp // 2
    assert want_tcp is None or n_tcp >= want_tcp // 2
    if want_zero is not None:
        v6 = dispatch_ethertype(recs) == 0x86DD
        zero = sum(1 for f, r, v in zip(sm.frames_of(hb), recs, v6) if um.is_udp_segmented(r, bool(v), mss)
                   and f[int(r["l4_off"]) + 6:int(r["l4_off"]) + 8] == b"\0\0")
        assert zero >= want_zero // 2
    assert check_against_oracle(hb, recs, mss)[0] == n_udp
    for other in (100, 300, 536):
        if other != mss:
            check_against_oracle(hb, recs, other)


@pytest.mark.parametrize("config,n,mss", [(11, 1024, 300), (6, 2048, 100)])
def test_flag_clear_is_the_tcp_model(config, n, mss):
    hb = gen.make_batch(config, n)
    recs = sm.oracle_records(hb)
    a, b = um.segment(hb, recs, mss), sm.segment(hb, recs, mss)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert um.segment(hb, recs, mss, True)[0] != b[0]
    shb = sm.pack(um.segment(hb, recs, mss, True)[0])
    srecs = sm.oracle_records(shb)
    for kw in ({}, {"trust_sums": True, "max_payload": 1000}):
        a, b = um.coalesce(shb, srecs, **kw), cm.coalesce(shb, srecs, **kw)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert int(um.coalesce(shb, srecs, udp=True)[2][0]) < int(b[2][0])


def test_flag_clear_on_hand_frames():
    hb = sm.pack(um.hand_frames(17))
    recs = sm.oracle_records(hb)
    assert um.segment(hb, recs, 17)[0] == sm.segment(hb, recs, 17)[0]
    shb = sm.pack(um.segment(hb, recs, 17, True)[0])
    srecs = sm.oracle_records(shb)
    assert um.coalesce(shb, srecs)[0] == cm.coalesce(shb, srecs)[0]


@pytest.mark.parametrize("mss", [7, 536, 1448])
def test_round_trip_in_the_model(mss):
    """coalesce(segment(F)) == F, with out_mss the mss and the merged checksum-zero datagram."""
    F = um.round_trip_frames(mss)
    assert len(F[0]) == 42 + 2 * mss and len(F[1]) == 42 + mss + 1 and len(F[2]) == 42 + um.TOP
    assert F[2][20] & 0x40 and not F[0][20] & 0x40
    hb = sm.pack(F)
    out, first, totals = um.segment(hb, sm.oracle_records(hb), mss, True)
    assert int(totals[0]) > 2 * len(F)
    shb = sm.pack(out)
    srecs = sm.oracle_records(shb)
    back, src_first, ctot, out_mss = um.coalesce(shb, srecs, udp=True)
    assert back == F
    assert np.array_equal(src_first[:len(F) + 1], first)
    assert (out_mss[:len(F)] == mss).all()
    # the case: a merged output whose computed checksum is 0, written 0xffff
    assert sum(1 for f in back if f[23] == 17 and f[12:14] == b"\x08\x00" and f[40:42] == b"\xff\xff") >= 1
    # without the flag only the TCP frame comes back
    plain = um.coalesce(shb, srecs)[0]
    assert plain == cm.coalesce(shb, srecs)[0] and F[6] in plain and F[0] not in plain


def test_the_checksum_zero_cases_are_hit():
    for mss in (7, 16, 17, 536, 1448):
        hb = sm.pack(um.hand_frames(mss))
        out, _, _ = um.segment(hb, sm.oracle_records(hb), mss, True)
        assert um.zero_sum_segments(out, sm.oracle_records(sm.pack(out))) >= 2, mss
    # the sum that gives 0: 0xffff in the field makes the oracle's verdict 0xffff too
    f = um.zero_sum_datagram(lambda pay: um.udp6(pay), 64, lambda f: 54)
    assert f[60:62] == b"\xff\xff"
    r = sm.oracle_records(sm.pack([f]))[0]
    assert r["status"] == 0 and int(r["l4_sum"]) == 0xffff


def test_zero_checksum_datagrams_in_the_model():
    """A datagram sent without a checksum is cut into segments that have one, and is never
    merged, sums trusted or not."""
    f = um.udp4(sm.payload_bytes(2000, 1), zero_csum=True)
    hb = sm.pack([f])
    recs = sm.oracle_records(hb)
    assert int(recs[0]["l4_sum"]) != 0xffff
    out, _, _ = um.segment(hb, recs, 500, True)
    assert len(out) == 4 and all(o[40:42] != b"\0\0" for o in out)
    pair = sm.pack([um.udp4(sm.payload_bytes(500, 1), zero_csum=True, ident=k) for k in (1, 2)])
    for trust in (False, True):
        assert int(um.coalesce(pair, sm.oracle_records(pair), trust_sums=trust, udp=True)[2][0]) == 2
    filled = sm.pack([um.udp4(sm.payload_bytes(500, 1), ident=k) for k in (1, 2)])
    assert int(um.coalesce(filled, sm.oracle_records(filled), udp=True)[2][0]) == 1


# ---- the ABI without a GPU: n == 0 returns before any launch --------------------------------

OK, E_INVAL = 0, -1
A = 1 << 20                                    # 16-byte aligned, never dereferenced addresses


@pytest.fixture(scope="module")
def lib():
    build_gpu()
    return engine.lib()


def seg_call(fn, src, mss=1448, flags=0):
    p = [A + (j << 16) for j in range(6)]
    return fn(ctypes.byref(src), p[0], mss, flags, p[1], 1 << 16, p[2], 64, p[3], p[4], p[5], None)


def co_call(fn, max_payload=65535, flags=0):
    p = [A + (j << 16) for j in range(8)]
    b = engine.Batch(A + (9 << 16), 1 << 16, A + (10 << 16), 0, 0, 0, 0)
    return fn(ctypes.byref(b), p[0], p[1], max_payload, flags, p[2], 1 << 16, p[3], 64, p[4], p[5],
              p[6], p[7], None)


def empty_sources(lib):
    b = engine.Batch(A + (9 << 16), 1 << 16, A + (10 << 16), 0, 0, 0, 0)
    c = engine.Chains(A + (9 << 16), 1 << 16, A + (10 << 16), A + (11 << 16), 4, 0)
    return ((lib.rpkt_gpu_segment_batch, b), (lib.rpkt_gpu_segment_chains, c))


def test_the_flags_each_entry_accepts(lib):
    for fn, src in empty_sources(lib):
        assert seg_call(fn, src, flags=0) == OK
        assert seg_call(fn, src, flags=16) == OK
        for bad in (17, 32, 18, 0x80000010, 1, 2, 0x80000000):
            assert seg_call(fn, src, flags=bad) == E_INVAL, bad
        for mss in (0, 65536, 0xffffffff):
            assert seg_call(fn, src, mss=mss, flags=16) == E_INVAL
        for mss in (1, 65535):
            assert seg_call(fn, src, mss=mss, flags=16) == OK
    fn = lib.rpkt_gpu_coalesce_batch
    for good in (0, 1, 16, 17):
        assert co_call(fn, flags=good) == OK, good
    for bad in (32, 18, 0x80000010, 2, 3, 4, 0x80000000):
        assert co_call(fn, flags=bad) == E_INVAL, bad
    for flags in (16, 17):
        for mp in (0, 65536, 0xffffffff):
            assert co_call(fn, max_payload=mp, flags=flags) == E_INVAL
        for mp in (1, 65535):
            assert co_call(fn, max_payload=mp, flags=flags) == OK


def test_constants_of_the_wrappers_and_the_rust_binding():
    assert engine.SEGMENT_UDP == engine.COALESCE_UDP == 16
    hdr = open(os.path.join(ROOT, "include", "rpkt_gpu.h")).read()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RPKT_[A-Z_]+_UDP)\s+(\d+)u\b", hdr)}
    assert c == {"RPKT_SEGMENT_UDP": 16, "RPKT_COALESCE_UDP": 16}
    ffi = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "ffi.rs")).read()
    rs = {m.group(1): int(m.group(2)) for m in
          re.finditer(r"pub const (RPKT_[A-Z_]+_UDP):\s*u32\s*=\s*(\d+);", ffi)}
    assert rs == c
    lib_rs = open(os.path.join(ROOT, "bindings", "rpkt-gpu", "src", "lib.rs")).read()
    for name in ("segment_batch_flags", "segment_chains_flags", "coalesce_batch_flags"):
        assert "pub unsafe fn %s(" % name in lib_rs
