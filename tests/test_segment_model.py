"""rpkt_gpu_segment_batch on the CPU: tests/segment_model.py (the model the GPU test compares
bytes against) anchored to the oracle's parse and to the segmentation rules read from the
frames themselves, and the entry's argument checks, which return before any launch."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from rpkt_amd import engine
from rpkt_amd.build import build_gpu
from rpkt_amd.records import dispatch_ethertype

import segment_model as sm

OK, E_INVAL, E_TOO_LARGE, E_ALIGN = 0, -1, -3, -4


def be(b, at, n):
    return int.from_bytes(b[at:at + n], "big")


def check_rules(hb, mss, want_segmented=None):
    """The model's output of hb at mss against the rules, each read from the frames: returns
    the number of segmented frames."""
    recs = sm.oracle_records(hb)
    out, first, totals = sm.segment(hb, recs, mss)
    assert int(totals[0]) == len(out) == int(first[-1])
    assert int(totals[1]) == sum(len(o) for o in out)
    blob, offs = sm.packed_output(out, len(out) + 2)
    orec = oracle.parse_batch(blob, len(out) + 2, sm.F6, offsets=offs)
    assert (orec["frame_len"][-2:] == 0).all()                      # the spare slots: empty frames
    v6 = dispatch_ethertype(recs) == 0x86DD
    n_seg = 0
    for i, f in enumerate(sm.frames_of(hb)):
        r, segs = recs[i], out[first[i]:first[i + 1]]
        if not sm.is_segmented(r, bool(v6[i]), mss):
            assert segs == [f], i                                   # byte-identical
            continue
        n_seg += 1
        l3, l4, po, pl = (int(r[k]) for k in ("l3_off", "l4_off", "payload_off", "payload_len"))
        assert len(segs) == -(-pl // mss) and len(segs) >= 2
        assert b"".join(s[po:] for s in segs) == f[po:po + pl], i   # the payload, nothing after it
        for k, s in enumerate(segs):
            q = orec[first[i] + k]
            p = len(s) - po
            assert p == (mss if k < len(segs) - 1 else pl - k * mss) and p > 0
            assert q["status"] == 0 and q["l4_sum"] == 0xffff, (i, k)
            assert q["payload_off"] == po and q["payload_len"] == p
            if v6[i]:
                assert be(s, l3 + 4, 2) == po - l3 - 40 + p
                assert s[l3:l3 + 4] + s[l3 + 6:l4] == f[l3:l3 + 4] + f[l3 + 6:l4]   # ext. headers
            else:
                assert q["ip_sum"] == 0xffff, (i, k)
                assert be(s, l3 + 2, 2) == po - l3 + p
                assert be(s, l3 + 4, 2) == (be(f, l3 + 4, 2) + k) & 0xffff
                assert s[l3:l3 + 2] + s[l3 + 6:l3 + 10] + s[l3 + 12:l4] == \
                    f[l3:l3 + 2] + f[l3 + 6:l3 + 10] + f[l3 + 12:l4]
            assert s[:l3] == f[:l3]
            assert be(s, l4 + 4, 4) == (be(f, l4 + 4, 4) + k * mss) & 0xffffffff
            keep = 0xff & ~((0 if k == len(segs) - 1 else sm.FIN | sm.PSH) | (sm.CWR if k else 0))
            assert s[l4 + 13] == f[l4 + 13] & keep
            assert s[l4:l4 + 4] + s[l4 + 8:l4 + 13] + s[l4 + 14:l4 + 16] + s[l4 + 18:po] == \
                f[l4:l4 + 4] + f[l4 + 8:l4 + 13] + f[l4 + 14:l4 + 16] + f[l4 + 18:po]
    if want_segmented is not None:
        assert n_seg == want_segmented
    return n_seg


def test_the_reference_example_frame():
    """rpkt-dpdk/examples/tso_tx.rs: 4000 bytes of 0xae at set_tso_segsz(1024)."""
    f = sm.tso_tx_frame()
    hb = sm.pack([f])
    assert check_rules(hb, 1024, want_segmented=1) == 1
    out, first, totals = sm.segment(hb, sm.oracle_records(hb), 1024)
    assert [len(s) - 54 for s in out] == [1024, 1024, 1024, 928] and list(first) == [0, 4]
    assert int(totals[1]) == 4000 + 4 * 54
    assert [be(s, 38, 4) for s in out] == [0x8e501902 + 1024 * k for k in range(4)]
    assert [s[47] for s in out] == [sm.ACK, sm.ACK, sm.ACK, sm.ACK | sm.PSH]
    assert all(set(s[54:]) == {0xae} for s in out)


@pytest.mark.parametrize("mss", sm.MSS_VALUES)
def test_hand_built_frames(mss):
    frames = sm.hand_frames(mss)
    n_seg = check_rules(sm.pack(frames, lead=3), mss)
    if mss == 65535:
        assert n_seg == 0                                  # no IP packet holds more
    else:
        assert n_seg >= 20                                 # lengths above mss and the variety
    recs = sm.oracle_records(sm.pack(frames))
    assert (recs["payload_off"] > 128).sum() >= 2          # headers past the 128-B window


def test_flags_and_wrap_around():
    f = sm.tcp4(sm.payload_bytes(100), ident=0xffff, seq=0xfffffff0, flags=sm.both_flags())
    hb = sm.pack([f])
    out, _, _ = sm.segment(hb, sm.oracle_records(hb), 30)
    assert [be(s, 18, 2) for s in out] == [0xffff, 0, 1, 2]
    assert [be(s, 38, 4) for s in out] == [0xfffffff0, 0x0e, 0x2c, 0x4a]
    assert [s[47] for s in out] == [sm.CWR | sm.ACK, sm.ACK, sm.ACK, sm.FIN | sm.PSH | sm.ACK]
    check_rules(hb, 30, want_segmented=1)


def test_a_checksum_of_zero_stays_zero():
    assert sm.csum_field(b"\xff\xff") == 0 and sm.csum_field(b"\xff\xfe\x00\x01") == 0
    assert sm.csum_field(b"\x00\x01") == 0xfffe and sm.fold_sum(b"\x01") == 0x0100


# ---- the C ABI: argument checks, no launch -------------------------------------------------

A = 1 << 20                                    # 16-byte aligned, never dereferenced addresses
ADDR = {k: A + (j << 16) for j, k in enumerate(
    ("recs", "out_frames", "out_offsets", "seg_first", "totals", "workspace"))}


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_segment_batch


def batch(n=10, frames=A + (9 << 16), frames_bytes=1 << 16, offsets=A + (8 << 16), stride=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, 0, n, 0)


def call(fn, b, mss=1448, flags=0, out_bytes=1 << 16, out_cap=64, **ptr):
    p = dict(ADDR, **ptr)
    return fn(ctypes.byref(b) if b is not None else None, p["recs"], mss, flags, p["out_frames"],
              out_bytes, p["out_offsets"], out_cap, p["seg_first"], p["totals"], p["workspace"],
              None)


def test_both_functions_are_exported_and_bound(fn):
    assert {"rpkt_gpu_segment_batch", "rpkt_gpu_segment_workspace_bytes"} <= set(engine.EXPORTS)
    assert callable(engine.segment_batch) and callable(engine.segment_workspace)
    ws = engine.lib().rpkt_gpu_segment_workspace_bytes
    assert ws(1) >= 32 and ws(70000) >= 70000 * 40 and ws(70000) % 16 == 0
    assert engine.lib().rpkt_gpu_abi_version() == 1


def test_argument_checks_in_the_documented_order(fn):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL batch / recs / any output / workspace, before the flags
    assert call(fn, None, flags=1) == E_INVAL
    for k in ADDR:
        assert call(fn, batch(frames_bytes=1 << 32), **{k: None}) == E_INVAL, k
    # 2. flags, mss: before n == 0
    for bad in (1, 2, 0x80000000):
        assert call(fn, batch(n=0), flags=bad) == E_INVAL
    for mss in (0, 65536, 0xffffffff):
        assert call(fn, batch(n=0), mss=mss) == E_INVAL
    assert call(fn, batch(n=0), mss=1) == OK and call(fn, batch(n=0), mss=65535) == OK
    # 3. n == 0: RPKT_OK, nothing else is looked at
    assert call(fn, batch(n=0, frames=None, frames_bytes=1 << 33, offsets=None), out_cap=0,
                out_bytes=1 << 33, recs=A + 1, totals=A + 4) == OK
    # 4. NULL frames_dev, before the sizes
    assert call(fn, batch(frames=None, frames_bytes=1 << 32)) == E_INVAL
    # 5. frames_bytes, then out_bytes, at the same limit, before the layout
    assert call(fn, batch(frames_bytes=1 << 32, offsets=None)) == E_TOO_LARGE
    assert call(fn, batch(offsets=None), out_bytes=1 << 32) == E_TOO_LARGE
    assert call(fn, batch(frames_bytes=0xffffff01)) == E_TOO_LARGE
    assert call(fn, batch(), out_bytes=0xffffff01) == E_TOO_LARGE
    # 6. the layout, before out_cap
    assert call(fn, batch(offsets=None, stride=0), out_cap=0, recs=A + 8) == E_INVAL
    # 7. out_cap == 0, before the alignment
    assert call(fn, batch(), out_cap=0, recs=ADDR["recs"] + 8) == E_INVAL
    # 8. alignment: recs, out_frames, workspace 16 B; totals 8 B
    for k in ("recs", "out_frames", "workspace"):
        assert call(fn, batch(), **{k: ADDR[k] + 8}) == E_ALIGN, k
    assert call(fn, batch(), totals=ADDR["totals"] + 4) == E_ALIGN
