"""The argument checks of rpkt_gpu_reassemble_batch and rpkt_gpu_reassemble_keys, in the
documented order (include/rpkt_gpu.h, at enum rpkt_err): rpkt_gpu_coalesce_batch's without a
max_payload, flags 0 or RPKT_REASSEMBLE_TRUST_SUMS; the batch entries' order for the keys.

CPU only, and skipped where a GPU is visible: the calls carry fake device addresses, so a
check dropped by mistake must fail at the launch (RPKT_E_HIP, no device) instead of running
a kernel on them."""
import ctypes

import pytest
import torch

from rpkt_amd import engine
from rpkt_amd.build import build_gpu

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="fake device addresses: never where a launch could run")

OK, E_INVAL, E_HIP, E_TOO_LARGE, E_ALIGN = 0, -1, -2, -3, -4
A = 1 << 20                                    # 16-byte aligned, never dereferenced addresses
REQUIRED = ("recs", "out_frames", "out_offsets", "src_first", "totals", "workspace")
ADDR = {k: A + (j << 16) for j, k in enumerate(REQUIRED + ("order", "keys"))}
FRAMES, OFFSETS = A + (9 << 16), A + (10 << 16)


@pytest.fixture(scope="module")
def L():
    build_gpu()
    return engine.lib()


def batch(n=10, frames=FRAMES, frames_bytes=1 << 16, offsets=OFFSETS, stride=0, frame_len=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, frame_len, n, 0)


def call(L, b, flags=0, out_bytes=1 << 16, out_cap=64, order=None, **ptr):
    p = dict(ADDR, **ptr)
    return L.rpkt_gpu_reassemble_batch(ctypes.byref(b) if b is not None else None, p["recs"], order,
                                       flags, p["out_frames"], out_bytes, p["out_offsets"], out_cap,
                                       p["src_first"], p["totals"], p["workspace"], None)


def keys(L, b, flags=0, **ptr):
    p = dict(ADDR, **ptr)
    return L.rpkt_gpu_reassemble_keys(ctypes.byref(b) if b is not None else None, p["recs"], flags,
                                      p["keys"], None)


def test_the_entries_are_exported_and_sized(L):
    assert {"rpkt_gpu_reassemble_batch", "rpkt_gpu_reassemble_workspace_bytes",
            "rpkt_gpu_reassemble_keys"} <= set(engine.EXPORTS)
    assert engine.REASSEMBLE_TRUST_SUMS == 1
    size = L.rpkt_gpu_reassemble_workspace_bytes
    assert size(0) == 0
    # a 32-B plan, a u64 destination and two u32 per position; per block of 256 a u64 pair and a u32
    sizes = [size(n) for n in (1, 255, 256, 257, 70000, 0xffffffff)]
    assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == 6
    for n, s in zip((1, 255, 256, 257, 70000, 0xffffffff), sizes):
        assert 48 * n <= s <= 48 * n + 20 * (n // 256 + 1) + 6 * 16


def test_argument_checks_in_the_documented_order(L):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL batch / recs / a required output / workspace, before the flags
    assert call(L, None, flags=2) == E_INVAL
    for k in REQUIRED:
        assert call(L, batch(n=0), flags=2, **{k: None}) == E_INVAL, k
        assert call(L, batch(n=0), **{k: None}) == E_INVAL, k       # even for no frames
    # 2. flags other than 0 and 1: before n == 0
    for bad in (2, 3, 16, 17, 0x80000000):
        assert call(L, batch(n=0), flags=bad) == E_INVAL
    # 3. n == 0: RPKT_OK, nothing else is looked at; order_dev may be NULL or not
    for flags in (0, 1):
        assert call(L, batch(n=0), flags=flags) == OK
        assert call(L, batch(n=0), flags=flags, order=ADDR["order"] + 2) == OK
    assert call(L, batch(n=0, frames=None, offsets=None, frames_bytes=1 << 33), out_cap=0,
                out_bytes=1 << 33, recs=A + 1, totals=A + 4) == OK
    # 4. NULL frames_dev, before the sizes; frames_bytes, then out_bytes at the same limit
    assert call(L, batch(frames=None, frames_bytes=1 << 32)) == E_INVAL
    assert call(L, batch(frames_bytes=1 << 32, offsets=None), out_cap=0) == E_TOO_LARGE
    assert call(L, batch(frames_bytes=0xffffff01), out_cap=0) == E_TOO_LARGE
    assert call(L, batch(offsets=None), out_bytes=1 << 32, out_cap=0) == E_TOO_LARGE
    assert call(L, batch(), out_bytes=0xffffff01, out_cap=0) == E_TOO_LARGE
    # 5. no layout, before out_cap
    assert call(L, batch(offsets=None), out_cap=0) == E_INVAL
    # 6. out_cap == 0, before the alignment
    assert call(L, batch(), out_cap=0, recs=ADDR["recs"] + 8) == E_INVAL
    # 7. alignment: totals 8 B; recs, out_frames, workspace 16 B
    assert call(L, batch(), totals=ADDR["totals"] + 4) == E_ALIGN
    for k in ("recs", "out_frames", "workspace"):
        assert call(L, batch(), **{k: ADDR[k] + 8}) == E_ALIGN, k
    assert call(L, batch(), totals=ADDR["totals"] + 8, src_first=ADDR["src_first"] + 4,
                out_offsets=ADDR["out_offsets"] + 4, order=ADDR["order"] + 4) == E_HIP   # a launch


def test_the_limits_are_accepted(L):
    """The largest sizes pass the checks and reach the launch (which fails: no device here)."""
    assert call(L, batch(frames_bytes=0xffffff00), out_bytes=0xffffff00, out_cap=0xffffffff,
                flags=1, order=ADDR["order"]) == E_HIP
    assert call(L, batch(n=0xffffffff)) == E_HIP
    assert call(L, batch(offsets=None, stride=1, frame_len=0)) == E_HIP


def test_keys_argument_checks_in_the_documented_order(L):
    # 1. NULL batch / recs / keys, before the flags
    assert keys(L, None, flags=2) == E_INVAL
    for k in ("recs", "keys"):
        assert keys(L, batch(n=0), flags=2, **{k: None}) == E_INVAL, k
        assert keys(L, batch(n=0), **{k: None}) == E_INVAL, k
    # 2. flags, before n == 0
    for bad in (2, 3, 16, 0x80000000):
        assert keys(L, batch(n=0), flags=bad) == E_INVAL
    # 3. n == 0: RPKT_OK, nothing else is looked at
    for flags in (0, 1):
        assert keys(L, batch(n=0, frames=None, offsets=None, frames_bytes=1 << 33), flags=flags,
                    recs=A + 1, keys=A + 4) == OK
    # 4. NULL frames_dev, then frames_bytes, then no layout
    assert keys(L, batch(frames=None, frames_bytes=1 << 32)) == E_INVAL
    assert keys(L, batch(frames_bytes=1 << 32, offsets=None)) == E_TOO_LARGE
    assert keys(L, batch(frames_bytes=0xffffff01), recs=ADDR["recs"] + 8) == E_TOO_LARGE
    assert keys(L, batch(offsets=None), recs=ADDR["recs"] + 8) == E_INVAL
    # 5. alignment: recs 16 B, keys 8 B
    assert keys(L, batch(), recs=ADDR["recs"] + 8) == E_ALIGN
    assert keys(L, batch(), keys=ADDR["keys"] + 4) == E_ALIGN
    assert keys(L, batch(), keys=ADDR["keys"] + 8) == E_HIP          # a launch


def test_keys_limits_are_accepted(L):
    assert keys(L, batch(frames_bytes=0xffffff00, n=0xffffffff), flags=1) == E_HIP
    assert keys(L, batch(offsets=None, stride=1, frame_len=0)) == E_HIP
