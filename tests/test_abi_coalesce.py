"""rpkt_gpu_coalesce_batch's argument checks, in the documented order (include/rpkt_gpu.h, at
enum rpkt_err): rpkt_gpu_segment_batch's with this entry's arguments in their places.

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
ADDR = {k: A + (j << 16) for j, k in enumerate(REQUIRED + ("order", "out_mss"))}


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_coalesce_batch


def batch(n=10, frames=A + (9 << 16), frames_bytes=1 << 16, offsets=A + (10 << 16), stride=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, 0, n, 0)


def call(fn, b, max_payload=65535, flags=0, out_bytes=1 << 16, out_cap=64, **ptr):
    p = dict(ADDR, **ptr)
    return fn(ctypes.byref(b) if b is not None else None, p["recs"], p["order"], max_payload, flags,
              p["out_frames"], out_bytes, p["out_offsets"], out_cap, p["src_first"], p["out_mss"],
              p["totals"], p["workspace"], None)


def test_the_workspace_sizes_are_pinned(fn):
    """rpkt_gpu_segment_workspace_bytes and rpkt_gpu_coalesce_workspace_bytes: the values of
    the layouts written out by hand (32 B of plan and a u64 per input, coalescing's u32 per
    input, 16 B and coalescing's u32 per block of 256; each region a multiple of 16 B)."""
    L = engine.lib()
    want = {0: (0, 0), 1: (64, 96), 255: (10224, 11264), 256: (10256, 11296), 257: (10320, 11376),
            70000: (2804384, 3085488)}
    for n, (seg, co) in want.items():
        assert L.rpkt_gpu_segment_workspace_bytes(n) == seg and seg % 16 == 0, n
        assert L.rpkt_gpu_coalesce_workspace_bytes(n) == co and co % 16 == 0, n


def test_argument_checks_in_the_documented_order(fn):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL batch / recs / a required output / workspace, before the flags
    assert call(fn, None, flags=2) == E_INVAL
    for k in REQUIRED:
        assert call(fn, batch(n=0), flags=2, **{k: None}) == E_INVAL, k
        assert call(fn, batch(n=0), **{k: None}) == E_INVAL, k      # even for an empty batch
    # order_dev and out_mss_dev are optional
    assert call(fn, batch(n=0), order=None, out_mss=None) == OK
    # 2. flags, then max_payload: before n == 0
    for bad in (2, 3, 4, 0x80000000):
        assert call(fn, batch(n=0), flags=bad) == E_INVAL
    for mp in (0, 65536, 0xffffffff):
        assert call(fn, batch(n=0), max_payload=mp) == E_INVAL
        assert call(fn, batch(n=0), max_payload=mp, flags=1) == E_INVAL
    for mp in (1, 65535):
        assert call(fn, batch(n=0), max_payload=mp) == OK
        assert call(fn, batch(n=0), max_payload=mp, flags=1) == OK  # RPKT_COALESCE_TRUST_SUMS
    # 3. n == 0: RPKT_OK, nothing else is looked at
    assert call(fn, batch(n=0, frames=None, frames_bytes=1 << 33, offsets=None), out_cap=0,
                out_bytes=1 << 33, recs=A + 1, totals=A + 4) == OK
    # 4. NULL frames_dev, before the sizes
    assert call(fn, batch(frames=None, frames_bytes=1 << 32)) == E_INVAL
    # 5. frames_bytes, then out_bytes, at the same limit, before the layout
    assert call(fn, batch(frames_bytes=1 << 32, offsets=None), out_bytes=1 << 32) == E_TOO_LARGE
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
    assert call(fn, batch(), totals=ADDR["totals"] + 8) == E_HIP    # every check passed: a launch


def test_the_limits_are_accepted(fn):
    """The largest sizes pass the checks (and fail only at the launch: no device here)."""
    assert call(fn, batch(frames_bytes=0xffffff00), out_bytes=0xffffff00, out_cap=0xffffffff) == E_HIP
    assert call(fn, batch(stride=64, offsets=None), order=None, out_mss=None, flags=1,
                max_payload=1) == E_HIP
