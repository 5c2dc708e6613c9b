"""rpkt_gpu_fragment_batch's argument checks, in the documented order (include/rpkt_gpu.h, at
enum rpkt_err): rpkt_gpu_segment_batch's with frag_first_dev in seg_first_dev's place, the flag
RPKT_FRAGMENT_IGNORE_DF and mtu in mss's place.

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
REQUIRED = ("recs", "out_frames", "out_offsets", "frag_first", "totals", "workspace")
ADDR = {k: A + (j << 16) for j, k in enumerate(REQUIRED)}
FRAMES, OFFSETS = A + (9 << 16), A + (10 << 16)


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_fragment_batch


def batch(n=10, frames=FRAMES, frames_bytes=1 << 16, offsets=OFFSETS, stride=0, frame_len=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, frame_len, n, 0)


def call(fn, b, mtu=1500, flags=0, ip6_ident=0, out_bytes=1 << 16, out_cap=64, **ptr):
    p = dict(ADDR, **ptr)
    return fn(ctypes.byref(b) if b is not None else None, p["recs"], mtu, flags, ip6_ident,
              p["out_frames"], out_bytes, p["out_offsets"], out_cap, p["frag_first"], p["totals"],
              p["workspace"], None)


def test_the_entry_is_exported_and_sized(fn):
    L = engine.lib()
    assert {"rpkt_gpu_fragment_batch", "rpkt_gpu_fragment_workspace_bytes"} <= set(engine.EXPORTS)
    assert engine.FRAGMENT_IGNORE_DF == 1
    assert L.rpkt_gpu_fragment_workspace_bytes(0) == 0
    # a 32-B plan and a u64 base per frame, a u64 pair per block of 256 frames
    for n in (1, 255, 256, 257, 70000, 0xffffffff):
        assert L.rpkt_gpu_fragment_workspace_bytes(n) % 16 == 0
        assert L.rpkt_gpu_fragment_workspace_bytes(n) >= 40 * n


def test_argument_checks_in_the_documented_order(fn):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL batch / recs / a required output / workspace, before the flags
    assert call(fn, None, flags=2) == E_INVAL
    for k in REQUIRED:
        assert call(fn, batch(n=0), flags=2, **{k: None}) == E_INVAL, k
        assert call(fn, batch(n=0), **{k: None}) == E_INVAL, k      # even for no frames
    # 2. flags other than 0 and 1, then mtu: before n == 0
    for bad in (2, 3, 16, 0x80000000):
        assert call(fn, batch(n=0), flags=bad) == E_INVAL
        assert call(fn, batch(n=0), flags=bad, mtu=0) == E_INVAL
    for mtu in (0, 65536, 0xffffffff):
        assert call(fn, batch(n=0), mtu=mtu) == E_INVAL
        assert call(fn, batch(n=0), mtu=mtu, flags=1) == E_INVAL
    # 3. n == 0: RPKT_OK, nothing else is looked at
    for mtu in (1, 65535):
        for flags in (0, 1):
            assert call(fn, batch(n=0), mtu=mtu, flags=flags, ip6_ident=0xffffffff) == OK
    assert call(fn, batch(n=0, frames=None, offsets=None, frames_bytes=1 << 33), out_cap=0,
                out_bytes=1 << 33, recs=A + 1, totals=A + 4) == OK
    # 4. NULL frames_dev, before the sizes; frames_bytes, then out_bytes at the same limit
    assert call(fn, batch(frames=None, frames_bytes=1 << 32)) == E_INVAL
    assert call(fn, batch(frames_bytes=1 << 32, offsets=None), out_cap=0) == E_TOO_LARGE
    assert call(fn, batch(frames_bytes=0xffffff01), out_cap=0) == E_TOO_LARGE
    assert call(fn, batch(offsets=None), out_bytes=1 << 32, out_cap=0) == E_TOO_LARGE
    assert call(fn, batch(), out_bytes=0xffffff01, out_cap=0) == E_TOO_LARGE
    # 5. no layout, before out_cap
    assert call(fn, batch(offsets=None), out_cap=0) == E_INVAL
    # 6. out_cap == 0, before the alignment
    assert call(fn, batch(), out_cap=0, recs=ADDR["recs"] + 8) == E_INVAL
    # 7. alignment: totals 8 B; recs, out_frames, workspace 16 B
    assert call(fn, batch(), totals=ADDR["totals"] + 4) == E_ALIGN
    for k in ("recs", "out_frames", "workspace"):
        assert call(fn, batch(), **{k: ADDR[k] + 8}) == E_ALIGN, k
    assert call(fn, batch(), totals=ADDR["totals"] + 8, frag_first=ADDR["frag_first"] + 4,
                out_offsets=ADDR["out_offsets"] + 4) == E_HIP       # a launch


def test_the_limits_are_accepted(fn):
    """The largest sizes pass the checks and reach the launch (which fails: no device here)."""
    assert call(fn, batch(frames_bytes=0xffffff00), out_bytes=0xffffff00, out_cap=0xffffffff,
                mtu=65535, flags=1, ip6_ident=0xffffffff) == E_HIP
    assert call(fn, batch(n=0xffffffff), mtu=1) == E_HIP
    assert call(fn, batch(offsets=None, stride=1, frame_len=0), mtu=1280) == E_HIP
