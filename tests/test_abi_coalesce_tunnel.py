"""rpkt_gpu_coalesce_tunnel_batch's argument checks, in the documented order (include/rpkt_gpu.h,
at enum rpkt_err): rpkt_gpu_coalesce_batch's, with tun_dev and inner_dev required and 16-byte
aligned along with outer_dev; order_dev and out_mss_dev may be NULL.

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
REQUIRED = ("outer", "tun", "inner", "out_frames", "out_offsets", "src_first", "totals", "workspace")
OPTIONAL = ("order", "out_mss")
ADDR = {k: A + (j << 16) for j, k in enumerate(REQUIRED + OPTIONAL)}
FRAMES, OFFSETS = A + (12 << 16), A + (13 << 16)


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_coalesce_tunnel_batch


def batch(n=10, frames=FRAMES, frames_bytes=1 << 16, offsets=OFFSETS, stride=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, 0, n, 0)


def call(fn, b, max_payload=65535, flags=0, out_bytes=1 << 16, out_cap=64, **ptr):
    p = dict(ADDR, **ptr)
    return fn(ctypes.byref(b) if b is not None else None, p["outer"], p["tun"], p["inner"],
              p["order"], max_payload, flags, p["out_frames"], out_bytes, p["out_offsets"], out_cap,
              p["src_first"], p["out_mss"], p["totals"], p["workspace"], None)


def test_the_entry_is_exported_and_sized():
    build_gpu()
    L = engine.lib()
    assert {"rpkt_gpu_coalesce_tunnel_batch", "rpkt_gpu_coalesce_tunnel_workspace_bytes"} <= \
        set(engine.EXPORTS)
    ws = L.rpkt_gpu_coalesce_tunnel_workspace_bytes
    # per position: a 32-byte plan, a u64 destination, a u32, the carrier's 16 bytes; per block
    # of 256 positions a u64 pair and a u32; each region rounded up to 16 bytes
    # n = 1: 32 + 16 + 16 + 16 + 16 + 16; n = 256: 8192 + 2048 + 1024 + 16 + 16 + 4096;
    # n = 257 (two blocks): 8224 + 2064 + 1040 + 32 + 16 + 4112
    assert [ws(n) for n in (0, 1, 256, 257)] == [0, 112, 15392, 15488]
    # the carrier's 16 bytes a position on top of the flat entry's
    for n in (1, 255, 256, 257, 70000):
        assert ws(n) % 16 == 0 and ws(n) == L.rpkt_gpu_coalesce_workspace_bytes(n) + 16 * n


def test_argument_checks_in_the_documented_order(fn):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL batch / a record array / a required output / workspace, before the flags
    assert call(fn, None, flags=2) == E_INVAL
    for k in REQUIRED:
        assert call(fn, batch(n=0), flags=2, **{k: None}) == E_INVAL, k
        assert call(fn, batch(n=0), **{k: None}) == E_INVAL, k       # even for no frames
    # 2. flags (TRUST_SUMS, UDP), then max_payload: before n == 0
    for bad in (2, 4, 8, 18, 32, 0x80000000):
        assert call(fn, batch(n=0), flags=bad) == E_INVAL
    for flags in (0, 1, 16, 17):
        for mp in (0, 65536, 0xffffffff):
            assert call(fn, batch(n=0), max_payload=mp, flags=flags) == E_INVAL
        for mp in (1, 65535):
            assert call(fn, batch(n=0), max_payload=mp, flags=flags) == OK
    # 3. n == 0: RPKT_OK, nothing else is looked at
    assert call(fn, batch(n=0, frames=None, offsets=None, frames_bytes=1 << 33), out_cap=0,
                out_bytes=1 << 33, outer=A + 1, tun=A + 2, inner=A + 3, totals=A + 4) == OK
    # 4. NULL frames_dev, before the sizes
    assert call(fn, batch(frames=None, frames_bytes=1 << 32)) == E_INVAL
    # 5. frames_bytes, then out_bytes at the same limit, before the layout
    assert call(fn, batch(frames_bytes=1 << 32, offsets=None)) == E_TOO_LARGE
    assert call(fn, batch(frames_bytes=0xffffff01, offsets=None)) == E_TOO_LARGE
    assert call(fn, batch(offsets=None), out_bytes=1 << 32) == E_TOO_LARGE
    assert call(fn, batch(offsets=None), out_bytes=0xffffff01) == E_TOO_LARGE
    # 6. no layout, before out_cap
    assert call(fn, batch(offsets=None), out_cap=0) == E_INVAL
    assert call(fn, batch(offsets=None, stride=64), out_cap=1, tun=ADDR["tun"] + 8) == E_ALIGN
    # 7. out_cap == 0, before the alignment
    assert call(fn, batch(), out_cap=0, outer=ADDR["outer"] + 8) == E_INVAL
    # 8. alignment: totals 8 B; the three record arrays, out_frames, workspace 16 B
    assert call(fn, batch(), totals=ADDR["totals"] + 4) == E_ALIGN
    for k in ("outer", "tun", "inner", "out_frames", "workspace"):
        assert call(fn, batch(), **{k: ADDR[k] + 8}) == E_ALIGN, k
    assert call(fn, batch(), totals=ADDR["totals"] + 8) == E_HIP     # a launch
    # order_dev and out_mss_dev are optional and carry no alignment of their own
    assert call(fn, batch(), order=None, out_mss=None) == E_HIP
    assert call(fn, batch(), order=ADDR["order"] + 4, out_mss=ADDR["out_mss"] + 2) == E_HIP


def test_the_limits_are_accepted(fn):
    """The largest sizes pass the checks (and fail only at the launch: no device here)."""
    assert call(fn, batch(frames_bytes=0xffffff00), out_bytes=0xffffff00, out_cap=0xffffffff,
                flags=17) == E_HIP
    assert call(fn, batch(n=0xffffffff), max_payload=65535) == E_HIP
    assert call(fn, batch(), max_payload=1) == E_HIP
