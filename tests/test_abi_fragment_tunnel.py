"""rpkt_gpu_fragment_tunnel_batch's argument checks, in the documented order (include/rpkt_gpu.h,
at enum rpkt_err): rpkt_gpu_segment_tunnel_batch's, with mtu in mss's place and any combination
of RPKT_FRAGMENT_IGNORE_DF and RPKT_FRAGMENT_TUNNEL_OUTER for the flags.

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
REQUIRED = ("outer", "tun", "inner", "out_frames", "out_offsets", "frag_first", "totals", "workspace")
ADDR = {k: A + (j << 16) for j, k in enumerate(REQUIRED)}
FRAMES, OFFSETS = A + (12 << 16), A + (13 << 16)


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_fragment_tunnel_batch


def batch(n=10, frames=FRAMES, frames_bytes=1 << 16, offsets=OFFSETS, stride=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, 0, n, 0)


def call(fn, b, mtu=1500, flags=0, ip6_ident=0, out_bytes=1 << 16, out_cap=64, **ptr):
    p = dict(ADDR, **ptr)
    return fn(ctypes.byref(b) if b is not None else None, p["outer"], p["tun"], p["inner"], mtu,
              flags, ip6_ident, p["out_frames"], out_bytes, p["out_offsets"], out_cap,
              p["frag_first"], p["totals"], p["workspace"], None)


def test_the_entry_is_exported_and_sized():
    build_gpu()
    L = engine.lib()
    assert {"rpkt_gpu_fragment_tunnel_batch", "rpkt_gpu_fragment_tunnel_workspace_bytes"} <= set(engine.EXPORTS)
    assert engine.FRAGMENT_TUNNEL_OUTER == 2 and engine.FRAGMENT_IGNORE_DF == 1
    ws = L.rpkt_gpu_fragment_tunnel_workspace_bytes
    assert ws(0) == 0
    # a 64-byte plan and an 8-byte output base a frame, then the block sums
    for n in (1, 255, 256, 257, 70000):
        assert ws(n) % 16 == 0 and ws(n) >= 72 * n
        assert ws(n) == L.rpkt_gpu_segment_tunnel_workspace_bytes(n)


def test_argument_checks_in_the_documented_order(fn):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL batch / a record array / a required output / workspace, before the flags
    assert call(fn, None, flags=4) == E_INVAL
    for k in REQUIRED:
        assert call(fn, batch(n=0), flags=4, **{k: None}) == E_INVAL, k
        assert call(fn, batch(n=0), **{k: None}) == E_INVAL, k       # even for no frames
    # 2. flags (any of IGNORE_DF | TUNNEL_OUTER), then mtu: before n == 0
    for bad in (4, 16, 17, 0x80000000):
        assert call(fn, batch(n=0), flags=bad) == E_INVAL
    for flags in (0, 1, 2, 3):
        for mtu in (0, 65536, 0xffffffff):
            assert call(fn, batch(n=0), mtu=mtu, flags=flags) == E_INVAL
        for mtu in (1, 65535):
            assert call(fn, batch(n=0), mtu=mtu, flags=flags) == OK
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


def test_the_limits_are_accepted(fn):
    """The largest sizes pass the checks (and fail only at the launch: no device here)."""
    assert call(fn, batch(frames_bytes=0xffffff00), out_bytes=0xffffff00, out_cap=0xffffffff,
                flags=3, ip6_ident=0xffffffff) == E_HIP
    assert call(fn, batch(n=0xffffffff), mtu=65535) == E_HIP
    assert call(fn, batch(), mtu=1, flags=2) == E_HIP
