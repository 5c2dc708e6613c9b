"""rpkt_gpu_fragment_chains' argument checks, in the documented order (include/rpkt_gpu.h, at
enum rpkt_err): rpkt_gpu_segment_chains' with mtu in mss's place and RPKT_FRAGMENT_IGNORE_DF
the only flag.

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
BUF, SEGS, FIRST = A + (9 << 16), A + (10 << 16), A + (11 << 16)


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_fragment_chains


def chains(n=10, n_segs=20, buf=BUF, buf_bytes=1 << 16, segs=SEGS, first=FIRST):
    return engine.Chains(buf, buf_bytes, segs, first, n_segs, n)


def call(fn, c, mtu=1500, flags=0, ip6_ident=7, out_bytes=1 << 16, out_cap=64, **ptr):
    p = dict(ADDR, **ptr)
    return fn(ctypes.byref(c) if c is not None else None, p["recs"], mtu, flags, ip6_ident,
              p["out_frames"], out_bytes, p["out_offsets"], out_cap, p["frag_first"], p["totals"],
              p["workspace"], None)


def test_the_entry_is_exported_and_sized(fn):
    L = engine.lib()
    assert {"rpkt_gpu_fragment_chains", "rpkt_gpu_fragment_chains_workspace_bytes"} <= set(engine.EXPORTS)
    assert engine.FRAGMENT_IGNORE_DF == 1
    # the plan -> scan -> write workspace of the flat entry, per chain
    for n in (0, 1, 255, 256, 257, 70000):
        assert L.rpkt_gpu_fragment_chains_workspace_bytes(n) == L.rpkt_gpu_fragment_workspace_bytes(n)
        assert L.rpkt_gpu_fragment_chains_workspace_bytes(n) % 16 == 0


def test_argument_checks_in_the_documented_order(fn):
    """One case per check; each also breaks a later check, which must not be the one
    reported."""
    # 1. NULL chains / recs / a required output / workspace, before the flags
    assert call(fn, None, flags=2) == E_INVAL
    for k in REQUIRED:
        assert call(fn, chains(n=0), flags=2, **{k: None}) == E_INVAL, k
        assert call(fn, chains(n=0), **{k: None}) == E_INVAL, k     # even for no chains
    # 2. flags, then mtu: before n_chains == 0
    for bad in (2, 3, 0x80000000):
        assert call(fn, chains(n=0), flags=bad) == E_INVAL
    assert call(fn, chains(n=0), flags=1) == OK
    for mtu in (0, 65536, 0xffffffff):
        assert call(fn, chains(n=0), mtu=mtu) == E_INVAL
        assert call(fn, chains(n=0), mtu=mtu, flags=1) == E_INVAL
    for mtu in (1, 65535):
        assert call(fn, chains(n=0), mtu=mtu) == OK
    # 3. n_chains == 0: RPKT_OK, nothing else is looked at
    assert call(fn, chains(n=0, buf=None, segs=None, first=None, buf_bytes=1 << 33,
                           n_segs=0xffffffff), out_cap=0, out_bytes=1 << 33, recs=A + 1,
                totals=A + 4, ip6_ident=0xffffffff) == OK
    # 4. the chains: NULL chain_first_dev, or with segments a NULL buf_dev / segs_dev, before
    #    the sizes; then buf_bytes and n_segs
    assert call(fn, chains(first=None, buf_bytes=1 << 32)) == E_INVAL
    assert call(fn, chains(buf=None, buf_bytes=1 << 32)) == E_INVAL
    assert call(fn, chains(segs=None, n_segs=0x80000000)) == E_INVAL
    assert call(fn, chains(buf_bytes=1 << 32), out_bytes=1 << 32, out_cap=0) == E_TOO_LARGE
    assert call(fn, chains(buf_bytes=0xffffff01), out_cap=0) == E_TOO_LARGE
    assert call(fn, chains(n_segs=0x80000000), out_cap=0) == E_TOO_LARGE
    # 5. out_bytes, at the same limit, before out_cap
    assert call(fn, chains(), out_bytes=1 << 32, out_cap=0) == E_TOO_LARGE
    assert call(fn, chains(), out_bytes=0xffffff01, out_cap=0) == E_TOO_LARGE
    # 6. out_cap == 0, before the alignment
    assert call(fn, chains(), out_cap=0, recs=ADDR["recs"] + 8) == E_INVAL
    assert call(fn, chains(segs=SEGS + 4), out_cap=0) == E_INVAL
    # 7. alignment: segs and totals 8 B; recs, out_frames, workspace 16 B
    assert call(fn, chains(segs=SEGS + 4)) == E_ALIGN
    assert call(fn, chains(), totals=ADDR["totals"] + 4) == E_ALIGN
    for k in ("recs", "out_frames", "workspace"):
        assert call(fn, chains(), **{k: ADDR[k] + 8}) == E_ALIGN, k
    assert call(fn, chains(segs=SEGS + 8), totals=ADDR["totals"] + 8, flags=1) == E_HIP   # a launch


def test_the_limits_are_accepted(fn):
    """The largest sizes pass the checks (and fail only at the launch: no device here);
    chains without segments need neither an arena nor a segment table."""
    assert call(fn, chains(buf_bytes=0xffffff00, n_segs=0x7fffffff), out_bytes=0xffffff00,
                out_cap=0xffffffff) == E_HIP
    assert call(fn, chains(n_segs=0, buf=None, segs=None), mtu=1) == E_HIP
    assert call(fn, chains(n=0xffffffff), mtu=65535, flags=1, ip6_ident=0xffffffff) == E_HIP
