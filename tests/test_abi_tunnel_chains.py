"""rpkt_gpu_parse_tunnel_chains refuses bad arguments before anything is launched (CPU
only: every call here returns from the argument checks)."""
import ctypes

import pytest

from rpkt_amd import engine
from rpkt_amd.build import build_gpu
from rpkt_amd.records import F_FLOW_EV

OK, E_INVAL, E_TOO_LARGE, E_ALIGN = 0, -1, -3, -4
A = 1 << 20                                    # a 16-byte aligned, never dereferenced address


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_parse_tunnel_chains


def chains(n=10, buf_bytes=1 << 16, segs=A, n_segs=10):
    return engine.Chains(A, buf_bytes, segs, A, n_segs, n)


def call(fn, c, flags=3, outer=A, tun=A, inner=A, ev=None, n_buckets=0):
    return fn(ctypes.byref(c) if c is not None else None, flags, outer, tun, inner, ev,
              n_buckets, None)


def test_null_chains_and_null_outputs(fn):
    assert call(fn, None) == E_INVAL
    for k in ("outer", "tun", "inner"):
        assert call(fn, chains(), **{k: None}) == E_INVAL
    assert call(fn, engine.Chains(A, 1 << 16, A, None, 10, 10)) == E_INVAL     # chain_first
    assert call(fn, engine.Chains(None, 1 << 16, A, A, 10, 10)) == E_INVAL     # buf with segments


def test_no_chains_is_ok_before_anything_else(fn):
    assert call(fn, chains(n=0)) == OK
    assert call(fn, chains(n=0), flags=3 | F_FLOW_EV, ev=None, n_buckets=0) == OK
    assert call(fn, chains(n=0), outer=None, tun=None, inner=None) == OK


def test_bad_flag(fn):
    for bad in (16, 64, 0x80000000):
        assert call(fn, chains(), flags=3 | bad) == E_INVAL
        assert call(fn, chains(n=0), flags=3 | bad) == E_INVAL


def test_misaligned_pointers(fn):
    assert call(fn, chains(segs=A + 4)) == E_ALIGN
    for k in ("outer", "tun", "inner"):
        assert call(fn, chains(), **{k: A + 8}) == E_ALIGN
    assert call(fn, chains(), flags=3 | F_FLOW_EV, ev=A + 4, n_buckets=16) == E_ALIGN


def test_arena_of_4_gib_is_too_large(fn):
    assert call(fn, chains(buf_bytes=1 << 32)) == E_TOO_LARGE
    assert call(fn, chains(n_segs=1 << 31)) == E_TOO_LARGE


def test_flow_events_need_a_buffer_and_buckets(fn):
    assert call(fn, chains(), flags=3 | F_FLOW_EV, ev=A, n_buckets=0) == E_INVAL
    assert call(fn, chains(), flags=3 | F_FLOW_EV, ev=None, n_buckets=16) == E_INVAL
    assert call(fn, chains(), flags=3 | F_FLOW_EV, ev=A, n_buckets=65536) == E_INVAL


def test_engine_wrapper_is_exported():
    assert "rpkt_gpu_parse_tunnel_chains" in engine.EXPORTS
    assert callable(engine.parse_tunnel_chains)
