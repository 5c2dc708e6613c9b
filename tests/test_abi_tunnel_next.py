"""rpkt_gpu_parse_tunnel_next refuses bad arguments before anything is launched (CPU only:
every call here returns from the argument checks), in rpkt_gpu_parse_tunnel_chains's order."""
import ctypes

import pytest

from rpkt_amd import engine
from rpkt_amd.build import build_gpu
from rpkt_amd.records import F_FLOW_EV, F_IPV6

OK, E_INVAL, E_TOO_LARGE, E_ALIGN = 0, -1, -3, -4
A = 1 << 20                                    # 16-byte aligned, never dereferenced addresses
B, C, D = A + (1 << 16), A + (2 << 16), A + (3 << 16)


@pytest.fixture(scope="module")
def fn():
    build_gpu()
    return engine.lib().rpkt_gpu_parse_tunnel_next


def batch(n=10, frames=A, frames_bytes=1 << 16, offsets=A, stride=0, frame_len=0):
    return engine.Batch(frames, frames_bytes, offsets, stride, frame_len, n, 0)


def call(fn, b, flags=3, tun=A, inner=B, tun_next=C, inner_next=D, ev=None, n_buckets=0):
    return fn(ctypes.byref(b) if b is not None else None, flags, tun, inner, tun_next,
              inner_next, ev, n_buckets, None)


def test_null_batch_and_null_pointers(fn):
    assert call(fn, None) == E_INVAL
    for k in ("tun", "inner", "tun_next", "inner_next"):
        assert call(fn, batch(), **{k: None}) == E_INVAL
    assert call(fn, batch(frames=None)) == E_INVAL
    assert call(fn, batch(offsets=None, stride=0)) == E_INVAL          # no layout


def test_no_frames_is_ok_before_anything_else(fn):
    assert call(fn, batch(n=0)) == OK
    assert call(fn, batch(n=0), flags=3 | F_FLOW_EV, ev=None, n_buckets=0) == OK
    assert call(fn, batch(n=0), tun=None, inner=None, tun_next=None, inner_next=None) == OK
    assert call(fn, batch(n=0), tun_next=A, inner_next=B) == OK


def test_bad_flag(fn):
    for bad in (16, 64, 0x80000000):
        assert call(fn, batch(), flags=3 | bad) == E_INVAL
        assert call(fn, batch(n=0), flags=3 | bad) == E_INVAL
    # every accepted flag passes the checks when its arguments are right (n == 0: no launch)
    assert call(fn, batch(n=0), flags=3 | F_IPV6 | F_FLOW_EV, ev=A, n_buckets=7) == OK


def test_an_output_that_aliases_its_input(fn):
    assert call(fn, batch(), tun_next=A) == E_INVAL
    assert call(fn, batch(), inner_next=B) == E_INVAL


def test_misaligned_pointers(fn):
    for k, v in (("tun", A), ("inner", B), ("tun_next", C), ("inner_next", D)):
        assert call(fn, batch(), **{k: v + 8}) == E_ALIGN
    assert call(fn, batch(), flags=3 | F_FLOW_EV, ev=A + 4, n_buckets=16) == E_ALIGN


def test_frames_of_4_gib_are_too_large(fn):
    assert call(fn, batch(frames_bytes=1 << 32)) == E_TOO_LARGE


def test_flow_events_need_a_buffer_and_buckets(fn):
    assert call(fn, batch(), flags=3 | F_FLOW_EV, ev=A, n_buckets=0) == E_INVAL
    assert call(fn, batch(), flags=3 | F_FLOW_EV, ev=None, n_buckets=16) == E_INVAL
    assert call(fn, batch(), flags=3 | F_FLOW_EV, ev=A, n_buckets=65536) == E_INVAL


def test_engine_wrappers_are_exported():
    assert "rpkt_gpu_parse_tunnel_next" in engine.EXPORTS
    assert callable(engine.parse_tunnel_next) and callable(engine.parse_tunnel_levels)
    assert engine.lib().rpkt_gpu_abi_version() == 1
