"""The argument-check matrix of the C ABI: for every checked entry point a valid call and a
list of named single mutations of it, and the calls made from them -- every subset of one or
two mutations.  The checks of an entry run in sequence and return early, so the pairs fix
their whole precedence.  Shared by tests/test_abi_status_matrix.py and the generator of its
expected statuses, tests/golden/make_abi_status.py.

Every device address is fake (aligned as its rule asks, never dereferenced): no call made
here may reach a launch, so the unmutated call is never made, and a mutation the library
accepts is not listed.  Only the request array of rpkt_gpu_fields_batch, the descriptors and
the ring slots are host memory.  Where no GPU is visible a launch fails with RPKT_E_HIP
instead of touching the fake addresses, which is why the test runs only there.
"""
import ctypes
import itertools

import numpy as np

from rpkt_amd import engine
from rpkt_amd.records import F_FLOW_EV, FIELD_REQ_DTYPE

E_HIP = -2
# fake device addresses, 64 KiB apart, all 16-byte aligned
FRAMES, OFFS, RECS, OPTS, OUTER, TUN, INNER, TUN2, INNER2, EV, EV1, AUX, SEGS, FIRST = (
    (1 << 20) + (k << 16) for k in range(14))


def put(**kw):
    return lambda s: s.update(kw)


def flag(key="flags"):
    def f(s):
        s[key] |= 0x80
    return f


def ev(**kw):
    return lambda s: s.update(ev_on=True, **kw)


def ptr(name, addr, align=0):
    """`name` null and, where it has an alignment rule, off it by half the alignment."""
    m = {name + "_null": put(**{name: None})}
    if align:
        m[name + "_misaligned"] = put(**{name: addr + align // 2})
    return m


def join(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


EV_MUTS = {"ev_null": ev(ev=None), "ev_0_buckets": ev(n_buckets=0),
           "ev_65536_buckets": ev(n_buckets=65536), "ev_misaligned": ev(ev=EV + 4)}
BATCH_MUTS = {"batch_null": put(b=False), "frames_null": put(frames=None),
              "too_large": put(frames_bytes=1 << 32), "no_layout": put(offsets=None),
              "n_0": put(n=0)}
CHAINS_MUTS = join({"chains_null": put(c=False), "too_large": put(buf_bytes=1 << 32),
                    "too_many_segs": put(n_segs=1 << 31), "n_0": put(n=0)},
                   ptr("buf", FRAMES), ptr("segs", SEGS, 8), ptr("chain_first", FIRST))


def batch_spec(**kw):
    """A packed batch of 10 frames (null offsets = no layout) and the usual arguments."""
    s = dict(b=True, frames=FRAMES, frames_bytes=1 << 16, offsets=OFFS, stride=0, frame_len=0,
             n=10, flags=3, ev_on=False, ev=EV, n_buckets=16)
    s.update(kw)
    return s


def chains_spec(**kw):
    s = dict(c=True, buf=FRAMES, buf_bytes=1 << 16, segs=SEGS, chain_first=FIRST, n_segs=10,
             n=10, flags=3, ev_on=False, ev=EV, n_buckets=16)
    s.update(kw)
    return s


def desc(s):
    return engine.Batch(s["frames"], s["frames_bytes"], s["offsets"], s["stride"],
                        s["frame_len"], s["n"], 0)


def bref(s, keep):
    if not s["b"]:
        return None
    keep.append(desc(s))
    return ctypes.byref(keep[-1])


def cref(s, keep):
    if not s["c"]:
        return None
    keep.append(engine.Chains(s["buf"], s["buf_bytes"], s["segs"], s["chain_first"],
                              s["n_segs"], s["n"]))
    return ctypes.byref(keep[-1])


def flags_of(s):
    return s["flags"] | (F_FLOW_EV if s["ev_on"] else 0)


def ring_args(slot_type, outputs):
    """Three slots: an empty one, a valid one, and the one the mutations apply to."""
    def args(s, keep):
        if not s["slots"]:
            return (None, s["n_slots"], flags_of(s), s["n_buckets"], None)
        arr = (slot_type * 3)()
        arr[1].batch, arr[1].flow_ev_dev = desc(batch_spec()), EV1
        arr[2].batch, arr[2].flow_ev_dev = desc(s), s["ev"]
        for name, addr in outputs.items():
            setattr(arr[1], name + "_dev", addr + 4096)
            setattr(arr[2], name + "_dev", s[name])
        keep.append(arr)
        return (arr, s["n_slots"], flags_of(s), s["n_buckets"], None)
    return args


def fields_args(s, keep):
    reqs = np.zeros(33, dtype=FIELD_REQ_DTYPE)
    reqs["bits"] = 8
    if s["bad_req"]:
        reqs["bits"][0] = 0
    keep.append(reqs)
    rp = reqs.ctypes.data_as(ctypes.c_void_p) if s["reqs"] else None
    return (bref(s, keep), s["layers"], rp, s["n_req"], s["values"], s["present"], None)


def fwd_args(s, keep):
    f = None
    if s["fwd"]:
        fwd = engine.Fwd()
        fwd.forbid_dev, fwd.n_forbid, fwd.flags = s["forbid"], s["n_forbid"], s["fwd_flags"]
        keep.append(fwd)
        f = ctypes.byref(fwd)
    return (bref(s, keep), f, s["keep"], None)


def rx_args(*outputs):
    return lambda s, keep: (bref(s, keep), flags_of(s)) + tuple(s[k] for k in outputs) + \
        (s["ev"], s["n_buckets"], None)


def chain_rx_args(*outputs):
    return lambda s, keep: (cref(s, keep), flags_of(s)) + tuple(s[k] for k in outputs) + \
        (s["ev"], s["n_buckets"], None)


RX = join(BATCH_MUTS, {"flag_unknown": flag()}, ptr("recs", RECS, 16), EV_MUTS)
RX_OPTS = join(RX, ptr("opts", OPTS, 16))
TUN3 = join(ptr("outer", OUTER, 16), ptr("tun", TUN, 16), ptr("inner", INNER, 16))
RING = join({"slots_null": put(slots=False), "n_slots_0": put(n_slots=0)},
            {k: v for k, v in BATCH_MUTS.items() if k not in ("batch_null", "n_0")},
            {"flag_unknown": flag()}, EV_MUTS)
TX = join(BATCH_MUTS, {"frames_misaligned": put(frames=FRAMES + 8), "flag_unknown": flag()},
          ptr("recs", RECS, 16))
WALK = join(BATCH_MUTS, ptr("recs", RECS, 16), ptr("opts", OPTS, 16))

# name -> (the valid call's description, its mutations, description -> argument tuple)
ENTRIES = {
    "rpkt_gpu_parse_batch": (batch_spec(recs=RECS), RX, rx_args("recs")),
    "rpkt_gpu_parse_batch_compact": (batch_spec(recs=RECS), RX, rx_args("recs")),
    "rpkt_gpu_parse_options_batch": (batch_spec(recs=RECS, opts=OPTS), RX_OPTS,
                                     rx_args("recs", "opts")),
    "rpkt_gpu_parse_options_batch_compact": (batch_spec(recs=RECS, opts=OPTS), RX_OPTS,
                                             rx_args("recs", "opts")),
    "rpkt_gpu_parse_ring": (batch_spec(slots=True, n_slots=3, recs=RECS),
                            join(RING, ptr("recs", RECS, 16)),
                            ring_args(engine.RingSlot, {"recs": RECS})),
    "rpkt_gpu_parse_ring_compact": (batch_spec(slots=True, n_slots=3, recs=RECS),
                                    join(RING, ptr("recs", RECS, 16)),
                                    ring_args(engine.RingSlot, {"recs": RECS})),
    "rpkt_gpu_parse_chains": (chains_spec(recs=RECS),
                              join(CHAINS_MUTS, {"flag_unknown": flag()}, ptr("recs", RECS, 16),
                                   EV_MUTS), chain_rx_args("recs")),
    "rpkt_gpu_parse_tunnel_batch": (batch_spec(outer=OUTER, tun=TUN, inner=INNER),
                                    join(BATCH_MUTS, {"flag_unknown": flag()}, TUN3, EV_MUTS),
                                    rx_args("outer", "tun", "inner")),
    "rpkt_gpu_parse_tunnel_ring": (batch_spec(slots=True, n_slots=3, outer=OUTER, tun=TUN,
                                              inner=INNER), join(RING, TUN3),
                                   ring_args(engine.TunRingSlot,
                                             {"outer": OUTER, "tun": TUN, "inner": INNER})),
    "rpkt_gpu_parse_tunnel_chains": (chains_spec(outer=OUTER, tun=TUN, inner=INNER),
                                     join(CHAINS_MUTS, {"flag_unknown": flag()}, TUN3, EV_MUTS),
                                     chain_rx_args("outer", "tun", "inner")),
    "rpkt_gpu_parse_tunnel_next": (
        batch_spec(tun=TUN, inner=INNER, tun_next=TUN2, inner_next=INNER2),
        join(BATCH_MUTS, {"flag_unknown": flag()}, ptr("tun", TUN, 16), ptr("inner", INNER, 16),
             ptr("tun_next", TUN2, 16), ptr("inner_next", INNER2, 16),
             {"tun_next_aliases": put(tun_next=TUN), "inner_next_aliases": put(inner_next=INNER)},
             EV_MUTS), rx_args("tun", "inner", "tun_next", "inner_next")),
    "rpkt_gpu_build_batch": (batch_spec(recs=RECS), TX,
                             lambda s, keep: (bref(s, keep), s["recs"], s["flags"], AUX, None)),
    "rpkt_gpu_build_tunnel_batch": (batch_spec(recs=RECS, tun=TUN), join(TX, ptr("tun", TUN, 16)),
                                    lambda s, keep: (bref(s, keep), s["recs"], s["tun"],
                                                     s["flags"], AUX, None)),
    "rpkt_gpu_forward_batch": (
        batch_spec(fwd=True, fwd_flags=0, forbid=AUX, n_forbid=4, keep=RECS),
        join(BATCH_MUTS, {"frames_misaligned": put(frames=FRAMES + 8), "fwd_null": put(fwd=False),
                          "flag_unknown": flag("fwd_flags"), "forbid_without_list": put(forbid=None)},
             ptr("keep", RECS)), fwd_args),
    "rpkt_gpu_options_batch": (batch_spec(recs=RECS, opts=OPTS), WALK,
                               lambda s, keep: (bref(s, keep), s["recs"], s["opts"], None)),
    "rpkt_gpu_options_batch_compact": (batch_spec(recs=RECS, opts=OPTS), WALK,
                                       lambda s, keep: (bref(s, keep), s["recs"], s["opts"], None)),
    "rpkt_gpu_layers_batch": (batch_spec(layers=RECS), join(BATCH_MUTS, ptr("layers", RECS, 16)),
                              lambda s, keep: (bref(s, keep), s["layers"], None)),
    "rpkt_gpu_fields_batch": (
        batch_spec(layers=RECS, reqs=True, n_req=2, bad_req=False, values=OPTS, present=AUX),
        join(BATCH_MUTS, ptr("layers", RECS, 16), ptr("values", OPTS, 8),
             {"reqs_null": put(reqs=False), "present_misaligned": put(present=AUX + 2),
              "n_req_0": put(n_req=0), "n_req_33": put(n_req=33), "bad_req": put(bad_req=True)}),
        fields_args),
    "rpkt_gpu_flow_count": (
        dict(ev=EV, n=10, n_buckets=16, counters=RECS, workspace=AUX),
        join(ptr("ev", EV), ptr("counters", RECS), ptr("workspace", AUX),
             {"0_buckets": put(n_buckets=0), "65536_buckets": put(n_buckets=65536),
              "n_0": put(n=0)}),
        lambda s, keep: (s["ev"], s["n"], s["n_buckets"], s["counters"], s["workspace"], None)),
    "rpkt_gpu_checksum_ranges": (
        dict(buf=FRAMES, buf_bytes=1 << 16, ranges=OFFS, n=10, out=RECS),
        join(ptr("buf", FRAMES), ptr("ranges", OFFS), ptr("out", RECS),
             {"too_large": put(buf_bytes=1 << 32), "n_0": put(n=0)}),
        lambda s, keep: (s["buf"], s["buf_bytes"], s["ranges"], s["n"], s["out"], None)),
    "rpkt_gpu_checksum_chains": (
        dict(buf=FRAMES, buf_bytes=1 << 16, segs=SEGS, n_segs=10, chain_first=FIRST, n=10,
             out=RECS, workspace=AUX),
        join(ptr("buf", FRAMES), ptr("segs", SEGS), ptr("chain_first", FIRST), ptr("out", RECS),
             ptr("workspace", AUX), {"too_large": put(buf_bytes=1 << 32), "n_0": put(n=0)}),
        lambda s, keep: (s["buf"], s["buf_bytes"], s["segs"], s["n_segs"], s["chain_first"],
                         s["n"], s["out"], s["workspace"], None)),
    "rpkt_gpu_flow_reduce": (
        dict(counters=RECS, n_buckets=16, root=-1, comm=AUX),
        join(ptr("counters", RECS, 8), ptr("comm", AUX),
             {"0_buckets": put(n_buckets=0), "65536_buckets": put(n_buckets=65536),
              "bad_root": put(root=-2)}),
        lambda s, keep: (s["counters"], s["n_buckets"], s["root"], s["comm"], None)),
}


def cases(entry):
    """The names of an entry's calls: "a" and "a+b" over its mutations, in list order."""
    names = list(ENTRIES[entry][1])
    return names + ["%s+%s" % p for p in itertools.combinations(names, 2)]


def run(L, entry, case):
    """The status `entry` returns for the valid call with `case`'s mutations applied."""
    spec, muts, args = ENTRIES[entry]
    s = dict(spec)
    for m in case.split("+"):
        muts[m](s)
    keep = []                                   # descriptors alive until the call returns
    return int(getattr(L, entry)(*args(s, keep)))
