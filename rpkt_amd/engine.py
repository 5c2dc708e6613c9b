"""Device batch API: rpkt's decode-and-verify chain over a device-resident batch.

Thin ctypes layer over the C ABI in include/rpkt_gpu.h (librpkt_gpu.so, HIP for
gfx950).  torch supplies device memory and the current HIP stream only; no torch
type crosses the ABI.  There is no CPU fallback: if the HIP library is missing
or no GPU is visible, every call raises.
"""
import ctypes
import os

import numpy as np

from .build import ABLATE_LIB, GPU_LIB
from .records import LAYERS_BYTES, OPTS_BYTES, REC_BYTES, REC16_BYTES, F_FLOW_EV

RPKT_OK = 0
ERRORS = {-1: "RPKT_E_INVAL", -2: "RPKT_E_HIP", -3: "RPKT_E_TOO_LARGE", -4: "RPKT_E_ALIGN",
          -5: "RPKT_E_COLL"}


class RpktError(RuntimeError):
    pass


class Batch(ctypes.Structure):
    """rpkt_batch_t"""
    _fields_ = [("frames_dev", ctypes.c_void_p), ("frames_bytes", ctypes.c_uint64),
                ("offsets_dev", ctypes.c_void_p), ("stride", ctypes.c_uint32),
                ("frame_len", ctypes.c_uint32), ("n", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class Chains(ctypes.Structure):
    """rpkt_chains_t"""
    _fields_ = [("buf_dev", ctypes.c_void_p), ("buf_bytes", ctypes.c_uint64),
                ("segs_dev", ctypes.c_void_p), ("chain_first_dev", ctypes.c_void_p),
                ("n_segs", ctypes.c_uint32), ("n_chains", ctypes.c_uint32)]


class RingSlot(ctypes.Structure):
    """rpkt_ring_slot_t"""
    _fields_ = [("batch", Batch), ("recs_dev", ctypes.c_void_p), ("flow_ev_dev", ctypes.c_void_p)]


class TunRingSlot(ctypes.Structure):
    """rpkt_tun_ring_slot_t"""
    _fields_ = [("batch", Batch), ("outer_dev", ctypes.c_void_p), ("tun_dev", ctypes.c_void_p),
                ("inner_dev", ctypes.c_void_p), ("flow_ev_dev", ctypes.c_void_p)]


class Fwd(ctypes.Structure):
    """rpkt_fwd_t"""
    _fields_ = [("dmac", ctypes.c_uint8 * 6), ("smac", ctypes.c_uint8 * 6),
                ("forbid_dev", ctypes.c_void_p), ("n_forbid", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


_i, _u32, _p, _sz = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
_B, _C = ctypes.POINTER(Batch), ctypes.POINTER(Chains)
_PARSE = [_B, _u32, _p, _p, _u32, _p]                 # batch, flags, recs, events, buckets, stream
_RING = [_u32, _u32, _u32, _p]                        # n_slots, flags, buckets, stream
_COMM = [ctypes.POINTER(_p), _i, _p, _i]
# every function of include/rpkt_gpu.h: name -> (restype, argtypes)
ABI = {
    "rpkt_gpu_abi_version": (_u32, []),
    "rpkt_gpu_build_info": (ctypes.c_char_p, []),
    "rpkt_gpu_status_name": (ctypes.c_char_p, [_i]),
    "rpkt_gpu_last_hip_error": (_i, []),
    "rpkt_gpu_device_info": (_i, [ctypes.c_char_p, _sz]),
    "rpkt_gpu_parse_batch": (_i, _PARSE),
    "rpkt_gpu_parse_batch_compact": (_i, _PARSE),
    "rpkt_gpu_parse_ring": (_i, [ctypes.POINTER(RingSlot)] + _RING),
    "rpkt_gpu_parse_ring_compact": (_i, [ctypes.POINTER(RingSlot)] + _RING),
    "rpkt_gpu_flow_workspace_bytes": (_sz, [_u32, _u32]),
    "rpkt_gpu_flow_count": (_i, [_p, _u32, _u32, _p, _p, _p]),
    "rpkt_gpu_checksum_ranges": (_i, [_p, ctypes.c_uint64, _p, _u32, _p, _p]),
    "rpkt_gpu_checksum_chains_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_checksum_chains": (_i, [_p, ctypes.c_uint64, _p, _u32, _p, _u32, _p, _p, _p]),
    "rpkt_gpu_parse_chains": (_i, [_C] + _PARSE[1:]),
    "rpkt_gpu_build_batch": (_i, [_B, _p, _u32, _p, _p]),
    "rpkt_gpu_build_tunnel_batch": (_i, [_B, _p, _p, _u32, _p, _p]),
    "rpkt_gpu_forward_batch": (_i, [_B, ctypes.POINTER(Fwd), _p, _p]),
    "rpkt_gpu_segment_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_segment_batch": (_i, [_B, _p, _u32, _u32, _p, ctypes.c_uint64, _p, _u32, _p, _p, _p,
                                    _p]),
    "rpkt_gpu_segment_chains_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_segment_chains": (_i, [_C, _p, _u32, _u32, _p, ctypes.c_uint64, _p, _u32, _p, _p, _p,
                                     _p]),
    "rpkt_gpu_segment_tunnel_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_segment_tunnel_batch": (_i, [_B, _p, _p, _p, _u32, _u32, _p, ctypes.c_uint64, _p, _u32,
                                           _p, _p, _p, _p]),
    "rpkt_gpu_segment_tunnel_chains_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_segment_tunnel_chains": (_i, [_C, _p, _p, _p, _u32, _u32, _p, ctypes.c_uint64, _p, _u32,
                                            _p, _p, _p, _p]),
    "rpkt_gpu_fragment_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_fragment_batch": (_i, [_B, _p, _u32, _u32, _u32, _p, ctypes.c_uint64, _p, _u32, _p, _p,
                                     _p, _p]),
    "rpkt_gpu_fragment_chains_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_fragment_chains": (_i, [_C, _p, _u32, _u32, _u32, _p, ctypes.c_uint64, _p, _u32, _p, _p,
                                      _p, _p]),
    "rpkt_gpu_fragment_tunnel_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_fragment_tunnel_batch": (_i, [_B, _p, _p, _p, _u32, _u32, _u32, _p, ctypes.c_uint64, _p,
                                            _u32, _p, _p, _p, _p]),
    "rpkt_gpu_reassemble_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_reassemble_batch": (_i, [_B, _p, _p, _u32, _p, ctypes.c_uint64, _p, _u32, _p, _p, _p,
                                       _p]),
    "rpkt_gpu_reassemble_keys": (_i, [_B, _p, _u32, _p, _p]),
    "rpkt_gpu_coalesce_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_coalesce_batch": (_i, [_B, _p, _p, _u32, _u32, _p, ctypes.c_uint64, _p, _u32, _p, _p,
                                     _p, _p, _p]),
    "rpkt_gpu_coalesce_tunnel_workspace_bytes": (_sz, [_u32]),
    "rpkt_gpu_coalesce_tunnel_batch": (_i, [_B, _p, _p, _p, _p, _u32, _u32, _p, ctypes.c_uint64, _p,
                                            _u32, _p, _p, _p, _p, _p]),
    "rpkt_gpu_options_batch":(_i, [_B, _p, _p, _p]),
    "rpkt_gpu_options_batch_compact": (_i, [_B, _p, _p, _p]),
    "rpkt_gpu_parse_options_batch": (_i, [_B, _u32, _p, _p, _p, _u32, _p]),
    "rpkt_gpu_parse_options_batch_compact": (_i, [_B, _u32, _p, _p, _p, _u32, _p]),
    "rpkt_gpu_parse_tunnel_batch": (_i, [_B, _u32, _p, _p, _p, _p, _u32, _p]),
    "rpkt_gpu_parse_tunnel_ring": (_i, [ctypes.POINTER(TunRingSlot)] + _RING),
    "rpkt_gpu_parse_tunnel_chains": (_i, [_C, _u32, _p, _p, _p, _p, _u32, _p]),
    "rpkt_gpu_parse_tunnel_next": (_i, [_B, _u32, _p, _p, _p, _p, _p, _u32, _p]),
    "rpkt_gpu_layers_batch": (_i, [_B, _p, _p]),
    "rpkt_gpu_fields_batch": (_i, [_B, _p, _p, _u32, _p, _p, _p]),
    "rpkt_gpu_flow_reduce": (_i, [_p, _u32, _i, _p, _p]),
    "rpkt_gpu_last_coll_error": (_i, []),
    "rpkt_gpu_coll_version": (_i, []),
    "rpkt_gpu_coll_unique_id": (_i, [_p]),
    "rpkt_gpu_comm_init": (_i, _COMM),
    "rpkt_gpu_comm_init_timeout": (_i, _COMM + [_i]),
    "rpkt_gpu_comm_destroy": (_i, [_p]),
    "rpkt_gpu_comm_abort": (_i, [_p]),
    "rpkt_flow_hash": (_u32, [_u32, _u32, ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint8]),
}
EXPORTS = list(ABI)
COLL_ID_BYTES = 128

_lib = None


def lib():
    """Load librpkt_gpu.so (fails loudly: there is no fallback path)."""
    global _lib
    if _lib is None:
        # Bind to the HIP runtime torch already carries: loading ours first would
        # pull a second runtime (/opt/rocm) into the process, and only one of the
        # two can own the device.
        import torch  # noqa: F401
        if not os.path.exists(GPU_LIB):
            raise RpktError("HIP engine not built: %s missing (run __graft_entry__.build())"
                            % GPU_LIB)
        L = ctypes.CDLL(GPU_LIB)
        for name, (restype, argtypes) in ABI.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


_ablate = None


def ablate_lib():
    """librpkt_gpu_ablate.so: the product entry points plus the development hooks
    (rpkt_gpu_debug_*: kernel ablation variants and streaming references) that tools/
    and bench.py's copy ceiling use.  Never used by the product path."""
    global _ablate
    if _ablate is None:
        lib()                                   # torch's HIP runtime first, as for lib()
        if not os.path.exists(ABLATE_LIB):
            raise RpktError("development library not built: %s missing" % ABLATE_LIB)
        _ablate = ctypes.CDLL(ABLATE_LIB)
    return _ablate


def device_info():
    buf = ctypes.create_string_buffer(512)
    lib().rpkt_gpu_device_info(buf, 512)
    return buf.value.decode()


def _check(rc, what):
    if rc != RPKT_OK:
        extra = ""
        if rc == -2:
            extra = " (hipError %d)" % lib().rpkt_gpu_last_hip_error()
        elif rc == -5:
            extra = " (ncclResult %d)" % lib().rpkt_gpu_last_coll_error()
        raise RpktError("%s failed: %s%s" % (what, ERRORS.get(rc, rc), extra))


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RpktError("no GPU visible: the rpkt_amd engine has no CPU path")
    return torch


def _stream_ptr(stream):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


class DeviceBatch:
    """A batch resident in HBM: frames (uint8) and, for packed layout, u32 offsets."""

    def __init__(self, frames, n, offsets=None, stride=0, frame_len=0):
        self.frames, self.n, self.offsets = frames, n, offsets
        self.stride, self.frame_len = stride, frame_len

    @classmethod
    def from_host(cls, hb, device="cuda"):
        torch = _torch()
        frames = torch.from_numpy(np.ascontiguousarray(hb.frames)).to(device)
        offs = None
        if hb.offsets is not None:
            offs = torch.from_numpy(hb.offsets.view(np.int32)).to(device)
        return cls(frames, hb.n, offs, hb.stride, hb.frame_len)

    def shard(self, lo, hi):
        """Frames [lo, hi) as a view (packed offsets stay absolute: no copy)."""
        if self.offsets is not None:
            return DeviceBatch(self.frames, hi - lo, self.offsets[lo:hi + 1])
        return DeviceBatch(self.frames[lo * self.stride:], hi - lo, None, self.stride,
                           self.frame_len)

    def desc(self):
        return Batch(self.frames.data_ptr(), self.frames.numel(),
                     self.offsets.data_ptr() if self.offsets is not None else None,
                     self.stride, self.frame_len, self.n, 0)


def _call(name, *args):
    """One call of the C ABI; RpktError unless it returns RPKT_OK."""
    _check(getattr(lib(), name)(*args), name)


def _bytes(n, per, device):
    """A uint8 tensor of n * per bytes on `device`."""
    torch = _torch()
    return torch.empty(n * per, dtype=torch.uint8, device=device)


def _events(flags, flow_ev, n, device):
    """The flow-event tensor of a call: the caller's, or with RPKT_F_FLOW_EV a fresh one."""
    if flags & F_FLOW_EV and flow_ev is None:
        torch = _torch()
        flow_ev = torch.empty(n, dtype=torch.int64, device=device)
    return flow_ev


def _ptr(t):
    return t.data_ptr() if t is not None else None


def alloc_records(n, device="cuda"):
    return _bytes(n, REC_BYTES, device)


def parse_batch(batch, flags=3, recs=None, flow_ev=None, n_buckets=0, stream=None):
    """rpkt_gpu_parse_batch: returns the uint8 record tensor (n * 80 bytes)."""
    return _parse("rpkt_gpu_parse_batch", batch, batch.frames.device, REC_BYTES, flags, recs,
                  flow_ev, n_buckets, stream)


def _parse(name, src, dev, rec_bytes, flags, recs, flow_ev, n_buckets, stream):
    """parse_batch, parse_batch_compact and parse_chains: one record per frame of `src`."""
    recs = _bytes(src.n, rec_bytes, dev) if recs is None else recs
    flow_ev = _events(flags, flow_ev, src.n, dev)
    _call(name, ctypes.byref(src.desc()), flags, recs.data_ptr(), _ptr(flow_ev), n_buckets,
          _stream_ptr(stream))
    return (recs, flow_ev) if flags & F_FLOW_EV else recs


def _parse_tunnel(name, src, dev, flags, outer, tun, inner, flow_ev, n_buckets, stream):
    """parse_tunnel_batch and parse_tunnel_chains: three records per frame of `src`."""
    outer = alloc_records(src.n, dev) if outer is None else outer
    inner = alloc_records(src.n, dev) if inner is None else inner
    tun = _bytes(src.n, 16, dev) if tun is None else tun
    flow_ev = _events(flags, flow_ev, src.n, dev)
    _call(name, ctypes.byref(src.desc()), flags, outer.data_ptr(), tun.data_ptr(),
          inner.data_ptr(), _ptr(flow_ev), n_buckets, _stream_ptr(stream))
    return (outer, tun, inner, flow_ev) if flags & F_FLOW_EV else (outer, tun, inner)


def parse_tunnel_batch(batch, flags=3, outer=None, tun=None, inner=None, stream=None,
                       flow_ev=None, n_buckets=0):
    """rpkt_gpu_parse_tunnel_batch: returns (outer records, rpkt_tun_t, inner records) as
    uint8 tensors (n * 80, n * 16, n * 80 bytes); with RPKT_F_FLOW_EV also the flow events
    (int64 tensor of n: the inner record's event when the tunnel decoded, else the outer's)."""
    return _parse_tunnel("rpkt_gpu_parse_tunnel_batch", batch, batch.frames.device, flags, outer,
                         tun, inner, flow_ev, n_buckets, stream)


def parse_tunnel_next(batch, tun, inner, flags=3, tun_next=None, inner_next=None, flow_ev=None,
                      n_buckets=0, stream=None):
    """rpkt_gpu_parse_tunnel_next: the next tunnel level of `batch` from the level before
    (`tun`, `inner`: parse_tunnel_batch's on this batch, or an earlier call's of this
    function).  Returns (tun_next, inner_next), uint8 tensors of n * 16 and n * 80 bytes, every
    offset a position in the outermost frame.  With RPKT_F_FLOW_EV, flow_ev (required: the
    level before's events) gets the innermost record's event where the next tunnel decoded
    and keeps its other entries."""
    dev = batch.frames.device
    tun_next = _bytes(batch.n, 16, dev) if tun_next is None else tun_next
    inner_next = alloc_records(batch.n, dev) if inner_next is None else inner_next
    _call("rpkt_gpu_parse_tunnel_next", ctypes.byref(batch.desc()), flags, tun.data_ptr(),
          inner.data_ptr(), tun_next.data_ptr(), inner_next.data_ptr(), _ptr(flow_ev), n_buckets,
          _stream_ptr(stream))
    return tun_next, inner_next


def parse_tunnel_levels(batch, flags=3, depth=2, n_buckets=0, stream=None, buffers=None):
    """`depth` tunnel levels of a batch on one stream: parse_tunnel_batch, then depth - 1
    parse_tunnel_next passes, each on the level before.  Returns (outer, levels), or with
    RPKT_F_FLOW_EV (outer, levels, flow_ev), where levels[k] is level k + 1's (tun, inner)
    and flow_ev holds each frame's innermost decoded flow.  `buffers`: two (tun, inner) tensor
    pairs to ping-pong between when only the last level is wanted (levels then holds the last
    two levels written; earlier ones are overwritten); by default every level gets its own
    tensors."""
    if depth < 1:
        raise RpktError("parse_tunnel_levels: depth %d" % depth)
    if buffers is not None and len(buffers) != 2:
        raise RpktError("parse_tunnel_levels: buffers takes two (tun, inner) pairs")
    t0, i0 = buffers[0] if buffers is not None else (None, None)
    res = parse_tunnel_batch(batch, flags, tun=t0, inner=i0, stream=stream, n_buckets=n_buckets)
    outer, ev = res[0], (res[3] if flags & F_FLOW_EV else None)
    levels = [(res[1], res[2])]
    for k in range(1, depth):
        tn, inn = buffers[k % 2] if buffers is not None else (None, None)
        levels.append(parse_tunnel_next(batch, levels[-1][0], levels[-1][1], flags, tn, inn,
                                        ev, n_buckets, stream))
    if buffers is not None:
        levels = levels[-2:]
    return (outer, levels, ev) if flags & F_FLOW_EV else (outer, levels)


def tunnel_ring_slots(batches, outers, tuns, inners, flow_evs=None):
    """The rpkt_tun_ring_slot_t array of a ring of tunnelled bursts: batch k with its outer
    record, tunnel record and inner record tensors (n * 80, n * 16, n * 80 bytes) and
    (optional) its flow-event tensor.  As ring_slots: build it once, keep the tensors alive
    and in place while it is used."""
    k = len(batches)
    if not (len(outers) == len(tuns) == len(inners) == k) or \
            (flow_evs is not None and len(flow_evs) != k):
        raise RpktError("tunnel_ring_slots: %d batches, %d/%d/%d record tensors"
                        % (k, len(outers), len(tuns), len(inners)))
    arr = (TunRingSlot * k)()
    for j, db in enumerate(batches):
        for t, per, what in ((outers[j], REC_BYTES, "outer"), (tuns[j], 16, "tunnel"),
                             (inners[j], REC_BYTES, "inner")):
            if t.numel() * t.element_size() < db.n * per:
                raise RpktError("tunnel_ring_slots: slot %d %s records too small" % (j, what))
        if flow_evs is not None and flow_evs[j].numel() * flow_evs[j].element_size() < 8 * db.n:
            raise RpktError("tunnel_ring_slots: slot %d flow-event tensor too small" % j)
        arr[j].batch = db.desc()
        arr[j].outer_dev = outers[j].data_ptr()
        arr[j].tun_dev = tuns[j].data_ptr()
        arr[j].inner_dev = inners[j].data_ptr()
        arr[j].flow_ev_dev = flow_evs[j].data_ptr() if flow_evs is not None else None
    return arr


def parse_tunnel_ring(slots, flags=3, n_buckets=0, stream=None):
    """rpkt_gpu_parse_tunnel_ring: every slot of `slots` (tunnel_ring_slots()) parsed as by
    parse_tunnel_batch, RPKT_RING_MAX_SLOTS slots per kernel launch."""
    _call("rpkt_gpu_parse_tunnel_ring", slots, len(slots), flags, n_buckets, _stream_ptr(stream))


def parse_batch_compact(batch, flags=3, recs=None, flow_ev=None, n_buckets=0, stream=None):
    """rpkt_gpu_parse_batch_compact: the same parse writing 16-byte rpkt_rec16_t
    records; returns the uint8 record tensor (n * 16 bytes)."""
    return _parse("rpkt_gpu_parse_batch_compact", batch, batch.frames.device, REC16_BYTES, flags,
                  recs, flow_ev, n_buckets, stream)


def ring_slots(batches, recs, flow_evs=None, compact=None):
    """The rpkt_ring_slot_t array of a receive ring: batch k, its record tensor and
    (optional) its flow-event tensor.  Build it once per ring and pass it to parse_ring
    on every pass: it holds device addresses only, so the batches and tensors must stay
    alive (and in place) as long as the array is used.  Every batch needs its record
    tensor (and flow-event tensor), each large enough for its frames: 80-B records, or
    16-B ones with compact=True (compact=None: either, checked again by parse_ring)."""
    if len(recs) != len(batches) or (flow_evs is not None and len(flow_evs) != len(batches)):
        raise RpktError("ring_slots: %d batches, %d record tensors, %s flow-event tensors"
                        % (len(batches), len(recs), len(flow_evs) if flow_evs is not None
                           else "no"))
    arr = (RingSlot * len(batches))()
    small = []
    for k, (db, r) in enumerate(zip(batches, recs)):
        have = r.numel() * r.element_size()
        if have < db.n * (REC16_BYTES if compact else REC_BYTES):
            if compact is False or have < db.n * REC16_BYTES:
                raise RpktError("ring_slots: slot %d holds %d record bytes for %d frames"
                                % (k, have, db.n))
            small.append(k)
        if flow_evs is not None and flow_evs[k].numel() * flow_evs[k].element_size() < 8 * db.n:
            raise RpktError("ring_slots: slot %d flow-event tensor too small" % k)
        arr[k].batch = db.desc()
        arr[k].recs_dev = r.data_ptr()
        arr[k].flow_ev_dev = flow_evs[k].data_ptr() if flow_evs is not None else None
    # record bytes the slots can hold: 80-B parses refused by parse_ring if any is 16-B sized
    arr._rpkt_compact_only = bool(small)
    return arr


def parse_ring(slots, flags=3, n_buckets=0, stream=None, compact=False):
    """rpkt_gpu_parse_ring[_compact]: every slot of `slots` (ring_slots(), with 80-B or,
    compact, 16-B record tensors) parsed as by parse_batch[_compact],
    RPKT_RING_MAX_SLOTS slots per kernel launch."""
    if not compact and getattr(slots, "_rpkt_compact_only", False):
        raise RpktError("parse_ring: some slot's records are sized for 16-B compact records")
    _call("rpkt_gpu_parse_ring_compact" if compact else "rpkt_gpu_parse_ring", slots, len(slots),
          flags, n_buckets, _stream_ptr(stream))


def flow_workspace(n, n_buckets, device="cuda"):
    torch = _torch()
    nb = int(lib().rpkt_gpu_flow_workspace_bytes(n, n_buckets))
    return torch.empty(max(nb, 16), dtype=torch.uint8, device=device)


def flow_count(flow_ev, n, n_buckets, counters=None, workspace=None, stream=None):
    """rpkt_gpu_flow_count: counters u64[(n_buckets+1)*4] (+= into `counters`)."""
    torch = _torch()
    dev = flow_ev.device
    if counters is None:
        counters = torch.zeros((n_buckets + 1) * 4, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = flow_workspace(n, n_buckets, dev)
    _call("rpkt_gpu_flow_count", flow_ev.data_ptr(), n, n_buckets, counters.data_ptr(),
          workspace.data_ptr(), _stream_ptr(stream))
    return counters


def flow_reduce(counters, n_buckets, comm, root=-1, stream=None):
    """rpkt_gpu_flow_reduce: sum `counters` (u64[(n_buckets+1)*4] as int64) over every
    rank of the RCCL communicator `comm` (an ncclComm_t as int, e.g. from
    nccl_comm_of()), in place; root -1 = all-reduce, else reduce to that rank."""
    if counters.numel() != (n_buckets + 1) * 4:
        raise RpktError("counters must hold (n_buckets + 1) * 4 words")
    _call("rpkt_gpu_flow_reduce", counters.data_ptr(), n_buckets, root, ctypes.c_void_p(int(comm)),
          _stream_ptr(stream))
    return counters


def nccl_comm_of(group=None):
    """The ncclComm_t (as int) of torch.distributed's RCCL process group for the current
    device, or None when the group's backend is not nccl (gloo rehearsals)."""
    torch = _torch()
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    g = group if group is not None else dist.group.WORLD
    if dist.get_backend(g) != "nccl":
        return None
    ptr = int(g._get_backend(torch.device("cuda", torch.cuda.current_device()))._comm_ptr())
    return ptr or None


def coll_unique_id():
    """rpkt_gpu_coll_unique_id: a fresh RCCL unique id (bytes) for rpkt_gpu_comm_init."""
    buf = (ctypes.c_uint8 * COLL_ID_BYTES)()
    _call("rpkt_gpu_coll_unique_id", buf)
    return bytes(buf)


def comm_init(world, uid, rank):
    """rpkt_gpu_comm_init on the current device: the library's own ncclComm_t (as int).
    Collective: returns when all `world` ranks have called it with the same id."""
    if len(uid) != COLL_ID_BYTES:
        raise RpktError("comm_init: the id must be %d bytes" % COLL_ID_BYTES)
    buf = (ctypes.c_uint8 * COLL_ID_BYTES).from_buffer_copy(uid)
    comm = ctypes.c_void_p()
    _call("rpkt_gpu_comm_init", ctypes.byref(comm), world, buf, rank)
    return int(comm.value)


def comm_init_timeout(world, uid, rank, timeout_ms):
    """rpkt_gpu_comm_init_timeout: the same join, aborted after `timeout_ms` when not every
    rank arrives (RpktError; last_coll_error() == 7 on a timeout)."""
    if len(uid) != COLL_ID_BYTES:
        raise RpktError("comm_init: the id must be %d bytes" % COLL_ID_BYTES)
    buf = (ctypes.c_uint8 * COLL_ID_BYTES).from_buffer_copy(uid)
    comm = ctypes.c_void_p()
    _call("rpkt_gpu_comm_init_timeout", ctypes.byref(comm), world, buf, rank, int(timeout_ms))
    return int(comm.value)


def last_coll_error():
    return int(lib().rpkt_gpu_last_coll_error())


def comm_destroy(comm):
    _call("rpkt_gpu_comm_destroy", ctypes.c_void_p(int(comm)))


def comm_abort(comm):
    _call("rpkt_gpu_comm_abort", ctypes.c_void_p(int(comm)))


def checksum_ranges(buf, ranges, out=None, stream=None):
    """rpkt_gpu_checksum_ranges: batched checksum::from_slice over (start, len) pairs."""
    torch = _torch()
    n = ranges.numel() // 2
    if out is None:
        out = torch.empty(n, dtype=torch.int16, device=buf.device)
    _call("rpkt_gpu_checksum_ranges", buf.data_ptr(), buf.numel(), ranges.data_ptr(), n,
          out.data_ptr(), _stream_ptr(stream))
    return out


def checksum_chains(buf, segs, chain_first, out=None, stream=None):
    """rpkt_gpu_checksum_chains: batched checksum::from_buf over segment chains.
    segs: int32 tensor of (start, len) pairs; chain_first: n_chains + 1 indices."""
    torch = _torch()
    n_segs = segs.numel() // 2
    n_chains = chain_first.numel() - 1
    if out is None:
        out = torch.empty(max(n_chains, 0), dtype=torch.int16, device=buf.device)
    ws = _bytes(int(lib().rpkt_gpu_checksum_chains_workspace_bytes(n_segs)), 1, buf.device)
    _call("rpkt_gpu_checksum_chains", buf.data_ptr(), buf.numel(), segs.data_ptr(), n_segs,
          chain_first.data_ptr(), n_chains, out.data_ptr(), ws.data_ptr(), _stream_ptr(stream))
    return out


class DeviceChains:
    """Mbuf chains resident in HBM: the segment arena, (offset, length) u32 pairs and
    the n + 1 chain_first indices (rpkt_chains_t)."""

    def __init__(self, buf, segs, chain_first, n):
        self.buf, self.segs, self.chain_first, self.n = buf, segs, chain_first, n

    @classmethod
    def from_host(cls, hc, device="cuda"):
        torch = _torch()
        host = np.ascontiguousarray(hc.buf)
        if not host.flags.writeable:                 # torch refuses read-only numpy memory
            host = host.copy()
        buf = torch.from_numpy(host).to(device)
        segs = torch.from_numpy(np.ascontiguousarray(hc.segs).view(np.int32).reshape(-1)).to(device)
        first = torch.from_numpy(np.ascontiguousarray(hc.chain_first).view(np.int32)).to(device)
        return cls(buf, segs, first, hc.n)

    @property
    def frames(self):
        return self.buf

    def desc(self):
        return Chains(self.buf.data_ptr(), self.buf.numel(), self.segs.data_ptr(),
                      self.chain_first.data_ptr(), self.segs.numel() // 2, self.n)


def parse_chains(chains, flags=3, recs=None, flow_ev=None, n_buckets=0, stream=None):
    """rpkt_gpu_parse_chains: returns the uint8 record tensor (n * 80 bytes)."""
    return _parse("rpkt_gpu_parse_chains", chains, chains.buf.device, REC_BYTES, flags, recs,
                  flow_ev, n_buckets, stream)


def parse_tunnel_chains(chains, flags=3, outer=None, tun=None, inner=None, stream=None,
                        flow_ev=None, n_buckets=0):
    """rpkt_gpu_parse_tunnel_chains: parse_tunnel_batch over mbuf chains.  Returns (outer
    records, rpkt_tun_t, inner records) as uint8 tensors (n * 80, n * 16, n * 80 bytes);
    with RPKT_F_FLOW_EV also the flow events (int64 tensor of n)."""
    return _parse_tunnel("rpkt_gpu_parse_tunnel_chains", chains, chains.buf.device, flags, outer,
                         tun, inner, flow_ev, n_buckets, stream)


def build_batch(batch, recs, flags=3, built=None, stream=None):
    """rpkt_gpu_build_batch: write each frame's headers from its record, in place in
    batch.frames (payload already there).  Returns the per-frame built flags (u8)."""
    built = _bytes(batch.n, 1, batch.frames.device) if built is None else built
    _call("rpkt_gpu_build_batch", ctypes.byref(batch.desc()), recs.data_ptr(), flags,
          built.data_ptr(), _stream_ptr(stream))
    return built


def build_tunnel_batch(batch, recs, tun, flags=3, built=None, stream=None):
    """rpkt_gpu_build_tunnel_batch: the outer headers of recs plus each frame's tunnel
    header of tun (uint8 tensors of n * 80 / n * 16 bytes); returns the built flags."""
    built = _bytes(batch.n, 1, batch.frames.device) if built is None else built
    _call("rpkt_gpu_build_tunnel_batch", ctypes.byref(batch.desc()), recs.data_ptr(),
          tun.data_ptr(), flags, built.data_ptr(), _stream_ptr(stream))
    return built


def forbid_list(addrs, device="cuda"):
    """Device copy of a forbidden-source list for forward_batch: IPv4 addresses as
    host-order u32 values, sorted ascending (the C ABI's binary search), int32 bits."""
    torch = _torch()
    a = np.unique(np.asarray(addrs, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to(device)


def forward_batch(batch, dmac, smac, forbid=None, keep=None, stream=None, flags=0):
    """rpkt_gpu_forward_batch (loopback_rx firewall: parse, verdict, rewrite in place).
    forbid: None or a tensor from forbid_list(); flags: 0 or RPKT_F_IPV6 (8), which also
    forwards untagged IPv6/UDP frames."""
    torch = _torch()
    keep = _bytes(batch.n, 1, batch.frames.device) if keep is None else keep
    f = Fwd()
    f.dmac[:] = list(bytes(dmac))
    f.smac[:] = list(bytes(smac))
    f.flags = flags
    if forbid is not None and forbid.numel():
        if forbid.dtype != torch.int32:
            raise RpktError("forbid must come from forbid_list() (sorted u32 as int32)")
        f.forbid_dev, f.n_forbid = forbid.data_ptr(), forbid.numel()
    _call("rpkt_gpu_forward_batch", ctypes.byref(batch.desc()), ctypes.byref(f), keep.data_ptr(),
          _stream_ptr(stream))
    return keep


def _workspace(name, n, device):
    """The workspace tensor of a re-framing entry for n inputs (rpkt_gpu_<name>_workspace_bytes)."""
    return _bytes(max(int(getattr(lib(), "rpkt_gpu_%s_workspace_bytes" % name)(n)), 16), 1, device)


def segment_workspace(n, device="cuda"):
    """The workspace tensor of segment_batch for n input frames
    (rpkt_gpu_segment_workspace_bytes)."""
    return _workspace("segment", n, device)


def _reframe_outputs(what, src, recs, cap_bound, bytes_bound, out_frames, out_offsets, out_cap,
                     out_bytes, first, first_name, totals, workspace, ws_name):
    """The output side of the re-framing call `what` on `src`: out_cap and out_bytes from the
    tensors given, else from the documented bounds cap_bound() and bytes_bound(out_cap); the
    tensors not given (`first`: the n + 1 indices); RpktError for ones that do not fit."""
    torch = _torch()
    dev, n = src.frames.device, src.n
    if out_cap is None:
        out_cap = out_offsets.numel() - 1 if out_offsets is not None else cap_bound()
    if out_bytes is None:
        out_bytes = out_frames.numel() if out_frames is not None else bytes_bound(out_cap)
    if out_frames is None:
        out_frames = _bytes(max(out_bytes, 16), 1, dev)
    if out_offsets is None:
        out_offsets = torch.empty(out_cap + 1, dtype=torch.int32, device=dev)
    if out_frames.numel() < out_bytes or out_offsets.numel() < out_cap + 1:
        raise RpktError("%s: outputs smaller than out_bytes / out_cap + 1" % what)
    first = torch.empty(n + 1, dtype=torch.int32, device=dev) if first is None else first
    totals = torch.empty(2, dtype=torch.int64, device=dev) if totals is None else totals
    workspace = _workspace(ws_name, n, dev) if workspace is None else workspace
    if recs.numel() != n * REC_BYTES or first.numel() < n + 1:
        raise RpktError("%s: records or %s do not fit %d frames" % (what, first_name, n))
    return out_frames, out_bytes, out_offsets, out_cap, first, totals, workspace


SEGMENT_UDP = 16


def _segment(name, src, what, recs, mss, out_frames, out_offsets, out_cap, out_bytes, seg_first,
             totals, workspace, stream, header_max, udp):
    """segment_batch and segment_chains: `src` (a DeviceBatch or DeviceChains) cut at `mss`
    into a packed DeviceBatch; the default sizes from the documented bound over src's bytes."""
    n, fbytes = src.n, src.frames.numel()
    out_frames, out_bytes, out_offsets, out_cap, seg_first, totals, workspace = _reframe_outputs(
        what, src, recs, lambda: n + fbytes // mss,
        lambda cap: fbytes + (cap - n) * (134 if header_max is None else header_max),
        out_frames, out_offsets, out_cap, out_bytes, seg_first, "seg_first", totals, workspace,
        "segment")
    _call(name, ctypes.byref(src.desc()), recs.data_ptr(), mss, SEGMENT_UDP if udp else 0,
          out_frames.data_ptr(), out_bytes, out_offsets.data_ptr(), out_cap, seg_first.data_ptr(),
          totals.data_ptr(), workspace.data_ptr(), _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), seg_first, totals


def segment_batch(batch, recs, mss, out_frames=None, out_offsets=None, out_cap=None,
                  out_bytes=None, seg_first=None, totals=None, workspace=None, stream=None,
                  header_max=None, udp=False):
    """rpkt_gpu_segment_batch: TCP segmentation (TSO) of `batch` at `mss`, located by `recs`
    (parse_batch's records of this batch); with udp=True (RPKT_SEGMENT_UDP) UDP datagrams longer
    than `mss` are cut too (UDP GSO).  Returns (out, seg_first, totals): `out` a packed
    DeviceBatch over out_cap slots (slots past totals[0] are empty frames), seg_first an int32
    tensor of n + 1 (the outputs of frame i are [seg_first[i], seg_first[i + 1])), totals an
    int64 tensor {n_out, out_bytes_needed}.  Nothing here reads the device: when totals
    exceeds out_cap / out_bytes the batch overflowed and `out` is unspecified.
    By default the outputs are sized from the documented bound: out_cap = n +
    frames_bytes // mss slots and out_bytes = frames_bytes + (out_cap - n) * header_max bytes,
    header_max (the longest payload_off of the batch) 134 unless given: Ethernet, two tags and
    60-B IPv4 and TCP headers; give it for IPv6 frames with long extension chains."""
    return _segment("rpkt_gpu_segment_batch", batch, "segment_batch", recs, mss, out_frames,
                    out_offsets, out_cap, out_bytes, seg_first, totals, workspace, stream, header_max,
                    udp)


def segment_chains_workspace(n, device="cuda"):
    """The workspace tensor of segment_chains for n chains
    (rpkt_gpu_segment_chains_workspace_bytes)."""
    return _workspace("segment_chains", n, device)


def segment_chains(chains, recs, mss, out_frames=None, out_offsets=None, out_cap=None,
                   out_bytes=None, seg_first=None, totals=None, workspace=None, stream=None,
                   header_max=None, udp=False):
    """rpkt_gpu_segment_chains: segment_batch over mbuf chains (a DeviceChains), read in
    place; `recs` are parse_chains' records of them, `udp` as for segment_batch.  The same
    return value: (out, seg_first, totals), `out` a packed, flat DeviceBatch of wire frames.
    The default sizes are segment_batch's with the arena's size, chains.buf.numel(), for
    frames_bytes: that bounds the chains' bytes only when segments do not overlap and are
    not shared between chains; size the outputs yourself otherwise."""
    if workspace is None:
        workspace = segment_chains_workspace(chains.n, chains.buf.device)
    return _segment("rpkt_gpu_segment_chains", chains, "segment_chains", recs, mss, out_frames,
                    out_offsets, out_cap, out_bytes, seg_first, totals, workspace, stream, header_max,
                    udp)


def segment_tunnel_workspace(n, device="cuda"):
    """The workspace tensor of segment_tunnel_batch for n input frames
    (rpkt_gpu_segment_tunnel_workspace_bytes)."""
    return _workspace("segment_tunnel", n, device)


def _segment_tunnel(name, src, what, outer, tun, inner, mss, out_frames, out_offsets, out_cap,
                    out_bytes, seg_first, totals, workspace, stream, header_max, udp):
    """segment_tunnel_batch and segment_tunnel_chains: _segment with the three tunnel record
    tensors and the tunnel bound."""
    n, fbytes = src.n, src.frames.numel()
    out_frames, out_bytes, out_offsets, out_cap, seg_first, totals, workspace = _reframe_outputs(
        what, src, outer, lambda: n + fbytes // mss,
        lambda cap: fbytes + (cap - n) * (272 if header_max is None else header_max),
        out_frames, out_offsets, out_cap, out_bytes, seg_first, "seg_first", totals, workspace,
        "segment_tunnel")
    if tun.numel() != n * 16 or inner.numel() != n * REC_BYTES:
        raise RpktError("%s: tunnel or inner records do not fit %d frames" % (what, n))
    _call(name, ctypes.byref(src.desc()), outer.data_ptr(), tun.data_ptr(), inner.data_ptr(), mss,
          SEGMENT_UDP if udp else 0, out_frames.data_ptr(), out_bytes, out_offsets.data_ptr(),
          out_cap, seg_first.data_ptr(), totals.data_ptr(), workspace.data_ptr(),
          _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), seg_first, totals


def segment_tunnel_batch(batch, outer, tun, inner, mss, out_frames=None, out_offsets=None,
                         out_cap=None, out_bytes=None, seg_first=None, totals=None, workspace=None,
                         stream=None, header_max=None, udp=False):
    """rpkt_gpu_segment_tunnel_batch: segmentation of the inner TCP (with udp=True,
    RPKT_SEGMENT_UDP, also the inner UDP) of the VXLAN / GTP-U / GRE frames of `batch` at `mss`,
    with the outer lengths and checksums fixed up; `outer`, `tun`, `inner` are
    parse_tunnel_batch's three tensors for this batch.  A frame without a tunnel is cut as
    segment_batch cuts it with its outer record.  The same return value as segment_batch:
    (out, seg_first, totals).  The default sizes are segment_batch's with header_max, the longest
    inner payload_off of the batch, 272 unless given: an outer Ethernet frame with two tags (22),
    a 60-B outer IPv4 header (a plain outer IPv6 header is 40), UDP (8), a 12-B GTP-U header with
    32 bytes of extension headers (VXLAN's 8 and GRE's 4..16 are shorter) and the 134 bytes
    segment_batch allows for the inner frame: 268, rounded up to 16; give it for outer IPv6
    extension headers or longer GTP-U extension chains."""
    return _segment_tunnel("rpkt_gpu_segment_tunnel_batch", batch, "segment_tunnel_batch", outer,
                           tun, inner, mss, out_frames, out_offsets, out_cap, out_bytes, seg_first,
                           totals, workspace, stream, header_max, udp)


def segment_tunnel_chains_workspace(n, device="cuda"):
    """The workspace tensor of segment_tunnel_chains for n chains
    (rpkt_gpu_segment_tunnel_chains_workspace_bytes)."""
    return _workspace("segment_tunnel_chains", n, device)


def segment_tunnel_chains(chains, outer, tun, inner, mss, out_frames=None, out_offsets=None,
                          out_cap=None, out_bytes=None, seg_first=None, totals=None,
                          workspace=None, stream=None, header_max=None, udp=False):
    """rpkt_gpu_segment_tunnel_chains: segment_tunnel_batch over mbuf chains (a DeviceChains),
    read in place; `outer`, `tun`, `inner` are parse_tunnel_chains' three tensors for them, `udp`
    and header_max as for segment_tunnel_batch.  The same return value: (out, seg_first, totals),
    `out` a packed, flat DeviceBatch of wire frames.  The default sizes are
    segment_tunnel_batch's with the arena's size, chains.buf.numel(), for frames_bytes, which
    bounds the chains' bytes under segment_chains' condition: no overlapping or shared segments."""
    if workspace is None:
        workspace = segment_tunnel_chains_workspace(chains.n, chains.buf.device)
    return _segment_tunnel("rpkt_gpu_segment_tunnel_chains", chains, "segment_tunnel_chains", outer,
                           tun, inner, mss, out_frames, out_offsets, out_cap, out_bytes, seg_first,
                           totals, workspace, stream, header_max, udp)


FRAGMENT_IGNORE_DF = 1


def fragment_workspace(n, device="cuda"):
    """The workspace tensor of fragment_batch for n input frames
    (rpkt_gpu_fragment_workspace_bytes)."""
    return _workspace("fragment", n, device)


def fragment_batch(batch, recs, mtu, ignore_df=False, ip6_ident=0, out_frames=None,
                   out_offsets=None, out_cap=None, out_bytes=None, frag_first=None, totals=None,
                   workspace=None, l3_header_max=60, stream=None):
    """rpkt_gpu_fragment_batch: IPv4 / IPv6 fragmentation of `batch` at the L3 MTU `mtu`, located
    by `recs` (parse_batch's records of this batch, with F_IPV6 for IPv6 frames to be cut).
    ignore_df (RPKT_FRAGMENT_IGNORE_DF) also cuts IPv4 packets that have DF set; ip6_ident + i is
    the identification in frame i's IPv6 Fragment headers.  Returns (out, frag_first, totals) as
    segment_batch returns (out, seg_first, totals), under the same overflow rule.
    By default the outputs are sized from the documented bound: out_cap = n + frames_bytes //
    max(8, (mtu - l3_header_max - 8) & ~7) slots, l3_header_max the longest per-fragment L3
    header of the batch (IPv4: ihl; IPv6: 40 and the extension headers up to the last Routing
    header), and out_bytes = frames_bytes + (out_cap - n) * (22 + l3_header_max + 8) bytes:
    Ethernet with two tags, that header and a Fragment header before each further slice."""
    return _fragment("rpkt_gpu_fragment_batch", batch, "fragment_batch", recs, mtu, ignore_df,
                     ip6_ident, out_frames, out_offsets, out_cap, out_bytes, frag_first, totals,
                     workspace, l3_header_max, stream)


def _fragment(name, src, what, recs, mtu, ignore_df, ip6_ident, out_frames, out_offsets, out_cap,
              out_bytes, frag_first, totals, workspace, l3_header_max, stream):
    """fragment_batch and fragment_chains: `src` (a DeviceBatch or DeviceChains) cut at `mtu`
    into a packed DeviceBatch; the default sizes from the documented bound over src's bytes."""
    n, fbytes = src.n, src.frames.numel()
    out_frames, out_bytes, out_offsets, out_cap, frag_first, totals, workspace = _reframe_outputs(
        what, src, recs,
        lambda: n + fbytes // max(8, (mtu - l3_header_max - 8) & ~7),
        lambda cap: fbytes + (cap - n) * (22 + l3_header_max + 8),
        out_frames, out_offsets, out_cap, out_bytes, frag_first, "frag_first", totals, workspace,
        "fragment")
    _call(name, ctypes.byref(src.desc()), recs.data_ptr(), mtu,
          FRAGMENT_IGNORE_DF if ignore_df else 0, ip6_ident & 0xffffffff, out_frames.data_ptr(),
          out_bytes, out_offsets.data_ptr(), out_cap, frag_first.data_ptr(), totals.data_ptr(),
          workspace.data_ptr(), _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), frag_first, totals


def fragment_chains_workspace(n, device="cuda"):
    """The workspace tensor of fragment_chains for n chains
    (rpkt_gpu_fragment_chains_workspace_bytes)."""
    return _workspace("fragment_chains", n, device)


def fragment_chains(chains, recs, mtu, ignore_df=False, ip6_ident=0, out_frames=None,
                    out_offsets=None, out_cap=None, out_bytes=None, frag_first=None, totals=None,
                    workspace=None, l3_header_max=60, stream=None):
    """rpkt_gpu_fragment_chains: fragment_batch over mbuf chains (a DeviceChains), read in place;
    `recs` are parse_chains' records of them (with F_IPV6 for IPv6 chains to be cut), ignore_df
    and ip6_ident as for fragment_batch.  The same return value: (out, frag_first, totals), `out`
    a packed, flat DeviceBatch of wire frames.  The default sizes are fragment_batch's with the
    arena's size, chains.buf.numel(), for frames_bytes: that bounds the chains' bytes only when
    segments do not overlap and are not shared between chains; size the outputs yourself
    otherwise."""
    if workspace is None:
        workspace = fragment_chains_workspace(chains.n, chains.buf.device)
    return _fragment("rpkt_gpu_fragment_chains", chains, "fragment_chains", recs, mtu, ignore_df,
                     ip6_ident, out_frames, out_offsets, out_cap, out_bytes, frag_first, totals,
                     workspace, l3_header_max, stream)


FRAGMENT_TUNNEL_OUTER = 2


def fragment_tunnel_workspace(n, device="cuda"):
    """The workspace tensor of fragment_tunnel_batch for n input frames
    (rpkt_gpu_fragment_tunnel_workspace_bytes)."""
    return _workspace("fragment_tunnel", n, device)


def fragment_tunnel_batch(batch, outer, tun, inner, mtu, ignore_df=False, outer_fallback=False,
                          ip6_ident=0, out_frames=None, out_offsets=None, out_cap=None,
                          out_bytes=None, frag_first=None, totals=None, workspace=None, stream=None,
                          header_max=None):
    """rpkt_gpu_fragment_tunnel_batch: fragmentation of the inner IPv4 packet of the VXLAN /
    GTP-U / GRE frames of `batch` before the encapsulation (RFC 4459 section 3.2), so that every
    output's OUTER IP packet is at most `mtu` bytes and carries outer headers of its own;
    `outer`, `tun`, `inner` are parse_tunnel_batch's three tensors for this batch.  A frame
    without a tunnel is cut as fragment_batch cuts it with its outer record; a tunnelled frame
    whose inner packet is not cut passes through, or with outer_fallback
    (RPKT_FRAGMENT_TUNNEL_OUTER) has its outer packet cut as fragment_batch would.  ignore_df and
    ip6_ident as for fragment_batch.  Returns (out, frag_first, totals) under fragment_batch's
    overflow rule.
    By default the outputs are sized from the documented bound with header_max, the longest
    copied header of the batch (an inner cut's inner l4_off; l4_off or U + 8 otherwise), 272
    unless given (segment_tunnel_batch's allowance): out_cap = n + frames_bytes //
    max(8, (mtu - header_max) & ~7) slots -- header_max also bounds the per-fragment prefix from
    the outer L3 on -- and out_bytes = frames_bytes + (out_cap - n) * header_max bytes."""
    n, fbytes = batch.n, batch.frames.numel()
    hmax = 272 if header_max is None else header_max
    out_frames, out_bytes, out_offsets, out_cap, frag_first, totals, workspace = _reframe_outputs(
        "fragment_tunnel_batch", batch, outer,
        lambda: n + fbytes // max(8, (mtu - hmax) & ~7 if mtu > hmax else 0),
        lambda cap: fbytes + (cap - n) * hmax,
        out_frames, out_offsets, out_cap, out_bytes, frag_first, "frag_first", totals, workspace,
        "fragment_tunnel")
    if tun.numel() != n * 16 or inner.numel() != n * REC_BYTES:
        raise RpktError("fragment_tunnel_batch: tunnel or inner records do not fit %d frames" % n)
    flags = (FRAGMENT_IGNORE_DF if ignore_df else 0) | (FRAGMENT_TUNNEL_OUTER if outer_fallback else 0)
    _call("rpkt_gpu_fragment_tunnel_batch", ctypes.byref(batch.desc()), outer.data_ptr(),
          tun.data_ptr(), inner.data_ptr(), mtu, flags, ip6_ident & 0xffffffff,
          out_frames.data_ptr(), out_bytes, out_offsets.data_ptr(), out_cap, frag_first.data_ptr(),
          totals.data_ptr(), workspace.data_ptr(), _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), frag_first, totals


REASSEMBLE_TRUST_SUMS = 1


def reassemble_workspace(n, device="cuda"):
    """The workspace tensor of reassemble_batch for n positions
    (rpkt_gpu_reassemble_workspace_bytes)."""
    return _workspace("reassemble", n, device)


def reassemble_batch(batch, recs, order=None, trust_sums=False, out_frames=None, out_offsets=None,
                     out_cap=None, out_bytes=None, src_first=None, totals=None, workspace=None,
                     stream=None):
    """rpkt_gpu_reassemble_batch: IPv4 / IPv6 reassembly of the fragments of `batch`, located by
    `recs` (parse_batch's records of this batch, with F_IPV6 for IPv6 fragments and the IP sum
    unless trust_sums), the positions taken in `order` (an int32 tensor of n frame indices, e.g.
    reassemble_order's; None: frame order).  Consecutive positions that hold consecutive
    fragments of one datagram become one frame; every other frame is copied.  Returns (out,
    src_first, totals) as coalesce_batch does, under the same overflow rule and with the same
    default sizes: out_cap = n slots and out_bytes = frames_bytes (give out_bytes when an order
    repeats frames)."""
    n = batch.n
    out_frames, out_bytes, out_offsets, out_cap, src_first, totals, workspace = _reframe_outputs(
        "reassemble_batch", batch, recs, lambda: max(n, 1), lambda cap: batch.frames.numel(),
        out_frames, out_offsets, out_cap, out_bytes, src_first, "src_first", totals, workspace,
        "reassemble")
    if order is not None and (order.numel() < n or order.element_size() != 4):
        raise RpktError("reassemble_batch: order takes %d 32-bit entries" % n)
    _call("rpkt_gpu_reassemble_batch", ctypes.byref(batch.desc()), recs.data_ptr(), _ptr(order),
          REASSEMBLE_TRUST_SUMS if trust_sums else 0, out_frames.data_ptr(), out_bytes,
          out_offsets.data_ptr(), out_cap, src_first.data_ptr(), totals.data_ptr(),
          workspace.data_ptr(), _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), src_first, totals


def reassemble_keys(batch, recs, trust_sums=False, keys=None, stream=None):
    """rpkt_gpu_reassemble_keys: the sort keys of `batch` for reassemble_batch, an int64 tensor of
    n holding the u64 bits: hash(source, destination, identification, protocol) and the fragment
    offset for an eligible fragment, 1 << 63 | i for every other frame."""
    torch = _torch()
    n = batch.n
    if recs.numel() != n * REC_BYTES:
        raise RpktError("reassemble_keys: records do not fit %d frames" % n)
    if keys is None:
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=batch.frames.device)
    if keys.numel() < n or keys.element_size() != 8:
        raise RpktError("reassemble_keys: keys takes %d 64-bit entries" % n)
    _call("rpkt_gpu_reassemble_keys", ctypes.byref(batch.desc()), recs.data_ptr(),
          REASSEMBLE_TRUST_SUMS if trust_sums else 0, keys.data_ptr(), _stream_ptr(stream))
    return keys[:n]


def reassemble_order(keys):
    """The order that brings each datagram's fragments together, ascending in offset, for
    reassemble_batch: the stable argsort of reassemble_keys' keys as UNSIGNED numbers (bit 63 of
    the int64 view is flipped first), the u32 indices in an int32 tensor on keys' device (CPU or
    GPU).  Frames that are no fragments come last, in arrival order."""
    import torch
    return torch.sort(keys ^ (-1 << 63), stable=True)[1].to(torch.int32)


COALESCE_TRUST_SUMS = 1
COALESCE_UDP = 16


def coalesce_workspace(n, device="cuda"):
    """The workspace tensor of coalesce_batch for n positions
    (rpkt_gpu_coalesce_workspace_bytes)."""
    return _workspace("coalesce", n, device)


def coalesce_batch(batch, recs, order=None, max_payload=65535, trust_sums=False, out_frames=None,
                   out_offsets=None, out_cap=None, out_bytes=None, src_first=None, out_mss=None,
                   totals=None, workspace=None, stream=None, udp=False):
    """rpkt_gpu_coalesce_batch: TCP receive coalescing (GRO) of `batch`, with udp=True
    (RPKT_COALESCE_UDP) of UDP datagrams too (UDP GRO), located by `recs`
    (parse_batch's records of this batch, with both sums unless trust_sums), the positions
    taken in `order` (an int32 tensor of n frame indices, e.g. flow_order's; None: frame
    order).  Returns (out, src_first, totals): `out` a packed DeviceBatch over out_cap slots
    (slots past totals[0] are empty frames), src_first an int32 tensor of n + 1 (output j is
    made of positions [src_first[j], src_first[j + 1])), totals an int64 tensor {n_out,
    out_bytes_needed}.  out_mss (optional, an int16 tensor of n) receives each merged output's
    segment size.  Nothing here reads the device: when totals exceeds out_cap / out_bytes the
    batch overflowed and `out` is unspecified.  By default the outputs are sized from the
    documented bound: out_cap = n slots and out_bytes = frames_bytes (without an order; with one
    give out_bytes when it repeats frames)."""
    n = batch.n
    out_frames, out_bytes, out_offsets, out_cap, src_first, totals, workspace = _reframe_outputs(
        "coalesce_batch", batch, recs, lambda: max(n, 1), lambda cap: batch.frames.numel(),
        out_frames, out_offsets, out_cap, out_bytes, src_first, "src_first", totals, workspace,
        "coalesce")
    if order is not None and (order.numel() < n or order.element_size() != 4):
        raise RpktError("coalesce_batch: order takes %d 32-bit entries" % n)
    if out_mss is not None and (out_mss.numel() < n or out_mss.element_size() != 2):
        raise RpktError("coalesce_batch: out_mss takes %d 16-bit entries" % n)
    _call("rpkt_gpu_coalesce_batch", ctypes.byref(batch.desc()), recs.data_ptr(), _ptr(order),
          max_payload, (COALESCE_TRUST_SUMS if trust_sums else 0) | (COALESCE_UDP if udp else 0),
          out_frames.data_ptr(), out_bytes, out_offsets.data_ptr(), out_cap, src_first.data_ptr(),
          _ptr(out_mss), totals.data_ptr(), workspace.data_ptr(), _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), src_first, totals


def coalesce_tunnel_workspace(n, device="cuda"):
    """The workspace tensor of coalesce_tunnel_batch for n positions
    (rpkt_gpu_coalesce_tunnel_workspace_bytes)."""
    return _workspace("coalesce_tunnel", n, device)


def coalesce_tunnel_batch(batch, outer, tun, inner, order=None, max_payload=65535, trust_sums=False,
                          out_frames=None, out_offsets=None, out_cap=None, out_bytes=None,
                          src_first=None, out_mss=None, totals=None, workspace=None, stream=None,
                          udp=False):
    """rpkt_gpu_coalesce_tunnel_batch: receive coalescing (GRO) of the inner TCP (with udp=True,
    RPKT_COALESCE_UDP, also the inner UDP) of the VXLAN / GTP-U / GRE frames of `batch`, with the
    outer lengths and checksums repaired: the inverse of segment_tunnel_batch.  `outer`, `tun`,
    `inner` are parse_tunnel_batch's three tensors for this batch (both sums unless trust_sums).
    A frame without a tunnel is merged as coalesce_batch merges it with its outer record.
    `order`, `max_payload`, `out_mss`, the default sizes and the return value (out, src_first,
    totals) are coalesce_batch's.  The flow events of parse_tunnel_batch(..., RPKT_F_FLOW_EV)
    are keyed by the inner flow where the tunnel decoded, so flow_order on them already
    brings each inner flow's segments together."""
    n = batch.n
    out_frames, out_bytes, out_offsets, out_cap, src_first, totals, workspace = _reframe_outputs(
        "coalesce_tunnel_batch", batch, outer, lambda: max(n, 1), lambda cap: batch.frames.numel(),
        out_frames, out_offsets, out_cap, out_bytes, src_first, "src_first", totals, workspace,
        "coalesce_tunnel")
    if tun.numel() != n * 16 or inner.numel() != n * REC_BYTES:
        raise RpktError("coalesce_tunnel_batch: tunnel or inner records do not fit %d frames" % n)
    if order is not None and (order.numel() < n or order.element_size() != 4):
        raise RpktError("coalesce_tunnel_batch: order takes %d 32-bit entries" % n)
    if out_mss is not None and (out_mss.numel() < n or out_mss.element_size() != 2):
        raise RpktError("coalesce_tunnel_batch: out_mss takes %d 16-bit entries" % n)
    _call("rpkt_gpu_coalesce_tunnel_batch", ctypes.byref(batch.desc()), outer.data_ptr(),
          tun.data_ptr(), inner.data_ptr(), _ptr(order), max_payload,
          (COALESCE_TRUST_SUMS if trust_sums else 0) | (COALESCE_UDP if udp else 0),
          out_frames.data_ptr(), out_bytes, out_offsets.data_ptr(), out_cap, src_first.data_ptr(),
          _ptr(out_mss), totals.data_ptr(), workspace.data_ptr(), _stream_ptr(stream))
    return DeviceBatch(out_frames, out_cap, out_offsets), src_first, totals


def flow_order(flow_ev):
    """The order that brings each flow's frames together for coalesce_batch: the stable
    argsort of the flow events' bucket field (bits 32..47), the u32 indices in an int32 tensor
    (as every index tensor of this module) on flow_ev's device (CPU or GPU).  Frames of one
    flow keep their arrival order; two flows that share a bucket merely stay interleaved and
    merge less."""
    import torch
    bucket = (flow_ev >> 32) & 0xffff
    return torch.sort(bucket, stable=True)[1].to(torch.int32)


def options_batch(batch, recs, opts=None, stream=None, compact=False):
    """rpkt_gpu_options_batch: IPv4 and TCP option walks of a parsed batch
    (recs from parse_batch, or from parse_batch_compact with compact=True:
    rpkt_gpu_options_batch_compact); returns the uint8 tensor of n * 64-byte rpkt_opts_t."""
    _torch()                                   # no GPU: RpktError before the size check
    if recs.numel() != batch.n * (REC16_BYTES if compact else REC_BYTES):
        raise RpktError("records: %d bytes for %d frames" % (recs.numel(), batch.n))
    opts = _bytes(batch.n, OPTS_BYTES, batch.frames.device) if opts is None else opts
    _call("rpkt_gpu_options_batch_compact" if compact else "rpkt_gpu_options_batch",
          ctypes.byref(batch.desc()), recs.data_ptr(), opts.data_ptr(), _stream_ptr(stream))
    return opts


def parse_options_batch(batch, flags=3, recs=None, opts=None, flow_ev=None, n_buckets=0,
                        stream=None, compact=False):
    """rpkt_gpu_parse_options_batch[_compact]: the parse and both option walks in one
    pass.  Returns (records, opts) -- n * 80 (or 16, compact) and n * 64 bytes, uint8 --
    plus the flow events when RPKT_F_FLOW_EV is set."""
    dev = batch.frames.device
    if recs is None:
        recs = _bytes(batch.n, REC16_BYTES if compact else REC_BYTES, dev)
    opts = _bytes(batch.n, OPTS_BYTES, dev) if opts is None else opts
    flow_ev = _events(flags, flow_ev, batch.n, dev)
    _call("rpkt_gpu_parse_options_batch_compact" if compact else "rpkt_gpu_parse_options_batch",
          ctypes.byref(batch.desc()), flags, recs.data_ptr(), opts.data_ptr(), _ptr(flow_ev),
          n_buckets, _stream_ptr(stream))
    return (recs, opts, flow_ev) if flags & F_FLOW_EV else (recs, opts)


def layers_batch(batch, out=None, stream=None):
    """rpkt_gpu_layers_batch: the protocol stack of every frame (pktfmt-derived
    walk); returns the uint8 tensor of n * 64-byte rpkt_layers_t."""
    out = _bytes(batch.n, LAYERS_BYTES, batch.frames.device) if out is None else out
    _call("rpkt_gpu_layers_batch", ctypes.byref(batch.desc()), out.data_ptr(), _stream_ptr(stream))
    return out


def fields_batch(batch, layers, reqs, values=None, present=None, stream=None):
    """rpkt_gpu_fields_batch: header-field getters over the layer walk.  `layers` is
    rpkt_gpu_layers_batch's output on the same batch, `reqs` a FIELD_REQ_DTYPE array
    (rpkt_amd.fields.requests builds one by protocol and field name).  Returns
    (values: int64 tensor n x n_req holding the u64 bits, present: int32 tensor n,
    bit r = request r)."""
    import numpy as np
    from .records import FIELD_REQ_DTYPE
    torch = _torch()
    reqs = np.ascontiguousarray(reqs, dtype=FIELD_REQ_DTYPE)
    k = int(reqs.size)
    dev = batch.frames.device
    if values is None:
        values = torch.empty((batch.n, k), dtype=torch.int64, device=dev)   # u64 bits
    if present is None:
        present = torch.empty(batch.n, dtype=torch.int32, device=dev)
    _call("rpkt_gpu_fields_batch", ctypes.byref(batch.desc()), layers.data_ptr(),
          reqs.ctypes.data_as(ctypes.c_void_p), k, values.data_ptr(), present.data_ptr(),
          _stream_ptr(stream))
    return values, present
