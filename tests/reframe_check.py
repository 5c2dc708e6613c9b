"""What the GPU tests of the entries that re-frame a batch share (rpkt_gpu_segment_batch,
rpkt_gpu_segment_chains, rpkt_gpu_coalesce_batch): the outputs on the device, pre-filled with
0xa5 and followed by guard elements, and the comparison of what a call left in them with a
model's (out_frames, first, totals)."""
import numpy as np

from oracle import oracle
from rpkt_amd import engine
from rpkt_amd.records import as_records

import segment_model as sm

GUARD = 256                                    # elements after each output buffer


class Outputs:
    """An entry's outputs on the device, 0xa5-filled, each with GUARD elements after it:
    frames, offsets, the n + 1 index tensor under the entry's name for it (`first`), the
    entry's own `extra` tensors ((name, count, dtype), ...), totals, and its workspace `ws`.
    call(...) is the engine function `fn` with all of them given."""

    def __init__(self, torch, n, out_cap, out_bytes, fn, ws, first, extra=()):
        def filled(count, dtype):
            t = torch.empty(count + GUARD, dtype=dtype, device="cuda")
            t.view(torch.uint8).fill_(0xa5)
            return t
        self.n, self.out_cap, self.out_bytes, self.fn, self.ws = n, out_cap, out_bytes, fn, ws
        self.frames = filled((out_bytes + 15) // 16 * 16, torch.uint8)
        self.offsets = filled(out_cap + 1, torch.int32)
        self.totals = filled(2, torch.int64)
        self.names = (first,) + tuple(name for name, _, _ in extra)
        for name, count, dtype in ((first, n + 1, torch.int32),) + tuple(extra):
            setattr(self, name, filled(count, dtype))

    def call(self, *args, fn=None):
        return (fn or self.fn)(*args, out_frames=self.frames, out_offsets=self.offsets,
                               out_cap=self.out_cap, out_bytes=self.out_bytes, totals=self.totals,
                               workspace=self.ws, **{k: getattr(self, k) for k in self.names})

    def host(self):
        """(frames, offsets, first, the extra tensors ..., totals) as unsigned numpy arrays."""
        def unsigned(t):
            return t.cpu().numpy().view("u%d" % t.element_size())
        return ((unsigned(self.frames), unsigned(self.offsets)) +
                tuple(unsigned(getattr(self, k)) for k in self.names) + (unsigned(self.totals),))


def first_diff(a, b):
    return int(np.nonzero(a != b)[0][0])


def check_outputs(o, odb, out, first, totals, what, parse_back=True, where=None):
    """What a call left in the Outputs `o` (odb: the DeviceBatch it returned) against a model's
    out_frames, first and totals: first and totals exact whatever the capacities, every guard
    intact and, unless the call overflows, the offsets, every output byte, 0xa5 after them and
    the GPU's parse of the GPU's output equal to the oracle's of the model's.  where(j): what
    else to say of output frame j when a byte differs.  False when the call overflowed."""
    n, out_cap, out_bytes, name = o.n, o.out_cap, o.out_bytes, o.names[0]
    n_out, need = int(totals[0]), int(totals[1])
    got = o.host()
    gf, go, gs, gt = got[0], got[1], got[2], got[-1]
    assert np.array_equal(gs[:n + 1], first), "%s: %s at %d" % (what, name, first_diff(gs[:n + 1], first))
    assert list(gt[:2]) == [n_out, need], "%s: totals %s, want %s" % (what, gt[:2], (n_out, need))
    assert (gs[n + 1:] == 0xa5a5a5a5).all() and (gt[2:] == 0xa5a5a5a5a5a5a5a5).all(), what
    assert (gf[out_bytes:] == 0xa5).all(), "%s: bytes past out_bytes written" % what
    assert (go[out_cap + 1:] == 0xa5a5a5a5).all(), "%s: offsets past out_cap written" % what
    if n_out > out_cap or need > out_bytes:
        return False                                                # overflow: the rest is unspecified
    blob, offs = sm.packed_output(out, out_cap)
    assert np.array_equal(go[:out_cap + 1], offs), "%s: out_offsets at %d" % (
        what, first_diff(go[:out_cap + 1], offs))
    if not np.array_equal(gf[:need], blob):
        at = first_diff(gf[:need], blob)
        j = int(np.searchsorted(offs, at, side="right")) - 1
        raise AssertionError("%s: output byte %d differs (output frame %d, its byte %d%s): gpu %#x want %#x"
                             % (what, at, j, at - int(offs[j]), where(j) if where else "", gf[at], blob[at]))
    assert (gf[need:out_bytes] == 0xa5).all(), "%s: bytes past out_bytes_needed written" % what
    if parse_back:
        # the GPU's parse over all out_cap slots of the GPU's output: the oracle's of the model's
        g = as_records(engine.parse_batch(odb, sm.F6).cpu().numpy())
        w = oracle.parse_batch(blob, out_cap, sm.F6, offsets=offs)
        assert g.tobytes() == w.tobytes(), "%s: the parse of the output differs" % what
    return True
