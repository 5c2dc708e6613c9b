"""A plain model of rpkt_gpu_segment_chains (include/rpkt_gpu.h): the chains are flattened
under rpkt_chains_t's documented clamps and handed to tests/segment_model.py, which is the
entry's definition.  Also the builder of hand-made chains both segment-chains tests use."""
import numpy as np

from oracle import oracle
from rpkt_amd import gen

import segment_model as sm


def chain_bytes(hc):
    """Chain p's bytes F_p for every p: a = min(chain_first[p], n_segs), b =
    min(max(chain_first[p + 1], a), n_segs), each segment clamped to the arena, empty
    segments contributing nothing."""
    buf = np.ascontiguousarray(hc.buf, dtype=np.uint8)
    fb = int(buf.size)
    segs = np.ascontiguousarray(hc.segs, dtype=np.uint32).reshape(-1, 2).astype(np.int64)
    n_segs = len(segs)
    off = np.minimum(segs[:, 0], fb)
    ln = np.minimum(segs[:, 1], fb - off)
    cf = np.ascontiguousarray(hc.chain_first, dtype=np.uint32).astype(np.int64)
    mem = buf.tobytes()
    out = []
    for p in range(len(cf) - 1):
        a = min(int(cf[p]), n_segs)
        b = min(max(int(cf[p + 1]), a), n_segs)
        out.append(b"".join(mem[int(off[k]):int(off[k] + ln[k])] for k in range(a, b)))
    return out


def flatten(hc):
    """The packed HostBatch F_0 .. F_{n-1} of the chains' bytes."""
    return sm.pack(chain_bytes(hc))


def segment_chains(hc, recs, mss):
    """(out_frames, seg_first, totals) of rpkt_gpu_segment_chains: segment_model's of the
    flattened batch with the same records."""
    return sm.segment(flatten(hc), recs, mss)


def chain_records(hc, flags=sm.F6):
    """oracle.parse_chains' records: what a caller normally passes."""
    return oracle.parse_chains(hc.buf, hc.segs, hc.chain_first, flags)


def flat_records(hc, flags=sm.F6):
    """The flat oracle's records of the flattened bytes: they say "segment this" wherever
    the cuts fall, so they drive header bytes across segment boundaries."""
    return sm.oracle_records(flatten(hc), flags)


def chains_of(frames, cuts, lead=0, seed=1, shuffle=True):
    """HostChains of `frames`, frame p cut at the positions cuts[p] (any order, repeats make
    empty segments, 0 an empty first one).  The segments lie in the arena in a seeded
    shuffled order, `lead` bytes from its start and an odd number of filler bytes apart, so
    every segment starts at its own byte phase; 16 spare bytes end the arena."""
    rng = np.random.default_rng(seed)
    pieces, first = [], [0]
    for f, cs in zip(frames, cuts):
        edges = [0] + sorted(min(int(c), len(f)) for c in cs) + [len(f)]
        pieces += [bytes(f[edges[k]:edges[k + 1]]) for k in range(len(edges) - 1)]
        first.append(len(pieces))
    order = rng.permutation(len(pieces)) if shuffle else np.arange(len(pieces))
    segs = np.zeros((len(pieces), 2), dtype=np.uint32)
    arena = bytearray(b"\xee" * lead)
    for k in order:
        arena += b"\xee" * (1 + 2 * int(rng.integers(0, 7)))
        segs[k] = (len(arena), len(pieces[k]))
        arena += pieces[k]
    buf = np.frombuffer(bytes(arena) + bytes(16), dtype=np.uint8).copy()
    return gen.HostChains(0, len(frames), seed, buf, segs, np.array(first, dtype=np.uint32),
                          np.array([len(f) for f in frames], dtype=np.uint32))


def room_cuts(frame, room):
    """The cuts of an mbuf-style layout: data rooms of `room` bytes."""
    return list(range(room, len(frame), room))
