"""A plain model of rpkt_gpu_fragment_chains (include/rpkt_gpu.h): the chains are flattened
under rpkt_chains_t's documented clamps and handed to tests/fragment_model.py, which is the
entry's definition.  Also the chain batches both fragment-chains tests use: the CPU test
(tests/test_fragment_chains_model.py) checks what each is built to reach, the GPU test
(tests/test_gpu_fragment_chains.py) runs them."""
import functools

import numpy as np

from rpkt_amd import gen

import fragment_model as fm
import segment_model as sm
from segment_chains_model import (chain_bytes, chain_records, chains_of, flat_records,  # noqa: F401
                                  flatten, room_cuts)

IDENT = 0xfffffffe                              # + p wraps at the batch's third chain
RECORDS = {"chain": chain_records, "flat": flat_records}


def fragment_chains(hc, recs, mtu, ignore_df=False, ip6_ident=0):
    """(out_frames, frag_first, totals) of rpkt_gpu_fragment_chains: fragment_model's of the
    flattened batch with the same records."""
    return fm.fragment(flatten(hc), recs, mtu, ignore_df, ip6_ident)


def cut(first):
    """Per chain: it was fragmented."""
    return np.diff(np.asarray(first).astype(np.int64)) > 1


def single_segment_chains(hb):
    """The packed HostBatch hb as chains of one segment each, over the same bytes."""
    segs = np.stack([hb.offsets[:-1], np.diff(hb.offsets.astype(np.int64)).astype(np.uint32)], axis=1)
    return gen.HostChains(0, hb.n, 0, hb.frames, np.ascontiguousarray(segs, dtype=np.uint32),
                          np.arange(hb.n + 1, dtype=np.uint32), hb.lens().astype(np.uint32))


def header_past_first_segment(hc, recs, first):
    """The cut chains whose [0, l4_off) extends past the first non-empty segment: the ones
    the entry reads through the gathered header."""
    n = 0
    for p in np.nonzero(cut(first))[0]:
        lens = hc.segs[int(hc.chain_first[p]):int(hc.chain_first[p + 1]), 1]
        n += int(lens[lens > 0][0]) < int(recs["l4_off"][p])
    return n


# ---- every two-segment cut ---------------------------------------------------------------

CUT_MTUS = (36, 68, 120, 208)


@functools.lru_cache(maxsize=None)
def cut_frames():
    """Eight small frames that between them reach every header rule: plain IPv4, ihl 60 with a
    NOOP mask over all 40 option bytes behind two tags, an input fragment with MF and padding,
    IPv6 with per-fragment headers of 40, 48 and 184 bytes and an extension walk past them."""
    return (fm.udp4(41), fm.udp4(100), fm.udp4(41, options=fm.OPTIONS_40, tags=2),
            fm.icmp4(41, options=fm.OPTIONS_MIX, frag=fm.MF | 0x10, pad=3),
            fm.udp6(41), fm.udp6(41, (fm.HBH,)), fm.tcp6(60, (fm.HBH, fm.AUTH, fm.RT0, fm.DEST)),
            fm.udp6(41, fm.LONG_EXTS, tags=1))


def cut_ranges():
    """[lo, hi) of each of cut_frames()' chains in the every-cut batch."""
    edges = np.cumsum([0] + [len(f) + 1 for f in cut_frames()])
    return list(zip(edges[:-1].tolist(), edges[1:].tolist()))


_every_cut = {}


def every_cut(lead, kind, mtu):
    """All two-segment cuts c in 0..len of cut_frames() as one batch at arena phase `lead`, the
    records of `kind` and the model's output with ignore_df and IDENT (the same for every lead:
    computed once)."""
    frames, cuts = [], []
    for f in cut_frames():
        frames += [f] * (len(f) + 1)
        cuts += [[c] for c in range(len(f) + 1)]
    hc = chains_of(frames, cuts, lead=lead, seed=7)
    if kind not in _every_cut:
        _every_cut[kind] = RECORDS[kind](hc)
    recs = _every_cut[kind]
    if (kind, mtu) not in _every_cut:
        _every_cut[kind, mtu] = fragment_chains(hc, recs, mtu, True, IDENT)
    return hc, recs, _every_cut[kind, mtu]


# ---- three and four segments --------------------------------------------------------------

def multi_cases():
    """(frame, hs, mtu, c) of the three- and four-segment case: udp4(100, OPTIONS_MIX), cut at
    mtu 68 and 76 into slices of c = 32 and 40 bytes after hs = l4_off = 50; udp6(100, (HBH,
    RT0)), hs = U = 86, whose per-fragment headers are 72 bytes: it passes through at 68 and 76
    (segment cuts as for the IPv4 frame) and is cut at 104 into slices of 24."""
    f4, f6 = fm.udp4(100, options=fm.OPTIONS_MIX), fm.udp6(100, (fm.HBH, fm.RT0))
    return [(f4, 50, 68, 32), (f4, 50, 76, 40), (f6, 86, 68, 32), (f6, 86, 76, 40), (f6, 86, 104, 24)]


def multi_cuts(hs, c):
    """tests/test_gpu_segment_chains.py's three- and four-segment cut lists with hs (l4_off;
    IPv6: U) for payload_off and hs + k * c for payload_off + k * mss: an empty first segment,
    an empty middle one, a 1-byte segment inside a slice, cuts exactly at the header's end and
    at slice ends, alone and together."""
    return [[0, 60], [0, 0, hs], [30, 30, 70], [hs, hs, hs + 1], [hs + 6, hs + 7],
            [hs + 7, hs + 8, hs + 9], [hs + c - 1, hs + c, hs + c + 1], [hs], [hs, hs + c],
            [hs + c, hs + 2 * c], [hs, hs + c, hs + 2 * c], [hs + 2 * c, hs + 2 * c + 7, hs + 100],
            [10, hs - 1, hs + 1], [hs - 20, hs - 19, hs - 18]]


# ---- the scan ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scan_block():
    """700 distinct chains of 64..200 B in two or three segments: fragment_model's UDP frames
    over IPv4 / IPv6 and config-6 fuzz frames, interleaved; the records of the flattened
    bytes; the model's output at mtu 68 with ignore_df and ip6_ident 0 (a tile's output then
    does not depend on its place)."""
    fuzz = [f for f in sm.frames_of(gen.make_batch(6, 4096)) if 64 <= len(f) <= 200][:300]
    assert len(fuzz) == 300
    hand = [fm.udp4(30 + k % 117, ident=k, options=fm.OPTIONS_MIX if k % 5 == 0 else b"") if k % 3 else
            fm.udp6(10 + k % 127) for k in range(400)]
    block = [f for pair in zip(hand[:300], fuzz) for f in pair] + hand[300:]
    assert all(64 <= len(f) <= 200 for f in block) and len(set(block)) > 600
    rng = np.random.default_rng(68)
    cuts = [sorted(rng.integers(1, len(f), size=1 + k % 2).tolist()) for k, f in enumerate(block)]
    hc = chains_of(block, cuts, lead=9, seed=68)
    recs = flat_records(hc)
    return hc, recs, fragment_chains(hc, recs, 68, True, 0)


def ident_fields(hc, recs, mtu, ignore_df=True):
    """{output j: offset of its IPv6 Fragment header's identification}, found where the model's
    outputs for ip6_ident 0 and 1 << 16 differ (n < 65536 chains: byte 1 of the field)."""
    a = fragment_chains(hc, recs, mtu, ignore_df, 0)[0]
    b = fragment_chains(hc, recs, mtu, ignore_df, 1 << 16)[0]
    at = {}
    for j, (x, y) in enumerate(zip(a, b)):
        if x != y:
            d = [k for k in range(len(x)) if x[k] != y[k]]
            assert len(d) == 1 and len(x) == len(y)
            at[j] = d[0] - 1
    return at


def tiled(hc1, recs1, want1, reps, mtu=68):
    """hc1's arena, segments, chains and records `reps` times over, and the model's output
    (want1: for ip6_ident 0) tiled the same way, chain p of tile r with the identification
    r * n + p in its Fragment headers."""
    out1, first1, tot1 = want1
    nb, ns = hc1.buf.size, hc1.n_segs
    segs = np.concatenate([hc1.segs + np.array([r * nb, 0], dtype=np.uint32) for r in range(reps)])
    chain_first = np.concatenate([hc1.chain_first[:-1] + np.uint32(r * ns) for r in range(reps)] +
                                 [np.array([reps * ns], dtype=np.uint32)])
    hc = gen.HostChains(0, reps * hc1.n, 0, np.tile(hc1.buf, reps), segs, chain_first,
                        np.tile(hc1.pkt_lens, reps))
    first = np.concatenate([first1[:-1].astype(np.uint64) + r * int(tot1[0]) for r in range(reps)] +
                           [np.array([reps * int(tot1[0])], dtype=np.uint64)]).astype(np.uint32)
    fields = [(j, at, int(np.searchsorted(first1, j, side="right")) - 1)
              for j, at in ident_fields(hc1, recs1, mtu).items()]
    out = []
    for r in range(reps):
        tile = list(out1)
        for j, at, p in fields:
            tile[j] = tile[j][:at] + (r * hc1.n + p).to_bytes(4, "big") + tile[j][at + 4:]
        out += tile
    return hc, np.tile(recs1, reps), (out, first, tot1 * np.uint64(reps))


# ---- descriptors ---------------------------------------------------------------------------

def descriptor_edge_chains():
    """chain_first entries past n_segs and decreasing, segment offsets and lengths past
    buf_bytes, chains sharing segments: four UDP frames that mtu 68 cuts, and the frames."""
    frames = [fm.udp4(60 + 30 * k, ident=k) for k in range(4)]
    hc = chains_of(frames, [[30], [], [10, 60], [54]], lead=2, seed=3)
    fb = hc.buf.size
    segs = hc.segs.copy()
    segs[7] = (segs[7][0], 0xffffffff)                          # a length past the arena
    segs[6] = (fb + 5, 7)                                       # an offset past the arena
    hc.segs = segs
    # chains: [0, 2), none (decreasing), [1, 6) sharing segments with its neighbours, [6, 8)
    # clamped from 1000, none (past n_segs), [2, 3) shared again
    hc.chain_first = np.array([0, 2, 1, 6, 1000, 2, 3], dtype=np.uint32)
    hc.n = 6
    return hc, frames


def no_segments(n=300):
    """n_segs == 0 with n chains: no arena, no segment table."""
    return gen.HostChains(0, n, 0, np.zeros(0, dtype=np.uint8), np.zeros((0, 2), dtype=np.uint32),
                          np.arange(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32))


# ---- the inverse ---------------------------------------------------------------------------

def inverse_frames(mtu=576):
    """The frames of hand_frames(mtu) whose IP packet ends at the frame's end and has neither
    DF nor the reserved bit: the ones reassembly gives back byte for byte."""
    keep = []
    hb = sm.pack(fm.hand_frames(mtu))
    for f, r in zip(fm.hand_frames(mtu), sm.oracle_records(hb)):
        l3 = int(r["l3_off"])
        if len(f) < l3 + 20:
            continue
        if f[l3 - 2:l3] == b"\x08\x00":
            ok = l3 + int.from_bytes(f[l3 + 2:l3 + 4], "big") == len(f) and not f[l3 + 6] & 0xc0
        elif f[l3 - 2:l3] == b"\x86\xdd" and len(f) >= l3 + 40:
            ok = l3 + 40 + int.from_bytes(f[l3 + 4:l3 + 6], "big") == len(f)
        else:
            ok = False
        if ok:
            keep.append(f)
    return keep
