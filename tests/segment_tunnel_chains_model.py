"""A plain model of rpkt_gpu_segment_tunnel_chains (include/rpkt_gpu.h): the chains are
flattened under rpkt_chains_t's documented clamps (tests/segment_chains_model.py) and handed to
tests/segment_tunnel_model.py with the same three record arrays, which is the entry's
definition.  Two sources of records, as for rpkt_gpu_segment_chains."""
import numpy as np

import segment_chains_model as scm
import segment_model as sm
import segment_tunnel_model as stm
import tunnel_chain_model as tcm


def segment(hc, outer, tun, inner, mss, udp=False):
    """(out_frames, seg_first, totals) of rpkt_gpu_segment_tunnel_chains."""
    return stm.segment(scm.flatten(hc), outer, tun, inner, mss, udp)


def chain_records(hc):
    """The chain tunnel parse's (outer, tun, inner): what a caller normally passes.  A header
    that straddles a segment end is a parse error or RPKT_T_BAD there."""
    return tcm.tunnel_chains(hc.buf, hc.segs, hc.chain_first, sm.F6)


def flat_records(hc):
    """The flat tunnel parse's records of the flattened bytes: they say "cut" wherever the
    segment ends fall, so they drive header bytes across arbitrary cuts."""
    return stm.tunnel_records(scm.flatten(hc))


RECORDS = {"chain": chain_records, "flat": flat_records}


def first_segment_lens(hc):
    """Each chain's first non-empty segment's length (0: the chain is empty), unclamped
    descriptors assumed."""
    out = np.zeros(hc.n, dtype=np.int64)
    for p in range(hc.n):
        lens = hc.segs[int(hc.chain_first[p]):int(hc.chain_first[p + 1]), 1]
        lens = lens[lens > 0]
        out[p] = int(lens[0]) if lens.size else 0
    return out


def header_past_first_segment(hc, outer, tun, inner, first):
    """How many of the chains the call cut have their header [0, payload_off) -- the inner
    record's for a tunnelled chain -- reaching past the first non-empty segment: the ones whose
    header bytes are gathered through the segment list."""
    cut = np.diff(first.astype(np.int64)) > 1
    po = np.where(np.asarray(tun["kind"]) != stm.NONE, inner["payload_off"], outer["payload_off"])
    return int((cut & (first_segment_lens(hc) < po.astype(np.int64))).sum())


def single_segment_chains(hb):
    """The HostChains with one segment per frame of the HostBatch hb, over hb's own bytes."""
    from rpkt_amd import gen
    segs = np.stack([hb.offsets[:-1], np.diff(hb.offsets.astype(np.int64)).astype(np.uint32)], axis=1)
    return gen.HostChains(0, hb.n, 0, hb.frames, np.ascontiguousarray(segs, dtype=np.uint32),
                          np.arange(hb.n + 1, dtype=np.uint32), hb.lens().astype(np.uint32))
