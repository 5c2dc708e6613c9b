#!/usr/bin/env python3
"""Time rpkt_gpu_fragment_batch against UDP segmentation and a device copy of the same bytes.

The workload: 32,768 Ether/IPv4/UDP datagrams of 32,768 B payload with DF clear (tools/
segment_time.py's UDP super-frames), fragmented at mtu 1500: 23 fragments a frame, 22 of 1480 B
of IP payload and a last one.  Two yardsticks run in the same interleaved rounds
(segment_time.time_legs: HIP events around `launches` calls, the first round thrown away, two
batches rotated so that no call finds its input in the cache the call before left):
  segment_udp   rpkt_gpu_segment_batch with RPKT_SEGMENT_UDP at mss 1472 on the same frames: the
                same 23 outputs a frame, with a payload sum and an L4 checksum each, which
                fragmentation does not have;
  device_copy   a copy of one batch's bytes.
Recorded: `fragment_over_udp_segment_per_output_byte`, (t / output bytes) of the one over the
other's, and `fragment_over_copy_per_byte`, (t / bytes moved) over the copy's (read + write).
The same run checks the output: 23 fragments a frame, offsets and MF in order, and a parse of
the output that finds every fragment's IPv4 header sum valid.

    python tools/fragment_time.py --chains [--out profiles/fragment/chains_times.json]
times rpkt_gpu_fragment_chains instead: the same datagrams laid out in 2048-byte data rooms
(segment_time.mbuf_chains: 17 segments a chain, each in a slot of its own of a shuffled arena),
the records from rpkt_gpu_parse_chains, in the same interleaved rounds as
  fragment_batch   the same bytes flat;
  device_copy      a copy of one batch's bytes: an ideal flatten costs at least that;
  segment_chains   rpkt_gpu_segment_chains with RPKT_SEGMENT_UDP at mss 1472 on the same chains.
Recorded: `chains_over_flatten_then_fragment`, t(fragment_chains) / (t(device_copy) +
t(fragment_batch)): what a caller without the entry must do; `chains_over_fragment_batch`; and
`chains_over_segment_chains_per_output_byte`.  The chains' output must equal the flat entry's
byte for byte, and passes the same checks."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from segment_time import (HBM_BYTES_PER_S, PAYLOAD, UDP_HDR, mbuf_chains, rfc1071, time_legs,  # noqa: E402
                          udp_super_frames)

MTU, MSS = 1500, 1472


def datagrams(n, seed):
    """udp_super_frames with DF clear and the header sum redone."""
    f = udp_super_frames(n, seed)
    hdr = f[0, :UDP_HDR].copy()
    hdr[20:22] = 0
    hdr[24:26] = 0
    ck = rfc1071(hdr[14:34])
    hdr[24:26] = (ck >> 8, ck & 255)
    f[:, :UDP_HDR] = hdr
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chains", action="store_true",
                    help="time rpkt_gpu_fragment_chains on the same datagrams as mbuf chains")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    a.out = a.out or ("profiles/fragment/chains_times.json" if a.chains else
                      "profiles/fragment/times.json")
    import torch
    from rpkt_amd import engine
    from rpkt_amd.records import as_records

    stream = torch.cuda.current_stream()
    n, flen = a.n, UDP_HDR + PAYLOAD
    P, c = 8 + PAYLOAD, (MTU - 20) & ~7
    per = -(-P // c)
    assert per == 23 and -(-PAYLOAD // MSS) == per
    n_out = n * per
    need, seg_need = n * (per * 34 + P), n * (per * UDP_HDR + PAYLOAD)
    dbs = [engine.DeviceBatch(torch.from_numpy(datagrams(n, seed).reshape(-1)).to("cuda"), n, stride=flen)
           for seed in (53, 5353)]
    recs = [engine.parse_batch(db, 0) for db in dbs]
    R = len(dbs)
    out_frames = torch.empty(need, dtype=torch.uint8, device="cuda")
    seg_out = torch.empty(seg_need, dtype=torch.uint8, device="cuda")
    out_offsets = torch.empty(n_out + 1, dtype=torch.int32, device="cuda")
    seg_offsets = torch.empty_like(out_offsets)
    frag_first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    seg_first = torch.empty_like(frag_first)
    totals, seg_totals = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
    ws, sws = engine.fragment_workspace(n), engine.segment_workspace(n)

    def fragment(k):
        engine.fragment_batch(dbs[k % R], recs[k % R], MTU, out_frames=out_frames,
                              out_offsets=out_offsets, frag_first=frag_first, totals=totals,
                              workspace=ws, stream=stream)

    def segment_udp(k):
        engine.segment_batch(dbs[k % R], recs[k % R], MSS, out_frames=seg_out, out_offsets=seg_offsets,
                             seg_first=seg_first, totals=seg_totals, workspace=sws, stream=stream,
                             udp=True)

    def copy(k):
        out_frames[:n * flen].copy_(dbs[k % R].frames)

    legs = {"fragment_batch": fragment, "segment_udp": segment_udp, "device_copy": copy}
    if a.chains:
        dcs = [mbuf_chains(torch, engine, db, n, seed, flen) for db, seed in zip(dbs, (17, 1717))]
        crecs = [engine.parse_chains(dc, 0) for dc in dcs]
        assert all(torch.equal(x, y) for x, y in zip(crecs, recs))
        chain_out = torch.empty(need, dtype=torch.uint8, device="cuda")
        chain_offsets, chain_first = torch.empty_like(out_offsets), torch.empty_like(frag_first)
        chain_totals = torch.zeros_like(totals)
        cws, scws = engine.fragment_chains_workspace(n), engine.segment_chains_workspace(n)

        def fragment_chains(k):
            engine.fragment_chains(dcs[k % R], crecs[k % R], MTU, out_frames=chain_out,
                                   out_offsets=chain_offsets, frag_first=chain_first,
                                   totals=chain_totals, workspace=cws, stream=stream)

        def segment_chains(k):
            engine.segment_chains(dcs[k % R], crecs[k % R], MSS, out_frames=seg_out,
                                  out_offsets=seg_offsets, seg_first=seg_first, totals=seg_totals,
                                  workspace=scws, stream=stream, udp=True)

        legs = {"fragment_chains": fragment_chains, "fragment_batch": fragment, "device_copy": copy,
                "segment_chains": segment_chains}
    med, ms = time_legs(torch, stream, legs, a.launches, a.rounds)

    # the workload is what it claims
    fragment(0)
    (segment_chains if a.chains else segment_udp)(0)
    torch.cuda.synchronize()
    if a.chains:                       # the chains' output is the flat entry's; checked below
        fragment_chains(0)
        torch.cuda.synchronize()
        assert chain_totals.cpu().tolist() == [n_out, need], chain_totals.cpu().tolist()
        assert torch.equal(chain_first, frag_first) and torch.equal(chain_offsets, out_offsets)
        assert torch.equal(chain_out, out_frames)
        out_frames, out_offsets, frag_first = chain_out, chain_offsets, chain_first
    assert totals.cpu().tolist() == [n_out, need], totals.cpu().tolist()
    assert seg_totals.cpu().tolist() == [n_out, seg_need], seg_totals.cpu().tolist()
    want_first = np.arange(n + 1, dtype=np.uint32) * per
    assert np.array_equal(frag_first.cpu().numpy().view(np.uint32), want_first)
    orec = as_records(engine.parse_batch(engine.DeviceBatch(out_frames, n_out, out_offsets), 3).cpu().numpy())
    k = np.arange(n_out) % per
    assert (orec["ip_sum"] == 0xffff).all() and (orec["ip_protocol"] == 17).all()
    assert np.array_equal(orec["ip_frag"], (k * c // 8) | np.where(k < per - 1, 0x2000, 0))
    assert (orec["ip_packet_len"][k < per - 1] == 20 + c).all()
    assert (orec["ip_packet_len"][k == per - 1] == 20 + P - (per - 1) * c).all()
    srec = as_records(engine.parse_batch(engine.DeviceBatch(seg_out, n_out, seg_offsets), 3).cpu().numpy())
    assert (srec["status"] == 0).all() and (srec["l4_sum"] == 0xffff).all()

    alg = n * flen + n * 80 + need + (n_out + 1) * 4
    salg = n * flen + n * 80 + seg_need + (n_out + 1) * 4
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "frames": n, "frame_len": flen, "mtu": MTU, "mss": MSS, "fragments": n_out,
           "bytes": {"frames_in": n * flen, "records_in": n * 80, "frames_out": need,
                     "offsets_out": (n_out + 1) * 4},
           "batches_rotated": R, "launches_per_round": a.launches, "rounds": a.rounds, "ms": {}}
    for name, v in med.items():
        res["ms"][name] = {"ms": round(v, 4), "rounds_ms": [round(x, 4) for x in ms[name]]}
    n_segs = n * -(-flen // 2048)
    moved = {"fragment_batch": alg, "segment_udp": salg, "device_copy": 2 * n * flen,
             "fragment_chains": alg + n_segs * 8 + (n + 1) * 4,
             "segment_chains": salg + n_segs * 8 + (n + 1) * 4}
    for name in med:
        res["ms"][name]["bytes"] = moved[name]
        res["ms"][name]["fraction_of_8TBs"] = round(moved[name] / (med[name] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["fragment_over_copy_per_byte"] = round(
        (med["fragment_batch"] / alg) / (med["device_copy"] / (2 * n * flen)), 4)
    if a.chains:
        res["segments_per_chain"] = n_segs // n
        res["ms"]["segment_chains"]["frames_out"] = seg_need
        res["chains_over_flatten_then_fragment"] = round(
            med["fragment_chains"] / (med["device_copy"] + med["fragment_batch"]), 4)
        res["chains_over_fragment_batch"] = round(med["fragment_chains"] / med["fragment_batch"], 4)
        res["chains_over_segment_chains_per_output_byte"] = round(
            (med["fragment_chains"] / need) / (med["segment_chains"] / seg_need), 4)
    else:
        res["ms"]["segment_udp"]["frames_out"] = seg_need
        res["fragment_over_udp_segment_per_output_byte"] = round(
            (med["fragment_batch"] / need) / (med["segment_udp"] / seg_need), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
