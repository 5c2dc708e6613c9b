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
the output that finds every fragment's IPv4 header sum valid."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from segment_time import HBM_BYTES_PER_S, PAYLOAD, UDP_HDR, rfc1071, time_legs, udp_super_frames  # noqa: E402

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
    ap.add_argument("--out", default="profiles/fragment/times.json")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
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

    med, ms = time_legs(torch, stream, {"fragment_batch": fragment, "segment_udp": segment_udp,
                                        "device_copy": copy}, a.launches, a.rounds)

    # the workload is what it claims
    fragment(0)
    segment_udp(0)
    torch.cuda.synchronize()
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
    for name, b in (("fragment_batch", alg), ("segment_udp", salg), ("device_copy", 2 * n * flen)):
        res["ms"][name]["bytes"] = b
        res["ms"][name]["fraction_of_8TBs"] = round(b / (med[name] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["ms"]["segment_udp"]["frames_out"] = seg_need
    res["fragment_over_udp_segment_per_output_byte"] = round(
        (med["fragment_batch"] / need) / (med["segment_udp"] / seg_need), 4)
    res["fragment_over_copy_per_byte"] = round(
        (med["fragment_batch"] / alg) / (med["device_copy"] / (2 * n * flen)), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
