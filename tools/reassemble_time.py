#!/usr/bin/env python3
"""Time rpkt_gpu_reassemble_batch against UDP coalescing and a device copy of the same bytes.

The workload: the 753,664 fragments rpkt_gpu_fragment_batch makes at mtu 1500 of tools/
fragment_time.py's 32,768 Ether/IPv4/UDP datagrams of 32,768 B payload (23 fragments a
datagram, in position order), brought back into 32,768 frames.  Two yardsticks run in the same
interleaved rounds (segment_time.time_legs: HIP events around `launches` calls, the first round
thrown away, two batches of 1.1 GB rotated so that no call finds its input in the Infinity Cache
the call before left):
  coalesce_udp  rpkt_gpu_coalesce_batch with RPKT_COALESCE_UDP on tools/segment_time.py's UDP
                segments (mss 1448, also 23 a datagram): the same number of positions merged into
                the same number of outputs, with a payload sum per position and an L4 checksum per
                output, which reassembly does not have;
  device_copy   a copy of one batch's input bytes.
Recorded: `reassemble_over_udp_coalesce_per_output_byte`, (t / output bytes) of the one over the
other's, and `reassemble_over_copy_per_byte`, (t / bytes moved) over the copy's (read + write).
rpkt_gpu_reassemble_keys is timed alone in the same rounds, and torch's sort of the keys
(engine.reassemble_order) separately: it is not this project's code.
The same run checks the output on both batches: it equals the fragmenter's input byte for byte.
(Every datagram of this workload has the same ident, so they are told apart by position only: the
fragments are taken in the fragmenter's order, and the keys are timed, not used.)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fragment_time import MTU, datagrams  # noqa: E402
from segment_time import HBM_BYTES_PER_S, MSS, PAYLOAD, UDP_HDR, time_legs, udp_super_frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/reassemble/times.json")
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
    nf = n * per
    frag_bytes, seg_bytes = n * (per * 34 + P), n * (per * UDP_HDR + PAYLOAD)

    srcs, frags, frecs, usrcs, usegs, urecs = [], [], [], [], [], []
    for seed in (53, 5353):
        db = engine.DeviceBatch(torch.from_numpy(datagrams(n, seed).reshape(-1)).to("cuda"), n, stride=flen)
        fdb, _, tot = engine.fragment_batch(db, engine.parse_batch(db, 0), MTU, out_cap=nf,
                                            out_bytes=frag_bytes)
        assert tot.cpu().tolist() == [nf, frag_bytes]
        srcs.append(db)
        frags.append(fdb)
        frecs.append(engine.parse_batch(fdb, 1))                      # the header sum only
        db = engine.DeviceBatch(torch.from_numpy(udp_super_frames(n, seed).reshape(-1)).to("cuda"), n,
                                stride=flen)
        sdb, _, tot = engine.segment_batch(db, engine.parse_batch(db, 0), MSS, out_cap=nf,
                                           out_bytes=seg_bytes, udp=True)
        assert tot.cpu().tolist() == [nf, seg_bytes]
        usrcs.append(db)
        usegs.append(sdb)
        urecs.append(engine.parse_batch(sdb, 3))
    R = len(frags)
    out_frames, udp_out = (torch.empty(n * flen, dtype=torch.uint8, device="cuda") for _ in range(2))
    out_offsets, udp_offsets = (torch.empty(n + 1, dtype=torch.int32, device="cuda") for _ in range(2))
    first, udp_first = (torch.empty(nf + 1, dtype=torch.int32, device="cuda") for _ in range(2))
    totals, udp_totals = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
    keys = torch.empty(nf, dtype=torch.int64, device="cuda")
    copy_out = torch.empty(frag_bytes, dtype=torch.uint8, device="cuda")
    ws, cws = engine.reassemble_workspace(nf), engine.coalesce_workspace(nf)

    def reassemble(k):
        engine.reassemble_batch(frags[k % R], frecs[k % R], out_frames=out_frames,
                                out_offsets=out_offsets, out_cap=n, out_bytes=n * flen, src_first=first,
                                totals=totals, workspace=ws, stream=stream)

    def coalesce_udp(k):
        engine.coalesce_batch(usegs[k % R], urecs[k % R], out_frames=udp_out, out_offsets=udp_offsets,
                              out_cap=n, out_bytes=n * flen, src_first=udp_first, totals=udp_totals,
                              workspace=cws, stream=stream, udp=True)

    def reassemble_keys(k):
        engine.reassemble_keys(frags[k % R], frecs[k % R], keys=keys, stream=stream)

    def key_sort(k):
        engine.reassemble_order(keys)

    def copy(k):
        copy_out.copy_(frags[k % R].frames[:frag_bytes])

    reassemble_keys(0)
    med, ms = time_legs(torch, stream, {"reassemble_batch": reassemble, "coalesce_udp": coalesce_udp,
                                        "reassemble_keys": reassemble_keys, "torch_sort_of_keys": key_sort,
                                        "device_copy": copy}, a.launches, a.rounds)

    # the output is the fragmenter's input (checked on both batches); the yardstick's is its source
    want_first = np.full(nf + 1, nf, dtype=np.uint32)
    want_first[:n + 1] = np.arange(n + 1, dtype=np.uint32) * per
    want_first[n] = nf
    for k in range(R):
        out_frames.fill_(0xa5)
        udp_out.fill_(0xa5)
        reassemble(k)
        coalesce_udp(k)
        torch.cuda.synchronize()
        assert totals.cpu().tolist() == [n, n * flen], totals.cpu().tolist()
        assert np.array_equal(first.cpu().numpy().view(np.uint32), want_first)
        assert torch.equal(out_frames, srcs[k].frames[:n * flen])
        orec = as_records(engine.parse_batch(engine.DeviceBatch(out_frames, n, out_offsets), 1).cpu().numpy())
        assert (orec["status"] == 0).all() and (orec["ip_sum"] == 0xffff).all()
        assert (orec["ip_frag"] == 0).all() and (orec["payload_len"] == PAYLOAD).all()
        assert udp_totals.cpu().tolist() == [n, n * flen], udp_totals.cpu().tolist()
        got, src = udp_out.view(n, flen), usrcs[k].frames[:n * flen].view(n, flen)
        assert torch.equal(got[:, :40], src[:, :40]) and torch.equal(got[:, 42:], src[:, 42:])
    alg = frag_bytes + nf * 80 + n * flen + (n + 1) * 4 + (nf + 1) * 4
    calg = seg_bytes + nf * 80 + n * flen + (n + 1) * 4 + (nf + 1) * 4
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "frames_out": n, "frame_len": flen, "mtu": MTU, "mss": MSS, "fragments": nf,
           "bytes": {"fragments_in": frag_bytes, "records_in": nf * 80, "frames_out": n * flen,
                     "offsets_out": (n + 1) * 4, "src_first_out": (nf + 1) * 4},
           "batches_rotated": R, "launches_per_round": a.launches, "rounds": a.rounds, "ms": {}}
    for name, v in med.items():
        res["ms"][name] = {"ms": round(v, 4), "rounds_ms": [round(x, 4) for x in ms[name]]}
    for name, b in (("reassemble_batch", alg), ("coalesce_udp", calg), ("device_copy", 2 * frag_bytes),
                    ("reassemble_keys", nf * 80 + nf * 8 + nf * 64)):
        res["ms"][name]["bytes"] = b
        res["ms"][name]["fraction_of_8TBs"] = round(b / (med[name] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["ms"]["coalesce_udp"]["segments_in"] = seg_bytes
    res["reassemble_over_udp_coalesce_per_output_byte"] = round(
        (med["reassemble_batch"] / (n * flen)) / (med["coalesce_udp"] / (n * flen)), 4)
    res["reassemble_over_copy_per_byte"] = round(
        (med["reassemble_batch"] / alg) / (med["device_copy"] / (2 * frag_bytes)), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
