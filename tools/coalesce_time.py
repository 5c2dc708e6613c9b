"""Time rpkt_gpu_coalesce_batch against a device-to-device copy of the same bytes and against
rpkt_gpu_segment_batch on the forward workload, all in one run (GPU box):

    python tools/coalesce_time.py [--out profiles/coalesce/times.json]

Workload: the inverse of tools/segment_time.py's.  Its 32,768 Ether/IPv4/TCP super-frames of
54 + 32,768 B are cut on the device at mss 1448 by rpkt_gpu_segment_batch into 753,664 segments
(54 + 1448 B, the last of each frame 54 + 912 B), parsed with both sums, and coalesced back into
32,768 frames: about 1.13 GB in and 1.07 GB out, past the 256-MB Infinity Cache.  Two such
batches (two seeds) are rotated.

Timed as tools/segment_time.py times its legs: warm-up launches for at least 0.3 s, then two
HIP events on the launch stream around LAUNCHES back-to-back calls (default 50), the three legs
in interleaved rounds (the first round thrown away; the figure is the median of the others).
The copy is torch's Tensor.copy_ of the coalescing's input frames.  Fractions are of 8 TB/s.

The split of the time between the eight kernels comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o co -- python tools/coalesce_time.py --trace-launches 6

The run also checks the output: 23 segments an output, every output the source super-frame
byte for byte (but its TCP checksum field, which the source leaves 0), and a parse of the
output with both sums finds every frame OK with valid IPv4 and TCP sums.

    python tools/coalesce_time.py --udp [--out profiles/udp_reframe/coalesce_times.json]

adds the same workload as UDP datagrams (tools/segment_time.py --udp's: a 42-byte header,
32,768 B of payload, cut at 1448 with RPKT_SEGMENT_UDP) coalesced with RPKT_COALESCE_UDP, in
the same interleaved rounds as the TCP leg (flags 0) and the device copy:
`udp_over_tcp_per_byte` and `udp_over_copy_per_byte` are same-run ratios.  Every output must
be the source datagram byte for byte but its checksum field, which the source leaves 0.

    python tools/coalesce_time.py --tunnel [--out profiles/coalesce/tunnel/times.json]

adds rpkt_gpu_coalesce_tunnel_batch: tools/segment_time.py --tunnel's workload (the same inner
super-frames behind 50 bytes of outer Ether / IPv4 / UDP / VXLAN, cut at 1448 by
rpkt_gpu_segment_tunnel_batch), located by a tunnel parse with both sums and coalesced back,
in the same interleaved rounds as the flat leg and the device copy:
`tunnel_over_tcp_per_output_byte` (the times over the output frame bytes),
`tunnel_over_tcp_per_byte` and `tunnel_over_copy_per_byte` (over the bytes moved) are same-run
ratios.  Every output must be the source frame byte for byte but the two checksum fields the
source leaves unfilled (the inner TCP's and the outer UDP's).  With --trace-launches the traced
calls are the tunnel entry's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from segment_time import (HBM_BYTES_PER_S, HDR, MSS, PAYLOAD, TUN_HDR, UDP_HDR, super_frames,  # noqa: E402
                          time_legs, udp_super_frames, vxlan_prefix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--udp", action="store_true",
                    help="also time RPKT_COALESCE_UDP on the same workload as UDP datagrams")
    ap.add_argument("--tunnel", action="store_true",
                    help="also time rpkt_gpu_coalesce_tunnel_batch on the same frames behind VXLAN")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="no timing: this many calls, for a kernel-trace or counter pass")
    a = ap.parse_args()
    a.out = a.out or ("profiles/udp_reframe/coalesce_times.json" if a.udp else
                      "profiles/coalesce/tunnel/times.json" if a.tunnel else "profiles/coalesce/times.json")
    import torch
    from rpkt_amd import engine
    from rpkt_amd.records import as_records

    stream = torch.cuda.current_stream()
    n, flen = a.n, HDR + PAYLOAD
    per = -(-PAYLOAD // MSS)
    n_seg, seg_bytes = n * per, n * (per * HDR + PAYLOAD)
    srcs, srecs, segs, recs = [], [], [], []
    for seed in (31, 3131):
        db = engine.DeviceBatch(torch.from_numpy(super_frames(n, seed).reshape(-1)).to("cuda"), n,
                                stride=flen)
        srcs.append(db)
        srecs.append(engine.parse_batch(db, 0))
        sdb, _, tot = engine.segment_batch(db, srecs[-1], MSS, out_cap=n_seg, out_bytes=seg_bytes)
        assert tot.cpu().tolist() == [n_seg, seg_bytes]
        segs.append(sdb)
        recs.append(engine.parse_batch(sdb, 3))
    R = len(segs)
    out_frames = torch.empty(max(n * flen, seg_bytes), dtype=torch.uint8, device="cuda")
    out_offsets = torch.empty(n_seg + 1, dtype=torch.int32, device="cuda")
    first = torch.empty(n_seg + 1, dtype=torch.int32, device="cuda")
    out_mss = torch.empty(n_seg, dtype=torch.int16, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = engine.coalesce_workspace(n_seg)
    sws = engine.segment_workspace(n)

    def coalesce(k):
        engine.coalesce_batch(segs[k % R], recs[k % R], out_frames=out_frames, out_offsets=out_offsets,
                              out_cap=n, out_bytes=n * flen, src_first=first, out_mss=out_mss,
                              totals=totals, workspace=ws, stream=stream)

    def copy(k):
        out_frames[:seg_bytes].copy_(segs[k % R].frames[:seg_bytes])

    def segment(k):
        engine.segment_batch(srcs[k % R], srecs[k % R], MSS, out_frames=out_frames,
                             out_offsets=out_offsets, out_cap=n_seg, out_bytes=seg_bytes,
                             seg_first=first, totals=totals, workspace=sws, stream=stream)

    legs = {"coalesce_batch": coalesce, "device_copy": copy, "segment_batch": segment}
    if a.tunnel:
        tlen, tseg_bytes = TUN_HDR + flen, n * (per * (TUN_HDR + HDR) + PAYLOAD)
        prefix = torch.from_numpy(vxlan_prefix()).to("cuda")
        tsrcs, tsegs, trecs = [], [], []
        for db in srcs:
            tdb = engine.DeviceBatch(torch.cat([prefix.expand(n, TUN_HDR), db.frames.view(n, flen)],
                                               dim=1).reshape(-1).contiguous(), n, stride=tlen)
            tsrcs.append(tdb)
            sdb, _, tot = engine.segment_tunnel_batch(tdb, *engine.parse_tunnel_batch(tdb, 0), MSS,
                                                      out_cap=n_seg, out_bytes=tseg_bytes)
            assert tot.cpu().tolist() == [n_seg, tseg_bytes]
            tsegs.append(sdb)
            trecs.append(engine.parse_tunnel_batch(sdb, 3))
        tun_out = torch.empty(n * tlen, dtype=torch.uint8, device="cuda")
        tun_offsets, tun_first = torch.empty_like(out_offsets), torch.empty_like(first)
        tun_mss, tun_totals = torch.empty_like(out_mss), torch.zeros_like(totals)
        tws = engine.coalesce_tunnel_workspace(n_seg)

        def coalesce_tunnel(k):
            engine.coalesce_tunnel_batch(tsegs[k % R], *trecs[k % R], out_frames=tun_out,
                                         out_offsets=tun_offsets, out_cap=n, out_bytes=n * tlen,
                                         src_first=tun_first, out_mss=tun_mss, totals=tun_totals,
                                         workspace=tws, stream=stream)

        legs = {"coalesce_tunnel": coalesce_tunnel, **legs}
    if a.trace_launches:
        for k in range(a.trace_launches):
            (coalesce_tunnel if a.tunnel else coalesce)(k)
        torch.cuda.synchronize()
        return
    if a.udp:
        ulen, useg_bytes = UDP_HDR + PAYLOAD, n * (per * UDP_HDR + PAYLOAD)
        usrcs, usegs, urecs = [], [], []
        for seed in (47, 4747):
            db = engine.DeviceBatch(torch.from_numpy(udp_super_frames(n, seed).reshape(-1)).to("cuda"), n,
                                    stride=ulen)
            usrcs.append(db)
            sdb, _, tot = engine.segment_batch(db, engine.parse_batch(db, 0), MSS, out_cap=n_seg,
                                               out_bytes=useg_bytes, udp=True)
            assert tot.cpu().tolist() == [n_seg, useg_bytes]
            usegs.append(sdb)
            urecs.append(engine.parse_batch(sdb, 3))
        udp_out = torch.empty(n * ulen, dtype=torch.uint8, device="cuda")
        udp_offsets, udp_first = torch.empty_like(out_offsets), torch.empty_like(first)
        udp_mss, udp_totals = torch.empty_like(out_mss), torch.zeros_like(totals)

        def coalesce_udp(k):
            engine.coalesce_batch(usegs[k % R], urecs[k % R], out_frames=udp_out, out_offsets=udp_offsets,
                                  out_cap=n, out_bytes=n * ulen, src_first=udp_first, out_mss=udp_mss,
                                  totals=udp_totals, workspace=ws, stream=stream, udp=True)

        legs = {"coalesce_udp": coalesce_udp, **legs}
    med, ms = time_legs(torch, stream, legs, a.launches, a.rounds)

    # the output is the source (checked on both batches)
    for k in range(R):
        out_frames.fill_(0xa5)
        coalesce(k)
        torch.cuda.synchronize()
        assert totals.cpu().tolist() == [n, n * flen], totals.cpu().tolist()
        sf = first.cpu().numpy().view(np.uint32)
        assert np.array_equal(sf[:n + 1], np.arange(n + 1, dtype=np.uint32) * per)
        assert (out_mss[:n] == MSS).all().item()
        got = out_frames[:n * flen].view(n, flen)
        src = srcs[k].frames.view(n, flen)
        assert torch.equal(got[:, :50], src[:, :50]) and torch.equal(got[:, 52:], src[:, 52:])
        odb = engine.DeviceBatch(out_frames, n, out_offsets)
        orec = as_records(engine.parse_batch(odb, 3).cpu().numpy())
        assert (orec["status"] == 0).all() and (orec["ip_sum"] == 0xffff).all()
        assert (orec["l4_sum"] == 0xffff).all() and (orec["payload_len"] == PAYLOAD).all()

    for k in range(R if a.udp else 0):                            # the UDP output is its source too
        udp_out.fill_(0xa5)
        coalesce_udp(k)
        torch.cuda.synchronize()
        assert udp_totals.cpu().tolist() == [n, n * ulen], udp_totals.cpu().tolist()
        assert torch.equal(udp_first[:n + 1], first[:n + 1]) and (udp_mss[:n] == MSS).all().item()
        got, src = udp_out.view(n, ulen), usrcs[k].frames.view(n, ulen)
        assert torch.equal(got[:, :40], src[:, :40]) and torch.equal(got[:, 42:], src[:, 42:])
        urec = as_records(engine.parse_batch(engine.DeviceBatch(udp_out, n, udp_offsets), 3).cpu().numpy())
        assert (urec["status"] == 0).all() and (urec["ip_protocol"] == 17).all()
        assert (urec["ip_sum"] == 0xffff).all() and (urec["l4_sum"] == 0xffff).all()
        assert (urec["payload_len"] == PAYLOAD).all()

    for k in range(R if a.tunnel else 0):                         # the tunnel output is its source too
        from rpkt_amd.records import as_tunnels
        tun_out.fill_(0xa5)
        coalesce_tunnel(k)
        torch.cuda.synchronize()
        assert tun_totals.cpu().tolist() == [n, n * tlen], tun_totals.cpu().tolist()
        assert torch.equal(tun_first[:n + 1], first[:n + 1]) and (tun_mss[:n] == MSS).all().item()
        got, src = tun_out.view(n, tlen), tsrcs[k].frames.view(n, tlen)
        uc, tc = 14 + 20 + 6, TUN_HDR + 50                        # the outer UDP and inner TCP checksums
        for lo, hi in ((0, uc), (uc + 2, tc), (tc + 2, tlen)):
            assert torch.equal(got[:, lo:hi], src[:, lo:hi]), (lo, hi)
        to, tt, ti = engine.parse_tunnel_batch(engine.DeviceBatch(tun_out, n, tun_offsets), 3)
        to, tt, ti = as_records(to.cpu().numpy()), as_tunnels(tt.cpu().numpy()), as_records(ti.cpu().numpy())
        assert (to["status"] == 0).all() and (tt["status"] == 0).all() and (ti["status"] == 0).all()
        assert (to["ip_sum"] == 0xffff).all() and (to["l4_sum"] == 0xffff).all()
        assert (ti["ip_sum"] == 0xffff).all() and (ti["l4_sum"] == 0xffff).all()
        assert (ti["payload_len"] == PAYLOAD).all()

    moved = {"frames_in": seg_bytes, "records_in": n_seg * 80, "offsets_in": (n_seg + 1) * 4,
             "frames_out": n * flen, "offsets_out": (n + 1) * 4, "src_first_out": (n_seg + 1) * 4,
             "out_mss_out": n_seg * 2}
    alg = sum(moved.values())
    seg_alg = n * flen + n * 80 + seg_bytes + (n_seg + 1) * 4       # tools/segment_time.py's count
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "segments": n_seg, "frames": n, "frame_len": flen, "mss": MSS, "bytes": moved,
           "batches_rotated": R, "launches_per_round": a.launches, "rounds": a.rounds, "ms": {}}
    for name, v in med.items():
        res["ms"][name] = {"ms": round(v, 4), "rounds_ms": [round(x, 4) for x in ms[name]]}
    for name, b in (("coalesce_batch", alg), ("device_copy", 2 * seg_bytes), ("segment_batch", seg_alg)):
        res["ms"][name]["bytes"] = b
        res["ms"][name]["fraction_of_8TBs"] = round(b / (med[name] * 1e-3) / HBM_BYTES_PER_S, 4)
    if a.udp:
        ualg = alg - seg_bytes - n * flen + useg_bytes + n * ulen
        res["udp"] = {"frame_len": ulen, "bytes": ualg}
        res["ms"]["coalesce_udp"]["bytes"] = ualg
        res["ms"]["coalesce_udp"]["fraction_of_8TBs"] = round(
            ualg / (med["coalesce_udp"] * 1e-3) / HBM_BYTES_PER_S, 4)
    if a.tunnel:
        # two more 80-B records and a 16-B tunnel record a position
        talg = alg - seg_bytes - n * flen + tseg_bytes + n * tlen + n_seg * (80 + 16)
        res["tunnel"] = {"frame_len": tlen, "bytes": talg, "frames_out": n * tlen}
        res["ms"]["coalesce_tunnel"]["bytes"] = talg
        res["ms"]["coalesce_tunnel"]["fraction_of_8TBs"] = round(
            talg / (med["coalesce_tunnel"] * 1e-3) / HBM_BYTES_PER_S, 4)
        res["tunnel_over_tcp_per_output_byte"] = round(
            (med["coalesce_tunnel"] / (n * tlen)) / (med["coalesce_batch"] / (n * flen)), 4)
        res["tunnel_over_tcp_per_byte"] = round(
            (med["coalesce_tunnel"] / talg) / (med["coalesce_batch"] / alg), 4)
        res["tunnel_over_copy_per_byte"] = round(
            (med["coalesce_tunnel"] / talg) / (med["device_copy"] / (2 * seg_bytes)), 4)
    per_byte = {name: med[name] / res["ms"][name]["bytes"] for name in legs}
    if a.udp:
        res["udp_over_tcp_per_byte"] = round(per_byte["coalesce_udp"] / per_byte["coalesce_batch"], 4)
        res["udp_over_copy_per_byte"] = round(per_byte["coalesce_udp"] / per_byte["device_copy"], 4)
    res["coalesce_over_copy_per_byte"] = round(per_byte["coalesce_batch"] / per_byte["device_copy"], 4)
    res["segment_over_copy_per_byte"] = round(per_byte["segment_batch"] / per_byte["device_copy"], 4)
    res["coalesce_over_segment_per_byte"] = round(
        per_byte["coalesce_batch"] / per_byte["segment_batch"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
