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
byte for byte, and passes the same checks.

    python tools/fragment_time.py --tunnel [--out profiles/fragment/tunnel_times.json]
times rpkt_gpu_fragment_tunnel_batch: the same datagrams behind segment_time.vxlan_prefix (50
bytes from the outer IP header to the inner one, so the inner packet is cut at mtu' 1450 into
slices of 1424 bytes: 24 tunnel packets a frame where the flat cut at 1480 gives 23), once with
a filled and once with a zero outer UDP checksum, in the same interleaved rounds as
  fragment_outer       rpkt_gpu_fragment_batch with the outer records on the same frames: what a
                       caller does without the entry (23 fragments of the OUTER packet);
  segment_tunnel_udp   rpkt_gpu_segment_tunnel_batch with RPKT_SEGMENT_UDP at mss 1424, the same
                       slice: the same copy, payload sum and outer patches, and an inner L4
                       checksum that fragmentation does not have;
  device_copy          a copy of one batch's bytes.
Recorded for each variant: `tunnel_over_segment_tunnel_udp_per_output_byte`,
`tunnel_over_fragment_outer_per_output_byte` and `tunnel_over_copy_per_byte`.  The same run
checks the output: the outputs a frame, every outer packet within the mtu, and a tunnel parse of
the output with every tunnel decoded and every sum valid."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from segment_time import (HBM_BYTES_PER_S, PAYLOAD, TUN_HDR, UDP_HDR, mbuf_chains, rfc1071,  # noqa: E402
                          time_legs, udp_super_frames, vxlan_prefix)

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


def vxlan_datagrams(n, seed):
    """segment_time.vxlan_prefix around datagrams(): (n, 50 + 42 + 32768) uint8, the outer
    lengths those of this inner frame, the outer DF clear (so that the outer packet can be cut
    too) and the outer UDP checksum the prefix's non-zero placeholder."""
    inner = datagrams(n, seed)
    p = vxlan_prefix()
    tot, ulen = 36 + inner.shape[1], 16 + inner.shape[1]
    p[16:18] = (tot >> 8, tot & 255)
    p[20:22] = 0
    p[24:26] = 0
    ck = rfc1071(p[14:34])
    p[24:26] = (ck >> 8, ck & 255)
    p[38:40] = (ulen >> 8, ulen & 255)
    f = np.empty((n, TUN_HDR + inner.shape[1]), dtype=np.uint8)
    f[:, :TUN_HDR] = p
    f[:, TUN_HDR:] = inner
    return f


def tunnel_main(a):
    """--tunnel: rpkt_gpu_fragment_tunnel_batch on VXLAN-wrapped datagrams, once with a filled
    and once with a zero outer UDP checksum (the module docstring has the legs)."""
    import torch
    from rpkt_amd import engine
    from rpkt_amd.records import as_records, as_tunnels

    stream = torch.cuda.current_stream()
    n, flen = a.n, TUN_HDR + UDP_HDR + PAYLOAD
    over, il4 = TUN_HDR, TUN_HDR + 34                              # outer l3 to inner l3; inner l4_off
    P, c = 8 + PAYLOAD, (MTU - over - 20) & ~7                      # the inner IP payload, the slice
    per = -(-P // c)
    mss = c                                                         # the same slice of UDP payload
    seg_per, seg_hdr = -(-PAYLOAD // mss), TUN_HDR + UDP_HDR
    oP, oc = flen - 34, (MTU - 20) & ~7                             # the outer cut of the same frame
    o_per = -(-oP // oc)
    need, seg_need, o_need = n * (per * il4 + P), n * (seg_per * seg_hdr + PAYLOAD), n * (o_per * 34 + oP)
    dbs = [engine.DeviceBatch(torch.from_numpy(vxlan_datagrams(n, seed).reshape(-1)).to("cuda"), n,
                              stride=flen) for seed in (53, 5353)]
    R = len(dbs)
    cap = n * max(per, seg_per, o_per)
    outs = {k: (torch.empty(b, dtype=torch.uint8, device="cuda"),
                torch.empty(cap + 1, dtype=torch.int32, device="cuda"),
                torch.empty(n + 1, dtype=torch.int32, device="cuda"),
                torch.zeros(2, dtype=torch.int64, device="cuda"))
            for k, b in (("tunnel", need), ("segment", seg_need), ("outer", o_need))}
    ws = {"tunnel": engine.fragment_tunnel_workspace(n), "segment": engine.segment_tunnel_workspace(n),
          "outer": engine.fragment_workspace(n)}
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "frames": n, "frame_len": flen, "mtu": MTU, "mss": mss, "over": over,
           "outputs_a_frame": {"fragment_tunnel": per, "segment_tunnel_udp": seg_per,
                               "fragment_outer": o_per},
           "bytes_out": {"fragment_tunnel": need, "segment_tunnel_udp": seg_need,
                         "fragment_outer": o_need},
           "batches_rotated": R, "launches_per_round": a.launches, "rounds": a.rounds}
    for variant in ("filled", "zero"):
        if variant == "zero":                                       # the outer UDP checksum field
            for db in dbs:
                db.frames.view(n, flen)[:, 40:42] = 0
        recs = [engine.parse_tunnel_batch(db, 0) for db in dbs]

        def call(fn, key, k, *args, **kw):
            f, o, first, tot = outs[key]
            fn(dbs[k % R], *args, out_frames=f, out_offsets=o, out_cap=cap, totals=tot,
               workspace=ws[key], stream=stream, **kw)

        def fragment_tunnel(k):
            call(engine.fragment_tunnel_batch, "tunnel", k, *recs[k % R], MTU, frag_first=outs["tunnel"][2])

        def fragment_outer(k):
            call(engine.fragment_batch, "outer", k, recs[k % R][0], MTU, frag_first=outs["outer"][2])

        def segment_tunnel_udp(k):
            call(engine.segment_tunnel_batch, "segment", k, *recs[k % R], mss, udp=True,
                 seg_first=outs["segment"][2])

        def copy(k):
            outs["tunnel"][0][:n * flen].copy_(dbs[k % R].frames)

        legs = {"fragment_tunnel": fragment_tunnel, "fragment_outer": fragment_outer,
                "segment_tunnel_udp": segment_tunnel_udp, "device_copy": copy}
        med, ms = time_legs(torch, stream, legs, a.launches, a.rounds)

        # the workload is what it claims: the outputs a frame, every outer packet within the
        # mtu, and a tunnel parse of the output with every sum valid
        fragment_tunnel(0), fragment_outer(0), segment_tunnel_udp(0)
        torch.cuda.synchronize()
        assert outs["tunnel"][3].cpu().tolist() == [n * per, need], outs["tunnel"][3].cpu().tolist()
        assert outs["outer"][3].cpu().tolist() == [n * o_per, o_need], outs["outer"][3].cpu().tolist()
        assert outs["segment"][3].cpu().tolist() == [n * seg_per, seg_need], outs["segment"][3].cpu().tolist()
        assert np.array_equal(outs["tunnel"][2].cpu().numpy().view(np.uint32),
                              np.arange(n + 1, dtype=np.uint32) * per)
        odb = engine.DeviceBatch(outs["tunnel"][0], n * per, outs["tunnel"][1][:n * per + 1])
        O, T, I = (view(t.cpu().numpy()) for t, view in
                   zip(engine.parse_tunnel_batch(odb, 3), (as_records, as_tunnels, as_records)))
        k = np.arange(n * per) % per
        assert (T["status"] == 0).all() and (T["kind"] == 1).all()
        assert (O["status"] == 0).all() and (O["ip_sum"] == 0xffff).all()
        assert (O["l4_sum"] == 0xffff).all() if variant == "filled" else True
        assert int(O["ip_packet_len"].max()) <= MTU and int(O["ip_packet_len"].max()) == over + 20 + c
        assert (I["ip_sum"] == 0xffff).all() and (I["ip_protocol"] == 17).all()
        assert np.array_equal(I["ip_frag"], (k * c // 8) | np.where(k < per - 1, 0x2000, 0))
        assert (I["ip_packet_len"][k < per - 1] == 20 + c).all()
        assert (I["ip_packet_len"][k == per - 1] == 20 + P - (per - 1) * c).all()

        alg = n * flen + n * 176 + need + (n * per + 1) * 4
        v = {"ms": {name: {"ms": round(t, 4), "rounds_ms": [round(x, 4) for x in ms[name]]}
                    for name, t in med.items()}}
        v["ms"]["fragment_tunnel"]["bytes"] = alg
        v["ms"]["fragment_tunnel"]["fraction_of_8TBs"] = round(
            alg / (med["fragment_tunnel"] * 1e-3) / HBM_BYTES_PER_S, 4)
        v["tunnel_over_segment_tunnel_udp_per_output_byte"] = round(
            (med["fragment_tunnel"] / need) / (med["segment_tunnel_udp"] / seg_need), 4)
        v["tunnel_over_fragment_outer_per_output_byte"] = round(
            (med["fragment_tunnel"] / need) / (med["fragment_outer"] / o_need), 4)
        v["tunnel_over_copy_per_byte"] = round(
            (med["fragment_tunnel"] / alg) / (med["device_copy"] / (2 * n * flen)), 4)
        res[variant + "_outer_udp_checksum"] = v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chains", action="store_true",
                    help="time rpkt_gpu_fragment_chains on the same datagrams as mbuf chains")
    ap.add_argument("--tunnel", action="store_true",
                    help="time rpkt_gpu_fragment_tunnel_batch on the same datagrams behind VXLAN")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.tunnel:
        a.out = a.out or "profiles/fragment/tunnel_times.json"
        return tunnel_main(a)
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
