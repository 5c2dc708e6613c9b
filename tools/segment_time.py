"""Time rpkt_gpu_segment_batch against a device-to-device copy of the same bytes (GPU box):

    python tools/segment_time.py [--out profiles/segment/times.json]

Workload: 32,768 Ether/IPv4/TCP super-frames of 54 + 32,768 B with random payload, strided,
mss 1448: 23 segments a frame, about 1 GiB in and 1.04 GiB out, past the 256-MB Infinity
Cache.  Two such batches (two seeds) are rotated; the records come from a parse of each.

Timed as bench.py times a leg: warm-up launches for at least 0.3 s, then two HIP events on
the launch stream around LAUNCHES back-to-back calls (default 50), the segmentation and the
copy in interleaved rounds (the first round thrown away; the figure is the median of the
others).  The copy is torch's Tensor.copy_ of the input frames into the output buffer: it
reads and writes frames_bytes each, about the bytes the segmentation moves, and is the
yardstick as DESIGN.md section 6 uses a same-run copy for the headline.  Fractions are of 8 TB/s.

The split of the time between plan + scan and write comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o seg -- python tools/segment_time.py --trace-launches 6

The run also checks the output: 23 segments a frame, and a parse of it with both sums finds
every segment OK with valid IPv4 and TCP sums.

    python tools/segment_time.py --chains [--out profiles/segment_chains/times.json]

times rpkt_gpu_segment_chains too, in the same interleaved rounds: the same super-frames as
mbuf chains (gen.make_chains' mbuf layout: 2048-B data rooms in 2176-B slots with 128 B of
headroom, the slots in a seeded shuffled order; 17 segments a chain, the last one 54 B), the
records from a parse of the chains.  The yardstick there is what a caller without the entry
must do, flatten and then segment: segment_batch on the flat batch plus one device copy of
the bytes (an ideal flatten costs at least that); `chains_over_flatten_then_segment` is
t(segment_chains) / (t(segment_batch) + t(device_copy)).  The chains' output must equal the
flat batch's, byte for byte.

    python tools/segment_time.py --udp [--out profiles/udp_reframe/segment_times.json]

adds the same workload as UDP datagrams (a 42-byte header, 32,768 B of payload, mss 1448) cut
with RPKT_SEGMENT_UDP, in the same interleaved rounds as the TCP leg (flags 0) and the device
copy: `udp_over_tcp_per_byte` and `udp_over_copy_per_byte` are same-run ratios.  Its output is
checked the same way: 23 segments a datagram, every one OK with valid IPv4 and UDP sums.

    python tools/segment_time.py --tunnel [--out profiles/segment/tunnel_times.json]

adds rpkt_gpu_segment_tunnel_batch on the same inner super-frames behind 50 bytes of outer
Ether / IPv4 / UDP / VXLAN (the outer UDP checksum field not 0, so every output's is filled),
located by a tunnel parse, in the same interleaved rounds as the TCP leg on the un-tunnelled
inner frames and the device copy: `tunnel_over_tcp_per_output_byte` (the times over the output
frame bytes), `tunnel_over_tcp_per_byte` and `tunnel_over_copy_per_byte` (over the bytes
moved) are same-run ratios.  Its output is checked by a tunnel parse with both sums: 23
segments a frame, every one decoded with valid outer and inner IPv4, UDP and TCP sums.  With
--trace-launches the traced calls are the tunnel entry's.

    python tools/segment_time.py --tunnel-chains [--out profiles/segment/tunnel_chains/times.json]

adds rpkt_gpu_segment_tunnel_chains on the --tunnel workload's VXLAN super-frames as mbuf chains
in the --chains layout (17 segments a chain, the last one 104 B), the records from
rpkt_gpu_parse_tunnel_chains, in the same interleaved rounds as every leg of --tunnel and
--chains and a device copy of the tunnelled frames' bytes.  The chains' output must equal the
flat tunnel entry's, byte for byte.  `tunnel_chains_over_flatten_then_segment_tunnel` is
t(segment_tunnel_chains) / (t(segment_tunnel_batch) + t(device copy of the same bytes)): what a
caller without the entry must do; `tunnel_chains_over_chains_per_output_byte` is against
rpkt_gpu_segment_chains on the un-tunnelled chains, the chain-side twin of
`tunnel_over_tcp_per_output_byte`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HDR, PAYLOAD, MSS = 54, 32768, 1448
UDP_HDR = 42
HBM_BYTES_PER_S = 8e12


def rfc1071(b):
    s = int(b.reshape(-1, 2).astype(np.uint32).dot(np.array([256, 1], dtype=np.uint32)).sum())
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return (~s) & 0xffff


def super_frames(n, seed):
    """(n, 54 + 32768) uint8: one header (the TCP checksum left 0: segmentation never reads
    it), random payload."""
    hdr = np.zeros(HDR, dtype=np.uint8)
    hdr[0:12] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2)
    hdr[12:14] = (8, 0)
    tot = 40 + PAYLOAD
    hdr[14:24] = (0x45, 0, tot >> 8, tot & 255, 0x12, 0x34, 0x40, 0, 64, 6)
    hdr[26:34] = (10, 0, 0, 1, 10, 0, 0, 2)
    ck = rfc1071(hdr[14:34])
    hdr[24:26] = (ck >> 8, ck & 255)
    hdr[34:38] = (0x13, 0x88, 0x01, 0xbb)
    hdr[38:42] = (0x10, 0x20, 0x30, 0x40)
    hdr[46:48] = (0x50, 0x18)                                     # header_len 20, ACK | PSH
    hdr[48:50] = (0x20, 0x00)
    f = np.frombuffer(np.random.default_rng(seed).bytes(n * (HDR + PAYLOAD)),
                      dtype=np.uint8).reshape(n, HDR + PAYLOAD).copy()
    f[:, :HDR] = hdr
    return f


def udp_super_frames(n, seed):
    """(n, 42 + 32768) uint8: one header (the UDP checksum left 0: segmentation fills it
    whatever it holds), random payload."""
    hdr = super_frames(1, 0)[0, :UDP_HDR].copy()
    tot = 28 + PAYLOAD
    hdr[16:18] = (tot >> 8, tot & 255)
    hdr[23] = 17
    hdr[24:26] = 0
    ck = rfc1071(hdr[14:34])
    hdr[24:26] = (ck >> 8, ck & 255)
    hdr[38:42] = ((8 + PAYLOAD) >> 8, (8 + PAYLOAD) & 255, 0, 0)
    f = np.frombuffer(np.random.default_rng(seed).bytes(n * (UDP_HDR + PAYLOAD)),
                      dtype=np.uint8).reshape(n, UDP_HDR + PAYLOAD).copy()
    f[:, :UDP_HDR] = hdr
    return f


TUN_HDR = 50


def vxlan_prefix():
    """The 50 bytes in front of an inner super-frame: Ether / IPv4 / UDP 4789 / VXLAN (the UDP
    checksum a non-zero placeholder: segmentation fills it whatever it holds)."""
    p = np.zeros(TUN_HDR, dtype=np.uint8)
    p[0:12] = (2, 0, 0, 0, 9, 1, 2, 0, 0, 0, 9, 2)
    p[12:14] = (8, 0)
    tot = 36 + HDR + PAYLOAD
    p[14:24] = (0x45, 0, tot >> 8, tot & 255, 0x43, 0x21, 0x40, 0, 64, 17)
    p[26:34] = (172, 16, 0, 1, 172, 16, 0, 2)
    ck = rfc1071(p[14:34])
    p[24:26] = (ck >> 8, ck & 255)
    ulen = 16 + HDR + PAYLOAD
    p[34:42] = (0xc0, 0x00, 0x12, 0xb5, ulen >> 8, ulen & 255, 0xbe, 0xef)
    p[42:50] = (0x08, 0, 0, 0, 0x12, 0x34, 0x56, 0)
    return p


ROOM, HEADROOM = 2048, 128                                        # gen.MBUF_ROOM, MBUF_HEADROOM


def mbuf_chains(torch, engine, db, n, seed, flen=HDR + PAYLOAD):
    """The `flen`-byte frames of the strided device batch `db` as DeviceChains in the mbuf
    layout, built on the device."""
    per = -(-flen // ROOM)
    rows = torch.zeros((n, per * ROOM), dtype=torch.uint8, device="cuda")
    rows[:, :flen] = db.frames.view(n, flen)
    slot = torch.from_numpy(np.random.default_rng(seed).permutation(n * per)).to("cuda")
    arena = torch.zeros((n * per, ROOM + HEADROOM), dtype=torch.uint8, device="cuda")
    arena[slot, HEADROOM:] = rows.view(n * per, ROOM)
    lens = torch.full((n, per), ROOM, dtype=torch.int64, device="cuda")
    lens[:, per - 1] = flen - (per - 1) * ROOM
    segs = torch.stack([slot * (ROOM + HEADROOM) + HEADROOM, lens.view(-1)], dim=1)
    first = torch.arange(n + 1, dtype=torch.int64, device="cuda") * per
    return engine.DeviceChains(arena.view(-1), segs.to(torch.int32).view(-1).contiguous(),
                               first.to(torch.int32), n)


def time_legs(torch, stream, legs, launches, rounds):
    """Time the functions of `legs` (name -> fn(k)) as the docstring above says: warm-up for at
    least 0.3 s, then rounds + 1 interleaved rounds of `launches` calls between two events, the
    first round thrown away.  Returns (median ms a call, every kept round's ms a call) by name."""
    import time
    k, t_w = 0, time.perf_counter()
    while k < 8 or time.perf_counter() - t_w < 0.3:
        for fn in legs.values():
            fn(k)
        k += 1
        if k % 8 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for r in range(rounds + 1):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for j in range(launches):
                fn(j)
            e1.record(stream)
            torch.cuda.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1) / launches)
    return {name: sorted(v)[len(v) // 2] for name, v in ms.items()}, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chains", action="store_true",
                    help="also time rpkt_gpu_segment_chains on the same frames as mbuf chains")
    ap.add_argument("--udp", action="store_true",
                    help="also time RPKT_SEGMENT_UDP on the same workload as UDP datagrams")
    ap.add_argument("--tunnel", action="store_true",
                    help="also time rpkt_gpu_segment_tunnel_batch on the same frames behind VXLAN")
    ap.add_argument("--tunnel-chains", action="store_true",
                    help="also time rpkt_gpu_segment_tunnel_chains on the VXLAN frames as mbuf "
                         "chains (implies --tunnel and --chains)")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-launches", type=int, default=0,
                    help="no timing: this many calls, for a kernel-trace pass")
    a = ap.parse_args()
    a.tunnel, a.chains = a.tunnel or a.tunnel_chains, a.chains or a.tunnel_chains
    a.out = a.out or ("profiles/segment/tunnel_chains/times.json" if a.tunnel_chains else
                      "profiles/segment/tunnel_times.json" if a.tunnel else
                      "profiles/udp_reframe/segment_times.json" if a.udp else
                      "profiles/segment_chains/times.json" if a.chains else "profiles/segment/times.json")
    import torch
    from rpkt_amd import engine
    from rpkt_amd.records import as_records

    stream = torch.cuda.current_stream()
    n, flen = a.n, HDR + PAYLOAD
    per = -(-PAYLOAD // MSS)
    n_out, need = n * per, n * (per * HDR + PAYLOAD)
    dbs, recs = [], []
    for seed in (31, 3131):
        db = engine.DeviceBatch(torch.from_numpy(super_frames(n, seed).reshape(-1)).to("cuda"), n,
                                stride=flen)
        dbs.append(db)
        recs.append(engine.parse_batch(db, 0))
    R = len(dbs)
    out_frames = torch.empty(need, dtype=torch.uint8, device="cuda")
    out_offsets = torch.empty(n_out + 1, dtype=torch.int32, device="cuda")
    seg_first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = engine.segment_workspace(n)

    def segment(k):
        engine.segment_batch(dbs[k % R], recs[k % R], MSS, out_frames=out_frames,
                             out_offsets=out_offsets, seg_first=seg_first, totals=totals,
                             workspace=ws, stream=stream)

    def copy(k):
        out_frames[:n * flen].copy_(dbs[k % R].frames)

    legs = {"segment_batch": segment, "device_copy": copy}
    if a.chains:
        dcs = [mbuf_chains(torch, engine, db, n, seed) for db, seed in zip(dbs, (17, 1717))]
        crecs = [engine.parse_chains(dc, 0) for dc in dcs]
        assert all(torch.equal(x, y) for x, y in zip(crecs, recs))
        chain_out = torch.empty(need, dtype=torch.uint8, device="cuda")
        chain_offsets, chain_first = torch.empty_like(out_offsets), torch.empty_like(seg_first)
        chain_totals = torch.zeros_like(totals)
        cws = engine.segment_chains_workspace(n)

        def segment_chains(k):
            engine.segment_chains(dcs[k % R], crecs[k % R], MSS, out_frames=chain_out,
                                  out_offsets=chain_offsets, seg_first=chain_first,
                                  totals=chain_totals, workspace=cws, stream=stream)

        legs = {"segment_chains": segment_chains, **legs}
    if a.udp:
        ulen = UDP_HDR + PAYLOAD
        uneed = n * (per * UDP_HDR + PAYLOAD)
        udbs = [engine.DeviceBatch(torch.from_numpy(udp_super_frames(n, seed).reshape(-1)).to("cuda"), n,
                                   stride=ulen) for seed in (47, 4747)]
        urecs = [engine.parse_batch(db, 0) for db in udbs]
        udp_out = torch.empty(uneed, dtype=torch.uint8, device="cuda")
        udp_offsets, udp_first = torch.empty_like(out_offsets), torch.empty_like(seg_first)
        udp_totals = torch.zeros_like(totals)

        def segment_udp(k):
            engine.segment_batch(udbs[k % R], urecs[k % R], MSS, out_frames=udp_out,
                                 out_offsets=udp_offsets, seg_first=udp_first, totals=udp_totals,
                                 workspace=ws, stream=stream, udp=True)

        legs = {"segment_udp": segment_udp, **legs}
    if a.tunnel:
        tlen = TUN_HDR + flen
        tneed = n * (per * (TUN_HDR + HDR) + PAYLOAD)
        prefix = torch.from_numpy(vxlan_prefix()).to("cuda")
        tdbs = [engine.DeviceBatch(torch.cat([prefix.expand(n, TUN_HDR), db.frames.view(n, flen)],
                                             dim=1).reshape(-1).contiguous(), n, stride=tlen)
                for db in dbs]
        trecs = [engine.parse_tunnel_batch(db, 0) for db in tdbs]
        tun_out = torch.empty(tneed, dtype=torch.uint8, device="cuda")
        tun_offsets, tun_first = torch.empty_like(out_offsets), torch.empty_like(seg_first)
        tun_totals = torch.zeros_like(totals)
        tws = engine.segment_tunnel_workspace(n)

        def segment_tunnel(k):
            engine.segment_tunnel_batch(tdbs[k % R], *trecs[k % R], MSS, out_frames=tun_out,
                                        out_offsets=tun_offsets, seg_first=tun_first,
                                        totals=tun_totals, workspace=tws, stream=stream)

        legs = {"segment_tunnel": segment_tunnel, **legs}
    if a.tunnel_chains:
        tdcs = [mbuf_chains(torch, engine, db, n, seed, tlen) for db, seed in zip(tdbs, (19, 1919))]
        tcrecs = [engine.parse_tunnel_chains(dc, 0) for dc in tdcs]
        assert all(torch.equal(x, y) for c, f in zip(tcrecs, trecs) for x, y in zip(c, f))
        tc_out = torch.empty(tneed, dtype=torch.uint8, device="cuda")
        tc_offsets, tc_first = torch.empty_like(out_offsets), torch.empty_like(seg_first)
        tc_totals = torch.zeros_like(totals)
        tcws = engine.segment_tunnel_chains_workspace(n)

        def segment_tunnel_chains(k):
            engine.segment_tunnel_chains(tdcs[k % R], *tcrecs[k % R], MSS, out_frames=tc_out,
                                         out_offsets=tc_offsets, seg_first=tc_first,
                                         totals=tc_totals, workspace=tcws, stream=stream)

        def copy_tunnel(k):
            tun_out[:n * tlen].copy_(tdbs[k % R].frames)

        legs = {"segment_tunnel_chains": segment_tunnel_chains, **legs,
                "device_copy_tunnel": copy_tunnel}
    if a.trace_launches:
        for k in range(a.trace_launches):
            (segment_tunnel_chains if a.tunnel_chains else segment_tunnel if a.tunnel else
             segment_chains if a.chains else segment)(k)
        torch.cuda.synchronize()
        return
    med, ms = time_legs(torch, stream, legs, a.launches, a.rounds)

    # the workload is what it claims (the last call ran on batch (launches - 1) % R)
    segment(0)
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [n_out, need], totals.cpu().tolist()
    first = seg_first.cpu().numpy().view(np.uint32)
    assert np.array_equal(first, np.arange(n + 1, dtype=np.uint32) * per)
    odb = engine.DeviceBatch(out_frames, n_out, out_offsets)
    orec = as_records(engine.parse_batch(odb, 3).cpu().numpy())
    assert (orec["status"] == 0).all() and (orec["ip_sum"] == 0xffff).all()
    assert (orec["l4_sum"] == 0xffff).all()
    last = np.arange(n_out) % per == per - 1
    assert (orec["payload_len"][~last] == MSS).all()
    assert (orec["payload_len"][last] == PAYLOAD - (per - 1) * MSS).all()

    if a.chains:                                                  # the same output from the chains
        segment_chains(0)
        torch.cuda.synchronize()
        assert torch.equal(chain_totals, totals) and torch.equal(chain_first, seg_first)
        assert torch.equal(chain_offsets, out_offsets) and torch.equal(chain_out, out_frames)

    if a.udp:                                                     # the UDP workload is what it claims
        segment_udp(0)
        torch.cuda.synchronize()
        assert udp_totals.cpu().tolist() == [n_out, uneed], udp_totals.cpu().tolist()
        assert torch.equal(udp_first, seg_first)
        urec = as_records(engine.parse_batch(engine.DeviceBatch(udp_out, n_out, udp_offsets), 3).cpu().numpy())
        assert (urec["status"] == 0).all() and (urec["ip_protocol"] == 17).all()
        assert (urec["ip_sum"] == 0xffff).all() and (urec["l4_sum"] == 0xffff).all()
        assert (urec["payload_len"][~last] == MSS).all()
        assert (urec["payload_len"][last] == PAYLOAD - (per - 1) * MSS).all()

    if a.tunnel:                                                  # the tunnel workload is what it claims
        from rpkt_amd.records import as_tunnels
        segment_tunnel(0)
        torch.cuda.synchronize()
        assert tun_totals.cpu().tolist() == [n_out, tneed], tun_totals.cpu().tolist()
        assert torch.equal(tun_first, seg_first)
        to, tt, ti = engine.parse_tunnel_batch(engine.DeviceBatch(tun_out, n_out, tun_offsets), 3)
        to, tt, ti = as_records(to.cpu().numpy()), as_tunnels(tt.cpu().numpy()), as_records(ti.cpu().numpy())
        assert (tt["kind"] == 1).all() and (tt["status"] == 0).all()
        assert (to["status"] == 0).all() and (ti["status"] == 0).all()
        assert (to["ip_sum"] == 0xffff).all() and (to["l4_sum"] == 0xffff).all()
        assert (ti["ip_sum"] == 0xffff).all() and (ti["l4_sum"] == 0xffff).all()
        assert (ti["payload_len"][~last] == MSS).all()
        assert (ti["payload_len"][last] == PAYLOAD - (per - 1) * MSS).all()

    if a.tunnel_chains:                                           # the same output from the chains
        segment_tunnel_chains(0)
        torch.cuda.synchronize()
        assert torch.equal(tc_totals, tun_totals) and torch.equal(tc_first, tun_first)
        assert torch.equal(tc_offsets, tun_offsets) and torch.equal(tc_out, tun_out)

    moved = {"frames_in": n * flen, "records_in": n * 80, "frames_out": need,
             "offsets_out": (n_out + 1) * 4}
    alg = sum(moved.values())
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "frames": n, "frame_len": flen, "mss": MSS, "segments": n_out, "bytes": moved,
           "batches_rotated": R, "launches_per_round": a.launches, "rounds": a.rounds, "ms": {}}
    for name, v in med.items():
        res["ms"][name] = {"ms": round(v, 4), "rounds_ms": [round(x, 4) for x in ms[name]]}
    res["ms"]["segment_batch"]["bytes"] = alg
    res["ms"]["segment_batch"]["fraction_of_8TBs"] = round(
        alg / (med["segment_batch"] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["ms"]["device_copy"]["bytes"] = 2 * n * flen
    res["ms"]["device_copy"]["fraction_of_8TBs"] = round(
        2 * n * flen / (med["device_copy"] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["segment_over_copy_per_byte"] = round(
        (med["segment_batch"] / alg) / (med["device_copy"] / (2 * n * flen)), 4)
    if a.chains:
        n_segs = dcs[0].segs.numel() // 2
        res["chains"] = {"room": ROOM, "slot": ROOM + HEADROOM, "segments": n_segs,
                         "arena_bytes": dcs[0].buf.numel()}
        calg = alg + n_segs * 8 + (n + 1) * 4
        res["ms"]["segment_chains"]["bytes"] = calg
        res["ms"]["segment_chains"]["fraction_of_8TBs"] = round(
            calg / (med["segment_chains"] * 1e-3) / HBM_BYTES_PER_S, 4)
        res["chains_over_flatten_then_segment"] = round(
            med["segment_chains"] / (med["segment_batch"] + med["device_copy"]), 4)
        res["chains_over_segment_batch"] = round(med["segment_chains"] / med["segment_batch"], 4)
    if a.udp:
        ualg = n * ulen + n * 80 + uneed + (n_out + 1) * 4
        res["udp"] = {"frame_len": ulen, "bytes": ualg}
        res["ms"]["segment_udp"]["bytes"] = ualg
        res["ms"]["segment_udp"]["fraction_of_8TBs"] = round(
            ualg / (med["segment_udp"] * 1e-3) / HBM_BYTES_PER_S, 4)
        res["udp_over_tcp_per_byte"] = round((med["segment_udp"] / ualg) / (med["segment_batch"] / alg), 4)
        res["udp_over_copy_per_byte"] = round(
            (med["segment_udp"] / ualg) / (med["device_copy"] / (2 * n * flen)), 4)
    if a.tunnel:
        talg = n * tlen + n * (80 + 16 + 80) + tneed + (n_out + 1) * 4
        res["tunnel"] = {"frame_len": tlen, "bytes": talg, "frames_out": tneed}
        res["ms"]["segment_tunnel"]["bytes"] = talg
        res["ms"]["segment_tunnel"]["fraction_of_8TBs"] = round(
            talg / (med["segment_tunnel"] * 1e-3) / HBM_BYTES_PER_S, 4)
        res["tunnel_over_tcp_per_output_byte"] = round(
            (med["segment_tunnel"] / tneed) / (med["segment_batch"] / need), 4)
        res["tunnel_over_tcp_per_byte"] = round(
            (med["segment_tunnel"] / talg) / (med["segment_batch"] / alg), 4)
        res["tunnel_over_copy_per_byte"] = round(
            (med["segment_tunnel"] / talg) / (med["device_copy"] / (2 * n * flen)), 4)
    if a.tunnel_chains:
        tn_segs = tdcs[0].segs.numel() // 2
        res["tunnel_chains"] = {"room": ROOM, "slot": ROOM + HEADROOM, "segments": tn_segs,
                                "arena_bytes": tdcs[0].buf.numel()}
        tcalg = talg + tn_segs * 8 + (n + 1) * 4
        res["ms"]["segment_tunnel_chains"]["bytes"] = tcalg
        res["ms"]["segment_tunnel_chains"]["fraction_of_8TBs"] = round(
            tcalg / (med["segment_tunnel_chains"] * 1e-3) / HBM_BYTES_PER_S, 4)
        res["ms"]["device_copy_tunnel"]["bytes"] = 2 * n * tlen
        res["ms"]["device_copy_tunnel"]["fraction_of_8TBs"] = round(
            2 * n * tlen / (med["device_copy_tunnel"] * 1e-3) / HBM_BYTES_PER_S, 4)
        res["tunnel_chains_over_flatten_then_segment_tunnel"] = round(
            med["segment_tunnel_chains"] / (med["segment_tunnel"] + med["device_copy_tunnel"]), 4)
        res["tunnel_chains_over_chains_per_output_byte"] = round(
            (med["segment_tunnel_chains"] / tneed) / (med["segment_chains"] / need), 4)
        res["tunnel_chains_over_segment_tunnel"] = round(
            med["segment_tunnel_chains"] / med["segment_tunnel"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
