"""Time rpkt_gpu_parse_tunnel_chains on jumbo overlay traffic in mbuf chains (GPU box):

    python tools/tunnel_chains_time.py [--out profiles/tunnel_chains/times.json]

Workload: 262,144 config-7 frames (8000 B), each wrapped on the host in a VXLAN / UDP / IPv4 /
Ethernet outer (50 B; checksums filled by oracle.build_batch), laid out in 2048-B segments
of 2176-B mempool slots (128-B headroom) in shuffled order, as gen.make_chains's "mbuf"
layout: 4 segments per chain.  Flags 3.  Timed with HIP events, median of 20 (the lower of
two interleaved rounds after a discarded one):
  new   rpkt_gpu_parse_tunnel_chains on the chains;
  a     rpkt_gpu_parse_chains on the same chains (one level, the same bytes);
  b     rpkt_gpu_parse_tunnel_batch on the flattened frames.
Algorithmic bytes = the chains' bytes + 176 B of records per chain; the fraction is of
8 TB/s.

    rocprofv3 --pmc FETCH_SIZE -T --output-format csv -d DIR -o fetch -- \\
        python tools/tunnel_chains_time.py --launches 8
    (the same with WRITE_SIZE / -o write), then
    python tools/tunnel_chains_time.py --summarise DIR --out ...

adds the HBM bytes per launch of the new kernel and of parse_chains_kernel (FETCH_SIZE
doubled, as tools/traffic.py reads it) against the algorithmic bytes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUTER = 50                                     # Ether 14 + IPv4 20 + UDP 8 + VXLAN 8
ROOM, SLOT, HEADROOM = 2048, 2176, 128
HBM_BYTES_PER_S = 8e12


def overlay_frames(n, threads=16):
    """(n, 8050) uint8: config 7's frames, each behind a VXLAN outer with valid checksums."""
    from oracle import oracle
    from rpkt_amd import gen
    hb = gen.make_batch(7, n, packed=True)
    inner = hb.frames[:int(hb.offsets[-1])].reshape(n, -1)
    flen = OUTER + inner.shape[1]
    f = np.zeros((n, flen), dtype=np.uint8)
    f[:, OUTER:] = inner
    k = np.arange(n, dtype=np.uint32)
    hdr = np.zeros(OUTER, dtype=np.uint8)
    hdr[0:12] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2)
    hdr[12:14] = (8, 0)
    hdr[14:24] = (0x45, 0, (flen - 14) >> 8, (flen - 14) & 255, 0, 0, 0x40, 0, 64, 17)
    hdr[26:34] = (10, 0, 0, 1, 10, 0, 0, 2)
    hdr[36:38] = (4789 >> 8, 4789 & 255)
    hdr[38:40] = ((flen - 34) >> 8, (flen - 34) & 255)
    hdr[42] = 0x08                                   # VXLAN: vni_present
    f[:, :OUTER] = hdr
    f[:, 28:30] = np.stack([k >> 8, k], 1).astype(np.uint8)        # source address, low half
    f[:, 34:36] = np.stack([(49152 + (k & 0x3fff)) >> 8, k], 1).astype(np.uint8)   # source port
    f[:, 46:49] = np.stack([k >> 16, k >> 8, k], 1).astype(np.uint8)               # vni
    flat = f.reshape(-1)
    recs = oracle.parse_batch(flat, n, 0, stride=flen, threads=threads)
    flat, built = oracle.build_batch(flat, n, recs, 3, stride=flen)
    assert built.all()
    return flat.reshape(n, flen)


def mbuf_chains(f, seed=7):
    """The frames as chains: ROOM-byte segments in shuffled SLOT-byte slots."""
    from rpkt_amd import gen
    n, flen = f.shape
    per = (flen + ROOM - 1) // ROOM
    slot = np.random.default_rng(seed).permutation(n * per).reshape(n, per)
    buf = np.zeros(n * per * SLOT, dtype=np.uint8)
    slots = buf.reshape(n * per, SLOT)
    segs = np.zeros((n, per, 2), dtype=np.uint32)
    for j in range(per):
        ln = min(ROOM, flen - j * ROOM)
        slots[slot[:, j], HEADROOM:HEADROOM + ln] = f[:, j * ROOM:j * ROOM + ln]
        segs[:, j, 0] = slot[:, j].astype(np.uint64) * SLOT + HEADROOM
        segs[:, j, 1] = ln
    first = (np.arange(n + 1, dtype=np.uint64) * per).astype(np.uint32)
    return gen.HostChains(7, n, seed, buf, segs.reshape(-1, 2), first,
                          np.full(n, flen, dtype=np.uint32))


def median_ms(torch, fn, reps=20):
    s = torch.cuda.current_stream()
    ts = []
    for _ in range(3):
        fn()
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def summarise(prof, res):
    """HBM bytes per launch from a FETCH_SIZE and a WRITE_SIZE pass (KiB counters; the read
    side doubled, tools/traffic.py) of --launches runs, per kernel."""
    from traffic import rows
    for kname in ("tunnel_chains_kernel", "parse_chains_kernel"):
        kib = {}
        for name in ("fetch", "write"):
            v = [float(r["Counter_Value"]) for r in rows(os.path.join(prof, name + "_counter_collection.csv"))
                 if r["Kernel_Name"].startswith(kname)][2:]            # warm-up launches skipped
            kib[name] = sum(v) / len(v)
        rd, wr = kib["fetch"] * 2048, kib["write"] * 1024
        res["pmc_" + kname] = {"hbm_read_bytes": rd, "hbm_write_bytes": wr,
                               "read_over_chain_bytes": round(rd / res["chain_bytes"], 4),
                               "traffic_over_algorithmic": round((rd + wr) / res["algorithmic_bytes"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/tunnel_chains/times.json")
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--launches", type=int, default=0,
                    help="no timing: this many launches of the new entry and of parse_chains")
    ap.add_argument("--summarise", default=None, help="add the PMC passes of this directory to --out")
    a = ap.parse_args()
    if a.summarise:
        with open(a.out) as fh:
            res = json.load(fh)
        summarise(a.summarise, res)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({k: v for k, v in res.items() if k.startswith("pmc_")}))
        return
    import torch
    from rpkt_amd import engine
    from rpkt_amd.records import TUN_STATUS, as_records, as_tunnels
    f = overlay_frames(a.n)
    n, flen = f.shape
    hc = mbuf_chains(f)
    dc = engine.DeviceChains.from_host(hc)
    out = (engine.alloc_records(n), torch.empty(n * 16, dtype=torch.uint8, device="cuda"),
           engine.alloc_records(n))
    recs = engine.alloc_records(n)
    if a.launches:
        for _ in range(a.launches):
            engine.parse_tunnel_chains(dc, 3, *out)
            engine.parse_chains(dc, 3, recs)
        torch.cuda.synchronize()
        return
    db = engine.DeviceBatch(torch.from_numpy(f.reshape(-1)).to("cuda"), n, stride=flen)
    fo = (engine.alloc_records(n), torch.empty(n * 16, dtype=torch.uint8, device="cuda"),
          engine.alloc_records(n))
    calls = {"new": lambda: engine.parse_tunnel_chains(dc, 3, *out),
             "a_parse_chains": lambda: engine.parse_chains(dc, 3, recs),
             "b_tunnel_batch_flat": lambda: engine.parse_tunnel_batch(db, 3, *fo)}
    # two interleaved rounds after a round that is thrown away (the entry timed first in a
    # fresh process read 7-9 % slower than in its second round); the figure is the lower median
    rounds = [{k: median_ms(torch, fn) for k, fn in calls.items()} for _ in range(3)][1:]
    ms = {k: min(r[k] for r in rounds) for k in calls}
    # the workload is what it claims: every tunnel decodes, every sum of both levels verifies,
    # and the records are the flat entry's
    o, t, i = (x.cpu().numpy() for x in out)
    t, i = as_tunnels(t), as_records(i)
    assert (t["status"] == TUN_STATUS["OK"]).all() and (as_records(o)["l4_sum"] == 0xffff).all()
    assert all(torch.equal(x, y) for x, y in zip(out, fo)), "chain records differ from the flat entry's"
    chain_bytes = n * flen
    alg = chain_bytes + 176 * n
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "flags": 3, "chains": n, "chain_len": flen, "segments_per_chain": int(hc.n_segs // n),
           "chain_bytes": chain_bytes, "algorithmic_bytes": alg,
           "inner_l4_sum_ok": float((i["l4_sum"] == 0xffff).mean()), "ms": {}}
    for k, v in ms.items():
        res["ms"][k] = {"ms": round(v, 4), "rounds_ms": [round(r[k], 4) for r in rounds],
                        "mpps": round(n / v / 1e3, 1),
                        "fraction_of_8TBs": round(alg / (v * 1e-3) / HBM_BYTES_PER_S, 4)}
    res["new_over_a"] = round(ms["new"] / ms["a_parse_chains"], 4)
    res["new_over_b"] = round(ms["new"] / ms["b_tunnel_batch_flat"], 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
