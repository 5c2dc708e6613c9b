"""Time rpkt_gpu_parse_tunnel_next against the level-1 call on the same frames (GPU box):

    python tools/tunnel_next_time.py [--out profiles/tunnel_next/times.json]

Workload: config 13's 1,048,576 frames of 1500 B (a VXLAN / GTP-U / GRE mix), each behind a
fixed 50-B Ethernet / IPv4 / UDP (checksum 0) / VXLAN header: two tunnel levels, 1550 B per
frame, strided.  Config 13's frames have one length, so one IPv4 header checksum serves
every row.  Config 13's flags (3 | RPKT_F_IPV6).  Two such batches (two generator seeds,
1.6 GB each: every launch reads frames the 256-MB Infinity Cache does not hold) are rotated.

Timed as bench.py times a leg: warm-up launches for at least 0.3 s, then two HIP events on
the launch stream around LAUNCHES back-to-back launches (default 200), the level-1 call
and the next-level pass in interleaved rounds (the first round thrown away; the figure is
the median of the others).

The pass's algorithmic bytes per frame: 96 B of records in (rpkt_tun_t + rpkt_rec_t), 96 B
out, the innermost header window (128 B from the innermost frame's 16-B-aligned start, cut
at the frame end) and the innermost L4 bytes, the bytes the two share counted once.  The
fraction is of 8 TB/s.  HBM bytes per launch of the two kernels come from counter passes of

    rocprofv3 --pmc FETCH_SIZE -T --output-format csv -d DIR -o fetch -- \\
        python tools/tunnel_next_time.py --pmc-launches 6

(and WRITE_SIZE / -o write), read as tools/traffic.py reads them.  The run also checks the records: every second tunnel decodes, and
level 2 of the wrapped frames equals level 1 of the bare config-13 frames moved by 50 B."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUTER = 50                                     # Ether 14 + IPv4 20 + UDP 8 + VXLAN 8
HBM_BYTES_PER_S = 8e12
WIN = 128


def rfc1071(b):
    s = int(b.reshape(-1, 2).astype(np.uint32).dot(np.array([256, 1], dtype=np.uint32)).sum())
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return (~s) & 0xffff


def wrapped(hb):
    """(n, 50 + frame) uint8: hb's equal-length frames behind one VXLAN outer header."""
    n = hb.n
    flen = hb.frame_len or hb.stride
    inner = hb.frames[:n * hb.stride].reshape(n, hb.stride)[:, :flen]
    tot = OUTER + flen
    hdr = np.zeros(OUTER, dtype=np.uint8)
    hdr[0:12] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2)
    hdr[12:14] = (8, 0)
    hdr[14:24] = (0x45, 0, (tot - 14) >> 8, (tot - 14) & 255, 0, 0, 0x40, 0, 64, 17)
    hdr[26:34] = (10, 0, 0, 1, 10, 0, 0, 2)
    ck = rfc1071(hdr[14:34])
    hdr[24:26] = (ck >> 8, ck & 255)
    hdr[34:38] = (0xc0, 0x00, 4789 >> 8, 4789 & 255)
    hdr[38:40] = ((tot - 34) >> 8, (tot - 34) & 255)              # UDP length; checksum 0
    hdr[42] = 0x08                                                # VXLAN: vni_present
    hdr[46:49] = (0x12, 0x34, 0x56)
    f = np.empty((n, tot), dtype=np.uint8)
    f[:, :OUTER] = hdr
    f[:, OUTER:] = inner
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/tunnel_next/times.json")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pmc-launches", type=int, default=0,
                    help="no timing: this many launches of each entry, for a counter pass")
    a = ap.parse_args()
    import time

    import torch
    from rpkt_amd import engine, gen
    from rpkt_amd.records import STATUS, TUN_STATUS, as_records, as_tunnels

    import nested_tunnel_ref as ref            # the offset moves of the tests' reference
    flags = gen.FLAGS[13]
    stream = torch.cuda.current_stream()
    dbs, outs, nxt, bare = [], [], [], None
    for seed in (13, 1313):
        hb = gen.make_batch(13, a.n, seed=seed)
        f = wrapped(hb)
        n, flen = f.shape
        db = engine.DeviceBatch(torch.from_numpy(f.reshape(-1)).to("cuda"), n, stride=flen)
        dbs.append(db)
        outs.append((engine.alloc_records(n), torch.empty(n * 16, dtype=torch.uint8, device="cuda"),
                     engine.alloc_records(n)))
        nxt.append((torch.empty(n * 16, dtype=torch.uint8, device="cuda"), engine.alloc_records(n)))
        if bare is None:                       # level 1 of the bare frames: the expected level 2
            _, bt, bi = engine.parse_tunnel_batch(engine.DeviceBatch.from_host(hb), flags)
            bare = (as_tunnels(bt.cpu().numpy()), as_records(bi.cpu().numpy()))
    R = len(dbs)

    def level1(k):
        engine.parse_tunnel_batch(dbs[k % R], flags, *outs[k % R], stream=stream)

    def level2(k):
        engine.parse_tunnel_next(dbs[k % R], outs[k % R][1], outs[k % R][2], flags, *nxt[k % R],
                                 stream=stream)

    if a.pmc_launches:
        for k in range(a.pmc_launches):
            level1(k)
            level2(k)
        torch.cuda.synchronize()
        return
    legs = {"level1_tunnel_batch": level1, "next_level": level2}
    k, t_w = 0, time.perf_counter()
    while k < 8 or time.perf_counter() - t_w < 0.3:               # clocks up, level 1 written
        level1(k)
        level2(k)
        k += 1
        if k % 8 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for r in range(a.rounds + 1):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for j in range(a.launches):
                fn(j)
            e1.record(stream)
            torch.cuda.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1) / a.launches)
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}

    # the workload is what it claims
    t1 = as_tunnels(outs[0][1].cpu().numpy())
    t2, i2 = as_tunnels(nxt[0][0].cpu().numpy()), as_records(nxt[0][1].cpu().numpy())
    assert (t1["status"] == TUN_STATUS["OK"]).all() and (t1["inner_off"] == OUTER).all()
    assert (t2["status"] == TUN_STATUS["OK"]).all()
    assert t2.tobytes() == ref.rebase_tunnels(bare[0], OUTER).tobytes(), "level-2 tunnels"
    assert i2.tobytes() == ref.rebase_records(bare[1], OUTER).tobytes(), "level-2 inner records"

    # algorithmic bytes: records in and out, the innermost window and L4 range (union)
    n, flen = dbs[0].n, dbs[0].stride
    off = (np.arange(n, dtype=np.int64) * flen + t2["inner_off"]).astype(np.int64)
    ws = off & ~15
    wend = np.minimum(ws + WIN, off + i2["frame_len"])
    ok = i2["status"] == STATUS["OK"]
    l4e = np.where(ok, np.arange(n, dtype=np.int64) * flen + i2["payload_off"].astype(np.int64) +
                   i2["payload_len"], wend)
    frame_bytes = int((np.maximum(l4e, wend) - ws).sum())
    alg = 192 * n + frame_bytes
    res = {"device": engine.device_info(), "build": engine.lib().rpkt_gpu_build_info().decode(),
           "flags": flags, "frames": n, "frame_len": flen, "batches_rotated": R,
           "launches_per_round": a.launches, "rounds": a.rounds,
           "innermost_l4_sum_ok": float((i2["l4_sum"][ok] == 0xffff).mean()),
           "next_level_algorithmic_bytes": alg,
           "next_level_bytes_per_frame": round(alg / n, 1),
           "level1_frame_bytes": n * flen, "ms": {}}
    for name, v in med.items():
        res["ms"][name] = {"ms": round(v, 4), "rounds_ms": [round(x, 4) for x in ms[name]],
                           "mpps": round(n / v / 1e3, 1)}
    res["ms"]["next_level"]["fraction_of_8TBs"] = round(
        alg / (med["next_level"] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["ms"]["level1_tunnel_batch"]["fraction_of_8TBs"] = round(
        (n * flen + 176 * n) / (med["level1_tunnel_batch"] * 1e-3) / HBM_BYTES_PER_S, 4)
    res["next_over_level1"] = round(med["next_level"] / med["level1_tunnel_batch"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
