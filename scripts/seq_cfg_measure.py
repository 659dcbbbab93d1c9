#!/usr/bin/env python3
"""What parameters per sequence cost the tracker (profiles/seq_cfg_measure.json; profiles/README.md "Parameters per sequence").

256 sequences, the benchmark's device-resident VGA frames (bench.make_frames, 24 frames walked forwards and backwards), profiling on: ms_total_gpu of
gf_tracker_stats per frame over 200 frames behind 4 warm-up ones.  Every measurement is a fresh process under a time limit of its own; the driver never opens
the GPU and stops at the first measurement that fails.

  p  the parent commit's library (--parent-lib), configs[1] (150 features, min_dist 30): the spread of its two runs is the yardstick
  n  this library, the same handle, no setter called (no table is allocated, the kernels get null pointers)
  m  this library, ONE handle of 500 / 12 whose sequences are split over 150 / 30 (b % 3 == 0: 86 sequences), 300 / 20 (b % 3 == 1: 85) and the handle's own
     500 / 12 (85)
  x, y, z  this library, three homogeneous handles of those sizes -- 86 sequences at 150 / 30, 85 at 300 / 20, 85 at 500 / 12 -- on the frames the same
     sequences see in (m): their sum is what a farm pays today for the fleet of (m)

run in the order p n p n [p n ...] m x y z (--pairs, 2 by default).  The bar for (n): the parent's own figure plus the larger of 1 % and the spread between
the first two parent runs; further pairs only add runs to compare, they do not widen the bar.

    python scripts/seq_cfg_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/seq_cfg_measure.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
N_FRAMES, WARM, TIMED = 24, 4, 200
SIZES = {0: (150, 30), 1: (300, 20), 2: (500, 12)}


def frame_of(k):
    m = k % (2 * N_FRAMES - 2)
    return m if m < N_FRAMES else 2 * N_FRAMES - 2 - m


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import numpy as np
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    if mode in "xyz":
        idx = torch.arange("xyz".index(mode), B, 3, device=dev)
        frames, depth = frames[:, idx].contiguous(), depth[idx].contiguous()
        max_cnt, min_dist = SIZES["xyz".index(mode)]
    elif mode == "m":
        max_cnt, min_dist = SIZES[2]
    else:
        max_cnt, min_dist = SIZES[0]
    nb = frames.shape[1]
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=nb, max_cnt=max_cnt, min_dist=min_dist))
    trk.set_profiling(True)
    if mode == "m":
        for b in range(B):
            if b % 3 != 2:
                trk.set_seq_cfg(b, max_cnt=SIZES[b % 3][0], min_dist=SIZES[b % 3][1])
    out_features = 0
    for k in range(WARM + TIMED):
        if k == WARM:
            trk.reset_stats()
        n = trk.trackImageBatchDevice([k / 15.0] * nb, frames.data_ptr() + frame_of(k) * nb * H * W, depth.data_ptr(), unpack=False)
        out_features = int(n.sum())
    st = trk.stats()
    return {"sequences": nb, "max_cnt": max_cnt, "min_dist": min_dist, "tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "pyramid_ms": st["ms_pyramid"] / TIMED,
            "lk_ms": st["ms_lk"] / TIMED, "detect_ms": st["ms_detect"] / TIMED, "tracked_per_frame": st["tracked_features"] / TIMED / nb,
            "features_last_frame": out_features}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--pairs", type=int, default=2, help="parent / this-commit pairs, alternating")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    ORDER = "pn" * max(a.pairs, 2) + "mxyz"
    runs = {m: [] for m in sorted(set(ORDER))}
    for m in ORDER:
        env = dict(os.environ)
        if m == "p":
            if not a.parent_lib:
                continue
            env["GF_LIB_PATH"] = os.path.abspath(a.parent_lib)
        out = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", m], env=env, capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("measurement %s failed with status %d, nothing more is started:\n%s" % (m, out.returncode, out.stderr[-2000:]))
        r = json.loads(out.stdout.strip().splitlines()[-1])
        runs[m].append(r)
        print(m, json.dumps(r), flush=True)
    res = {"order": ORDER, "timed_frames": TIMED, "runs": runs}
    g = {m: [r["tracker_gpu_ms"] for r in rs] for m, rs in runs.items()}
    if g["p"]:
        spread = max(g["p"][:2]) - min(g["p"][:2])
        res["parent_ms"], res["parent_spread_ms"] = g["p"], spread
        mean = sum(g["p"][:2]) / 2
        res["bar_ms"] = mean + max(0.01 * mean, spread)       # against the mean of the (n) runs
    res["unset_ms"] = g["n"]
    res["unset_mean_ms"] = sum(g["n"]) / len(g["n"])
    res["mixed_ms"] = g["m"][0]
    res["three_handles_ms"] = {m: g[m][0] for m in "xyz"}
    res["three_handles_sum_ms"] = sum(g[m][0] for m in "xyz")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
