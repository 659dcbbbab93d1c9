#!/usr/bin/env python3
"""What the region of interest costs the detector (profiles/roi_measure.json; profiles/README.md "Region of interest").

configs[1] (150 features, min_dist 30), 256 sequences, the benchmark's device-resident VGA frames (bench.make_frames), profiling on: ms_detect of
gf_tracker_stats per frame.  Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first
measurement that fails.

  p  the parent commit's library (--parent-lib), no region of interest: its runs' spread is the yardstick
  n  this library, no region of interest (the handle never allocates the table)
  w  this library, an all-255 region on all 256 sequences (the table exists, the AND changes nothing)
  a  this library, region A (the bottom third excluded) on all 256 sequences
  k  this library: gf_tracker_set_roi_some_device for 256 masks, host clock around the call (packing kernel, 256 copies of the words back to the host copy,
     one synchronise), against the kernel's byte floor: 256 x 640 x 480 bytes in, 256 x 16 x 640 words out

run in the order p n p n p n p n p n w a w a w a w a w a k.

    python scripts/roi_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/roi_measure.json
    python scripts/roi_measure.py --one k      # one measurement in this process (what rocprofv3 --kernel-trace --stats is pointed at for roi_pack_kernel alone)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, MAX_CNT, MIN_DIST, W, H = 256, 150, 30, 640, 480
WARM, TIMED = 4, 20
ORDER = "pnpnpnpnpnwawawawawak"


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import numpy as np
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    if mode == "k":
        trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=MAX_CNT, min_dist=MIN_DIST))
        masks = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (B, H, W)).astype(np.uint8) * 255).to(dev)
        torch.cuda.synchronize()
        seqs = np.arange(B, dtype=np.int32)
        ms = []
        for _ in range(12):
            t0 = time.perf_counter()
            trk.set_roi_device(seqs, masks.data_ptr())
            ms.append(1e3 * (time.perf_counter() - t0))
        ms = ms[2:]
        return {"set_roi_device_ms_median": statistics.median(ms), "set_roi_device_ms_min": min(ms), "bytes_in": B * W * H, "bytes_out": B * 4 * W * ((H + 29) // 30)}
    n_frames = WARM + TIMED + 1
    frames, depth = bench.make_frames(n_frames, B, 1000, dev)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=MAX_CNT, min_dist=MIN_DIST))
    trk.set_profiling(True)
    if mode in "wa":
        R = np.full((H, W), 255, np.uint8)
        if mode == "a":
            R[H - H // 3:, :] = 0
        masks = torch.from_numpy(np.broadcast_to(R, (B, H, W)).copy()).to(dev)
        torch.cuda.synchronize()
        trk.set_roi_device(np.arange(B, dtype=np.int32), masks.data_ptr())
    fewest = MAX_CNT
    for k in range(WARM + TIMED):
        if k == WARM:
            trk.reset_stats()
        n = trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + k * B * H * W, depth.data_ptr(), unpack=False)
        fewest = min(fewest, int(n.min()))
    st = trk.stats()
    return {"detect_ms": st["ms_detect"] / TIMED, "lk_ms": st["ms_lk"] / TIMED, "tracker_gpu_ms": st["ms_total_gpu"] / TIMED,
            "tracked_per_frame": st["tracked_features"] / TIMED / B, "output_per_frame": st["output_features"] / TIMED / B, "fewest_features": fewest}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
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
    res = {"order": ORDER, "batch": B, "timed_frames": TIMED, "runs": runs}
    for m, rs in runs.items():
        if rs and "detect_ms" in rs[0]:
            d = [r["detect_ms"] for r in rs]
            res["detect_ms_" + m] = {"median": statistics.median(d), "min": min(d), "max": max(d)}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
