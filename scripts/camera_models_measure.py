#!/usr/bin/env python3
"""What camera models per sequence cost (profiles/camera_models_measure.json; profiles/README.md "Camera models").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

  p / n  a handle that sets no camera: the parent commit's library (--parent-lib) and this one alternating (p n p n p n), 256 VGA sequences, configs[1] (150
         features, min_dist 30), the benchmark's device-resident frames, profiling on: ms_total_gpu of gf_tracker_stats per frame over 200 frames behind 4
         warm-up ones.  The bar comes from the parent alone: the mean of its runs plus its own spread; the mean of the (n) runs is held against it.
  d / h  256 Kannala-Brandt sequences at 150 features on the same frames, lifted on the device (d, GF_CAMERA_LIFT_HOST=0) and on the host (h, =1), alternating:
         wall time of a tracker call (a host clock around the call, which ends in a stream synchronisation), the per-sequence host stage behind the detection
         (ms_host_post: after_detect on the pool), the detection stage of the profile (which holds the lift kernel) and the tracker's GPU time.  No bar: the two
         are compared, the spread of the runs beside them.
  k      the kernel alone: gf_camera_lift_batch_device on 256 sequences of 150 points resident on the device, all Kannala-Brandt / all MEI / all PINHOLE / the three
         mixed, device events around windows of 40 calls (each call also stages its camera table and waits for its stream: the figure is a call, an upper bound
         of the kernel)

    python scripts/camera_models_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/camera_models_measure.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
N_FRAMES, WARM, TIMED = 24, 4, 200
KB = ("KANNALA_BRANDT", [285.5, 286.25, 320.5, 240.25], [-0.012, 0.006, -0.003, 0.0006], 0.0)      # the fixture's full monotone set
MEI = ("MEI", [470.5, 468.25, 320.5, 240.25], [-0.02, 0.003, 2e-4, -1e-4], 1.0)
PIN = ("PINHOLE", [603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656], [0.148, -0.468, 1.6e-3, -8.9e-3], 0.0)


def frame_of(k):
    m = k % (2 * N_FRAMES - 2)
    return m if m < N_FRAMES else 2 * N_FRAMES - 2 - m


def tracker(with_camera):
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=150, min_dist=30))
    if with_camera:
        cam = gfamd.CameraModel.make(*KB)
        for b in range(B):
            trk.set_seq_camera(b, cam)
    trk.set_profiling(True)
    wall = 0.0
    for k in range(WARM + TIMED):
        if k == WARM:
            trk.reset_stats()
            wall = 0.0
        t0 = time.perf_counter()
        n = trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)
        wall += time.perf_counter() - t0
    st = trk.stats()
    return {"sequences": B, "tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "pyramid_ms": st["ms_pyramid"] / TIMED, "lk_ms": st["ms_lk"] / TIMED,
            "detect_ms": st["ms_detect"] / TIMED, "host_post_ms": st["ms_host_post"] / TIMED, "wait_detect_ms": st["ms_wait_detect"] / TIMED,
            "call_wall_ms": 1000.0 * wall / TIMED, "features_last_frame": int(n.sum())}


def kernel():
    import numpy as np
    import torch
    import gfamd
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    n = 150
    uv = torch.from_numpy(np.stack([rng.uniform(0, W - 1, B * n), rng.uniform(0, H - 1, B * n)], 1).astype(np.float32)).to(dev)
    un = torch.zeros((B * n, 2), dtype=torch.float32, device=dev)
    sets = {"kannala_brandt": [gfamd.CameraModel.make(*KB)] * B, "mei": [gfamd.CameraModel.make(*MEI)] * B, "pinhole": [gfamd.CameraModel.make(*PIN)] * B,
            "mixed": [gfamd.CameraModel.make(*(KB, MEI, PIN)[b % 3]) for b in range(B)]}
    torch.cuda.synchronize()
    out = {}
    for _ in range(3):
        for cams in sets.values():
            gfamd.camera_lift_device(cams, [n] * B, uv.data_ptr(), None, un.data_ptr())
    for name, cams in sets.items():
        us = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(40):
                gfamd.camera_lift_device(cams, [n] * B, uv.data_ptr(), None, un.data_ptr())
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / 40)
        out[name] = {"call_us": us, "call_median_us": sorted(us)[2]}
    return out


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    if mode in "pn":
        return tracker(False)
    if mode in "dh":
        return tracker(True)
    return kernel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--pairs", type=int, default=3, help="pairs of each alternating comparison")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = "pn" * max(a.pairs, 3) + "dh" * max(a.pairs, 3) + "k"
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
        env = dict(os.environ)
        if m == "p":
            if not a.parent_lib:
                continue
            env["GF_LIB_PATH"] = os.path.abspath(a.parent_lib)
        if m in "dh":
            env["GF_CAMERA_LIFT_HOST"] = "1" if m == "h" else "0"
        out = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", m], env=env, capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("measurement %s failed with status %d, nothing more is started:\n%s" % (m, out.returncode, out.stderr[-2000:]))
        r = json.loads(out.stdout.strip().splitlines()[-1])
        runs[m].append(r)
        print(m, json.dumps(r), flush=True)
    res = {"order": order, "timed_frames": TIMED, "runs": runs}
    p, n = [r["tracker_gpu_ms"] for r in runs["p"]], [r["tracker_gpu_ms"] for r in runs["n"]]
    if p:
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res["parent_ms"], res["parent_mean_ms"], res["parent_spread_ms"] = p, mean, spread
        res["bar_ms"] = mean + spread
    res["unset_ms"], res["unset_mean_ms"] = n, sum(n) / len(n)
    if p:
        res["unset_meets_bar"] = res["unset_mean_ms"] <= res["bar_ms"]
    for key in ("call_wall_ms", "host_post_ms", "detect_ms", "tracker_gpu_ms"):
        for m, name in (("d", "device"), ("h", "host")):
            v = [r[key] for r in runs[m]]
            res["used_%s_%s" % (name, key)] = {"runs": v, "mean": sum(v) / len(v), "spread": max(v) - min(v)}
    d, h = res["used_device_call_wall_ms"], res["used_host_call_wall_ms"]
    res["device_lift_faster_by_ms"] = h["mean"] - d["mean"]
    res["device_lift_wins"] = res["device_lift_faster_by_ms"] > max(d["spread"], h["spread"])
    res["kernel"] = {k: v["call_median_us"] for k, v in runs["k"][0].items()}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
