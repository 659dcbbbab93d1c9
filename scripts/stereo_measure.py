#!/usr/bin/env python3
"""What the stereo branch costs (profiles/stereo_measure.json; profiles/README.md "Stereo").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.  The tracker
runs are those of scripts/camera_models_measure.py: 256 VGA sequences, 150 features, min_dist 30, the benchmark's device-resident frames, 200 timed frames behind 4
warm-up ones.

  p / n  a handle that sets no stereo, the parent commit's library (--parent-lib) / this one, alternating (p n p n p n): ms_total_gpu per frame.  The bar comes
         from the parent alone: the mean of its runs plus its own spread.
  o / s  256 sequences by reference (gf_tracker_track_batch_device_refs), the switch off / on with a PINHOLE_FULL right camera, the right frame being the left
         frame moved 8 px to the left: ms_total_gpu, the temporal LK stage and the wall time of a call.  No bar fixed in advance.
  g      for comparison, the same matches made by a second handle of 256 sequences that tracks the right frames: it takes the left frame and then the right frame
         of every stereo frame, so that its temporal LK (the kernel gf_lk_track exposes) runs from left to right on all of the left frame's points, with the
         reverse check; what the right-frame calls cost (ms_total_gpu and wall time) stands beside what the switch adds to a call.
  t      ten frames of (s) for a `rocprofv3 --kernel-trace --stats` run of its own (--trace-csv names the kernel_stats file such a run left): the stereo kernel's
         time beside the temporal launch's, the pyramid kernels', and the launches per frame.

    python scripts/stereo_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --trace-csv DIR/..._kernel_stats.csv --out profiles/stereo_measure.json
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd"), os.path.join(ROOT, "scripts")]
FULL = dict(proj=[504.5, 504.75, 322.5, 241.25], dist=[0.52, -2.7, 4e-4, -1.5e-4, 1.5, 0.4, -2.5, 1.4])
SHIFT = 8


def by_refs(stereo, timed):
    import torch
    import bench
    import gfamd
    import camera_models_measure as cm
    frames, _ = bench.make_frames(cm.N_FRAMES, cm.B, 1000, torch.device("cuda:0"))
    right = torch.roll(frames, -SHIFT, dims=3)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=cm.B, max_cnt=150, min_dist=30, depth_cam=0))
    if stereo:
        cam = gfamd.CameraModelEx.make("PINHOLE_FULL", FULL["proj"], FULL["dist"])
        for b in range(cm.B):
            trk.set_seq_stereo(b, cam)
    trk.set_profiling(True)
    px = cm.H * cm.W
    tables = []
    for f in range(cm.N_FRAMES):
        gl = gfamd.frame_refs([(frames.data_ptr() + (f * cm.B + b) * px, cm.W) for b in range(cm.B)])
        gr = gfamd.frame_refs([(right.data_ptr() + (f * cm.B + b) * px, cm.W) for b in range(cm.B)])
        tables.append((gl, gr))
    out = None
    wall = 0.0
    for k in range(cm.WARM + timed):
        if k == cm.WARM:
            trk.reset_stats()
            wall = 0.0
        gl, gr = tables[cm.frame_of(k)]
        t0 = time.perf_counter()
        n = trk.trackImageBatchDeviceRefs([k / 15.0] * cm.B, gl, gr if stereo else None, unpack=False)
        wall += time.perf_counter() - t0
    st, ss = trk.stats(), trk.stereo_stats()
    out = {"sequences": cm.B, "tracker_gpu_ms": st["ms_total_gpu"] / timed, "pyramid_ms": st["ms_pyramid"] / timed, "lk_ms": st["ms_lk"] / timed,
           "detect_ms": st["ms_detect"] / timed, "host_post_ms": st["ms_host_post"] / timed, "call_wall_ms": 1000.0 * wall / timed,
           "observations_last_frame": int(n.sum()), "stereo_stats": ss, "lift_stats": trk.camera_lift_stats(), "lk_launches": st["lk_launches"]}
    return out


def second_handle(timed=200):
    import torch
    import bench
    import gfamd
    import camera_models_measure as cm
    frames, _ = bench.make_frames(cm.N_FRAMES, cm.B, 1000, torch.device("cuda:0"))
    right = torch.roll(frames, -SHIFT, dims=3)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=cm.B, max_cnt=150, min_dist=30, depth_cam=0))
    trk.set_profiling(True)
    px = cm.B * cm.H * cm.W
    wall = gpu = 0.0
    tracked = 0
    for k in range(cm.WARM + timed):
        if k == cm.WARM:
            wall = gpu = 0.0
            tracked = 0
        f = cm.frame_of(k)
        trk.trackImageBatchDevice([k / 15.0] * cm.B, frames.data_ptr() + f * px, None, unpack=False)
        before = trk.stats()
        t0 = time.perf_counter()
        trk.trackImageBatchDevice([k / 15.0 + 0.01] * cm.B, right.data_ptr() + f * px, None, unpack=False)
        wall += time.perf_counter() - t0
        after = trk.stats()
        gpu += after["ms_total_gpu"] - before["ms_total_gpu"]
        tracked += after["tracked_features"] - before["tracked_features"]
    return {"sequences": cm.B, "right_call_gpu_ms": gpu / timed, "right_call_wall_ms": 1000.0 * wall / timed, "matched_per_frame": tracked / timed}


def one(mode):
    if mode in "pn":
        import camera_models_measure as cm
        return cm.tracker(False)
    if mode in "os":
        return by_refs(mode == "s", 200)
    if mode == "t":
        return by_refs(True, 6)      # 4 warm-up + 6 frames: ten frames in the trace
    return second_handle()


def trace_summary(path, frames=10):
    rows = list(csv.DictReader(open(path)))
    want = ("stereo_lk_sized_kernel", "lk_track", "pyr_", "camera_lift_kernel", "select_", "detect")
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if not any(w in name for w in want):
            continue
        short = name.split("(")[0].split("::")[-1]
        calls = int(r.get("Calls") or 0)
        total_ns = float(r.get("TotalDurationNs") or 0)
        out[short] = {"launches": calls, "launches_per_frame": calls / frames, "mean_us": total_ns / max(calls, 1) / 1000.0, "total_us_per_frame": total_ns / frames / 1000.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace-csv")
    ap.add_argument("--out")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = ("pn" * 3 if a.parent_lib else "nnn") + "os" * 3 + "ggg"
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
        env = dict(os.environ)
        if m == "p":
            env["GF_LIB_PATH"] = os.path.abspath(a.parent_lib)
        out = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", m], env=env, capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("measurement %s failed with status %d, nothing more is started:\n%s" % (m, out.returncode, out.stderr[-2000:]))
        r = json.loads(out.stdout.strip().splitlines()[-1])
        runs[m].append(r)
        print(m, json.dumps(r), flush=True)
    res = {"order": order, "timed_frames": 200, "runs": runs}
    n = [r["tracker_gpu_ms"] for r in runs["n"]]
    res["unset_ms"], res["unset_mean_ms"] = n, sum(n) / len(n)
    if runs.get("p"):
        p = [r["tracker_gpu_ms"] for r in runs["p"]]
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res.update(parent_ms=p, parent_mean_ms=mean, parent_spread_ms=spread, bar_ms=mean + spread, unset_meets_bar=res["unset_mean_ms"] <= mean + spread)
    for key in ("tracker_gpu_ms", "lk_ms", "pyramid_ms", "call_wall_ms", "host_post_ms"):
        for m, name in (("o", "off"), ("s", "on")):
            v = [r[key] for r in runs[m]]
            res["switch_%s_%s" % (name, key)] = {"runs": v, "mean": sum(v) / len(v), "spread": max(v) - min(v)}
    res["switch_on_costs_gpu_ms"] = res["switch_on_tracker_gpu_ms"]["mean"] - res["switch_off_tracker_gpu_ms"]["mean"]
    res["switch_on_costs_call_ms"] = res["switch_on_call_wall_ms"]["mean"] - res["switch_off_call_wall_ms"]["mean"]
    g = runs["g"]
    res["second_handle_right_call_gpu_ms"] = {"runs": [r["right_call_gpu_ms"] for r in g], "mean": sum(r["right_call_gpu_ms"] for r in g) / len(g)}
    res["second_handle_right_call_wall_ms"] = {"runs": [r["right_call_wall_ms"] for r in g], "mean": sum(r["right_call_wall_ms"] for r in g) / len(g)}
    res["second_handle_minus_switch_gpu_ms"] = res["second_handle_right_call_gpu_ms"]["mean"] - res["switch_on_costs_gpu_ms"]
    res["second_handle_minus_switch_call_ms"] = res["second_handle_right_call_wall_ms"]["mean"] - res["switch_on_costs_call_ms"]
    if a.trace_csv:
        res["kernel_trace_ten_frames"] = trace_summary(a.trace_csv)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
