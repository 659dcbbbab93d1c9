#!/usr/bin/env python3
"""What the stereo depth costs (profiles/stereo_depth_measure.json; profiles/README.md "Stereo depth").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.  The tracker
runs are those of scripts/stereo_measure.py: 256 VGA sequences, 150 features, min_dist 30, the benchmark's device-resident frames, 200 timed frames behind 4
warm-up ones, the right frame being the left frame moved 8 px to the left, a PINHOLE_FULL right camera.

  p / n  a handle that sets no stereo, the parent commit's library (--parent-lib) / this one, alternating (p n p n p n): ms_total_gpu per frame.  The bar comes
         from the parent alone: the mean of its runs plus its own spread.
  o      256 stereo sequences by reference, the depth switch off: ms_total_gpu and the wall time of a call
  d      the same with the switch on, the device form (stereo_depth_kernel, one launch per call)
  h      the same with GF_STEREO_DEPTH_HOST=1 (gfsd::depth_of inside stereo_stage, no launch)
  t / u  ten frames of (d) / of (o) for a `rocprofv3 --kernel-trace --stats` run of their own (--trace-csv / --trace-off-csv name the kernel_stats files such
         runs left): stereo_depth_kernel's launches and time beside camera_lift_kernel's, and that a handle without the switch launches none.

    python scripts/stereo_depth_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --trace-csv ON_kernel_stats.csv --trace-off-csv OFF_kernel_stats.csv \\
        --bench-txt BENCH.txt --out profiles/stereo_depth_measure.json

--bench-txt: bench.py's result lines, each behind the word `parent` or `this`.  Blocks of an existing --out file that this script does not measure -- closed_loop
(the figures tests/test_stereo_depth_estimator_gpu.py prints) and kernel_resources (the compiler's resource remarks) -- are carried over into the new file.
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
BASELINE, FOCAL = 0.05, 504.5


def by_refs(depth, timed):
    import torch
    import bench
    import gfamd
    import camera_models_measure as cm
    import stereo_measure as sm
    frames, _ = bench.make_frames(cm.N_FRAMES, cm.B, 1000, torch.device("cuda:0"))
    right = torch.roll(frames, -sm.SHIFT, dims=3)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=cm.B, max_cnt=150, min_dist=30, depth_cam=0))
    cam = gfamd.CameraModelEx.make("PINHOLE_FULL", sm.FULL["proj"], sm.FULL["dist"])
    rig = gfamd.StereoDepthCfg.make((1, 0, 0, 0, 1, 0, 0, 0, 1), (BASELINE, 0.0, 0.0), 10.0)
    for b in range(cm.B):
        trk.set_seq_stereo(b, cam)
        if depth:
            trk.set_seq_stereo_depth(b, rig)
    trk.set_profiling(True)
    px = cm.H * cm.W
    tables = []
    for f in range(cm.N_FRAMES):
        gl = gfamd.frame_refs([(frames.data_ptr() + (f * cm.B + b) * px, cm.W) for b in range(cm.B)])
        gr = gfamd.frame_refs([(right.data_ptr() + (f * cm.B + b) * px, cm.W) for b in range(cm.B)])
        tables.append((gl, gr))
    wall = 0.0
    for k in range(cm.WARM + timed):
        if k == cm.WARM:
            trk.reset_stats()
            wall = 0.0
        gl, gr = tables[cm.frame_of(k)]
        t0 = time.perf_counter()
        n = trk.trackImageBatchDeviceRefs([k / 15.0] * cm.B, gl, gr, unpack=False)
        wall += time.perf_counter() - t0
    st = trk.stats()
    return {"sequences": cm.B, "tracker_gpu_ms": st["ms_total_gpu"] / timed, "detect_ms": st["ms_detect"] / timed, "host_post_ms": st["ms_host_post"] / timed,
            "call_wall_ms": 1000.0 * wall / timed, "observations_last_frame": int(n.sum()), "stereo_stats": trk.stereo_stats(), "stereo_depth_stats": trk.stereo_depth_stats(),
            "lift_stats": trk.camera_lift_stats()}


def one(mode):
    if mode in "pn":
        import camera_models_measure as cm
        return cm.tracker(False)
    if mode in "odh":
        return by_refs(mode != "o", 200)
    return by_refs(mode == "t", 6)      # 4 warm-up + 6 frames: ten frames in the trace


def trace_summary(path, frames=10):
    want = ("stereo_depth_kernel", "stereo_lk_sized_kernel", "camera_lift_kernel")
    out = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if not any(w in name for w in want):
            continue
        short = name.split("(")[0].split("::")[-1]
        calls = int(r.get("Calls") or 0)
        total_ns = float(r.get("TotalDurationNs") or 0)
        out[short] = {"launches": calls, "launches_per_frame": calls / frames, "mean_us": total_ns / max(calls, 1) / 1000.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace-csv")
    ap.add_argument("--trace-off-csv")
    ap.add_argument("--bench-txt", help="lines `parent {json}` / `this {json}`: bench.py's result lines with the parent's library (GF_LIB_PATH) and this one, alternating")
    ap.add_argument("--out", help="written anew; blocks of an existing file that this run does not produce (closed_loop, kernel_resources, ...) are carried over")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = ("pn" * 3 if a.parent_lib else "nnn") + "odh" * 3
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
        env = dict(os.environ)
        env.pop("GF_STEREO_DEPTH_HOST", None)
        if m == "p":
            env["GF_LIB_PATH"] = os.path.abspath(a.parent_lib)
        if m == "h":
            env["GF_STEREO_DEPTH_HOST"] = "1"
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
    for key in ("tracker_gpu_ms", "call_wall_ms", "host_post_ms"):
        for m, name in (("o", "off"), ("d", "device"), ("h", "host")):
            v = [r[key] for r in runs[m]]
            res["depth_%s_%s" % (name, key)] = {"runs": v, "mean": sum(v) / len(v), "spread": max(v) - min(v)}
    for name in ("device", "host"):
        res["depth_%s_costs_call_ms" % name] = res["depth_%s_call_wall_ms" % name]["mean"] - res["depth_off_call_wall_ms"]["mean"]
        res["depth_%s_costs_gpu_ms" % name] = res["depth_%s_tracker_gpu_ms" % name]["mean"] - res["depth_off_tracker_gpu_ms"]["mean"]
    res["faster_form"] = "device" if res["depth_device_call_wall_ms"]["mean"] <= res["depth_host_call_wall_ms"]["mean"] else "host"
    if a.trace_csv:
        res["kernel_trace_ten_frames_switch_on"] = trace_summary(a.trace_csv)
    if a.trace_off_csv:
        res["kernel_trace_ten_frames_switch_off"] = trace_summary(a.trace_off_csv)
    if a.bench_txt:
        ms = {"parent": [], "this": []}
        for line in open(a.bench_txt):
            who, text = line.split(" ", 1)
            ms[who].append(json.loads(text)["ms_per_step"])
        res["bench_ms_per_step"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5, the parent's library and this one alternating", "parent": ms["parent"], "this": ms["this"],
                                    "parent_mean": sum(ms["parent"]) / len(ms["parent"]), "this_mean": sum(ms["this"]) / len(ms["this"])}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        if os.path.exists(a.out):   # what other tools put there (the closed loop's figures from its test, the compiler's resource remarks) stays
            for k, v in json.load(open(a.out)).items():
                res.setdefault(k, v)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
