#!/usr/bin/env python3
"""What the depth registration costs (profiles/depth_reg_measure.json; profiles/README.md "Depth registration").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

  p / n  a handle that sets nothing: the parent commit's library (--parent-lib) and this one alternating (p n p n p n), 256 VGA sequences, configs[1] (150
         features, min_dist 30), the benchmark's device-resident frames, profiling on: ms_total_gpu of gf_tracker_stats per frame over 200 frames behind 4
         warm-up ones.  The bar comes from the parent alone: the mean of its runs plus the larger of 1 % and its own spread; the mean of the (n) runs is held
         against it.
  a / b  used: 256 sequences, each with a D435-like registration (15 mm baseline, a few milliradians, colour distortion), every sequence its own raw frame in
         device memory, through gf_tracker_track_batch_device_refs.  a: VGA depth to VGA colour.  b: 848 x 480 depth to 1280 x 720 colour.  Recorded: the
         hipEvent time of the two kernels per call (gf_tracker_get_depth_reg_stats), ms_total_gpu and the wall time of the call; next to them a device copy of
         the same input bytes (torch, timed by events) and the time the kernels' algorithmic bytes -- 2 read + 4 atomic per covered pixel (counted by the numpy
         restatement of tests/depth_reg_ref.py on the frame) + 4 read + 4 re-primed + 2 written per output pixel -- take at 6.29 TB/s, the measured HBM rate
  A / B  the same calls on a handle without any registration, fed the frames registered beforehand (gf_depth_register_batch_device): what the fleet pays is a - A
  t      ten frames of (a), no warm-up, under `rocprofv3 --kernel-trace --stats` (the program after `--`, a run of its own): launches per kernel name

    python scripts/depth_reg_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/depth_reg_measure.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
N_FRAMES, WARM, TIMED = 24, 4, 200
USED_FRAMES, USED_WARM, USED_TIMED = 8, 4, 40
HBM_TBS = 6.29
SHAPES = {"a": ((640, 480), (640, 480)), "b": ((848, 480), (1280, 720))}   # depth size, colour size
TRACE_FRAMES = 10


def frame_of(k, n=N_FRAMES):
    m = k % (2 * n - 2)
    return m if m < n else 2 * n - 2 - m


def unused():
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=150, min_dist=30))
    trk.set_profiling(True)
    for k in range(WARM + TIMED):
        if k == WARM:
            trk.reset_stats()
        n = trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)
    st = trk.stats()
    return {"sequences": B, "features_last_frame": int(n.sum()), "tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "pyramid_ms": st["ms_pyramid"] / TIMED,
            "lk_ms": st["ms_lk"] / TIMED, "detect_ms": st["ms_detect"] / TIMED}


def used(mode, warm=USED_WARM, timed=USED_TIMED):
    """a / b: registered in the call; A / B: the same handle without a registration on frames registered beforehand"""
    import numpy as np
    import torch
    import gfamd
    import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import depth_reg_ref as ref
    (wd, hd), (wc, hc) = SHAPES[mode.lower()]
    in_call = mode.islower()
    fc, fd = 0.94 * wc, (0.70 if mode.lower() == "b" else 0.94) * wd   # the depth camera of (b) sees a wider field than the colour camera, as a D435's does
    colour = (fc, fc, wc / 2 - 0.3, hc / 2 + 0.4, 0.08, -0.12, 0.0006, -0.0004)
    reg = ref.make_reg(wd, hd, fd, fd, wd / 2 + 0.2, hd / 2 - 0.1, 0.001, ref.rot(0.004, -0.003, 0.002), (0.015, 0.0004, -0.0003))
    scene = ref.scene(wd, hd, 0.001, 11)
    _, census = ref.register(scene, reg, colour, wc, hc, scatter=False)
    cfg = gfamd.default_cfg(width=wc, height=hc, batch=B, max_cnt=150, min_dist=30)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.k1, cfg.k2, cfg.p1, cfg.p2 = colour
    trk = gfamd.FeatureTracker(cfg)
    gray = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in synth.tracker_sequence(3100, USED_FRAMES, wc, hc)]
    raw = torch.from_numpy(scene.view(np.int16)).cuda().unsqueeze(0).repeat(B, 1, 1).contiguous()   # every sequence its own frame
    dreg, cam = gfamd.DepthReg.make(wd, hd, reg["fx"], reg["fy"], reg["cx"], reg["cy"], reg["scale"], reg["R"], reg["T"]), gfamd.CameraModel.make(gfamd.CAMERA_PINHOLE, colour[:4], colour[4:])
    out = {"sequences": B, "depth": [wd, hd], "colour": [wc, hc], "census": census}
    if in_call:
        for b in range(B):
            trk.set_seq_depth_reg(b, dreg)
        depth_refs = [(raw[b].data_ptr(), 2 * wd) for b in range(B)]
        # a device copy of the same input bytes
        dst = torch.empty_like(raw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dst.copy_(raw)
        torch.cuda.synchronize()
        reps = 20
        e0.record()
        for _ in range(reps):
            dst.copy_(raw)
        e1.record()
        torch.cuda.synchronize()
        out["copy_input_ms"] = e0.elapsed_time(e1) / reps
        del dst
        covered, px = census["covered"] * B, wc * hc * B
        out["algorithmic_bytes"] = 2 * wd * hd * B + 4 * covered + (4 + 4 + 2) * px
        out["algorithmic_ms_at_hbm"] = out["algorithmic_bytes"] / (HBM_TBS * 1e12) * 1e3
        out["atomic_bytes"] = 4 * covered
    else:
        pre = torch.empty((B, hc, wc), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        gfamd.depth_register_device([(raw[b].data_ptr(), 2 * wd) for b in range(B)], [dreg] * B, [cam] * B, [(wc, hc)] * B, [(pre[b].data_ptr(), 2 * wc) for b in range(B)])
        depth_refs = [(pre[b].data_ptr(), 2 * wc) for b in range(B)]
    trk.set_profiling(True)
    depth_refs = gfamd.frame_refs(depth_refs)
    calls = []
    for k in range(warm + timed):
        if k == warm:
            trk.reset_stats()
        g = gfamd.frame_refs([(gray[frame_of(k, USED_FRAMES)].data_ptr(), wc)] * B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = trk.trackImageBatchDeviceRefs([k / 15.0] * B, g, depth_refs, unpack=False)
        if k >= warm:
            calls.append((time.perf_counter() - t0) * 1e3)
    st, rs = trk.stats(), trk.depth_reg_stats()
    out.update({"features_last_frame": int(n.sum()), "call_ms": sum(calls) / len(calls), "tracker_gpu_ms": st["ms_total_gpu"] / timed, "lk_ms": st["ms_lk"] / timed,
                "detect_ms": st["ms_detect"] / timed, "reg_launches": rs["launches"], "reg_frames": rs["frames"], "reg_kernels_ms": rs["kernel_ms"] / timed})
    return out


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    if mode in "pn":
        return unused()
    if mode == "r":       # what (t) traces: ten frames of (a) from its first
        return used("a", 0, TRACE_FRAMES)
    return used(mode)


def trace():
    """launches per kernel name of `--one r` under rocprofv3; the driver only starts it and reads its files"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["timeout", "-k", "10", "170", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                              sys.executable, os.path.abspath(__file__), "--one", "r"], capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("the traced run failed with status %d, nothing more is started:\n%s" % (out.returncode, out.stderr[-2000:]))
        run = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
        counts, total_ns = {}, {}
        for fn in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(fn)):
                name = r["Kernel_Name"].split("(")[0]
                counts[name] = counts.get(name, 0) + 1
                total_ns[name] = total_ns.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    of = lambda part, t=counts: sum(v for k, v in t.items() if part in k)
    res = {"frames": TRACE_FRAMES, "sequences": run["sequences"], "launches": dict(sorted(counts.items())), "depth_scatter": of("depth_scatter"), "depth_finish": of("depth_finish"),
           "depth_scatter_ms_per_frame": of("depth_scatter", total_ns) / 1e6 / TRACE_FRAMES, "depth_finish_ms_per_frame": of("depth_finish", total_ns) / 1e6 / TRACE_FRAMES,
           "reg_launches_from_stats": run["reg_launches"]}
    res["matches_rule"] = bool(res["depth_scatter"] == res["depth_finish"] == TRACE_FRAMES and res["reg_launches_from_stats"] == 2 * TRACE_FRAMES)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--pairs", type=int, default=3, help="parent / this-commit pairs, alternating")
    ap.add_argument("--limit", type=int, default=170, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = "pn" * max(a.pairs, 2) + "aAbBt"
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
        if m == "t":
            runs[m].append(trace())
            print(m, json.dumps(runs[m][-1]), flush=True)
            continue
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
    res = {"order": order, "timed_frames": TIMED, "used_timed_frames": USED_TIMED, "hbm_tb_per_s": HBM_TBS, "runs": runs}
    p, n = [r["tracker_gpu_ms"] for r in runs["p"]], [r["tracker_gpu_ms"] for r in runs["n"]]
    if p:
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res["parent_ms"], res["parent_mean_ms"], res["parent_spread_ms"] = p, mean, spread
        res["bar_ms"] = mean + max(0.01 * mean, spread)
    res["unset_ms"], res["unset_mean_ms"] = n, sum(n) / len(n)
    if p:
        res["unset_meets_bar"] = res["unset_mean_ms"] <= res["bar_ms"]
    for m in "ab":
        u, v = runs[m][0], runs[m.upper()][0]
        res["used_" + m] = {"depth": u["depth"], "colour": u["colour"], "reg_kernels_ms": u["reg_kernels_ms"], "copy_input_ms": u["copy_input_ms"],
                            "algorithmic_ms_at_hbm": u["algorithmic_ms_at_hbm"], "atomic_tb_per_s_if_atomic_bound": u["atomic_bytes"] / (u["reg_kernels_ms"] * 1e-3) / 1e12,
                            "tracker_gpu_ms": u["tracker_gpu_ms"], "tracker_gpu_ms_registered_beforehand": v["tracker_gpu_ms"], "call_ms": u["call_ms"],
                            "call_ms_registered_beforehand": v["call_ms"], "same_features": u["features_last_frame"] == v["features_last_frame"]}
    res["trace"] = {k: v for k, v in runs["t"][0].items() if k != "launches"}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
