#!/usr/bin/env python3
"""What a frame size per sequence costs (profiles/seq_size_measure.json; profiles/README.md "A frame size per sequence").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

  p / n  a handle that sets nothing: the parent commit's library (--parent-lib) and this one alternating (p n p n p n), 256 VGA sequences, configs[1] (150
         features, min_dist 30), the benchmark's device-resident frames, profiling on: ms_total_gpu of gf_tracker_stats per frame over 200 frames behind 4
         warm-up ones.  The bar comes from the parent alone: the mean of its runs plus the larger of 1 % and its own spread; the mean of the (n) runs is held
         against it.
  k      the price of geometry from a table: 256 sequences that all have the VGA size, in a 640 x 480 handle (the unsized forms) and in a 644 x 481 handle whose
         sequences are all set to 640 x 480 (the sized forms), in ONE process on the same device frames, the two handles taking turns frame by frame: the stages'
         times from each handle's device events, 200 frames behind 4 warm-up ones
  m      one 1280 x 720 handle with 64 sequences each of 1280 x 720, 752 x 480, 640 x 480 and 320 x 240 (sequence b has size b % 4)
  w x y z  four homogeneous handles of 64 sequences of those sizes on the frames the same sequences see in (m): their sum is what the fleet pays today
  t      ten frames of the mixed handle of (m), no warm-up, under `rocprofv3 --kernel-trace --stats` (the program after `--`, a run of its own): launches per
         kernel name, held against the rule that no count follows the number of sequences -- LK one launch per frame that has points, the detector and each
         selection kernel at most one per frame, the pyramid the sum of the four sizes' routes per frame

    python scripts/seq_size_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/seq_size_measure.json
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
FLEET = [(1280, 720), (752, 480), (640, 480), (320, 240)]
FLEET_FRAMES, FLEET_WARM, FLEET_TIMED = 8, 4, 40
STAGES = ("ms_total_gpu", "ms_pyramid", "ms_lk", "ms_detect")


def frame_of(k, n=N_FRAMES):
    m = k % (2 * n - 2)
    return m if m < n else 2 * n - 2 - m


def vga(sized, capacity=(W, H)):
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(width=capacity[0], height=capacity[1], batch=B, max_cnt=150, min_dist=30))
    if sized:
        for b in range(B):
            trk.set_seq_size(b, W, H)
    trk.set_profiling(True)
    for k in range(WARM + TIMED):
        if k == WARM:
            trk.reset_stats()
        n = trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)
    st = trk.stats()
    out = {"sequences": B, "features_last_frame": int(n.sum()), "lk_launches": st["lk_launches"]}
    out.update({s[3:] + "_ms" if s != "ms_total_gpu" else "tracker_gpu_ms": st[s] / TIMED for s in STAGES})
    return out


def kernel():
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    plain = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=150, min_dist=30))
    sized = gfamd.FeatureTracker(gfamd.default_cfg(width=644, height=481, batch=B, max_cnt=150, min_dist=30))
    for b in range(B):
        sized.set_seq_size(b, W, H)
    out = {}
    for t in (plain, sized):
        t.set_profiling(True)
    for k in range(WARM + TIMED):
        for t in ((plain, sized) if k % 2 == 0 else (sized, plain)):     # the forms take turns, and turns at going first
            if k == WARM:
                t.reset_stats()
            t.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)
    for name, t in (("unsized", plain), ("sized", sized)):
        st = t.stats()
        out[name] = {s[3:] + "_ms" if s != "ms_total_gpu" else "tracker_gpu_ms": st[s] / TIMED for s in STAGES}
        out[name]["lk_launches"] = st["lk_launches"]
    return out


def fleet(mode, warm=FLEET_WARM, timed=FLEET_TIMED):
    """m: the mixed handle; w x y z: the homogeneous handle of FLEET["wxyz".index(mode)]; sequence b of the mixed handle sees the frames of its size"""
    import numpy as np
    import torch
    import gfamd
    import synth
    per = B // 4
    which = list(range(4)) if mode == "m" else ["wxyz".index(mode)]
    blocks, depths = {}, {}
    for i in which:
        w, h = FLEET[i]
        seq = synth.tracker_sequence(3000 + i, FLEET_FRAMES, w, h)
        blocks[i] = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in seq]
        depths[i] = torch.full((h, w), 1800, dtype=torch.int16).cuda()
    if mode == "m":
        trk = gfamd.FeatureTracker(gfamd.default_cfg(width=1280, height=720, batch=B, max_cnt=150, min_dist=30))
        size_of = [FLEET[b % 4] for b in range(B)]
        for b in range(B):
            trk.set_seq_size(b, *size_of[b])
        pick = [b % 4 for b in range(B)]
    else:
        w, h = FLEET[which[0]]
        trk = gfamd.FeatureTracker(gfamd.default_cfg(width=w, height=h, batch=per, max_cnt=150, min_dist=30))
        pick = [which[0]] * per
    n_seq = len(pick)
    trk.set_profiling(True)
    calls = []
    for k in range(warm + timed):
        if k == warm:
            trk.reset_stats()
        f = frame_of(k, FLEET_FRAMES)
        gray = [(blocks[i][f].data_ptr(), FLEET[i][0]) for i in pick]          # every sequence of a size reads the same device frame: by reference
        dep = [(depths[i].data_ptr(), 2 * FLEET[i][0]) for i in pick]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = trk.trackImageSomeDeviceRefs(list(range(n_seq)), [k / 15.0] * n_seq, gray, dep, unpack=False)
        if k >= warm:
            calls.append((time.perf_counter() - t0) * 1e3)
    st = trk.stats()
    out = {"sequences": n_seq, "features_last_frame": int(n.sum()), "call_ms": sum(calls) / len(calls), "lk_launches": st["lk_launches"],
           "pyramid_launches": sum(st[k] for k in st if k.startswith("pyr_"))}
    out.update({s[3:] + "_ms" if s != "ms_total_gpu" else "tracker_gpu_ms": st[s] / timed for s in STAGES})
    return out


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    if mode in "pn":
        return vga(False)
    if mode == "k":
        return kernel()
    if mode == "r":       # what (t) traces: ten frames of the mixed handle from its first
        return fleet("m", 0, TRACE_FRAMES)
    return fleet(mode)


# kernel names of the tracker's front end as they appear in a trace (substrings), and what ten frames of the mixed handle may launch of each
TRACE_FRAMES = 10
PYRAMID = ("pyr_head", "pyr_level0", "pyr_down")


def trace():
    """launches per kernel name of `--one r` under rocprofv3; the driver only starts it and reads its files"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["timeout", "-k", "10", "170", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                              sys.executable, os.path.abspath(__file__), "--one", "r"], capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("the traced run failed with status %d, nothing more is started:\n%s" % (out.returncode, out.stderr[-2000:]))
        run = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
        counts = {}
        for fn in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(fn)):
                name = r["Kernel_Name"].split("(")[0]
                counts[name] = counts.get(name, 0) + 1
    of = lambda part: sum(v for k, v in counts.items() if part in k)
    res = {"frames": TRACE_FRAMES, "sequences": run["sequences"], "launches": dict(sorted(counts.items())),
           "lk": of("lk_track"), "detector": of("detect_strip"), "select_topk": of("select_topk"), "select_corners": of("select_corners"),
           "pyramid": sum(of(p) for p in PYRAMID), "pyramid_from_stats": run["pyramid_launches"], "lk_from_stats": run["lk_launches"]}
    res["matches_rule"] = bool(res["lk"] == res["lk_from_stats"] == TRACE_FRAMES - 1 and res["detector"] <= TRACE_FRAMES and res["select_topk"] <= TRACE_FRAMES and
                               1 <= res["select_corners"] <= TRACE_FRAMES and res["pyramid"] == res["pyramid_from_stats"] == 12 * TRACE_FRAMES and
                               all("sized" in k for k in counts if "lk_track" in k or "detect_strip" in k or "select_" in k))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--pairs", type=int, default=3, help="parent / this-commit pairs, alternating")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = "pn" * max(a.pairs, 2) + "kmwxyzt"
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
    res = {"order": order, "timed_frames": TIMED, "fleet_timed_frames": FLEET_TIMED, "runs": runs}
    p, n = [r["tracker_gpu_ms"] for r in runs["p"]], [r["tracker_gpu_ms"] for r in runs["n"]]
    if p:
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res["parent_ms"], res["parent_mean_ms"], res["parent_spread_ms"] = p, mean, spread
        res["bar_ms"] = mean + max(0.01 * mean, spread)
    res["unset_ms"], res["unset_mean_ms"] = n, sum(n) / len(n)
    if p:
        res["unset_meets_bar"] = res["unset_mean_ms"] <= res["bar_ms"]
    res["table_geometry"] = {key: {"unsized_ms": runs["k"][0]["unsized"][key], "sized_ms": runs["k"][0]["sized"][key]} for key in ("tracker_gpu_ms", "pyramid_ms", "lk_ms", "detect_ms")}
    res["trace"] = {k: v for k, v in runs["t"][0].items() if k != "launches"}
    res["mixed_handle"] = {k: runs["m"][0][k] for k in ("tracker_gpu_ms", "call_ms", "pyramid_ms", "lk_ms", "detect_ms", "lk_launches", "pyramid_launches")}
    res["four_handles"] = {m: {k: runs[m][0][k] for k in ("tracker_gpu_ms", "call_ms", "pyramid_ms", "lk_ms", "detect_ms")} for m in "wxyz"}
    res["four_handles_sum"] = {k: sum(res["four_handles"][m][k] for m in "wxyz") for k in ("tracker_gpu_ms", "call_ms", "pyramid_ms", "lk_ms", "detect_ms")}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
