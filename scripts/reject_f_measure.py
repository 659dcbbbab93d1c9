#!/usr/bin/env python3
"""What rejectWithF costs (profiles/reject_f_measure.json; profiles/README.md "rejectWithF").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

  p / n  a handle that never calls the setter: the parent commit's library (--parent-lib) and this one alternating (p n p n p n), 256 VGA sequences, 150
         features, min_dist 30, the benchmark's device-resident frames, profiling on: ms_total_gpu of gf_tracker_stats per frame over 200 frames behind 4
         warm-up ones.  The bar comes from the parent alone: the mean of its runs plus the larger of 1 % and its own spread; the mean of the (n) runs is held
         against it.
  d / h  used: the same 256 sequences with the switch on (F_threshold 1.0), three runs each, alternating.  d: the device form, reject_f_kernel behind LK.
         h: GF_REJECT_F_HOST=1, gfrf::reject inside the host stage on the handle's pool.  Recorded per frame: the kernel's hipEvent time
         (gf_tracker_get_reject_f_stats), ms_total_gpu, the wall time of the call, candidates and rejected
  o      the same run with the switch off in this library, for the wall time of a call without the stage
  t      ten frames of (d), no warm-up, under `rocprofv3 --kernel-trace --stats` (the program after `--`, a run of its own): launches per kernel name

    python scripts/reject_f_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/reject_f_measure.json
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
USED_WARM, USED_TIMED = 4, 100
TRACE_FRAMES = 10


def frame_of(k, n=N_FRAMES):
    m = k % (2 * n - 2)
    return m if m < n else 2 * n - 2 - m


def run(on, warm, timed):
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=150, min_dist=30))
    if on:
        for b in range(B):
            trk.set_seq_reject_f(b, f_threshold=1.0, seed=b)
    trk.set_profiling(True)
    calls = []
    for k in range(warm + timed):
        if k == warm:
            trk.reset_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)
        if k >= warm:
            calls.append((time.perf_counter() - t0) * 1e3)
    st = trk.stats()
    out = {"sequences": B, "features_last_frame": int(n.sum()), "tracker_gpu_ms": st["ms_total_gpu"] / timed, "pyramid_ms": st["ms_pyramid"] / timed,
           "lk_ms": st["ms_lk"] / timed, "detect_ms": st["ms_detect"] / timed, "call_ms": sum(calls) / len(calls), "wait_lk_ms": st["ms_wait_lk"] / timed,
           "host_mid_ms": st["ms_host_mid"] / timed}
    if on:
        rf = trk.reject_f_stats()
        out.update({"rf_launches": rf["launches"], "rf_sequences": rf["sequences"], "rf_candidates_per_frame": rf["candidates"] / timed, "rf_rejected_per_frame": rf["rejected"] / timed,
                    "rf_no_model": rf["no_model"], "rf_kernel_ms": rf["kernel_ms"] / timed})
    return out


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    if mode in "pn":
        return run(False, WARM, TIMED)
    if mode == "o":
        return run(False, USED_WARM, USED_TIMED)
    if mode == "r":       # what (t) traces: ten frames of (d) from its first
        return run(True, 0, TRACE_FRAMES)
    return run(True, USED_WARM, USED_TIMED)


def trace():
    """launches per kernel name of `--one r` under rocprofv3; the driver only starts it and reads its files"""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["timeout", "-k", "10", "170", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                              sys.executable, os.path.abspath(__file__), "--one", "r"], capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("the traced run failed with status %d, nothing more is started:\n%s" % (out.returncode, out.stderr[-2000:]))
        run_ = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
        counts, total_ns = {}, {}
        for fn in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(fn)):
                name = r["Kernel_Name"].split("(")[0]
                counts[name] = counts.get(name, 0) + 1
                total_ns[name] = total_ns.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    of = lambda part, t=counts: sum(v for k, v in t.items() if part in k)
    own = {k: v for k, v in sorted(counts.items()) if "gf::" in k or "gfrf::" in k or "gfcopy::" in k}   # the project's own: the frame generator's torch kernels are no evidence
    res = {"frames": TRACE_FRAMES, "sequences": run_["sequences"], "launches": own, "reject_f_kernel": of("reject_f_kernel"),
           "reject_f_kernel_ms_per_launch": of("reject_f_kernel", total_ns) / 1e6 / max(of("reject_f_kernel"), 1), "rf_launches_from_stats": run_["rf_launches"]}
    res["matches_rule"] = bool(res["reject_f_kernel"] == res["rf_launches_from_stats"] == TRACE_FRAMES - 1)   # the first frame has no tracked point
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
    order = "pn" * max(a.pairs, 2) + "dh" * 3 + "ot"
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
        if m == "t":
            runs[m].append(trace())
            print(m, json.dumps(runs[m][-1]), flush=True)
            continue
        env = dict(os.environ)
        env.pop("GF_REJECT_F_HOST", None)
        if m == "p":
            if not a.parent_lib:
                continue
            env["GF_LIB_PATH"] = os.path.abspath(a.parent_lib)
        if m == "h":
            env["GF_REJECT_F_HOST"] = "1"
        out = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", m], env=env, capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("measurement %s failed with status %d, nothing more is started:\n%s" % (m, out.returncode, out.stderr[-2000:]))
        r = json.loads(out.stdout.strip().splitlines()[-1])
        runs[m].append(r)
        print(m, json.dumps(r), flush=True)
    res = {"order": order, "timed_frames": TIMED, "used_timed_frames": USED_TIMED, "runs": runs}
    p, n = [r["tracker_gpu_ms"] for r in runs["p"]], [r["tracker_gpu_ms"] for r in runs["n"]]
    if p:
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res["parent_ms"], res["parent_mean_ms"], res["parent_spread_ms"] = p, mean, spread
        res["bar_ms"] = mean + max(0.01 * mean, spread)
    res["unset_ms"], res["unset_mean_ms"] = n, sum(n) / len(n)
    if p:
        res["unset_meets_bar"] = res["unset_mean_ms"] <= res["bar_ms"]
    mean_of = lambda m, key: sum(r[key] for r in runs[m]) / len(runs[m])
    res["used"] = {"device": {k: mean_of("d", k) for k in ("rf_kernel_ms", "tracker_gpu_ms", "call_ms", "rf_candidates_per_frame", "rf_rejected_per_frame")},
                   "host": {k: mean_of("h", k) for k in ("rf_kernel_ms", "tracker_gpu_ms", "call_ms", "rf_candidates_per_frame", "rf_rejected_per_frame")},
                   "off_call_ms": mean_of("o", "call_ms"), "device_call_ms_runs": [r["call_ms"] for r in runs["d"]], "host_call_ms_runs": [r["call_ms"] for r in runs["h"]]}
    res["used"]["same_counts"] = res["used"]["device"]["rf_rejected_per_frame"] == res["used"]["host"]["rf_rejected_per_frame"]
    res["used"]["faster_form"] = "device" if res["used"]["device"]["call_ms"] <= res["used"]["host"]["call_ms"] else "host"
    res["trace"] = {k: v for k, v in runs["t"][0].items() if k != "launches"}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
