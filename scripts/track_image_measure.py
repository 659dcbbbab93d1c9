#!/usr/bin/env python3
"""What the track image costs (profiles/track_image_measure.json; profiles/README.md "Track image").

256 sequences, the benchmark's device-resident VGA frames (bench.make_frames, 24 frames walked forwards and backwards), configs[1] (150 features, min_dist 30).
Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

Cost when unused: ms_total_gpu of gf_tracker_stats per frame over 200 frames behind 4 warm-up ones, profiling on,
  p  the parent commit's library (--parent-lib)
  n  this library, the switch never set (nothing is allocated, recorded or launched for it)
in the order p n p n.  Bar for (n): the parent's own figure plus the larger of 1 % and the spread of its first two runs (the rule of scripts/seq_cfg_measure.py).

Cost when used (u): this library, the switch on for every sequence, 30 frames tracked; then the wall clock of gf_tracker_track_image_some_device for all 256
sequences into tight device images, median of 50 calls behind 5 warm-up ones; in the same process the same median for a device-to-device copy of 256 x 614 400
bytes, which has the HBM traffic of 307 KB read + 921 KB written per frame.  Bar: the call takes at most 2 x the copy.  The same call for 1 sequence is
recorded beside it (launch-bound; no bar), and for all 256 into images at base + 1 with a pitch of 3 x 640 + 5 (no 16-byte store form; no bar).

    python scripts/track_image_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/track_image_measure.json
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
USED_FRAMES, CALLS_WARM, CALLS = 30, 5, 50


def frame_of(k):
    m = k % (2 * N_FRAMES - 2)
    return m if m < N_FRAMES else 2 * N_FRAMES - 2 - m


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=150, min_dist=30))
    trk.set_profiling(True)
    if mode == "u":
        trk.set_show_track(True)
    n_frames = USED_FRAMES if mode == "u" else WARM + TIMED
    for k in range(n_frames):
        if k == WARM:
            trk.reset_stats()
        trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)
    st = trk.stats()
    timed = n_frames - WARM
    res = {"tracker_gpu_ms": st["ms_total_gpu"] / timed, "tracked_per_frame": st["tracked_features"] / timed / B}
    if mode != "u":
        return res

    def clock(fn):
        t = []
        for k in range(CALLS_WARM + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if k >= CALLS_WARM:
                t.append((t1 - t0) * 1e3)
        return median(t), min(t), max(t)

    tight = torch.zeros((B, H, 3 * W), dtype=torch.uint8, device=dev)
    refs = gfamd.frame_refs([(tight.data_ptr() + b * H * 3 * W, 3 * W) for b in range(B)])
    seqs = list(range(B))
    pitch = 3 * W + 5
    odd = torch.zeros(B * H * pitch + 16, dtype=torch.uint8, device=dev)
    odd_refs = gfamd.frame_refs([(odd.data_ptr() + 1 + b * H * pitch, pitch) for b in range(B)])
    src, dst = torch.zeros(B * 614400, dtype=torch.uint8, device=dev), torch.zeros(B * 614400, dtype=torch.uint8, device=dev)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    res["draw_256_ms"], res["draw_256_min_ms"], res["draw_256_max_ms"] = clock(lambda: trk.track_image_device(seqs, refs))
    res["copy_256x614400_ms"], res["copy_min_ms"], res["copy_max_ms"] = clock(copy)
    one_ref = gfamd.frame_refs([(tight.data_ptr(), 3 * W)])
    res["draw_1_ms"] = clock(lambda: trk.track_image_device([0], one_ref))[0]
    res["draw_256_odd_pitch_ms"] = clock(lambda: trk.track_image_device(seqs, odd_refs))[0]
    res["ratio_to_copy"] = res["draw_256_ms"] / res["copy_256x614400_ms"]
    res["painted_fraction_seq0"] = float((tight[0].view(H, W, 3).float().std(dim=2) > 0).float().mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = "pnpnu" if a.parent_lib else "nnu"
    runs = {m: [] for m in "pnu"}
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
    res = {"order": order, "timed_frames": TIMED, "runs": runs}
    g = {m: [r["tracker_gpu_ms"] for r in rs] for m, rs in runs.items()}
    res["unset_ms"] = g["n"]
    res["unset_mean_ms"] = sum(g["n"]) / len(g["n"])
    if g["p"]:
        spread = max(g["p"][:2]) - min(g["p"][:2])
        mean = sum(g["p"][:2]) / 2
        res["parent_ms"], res["parent_spread_ms"] = g["p"], spread
        res["unused_bar_ms"] = mean + max(0.01 * mean, spread)
        res["unused_within_bar"] = res["unset_mean_ms"] <= res["unused_bar_ms"]
    u = runs["u"][0]
    res["used"] = u
    res["used_bar_ratio"] = 2.0
    res["used_within_bar"] = u["ratio_to_copy"] <= 2.0
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
