#!/usr/bin/env python3
"""What the sequence list costs a full batch and what a short list saves (profiles/tracker_subset_measure.json).

configs[1] (150 features, min_dist 30), 256 sequences, device-resident VGA frames, profiling on.  Every measurement is a fresh process under a time limit of its
own; the driver itself never opens the GPU and stops at the first measurement that fails.

  a  the parent commit's library (--parent-lib), trackImageBatchDevice: repeated five times, its median and spread are the yardstick
  b  this library, trackImageBatchDevice          c  this library, trackImageSomeDevice with all 256 listed
  d  128 of 256 listed, alternating halves        e  32 of 256 listed, in rotation

run in the order a b c a d e a b c a d e a b c.  Every sequence consumes its own frames in order (a sequence listed every n-th call sees its next frame then),
so all forms track the same steady-state motion; a sequence walks its 52 frames forth and back (the motion reverses, the tracks go on), which lets the timed
window be 480 calls; the frames of a call are gathered into one block outside the timed region, the same way for every form.

    python scripts/tracker_subset_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/tracker_subset_measure.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, MAX_CNT, MIN_DIST, W, H = 256, 150, 30, 640, 480
NSEED, N_FRAMES, WARM_FRAMES, TIMED_CALLS = 8, 52, 4, 480
ORDER = "abcadeabcadeabc"
LISTED = {"a": 256, "b": 256, "c": 256, "d": 128, "e": 32}


def handover_bytes(n, with_list):
    """bytes of the four hand-overs of one call for n listed sequences (gf_tracker.hip, track_core): down before LK, up behind it, down before the detection, up"""
    cap = (MAX_CNT + 3) & ~3
    return (4 * n * with_list + 4 * n + 8 * n * cap) + n * cap * (8 + 1 + 1 + 2 + 8) + (4 * n * with_list + 8 * n * cap + 12 * n) + (4 * n + 8 * n * cap + 2 * n * cap + 4 * n)


def the_list(mode, k):
    n = LISTED[mode]
    first = (k * n) % B
    return range(first, first + n)


def one(mode, frames_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import numpy as np
    import torch
    import gfamd
    frames = torch.from_numpy(np.load(frames_path)).cuda()          # [frame][seed][H][W]
    depth = torch.full((B, H, W), 1500, dtype=torch.int16).cuda()
    seed_of = torch.arange(B).cuda() % NSEED
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=MAX_CNT, min_dist=MIN_DIST))
    trk.set_profiling(True)
    period = B // LISTED[mode]
    wall, listed, fewest = [], 0, MAX_CNT
    for k in range((WARM_FRAMES + TIMED_CALLS // period) * period):
        if k == WARM_FRAMES * period:
            trk.reset_stats()
        L = np.arange(the_list(mode, k).start, the_list(mode, k).stop, dtype=np.int32)
        fi = k // period                                             # how many frames every listed sequence has had
        at = fi % (2 * N_FRAMES - 2)
        block = frames[at if at < N_FRAMES else 2 * N_FRAMES - 2 - at][seed_of[int(L[0]):int(L[0]) + len(L)]].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode in "ab":
            n = trk.trackImageBatchDevice([0.0666 * fi] * B, block.data_ptr(), depth.data_ptr(), unpack=False)
        else:
            n = trk.trackImageSomeDevice(L, [0.0666 * fi] * len(L), block.data_ptr(), depth.data_ptr(), unpack=False)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= WARM_FRAMES * period:
            wall.append(dt)
            listed += len(L)
            fewest = min(fewest, int(n.min()))
    st = trk.stats()
    calls = st["frames"]
    assert calls == len(wall) and st.get("sequence_frames", listed) in (0, listed)     # (the parent's library does not write the member)
    res = {"mode": mode, "listed": LISTED[mode], "calls": calls, "ms_total_gpu": st["ms_total_gpu"] / calls, "ms_wall_median": statistics.median(wall),
           "ms_wall_mean": sum(wall) / calls, "handover_bytes": handover_bytes(LISTED[mode], mode != "a"),
           "tracked_per_sequence_frame": st["tracked_features"] / listed, "fewest_features_returned": fewest}
    for key in ("ms_pyramid", "ms_lk", "ms_detect", "ms_host_pre", "ms_wait_lk", "ms_host_mid", "ms_wait_detect", "ms_host_post"):
        res[key] = st[key] / calls
    trk.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libgroundfusion_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_subset_measure.json"))
    ap.add_argument("--limit", type=int, default=150, help="seconds each measurement may take")
    ap.add_argument("--one", nargs=2, metavar=("MODE", "FRAMES"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(*args.one)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: the parent commit's library is needed for the yardstick")
    sys.path[:0] = [os.path.join(ROOT, "ground-fusion_amd")]
    import numpy as np
    import synth
    n_frames = N_FRAMES
    seqs = [synth.tracker_sequence(1000 + s, n_frames) for s in range(NSEED)]
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "frames.npy")
        np.save(path, np.stack([np.stack([seqs[s][k] for s in range(NSEED)]) for k in range(n_frames)]))
        for mode in ORDER:
            env = dict(os.environ)
            if mode == "a":
                env["GF_LIB_PATH"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("GF_LIB_PATH", None)
            p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", mode, path], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-3000:])
                sys.exit("measurement %s failed with status %d: nothing more is started" % (mode, p.returncode))
            runs.append(json.loads(line[0][7:]))
            print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in runs[-1].items() if k in ("mode", "ms_total_gpu", "ms_wall_median")}, flush=True)
    out = {"workload": "configs[1]: %d features / min_dist %d, %d sequences, %d x %d device-resident frames, profiling on, %d timed calls behind %d warm-up frames per sequence"
                       % (MAX_CNT, MIN_DIST, B, W, H, TIMED_CALLS, WARM_FRAMES), "order": ORDER, "runs": runs, "summary": {}}
    for key in ("ms_total_gpu", "ms_wall_median"):
        by = {m: [r[key] for r in runs if r["mode"] == m] for m in LISTED}
        s = {m: statistics.median(v) for m, v in by.items()}
        s["a_values"] = by["a"]
        s["a_spread"] = max(by["a"]) - min(by["a"])
        s["full_batch_within_yardstick"] = s["b"] <= max(by["a"]) and s["c"] <= max(by["a"])
        s["shorter_lists_cost_less"] = s["c"] - s["d"] > s["a_spread"] and s["d"] - s["e"] > s["a_spread"]
        out["summary"][key] = s
    out["summary"]["handover_bytes"] = {m: handover_bytes(n, m != "a") for m, n in LISTED.items()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
