#!/usr/bin/env python3
"""What exclusion boxes cost (profiles/roi_boxes_measure.json; profiles/README.md "Exclusion boxes").

256 sequences, the benchmark's device-resident VGA frames (bench.make_frames, 24 frames walked forwards and backwards), configs[1] (150 features, min_dist 30).
Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

Cost when unused: ms_total_gpu of gf_tracker_stats per frame over 100 frames behind 4 warm-up ones, profiling on,
  p  the parent commit's library (--parent-lib)
  n  this library, no box setter ever called (nothing is allocated, copied or launched for boxes)
in the order p n p n p n.  Bar for the mean of (n): the parent's mean plus the parent's own spread (maximum minus minimum of its runs).

Cost when used (u): this library, two handles on the same frames, 40 frames behind 4 warm-up ones, eight new boxes per sequence and frame:
  boxes  gf_tracker_set_boxes_some for all 256 sequences, then the track call
  masks  gf_tracker_set_roi_some_device with 256 device masks of the same rasters (made before the clock starts), then the track call
Medians of the wall clock of each setter and each track call.  The box setter does not wait for its kernel, which then runs inside the track call's wait, so what
the box path adds to a frame is its setter's wall time plus what its track call takes longer than the mask path's.  Bar: that is at most half of the mask
path's setter time.  Both handles must report the same number of features on every frame.
Next to it the compose kernel for all 256 sequences (wall clock from the setter to a device synchronisation, median of 40) and a device fill of the same
10.5 MB measured the same way.  Nothing else has been measured about what bounds the kernel.

    python scripts/roi_boxes_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/roi_boxes_measure.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
N_FRAMES, WARM, TIMED = 24, 4, 100
USED_WARM, USED = 4, 40
BOXES, RING = 8, 4


def frame_of(k):
    m = k % (2 * N_FRAMES - 2)
    return m if m < N_FRAMES else 2 * N_FRAMES - 2 - m


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import numpy as np
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    torch.cuda.synchronize()
    cfg = dict(batch=B, max_cnt=150, min_dist=30)

    def track(trk, k):
        return trk.trackImageBatchDevice([k / 15.0] * B, frames.data_ptr() + frame_of(k) * B * H * W, depth.data_ptr(), unpack=False)

    if mode != "u":
        trk = gfamd.FeatureTracker(gfamd.default_cfg(**cfg))
        trk.set_profiling(True)
        for k in range(WARM + TIMED):
            if k == WARM:
                trk.reset_stats()
            track(trk, k)
        st = trk.stats()
        return {"tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "tracked_per_frame": st["tracked_features"] / TIMED / B}

    rng = np.random.default_rng(11)
    x0, y0 = rng.integers(-20, W - 20, (RING, B, BOXES)), rng.integers(-20, H - 20, (RING, B, BOXES))
    boxes = np.ascontiguousarray(np.stack([x0, y0, x0 + rng.integers(10, 120, x0.shape), y0 + rng.integers(10, 120, x0.shape)], -1), np.int32)   # [RING, B, BOXES, 4]
    masks = torch.full((RING, B, H, W), 255, dtype=torch.uint8, device=dev)
    for r in range(RING):
        for b in range(B):
            for xa, ya, xb, yb in boxes[r, b]:
                masks[r, b, max(ya, 0):max(yb + 1, 0), max(xa, 0):max(xb + 1, 0)] = 0
    torch.cuda.synchronize()
    seqs = np.arange(B, dtype=np.int32)
    first = np.arange(0, (B + 1) * BOXES, BOXES, dtype=np.int32)
    L = gfamd.lib()
    by_boxes, by_masks = gfamd.FeatureTracker(gfamd.default_cfg(**cfg)), gfamd.FeatureTracker(gfamd.default_cfg(**cfg))

    def set_boxes(r):
        rc = L.gf_tracker_set_boxes_some(by_boxes.h, B, seqs.ctypes.data_as(C.POINTER(C.c_int)), first.ctypes.data_as(C.POINTER(C.c_int)), boxes[r].ctypes.data_as(C.POINTER(gfamd.Box)))
        assert rc == 0, L.gf_last_error()

    def set_masks(r):
        rc = L.gf_tracker_set_roi_some_device(by_masks.h, B, seqs.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(masks[r].data_ptr()))
        assert rc == 0, L.gf_last_error()

    t = {"box_setter": [], "box_track": [], "mask_setter": [], "mask_track": []}
    for k in range(USED_WARM + USED):
        r = k % RING
        counts = []
        for setter, trk, name in ((set_boxes, by_boxes, "box"), (set_masks, by_masks, "mask")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            setter(r)
            t1 = time.perf_counter()
            n = track(trk, k)
            t2 = time.perf_counter()
            counts.append(np.array(n).copy())
            if k >= USED_WARM:
                t[name + "_setter"].append((t1 - t0) * 1e3)
                t[name + "_track"].append((t2 - t1) * 1e3)
        assert np.array_equal(counts[0], counts[1]), "frame %d: the two paths report different numbers of features" % k
    res = {k + "_ms": median(v) for k, v in t.items()}
    res["box_path_adds_ms"] = res["box_setter_ms"] + (res["box_track_ms"] - res["mask_track_ms"])
    res["ratio_to_mask_setter"] = res["box_path_adds_ms"] / res["mask_setter_ms"]
    res["features_per_frame"] = float(np.mean(counts[0]))

    def clock(fn):
        out = []
        for k in range(USED_WARM + USED):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return median(out[USED_WARM:])

    table = torch.zeros(B * 16 * W, dtype=torch.int32, device=dev)   # 256 tables of 16 bands x 640 words: 10.5 MB
    res["compose_256_ms"] = clock(lambda k: set_boxes(k % RING))
    res["fill_10p5MB_ms"] = clock(lambda k: table.fill_(k))
    res["table_bytes"] = int(table.numel() * 4)
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
    order = "pnpnpnu" if a.parent_lib else "nnnu"
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
    g = {m: [r["tracker_gpu_ms"] for r in rs] for m, rs in runs.items() if m != "u"}
    res["unused_ms"] = g["n"]
    res["unused_mean_ms"] = sum(g["n"]) / len(g["n"])
    if g["p"]:
        res["parent_ms"] = g["p"]
        res["parent_mean_ms"] = sum(g["p"]) / len(g["p"])
        res["parent_spread_ms"] = max(g["p"]) - min(g["p"])
        res["unused_bar_ms"] = res["parent_mean_ms"] + res["parent_spread_ms"]
        res["unused_within_bar"] = res["unused_mean_ms"] <= res["unused_bar_ms"]
    u = runs["u"][0]
    res["used"] = u
    res["used_bar_ratio"] = 0.5
    res["used_within_bar"] = u["ratio_to_mask_setter"] <= 0.5
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
