#!/usr/bin/env python3
"""What device frames by reference cost the tracker (profiles/frame_refs_measure.json; profiles/README.md "Frames by reference").

256 sequences, the benchmark's device-resident VGA frames (bench.make_frames, 24 frames walked forwards and backwards), 150 features / min_dist 30, profiling
on: ms_total_gpu of gf_tracker_stats per frame over 150 frames behind 4 warm-up ones.  Every measurement is a fresh process under a time limit of its own; the
driver never opens the GPU and stops at the first measurement that fails.

  p  the parent commit's library (--parent-lib), the tight entry point gf_tracker_track_batch_device
  t  this library, the same call                                                  (a) t against p: three alternating runs each, medians; margin = max - min of p
  r  this library, gf_tracker_track_batch_device_refs, every frame an allocation of its own at a 16-byte-aligned base, pitch = width
                                                                                  (b) r against t, the same margin
  u  the same with every frame at base + 1 and a pitch of width + 37: the unaligned load form of the head kernel      (d) recorded; pyramid_ms says where
  c  what a caller pays today, wall clock per frame: 256 frames that lie in surfaces of their own (pitch 768) gathered into one tight buffer with one
     hipMemcpy2DAsync each and handed to the tight entry point, next to the _refs call on the same surfaces           (c) the ratio, recorded

    python scripts/frame_refs_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/frame_refs_measure.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
N_FRAMES, WARM, TIMED = 24, 4, 150
MAX_CNT, MIN_DIST = 150, 30


def frame_of(k):
    m = k % (2 * N_FRAMES - 2)
    return m if m < N_FRAMES else 2 * N_FRAMES - 2 - m


def scattered(torch, frames, offset, pitch):
    """every frame of [n, B, H, W] in an allocation of its own, row 0 at byte `offset`, rows `pitch` bytes apart: ([n][B] (address, pitch), the tensors)"""
    keep, refs = [], []
    for k in range(frames.shape[0]):
        row = []
        for b in range(frames.shape[1]):
            buf = torch.empty(offset + H * pitch, dtype=torch.uint8, device=frames.device)
            buf[offset:].view(H, pitch)[:, :W].copy_(frames[k, b])
            keep.append(buf)
            row.append((buf.data_ptr() + offset, pitch))
        refs.append(row)
    return refs, keep


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import ctypes as C
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    refs = None
    if mode in "ruc":
        refs, keep = scattered(torch, frames, 1 if mode == "u" else 0, {"r": W, "u": W + 37, "c": 768}[mode])
    drefs = gfamd.frame_refs([(depth.data_ptr() + b * H * W * 2, W * 2) for b in range(B)])
    tables = None if refs is None else [gfamd.frame_refs(r) for r in refs]      # built once, as a producer with a fixed pool of surfaces would
    torch.cuda.synchronize()

    def run(by_ref, gather=None):
        trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=MAX_CNT, min_dist=MIN_DIST))
        trk.set_profiling(True)
        wall = 0.0
        for k in range(WARM + TIMED):
            if k == WARM:
                trk.reset_stats()
                wall = 0.0
            ts, f = [k / 15.0] * B, frame_of(k)
            t0 = time.perf_counter()
            if by_ref:
                n = trk.trackImageBatchDeviceRefs(ts, tables[f], drefs, unpack=False)
            else:
                n = trk.trackImageBatchDevice(ts, gather(f) if gather else frames.data_ptr() + f * B * H * W, depth.data_ptr(), unpack=False)
            wall += time.perf_counter() - t0
        st = trk.stats()
        trk.close()
        return {"tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "pyramid_ms": st["ms_pyramid"] / TIMED, "lk_ms": st["ms_lk"] / TIMED, "detect_ms": st["ms_detect"] / TIMED,
                "wall_ms": 1e3 * wall / TIMED, "tracked_per_frame": st["tracked_features"] / TIMED / B, "features_last_frame": int(n.sum()),
                "frames_unaligned_per_frame": st.get("frames_unaligned", 0) / TIMED if by_ref else 0}

    if mode in "pt":
        return run(False)
    if mode in "ru":
        return run(True)
    # (c): the gather a caller writes today -- one pitched device copy per sequence into a tight buffer, then the tight entry point
    loaded = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l]      # the HIP runtime torch and the library already share: never a second copy
    hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    tight = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def gather(f):
        for b in range(B):
            if hip.hipMemcpy2DAsync(tight.data_ptr() + b * H * W, W, refs[f][b][0], refs[f][b][1], W, H, 3, None) != 0:     # 3: hipMemcpyDeviceToDevice
                raise SystemExit("hipMemcpy2DAsync failed")
        if hip.hipStreamSynchronize(None) != 0:      # the tracker's stream does not wait for the null stream
            raise SystemExit("hipStreamSynchronize failed")
        return tight.data_ptr()

    g, r = run(False, gather), run(True)
    return {"gather_then_tight": g, "by_reference": r, "wall_ratio": g["wall_ms"] / r["wall_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=3, help="alternating runs of p, t and r each")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    order = ("ptr" if a.parent_lib else "tr") * a.runs + "uc"
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
    res = {"order": order, "timed_frames": TIMED, "sequences": B, "max_cnt": MAX_CNT, "min_dist": MIN_DIST, "runs": runs}
    g = {m: [r["tracker_gpu_ms"] for r in runs[m]] for m in "ptr" if m in runs}
    med = {m: statistics.median(v) for m, v in g.items()}
    res["median_ms"] = med
    if "p" in g:
        margin = max(g["p"]) - min(g["p"])
        res["parent_ms"], res["margin_ms"] = g["p"], margin
        res["a_tight_this_minus_parent_ms"] = med["t"] - med["p"]
        res["a_inside_margin"] = med["t"] <= med["p"] + margin
        res["b_refs_minus_tight_ms"] = med["r"] - med["t"]
        res["b_inside_margin"] = med["r"] <= med["t"] + margin
    u = runs["u"][0]
    res["d_unaligned_ms"] = u["tracker_gpu_ms"]
    res["d_unaligned_pyramid_ms"] = u["pyramid_ms"]
    res["d_aligned_pyramid_ms"] = statistics.median(r["pyramid_ms"] for r in runs["r"])
    res["c_wall_ms"] = {"gather_then_tight": runs["c"][0]["gather_then_tight"]["wall_ms"], "by_reference": runs["c"][0]["by_reference"]["wall_ms"], "ratio": runs["c"][0]["wall_ratio"]}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
