#!/usr/bin/env python3
"""What a pixel format per sequence costs (profiles/seq_format_measure.json; profiles/README.md "Formats per sequence").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.

  p / n  a handle that sets nothing: the parent commit's library (--parent-lib) and this one alternating (p n p n p n), 256 VGA sequences, configs[1] (150
         features, min_dist 30), the benchmark's device-resident frames, profiling on: ms_total_gpu of gf_tracker_stats per frame over 200 frames behind 4
         warm-up ones.  The bar comes from the parent alone: the mean of its runs plus the larger of 1 % and its own spread; the mean of the (n) runs is held
         against it.
  k      the kernel: gf_cvt_gray_mixed_device on 256 VGA frames that all have one format against gf_cvt_gray_batch_device on the same frames, for BGR8,
         BAYER_RGGB8 and YUV422_UYVY: device events, 5 warm-up rounds, 5 windows of 60 launches, the formats and the two entry points taking turns in one process
  m      one handle of 256 VGA sequences, 64 each MONO8, BAYER_RGGB8, YUV422_UYVY and BGR8 (b % 4), the second and fourth equalised
  w x y z  four homogeneous handles of 64 sequences with those settings on the frames the same sequences see in (m): their sum is what the fleet pays today

    python scripts/seq_format_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/seq_format_measure.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
N_FRAMES, WARM, TIMED = 24, 4, 200
FLEET = [(0, 0), (8, 1), (12, 0), (2, 1)]      # (pixel_format, equalize) of sequence b % 4: MONO8, BAYER_RGGB8 + CLAHE, YUV422_UYVY, BGR8 + CLAHE
KERNEL_FORMATS = [("bgr8", 2, 3), ("bayer_rggb8", 8, 1), ("yuv422_uyvy", 12, 2)]


def frame_of(k):
    m = k % (2 * N_FRAMES - 2)
    return m if m < N_FRAMES else 2 * N_FRAMES - 2 - m


def unset():
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
    return {"sequences": B, "tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "pyramid_ms": st["ms_pyramid"] / TIMED, "lk_ms": st["ms_lk"] / TIMED,
            "detect_ms": st["ms_detect"] / TIMED, "features_last_frame": int(n.sum())}


def encode_on_device(gray, fmt):
    """[n, H, W] u8 device frames -> frames of format fmt with the same luma texture (flat u8 tensor)"""
    import torch
    if fmt == 0 or fmt == 8:
        return gray.contiguous().reshape(-1)      # a mosaic of a gray scene: every site holds the gray value
    if fmt == 12:
        return torch.stack([torch.full_like(gray, 128), gray], dim=-1).contiguous().reshape(-1)
    return torch.stack([gray, gray, gray], dim=-1).contiguous().reshape(-1)


def fleet(mode):
    import numpy as np
    import torch
    import bench
    import gfamd
    dev = torch.device("cuda:0")
    frames, depth = bench.make_frames(N_FRAMES, B, 1000, dev)
    which = None if mode == "m" else "wxyz".index(mode)
    seqs = list(range(B)) if which is None else list(range(which, B, 4))
    nb = len(seqs)
    own = (0, 0) if which is None else FLEET[which]
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=nb, max_cnt=150, min_dist=30, pixel_format=own[0], equalize=own[1]))
    trk.set_profiling(True)
    if which is None:
        for b in range(B):
            if FLEET[b % 4] != (0, 0):
                trk.set_seq_format(b, FLEET[b % 4][0], FLEET[b % 4][1])
    # the frames of every step, each sequence in its format, back to back in list order
    blocks = []
    for f in range(N_FRAMES):
        blocks.append(torch.cat([encode_on_device(frames[f, b:b + 1], FLEET[b % 4][0]) for b in seqs]))
    dd = depth[torch.tensor(seqs, device=dev)].contiguous()
    torch.cuda.synchronize()
    for k in range(WARM + TIMED):
        if k == WARM:
            trk.reset_stats()
        n = trk.trackImageBatchDevice([k / 15.0] * nb, blocks[frame_of(k)].data_ptr(), dd.data_ptr(), unpack=False)
    st = trk.stats()
    return {"sequences": nb, "tracker_gpu_ms": st["ms_total_gpu"] / TIMED, "convert_ms": st["ms_convert"] / TIMED, "equalize_ms": st["ms_equalize"] / TIMED,
            "pyramid_ms": st["ms_pyramid"] / TIMED, "host_pre_ms": st["ms_host_pre"] / TIMED, "features_last_frame": int(np.sum(n))}


def kernel():
    import numpy as np
    import torch
    import gfamd
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    dst = torch.zeros(B * H * W, dtype=torch.uint8, device=dev)
    cases = []
    for name, fmt, bpp in KERNEL_FORMATS:
        src = torch.randint(0, 256, (B * H * W * bpp,), dtype=torch.uint8, device=dev, generator=gen)
        refs = np.zeros((B, 2), np.uint64)
        refs[:, 0] = src.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(H * W * bpp)
        refs[:, 1] = W * bpp
        cases.append((name, fmt, bpp, src, torch.from_numpy(refs.view(np.int64)).to(dev), torch.full((B,), fmt, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()

    def launch(case, mixed):
        name, fmt, bpp, src, d_refs, d_fmt = case
        if mixed:
            gfamd.cvt_gray_mixed_device(d_refs.data_ptr(), d_fmt.data_ptr(), dst.data_ptr(), B, W, H)
        else:
            gfamd.cvt_gray_device(src.data_ptr(), W * bpp, fmt, dst.data_ptr(), B, W, H)

    out = {c[0]: {"batch_us": [], "mixed_us": []} for c in cases}
    for c in cases:                                   # the two entry points give the same bytes
        launch(c, False)
        a = dst.clone()
        dst.zero_()
        launch(c, True)
        torch.cuda.synchronize()
        assert torch.equal(a, dst), c[0]
    for _ in range(5):
        for c in cases:
            launch(c, False)
            launch(c, True)
    torch.cuda.synchronize()
    for _ in range(5):
        for c in cases:
            for mixed in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(60):
                    launch(c, mixed)
                e1.record()
                e1.synchronize()
                out[c[0]]["mixed_us" if mixed else "batch_us"].append(e0.elapsed_time(e1) * 1000.0 / 60)
    for v in out.values():
        v["batch_median_us"], v["mixed_median_us"] = sorted(v["batch_us"])[2], sorted(v["mixed_us"])[2]
        v["mixed_over_batch"] = v["mixed_median_us"] / v["batch_median_us"]
    return out


def one(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    if mode in "pn":
        return unset()
    if mode == "k":
        return kernel()
    return fleet(mode)


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
    order = "pn" * max(a.pairs, 2) + "kmwxyz"
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
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
    res = {"order": order, "timed_frames": TIMED, "runs": runs}
    p, n = [r["tracker_gpu_ms"] for r in runs["p"]], [r["tracker_gpu_ms"] for r in runs["n"]]
    if p:
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res["parent_ms"], res["parent_mean_ms"], res["parent_spread_ms"] = p, mean, spread
        res["bar_ms"] = mean + max(0.01 * mean, spread)
    res["unset_ms"], res["unset_mean_ms"] = n, sum(n) / len(n)
    if p:
        res["unset_meets_bar"] = res["unset_mean_ms"] <= res["bar_ms"]
    res["kernel"] = {k: {q: v[q] for q in ("batch_median_us", "mixed_median_us", "mixed_over_batch")} for k, v in runs["k"][0].items()}
    res["mixed_handle_ms"] = runs["m"][0]["tracker_gpu_ms"]
    res["four_handles_ms"] = {m: runs[m][0]["tracker_gpu_ms"] for m in "wxyz"}
    res["four_handles_sum_ms"] = sum(res["four_handles_ms"].values())
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
