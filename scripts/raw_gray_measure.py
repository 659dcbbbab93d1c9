#!/usr/bin/env python3
"""What the raw-format conversions cost (profiles/raw_gray_measure.json; profiles/README.md "Raw frames").

1. The conversion kernels alone: 256 frames of 640 x 480, resident on the device, gf_cvt_gray_batch_device timed with device events around each launch; after
   a warm-up the formats take turns (rgb8, the four Bayer patterns, the two YUV orders, mono16, rgb8, ...) within this process, 60 launches each.  rgb8 is the
   kernel the colour-frame change brought and this change does not touch: its median is the bar for every raw format, which moves half (Bayer: 157 MB) or
   three quarters (YUV 4:2:2, MONO16: 236 MB) of rgb8's 315 MB.  Reported per format: median, minimum, maximum, bytes over the median, and that rate's share of
   the achievable HBM rate.
2. The whole frame: ms_total_gpu per frame of a bayer_rggb8 handle against a MONO8 handle that is given the converted frames (configs[1]: 150 features,
   min_dist 30, 256 sequences, profiling on), as a figure.

One command; it fails without a device.

    python scripts/raw_gray_measure.py --out profiles/raw_gray_measure.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 256, 640, 480
WARM, TIMED = 5, 60
HBM_ACHIEVABLE = 6.3e12     # bytes per second, a streaming kernel on the MI355X (8 TB/s peak)
T_WARM, T_TIMED = 3, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd")]
    import numpy as np
    import torch
    import gfamd
    if gfamd.device_count() < 1:
        raise SystemExit("raw_gray_measure: no HIP device")
    import bench
    dev = torch.device("cuda:0")
    formats = [("rgb8", gfamd.PIX_RGB8, 3)] + [(e, f, gfamd.PIX_RAW_BYTES[f]) for e, f in gfamd.PIX_RAW_OF_ENCODING.items()]
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    src = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, device=dev, generator=gen)
    dst = torch.zeros(B * H * W, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ms = {e: [] for e, _, _ in formats}
    for it in range(WARM + TIMED):
        for e, f, bpp in formats:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            gfamd.cvt_gray_device(src.data_ptr(), W * bpp, f, dst.data_ptr(), B, W, H)
            t1.record()
            t1.synchronize()
            if it >= WARM:
                ms[e].append(t0.elapsed_time(t1))
    res = {"batch": B, "width": W, "height": H, "launches_per_format": TIMED, "kernels": {}}
    bar = statistics.median(ms["rgb8"])
    for e, f, bpp in formats:
        med = statistics.median(ms[e])
        nbytes = B * W * H * (bpp + 1)
        res["kernels"][e] = {"ms_median": med, "ms_min": min(ms[e]), "ms_max": max(ms[e]), "bytes": nbytes, "bytes_per_s": nbytes / (med * 1e-3),
                             "share_of_achievable_hbm": nbytes / (med * 1e-3) / HBM_ACHIEVABLE, "bar_ms": bar, "bar_met": bool(med <= bar)}
        print(e, json.dumps(res["kernels"][e]), flush=True)
    del src, dst
    # ---- the whole frame
    n = T_WARM + T_TIMED
    frames, depth = bench.make_frames(n, B, 1000, dev)          # textured frames, read as mosaics
    gray = torch.empty_like(frames)
    torch.cuda.synchronize()
    for k in range(n):
        gfamd.cvt_gray_device(frames.data_ptr() + k * B * H * W, W, gfamd.PIX_BAYER_RGGB8, gray.data_ptr() + k * B * H * W, B, W, H)
    torch.cuda.synchronize()
    for name, fmt, buf in (("bayer_rggb8", gfamd.PIX_BAYER_RGGB8, frames), ("mono8", gfamd.PIX_MONO8, gray)):
        trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=B, max_cnt=150, min_dist=30, pixel_format=fmt))
        trk.set_profiling(True)
        fewest = 150
        for k in range(n):
            if k == T_WARM:
                trk.reset_stats()
            cnt = trk.trackImageBatchDevice([k / 15.0] * B, buf.data_ptr() + k * B * H * W, depth.data_ptr(), unpack=False)
            fewest = min(fewest, int(np.min(cnt)))
        st = trk.stats()
        res["tracker_" + name] = {"ms_total_gpu_per_frame": st["ms_total_gpu"] / T_TIMED, "ms_convert_per_frame": st["ms_convert"] / T_TIMED,
                                  "output_per_frame": st["output_features"] / T_TIMED / B, "fewest_features": fewest}
        print("tracker", name, json.dumps(res["tracker_" + name]), flush=True)
        trk.close()
    print(json.dumps({"bars_met": {e: v["bar_met"] for e, v in res["kernels"].items()}}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
