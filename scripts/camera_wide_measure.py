#!/usr/bin/env python3
"""What the PINHOLE_FULL and SCARAMUZZA cameras cost (profiles/camera_wide_measure.json; profiles/README.md "Wide camera models").

Every measurement is a fresh process under a time limit of its own; the driver never opens the GPU and stops at the first measurement that fails.  Parent and
this commit alternate.  The tracker runs are those of scripts/camera_models_measure.py (256 VGA sequences, 150 features, min_dist 30, the benchmark's
device-resident frames, 200 timed frames behind 4 warm-up ones), the registration runs those of scripts/depth_reg_measure.py (its shape `a`: 256 VGA depth frames
to VGA colour, 40 timed calls).

  p / n  a handle that sets no camera, the parent's library (--parent-lib) / this one: ms_total_gpu per frame.  Bar: the parent's mean plus its own spread.
  K / k  256 KANNALA_BRANDT sequences, parent / this one -- the shared lift kernel now holds two more models: ms_total_gpu and the wall time per tracker call.
         Same bar, on ms_total_gpu.
  f / F  256 PINHOLE_FULL sequences lifted on the device (GF_CAMERA_LIFT_HOST=0) / on the host (=1): wall time of a tracker call.  s / S: the same for SCARAMUZZA.
  R / r  256 registrations onto PINHOLE colour cameras, parent / this one: hipEvent time of the two kernels per call.  Bar: the parent's mean plus its spread.
  q      the same 256 registrations onto PINHOLE_FULL colour cameras (this commit): a figure without a bar.

    python scripts/camera_wide_measure.py --parent-lib /path/to/parent/libgroundfusion_hip.so --out profiles/camera_wide_measure.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ground-fusion_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]
FULL = dict(proj=[504.5, 504.75, 322.5, 241.25], dist=[0.52, -2.7, 4e-4, -1.5e-4, 1.5, 0.4, -2.5, 1.4])      # the fixture's full_kinect8
SCA = dict(poly=[-241.5, 0.0, 1.4e-3, -1.5e-7, 2.5e-9], inv_poly=[380.0, 240.0, 14.0, 5.0, 8.0, 2.0], affine=[1.0005, 2e-4, -3e-4, 318.5, 241.25])
KINECT8_TAIL = (1.5, 0.4, -2.5, 1.4)


def tracker(cam):
    """camera_models_measure.tracker with any camera on every sequence"""
    import torch
    import bench
    import gfamd
    import camera_models_measure as cm
    frames, depth = bench.make_frames(cm.N_FRAMES, cm.B, 1000, torch.device("cuda:0"))
    torch.cuda.synchronize()
    trk = gfamd.FeatureTracker(gfamd.default_cfg(batch=cm.B, max_cnt=150, min_dist=30))
    for b in range(cm.B):
        trk.set_seq_camera(b, cam)
    trk.set_profiling(True)
    wall = 0.0
    for k in range(cm.WARM + cm.TIMED):
        if k == cm.WARM:
            trk.reset_stats()
            wall = 0.0
        t0 = time.perf_counter()
        n = trk.trackImageBatchDevice([k / 15.0] * cm.B, frames.data_ptr() + cm.frame_of(k) * cm.B * cm.H * cm.W, depth.data_ptr(), unpack=False)
        wall += time.perf_counter() - t0
    st = trk.stats()
    return {"tracker_gpu_ms": st["ms_total_gpu"] / cm.TIMED, "detect_ms": st["ms_detect"] / cm.TIMED, "host_post_ms": st["ms_host_post"] / cm.TIMED,
            "call_wall_ms": 1000.0 * wall / cm.TIMED, "features_last_frame": int(n.sum())}


def registration_full():
    """depth_reg_measure.used("a") with the colour camera's eight coefficients: PINHOLE_FULL"""
    import numpy as np
    import torch
    import gfamd
    import synth
    import depth_reg_measure as dm
    import depth_reg_ref as ref
    (wd, hd), (wc, hc) = dm.SHAPES["a"]
    fc, fd = 0.94 * wc, 0.94 * wd
    proj, dist = (fc, fc, wc / 2 - 0.3, hc / 2 + 0.4), (0.08, -0.12, 0.0006, -0.0004) + KINECT8_TAIL
    reg = ref.make_reg(wd, hd, fd, fd, wd / 2 + 0.2, hd / 2 - 0.1, 0.001, ref.rot(0.004, -0.003, 0.002), (0.015, 0.0004, -0.0003))
    cfg = gfamd.default_cfg(width=wc, height=hc, batch=dm.B, max_cnt=150, min_dist=30)
    trk = gfamd.FeatureTracker(cfg)
    gray = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in synth.tracker_sequence(3100, dm.USED_FRAMES, wc, hc)]
    raw = torch.from_numpy(ref.scene(wd, hd, 0.001, 11).view(np.int16)).cuda().unsqueeze(0).repeat(dm.B, 1, 1).contiguous()
    dreg, cam = gfamd.DepthReg.make(wd, hd, reg["fx"], reg["fy"], reg["cx"], reg["cy"], reg["scale"], reg["R"], reg["T"]), gfamd.CameraModelEx.make("PINHOLE_FULL", proj, dist)
    for b in range(dm.B):
        trk.set_seq_camera(b, cam)
        trk.set_seq_depth_reg(b, dreg)
    trk.set_profiling(True)
    depth_refs = gfamd.frame_refs([(raw[b].data_ptr(), 2 * wd) for b in range(dm.B)])
    for k in range(dm.USED_WARM + dm.USED_TIMED):
        if k == dm.USED_WARM:
            trk.reset_stats()
        g = gfamd.frame_refs([(gray[dm.frame_of(k, dm.USED_FRAMES)].data_ptr(), wc)] * dm.B)
        n = trk.trackImageBatchDeviceRefs([k / 15.0] * dm.B, g, depth_refs, unpack=False)
    st, rs = trk.stats(), trk.depth_reg_stats()
    return {"features_last_frame": int(n.sum()), "tracker_gpu_ms": st["ms_total_gpu"] / dm.USED_TIMED, "reg_launches": rs["launches"], "reg_frames": rs["frames"],
            "reg_kernels_ms": rs["kernel_ms"] / dm.USED_TIMED}


def one(mode):
    import gfamd
    if mode in "pn":
        import camera_models_measure as cm
        return cm.tracker(False)
    if mode in "Kk":
        import camera_models_measure as cm
        return cm.tracker(True)
    if mode in "fF":
        return tracker(gfamd.CameraModelEx.make("PINHOLE_FULL", **FULL))
    if mode in "sS":
        return tracker(gfamd.CameraModelEx.make("SCARAMUZZA", **SCA))
    if mode in "Rr":
        import depth_reg_measure as dm
        return dm.used("a")
    return registration_full()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--pairs", type=int, default=3, help="pairs of each alternating comparison")
    ap.add_argument("--limit", type=int, default=150, help="time limit of one measurement [s]")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one)))
        return
    if not a.parent_lib:
        raise SystemExit("--parent-lib: the bars come from the parent commit's library")
    order = ("pn" + "Kk" + "fF" + "sS" + "Rr") * max(a.pairs, 3) + "q" * max(a.pairs, 3)
    runs = {m: [] for m in sorted(set(order))}
    for m in order:
        env = dict(os.environ)
        if m in "pKR":
            env["GF_LIB_PATH"] = os.path.abspath(a.parent_lib)
        if m in "fFsS":
            env["GF_CAMERA_LIFT_HOST"] = "1" if m in "FS" else "0"
        out = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", m], env=env, capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit("measurement %s failed with status %d, nothing more is started:\n%s" % (m, out.returncode, out.stderr[-2000:]))
        r = json.loads(out.stdout.strip().splitlines()[-1])
        runs[m].append(r)
        print(m, json.dumps(r), flush=True)
    res = {"order": order, "runs": runs}

    def held(name, parent, child, key):
        p, c = [r[key] for r in runs[parent]], [r[key] for r in runs[child]]
        mean, spread = sum(p) / len(p), max(p) - min(p)
        res[name] = {"key": key, "parent": p, "parent_mean": mean, "parent_spread": spread, "bar": mean + spread, "this": c, "this_mean": sum(c) / len(c),
                     "meets_bar": sum(c) / len(c) <= mean + spread}
    held("nothing_set", "p", "n", "tracker_gpu_ms")
    held("shared_kernel_kannala_brandt", "K", "k", "tracker_gpu_ms")
    held("shared_kernel_kannala_brandt_call", "K", "k", "call_wall_ms")
    held("registration_pinhole", "R", "r", "reg_kernels_ms")
    for name, dev, host in (("pinhole_full", "f", "F"), ("scaramuzza", "s", "S")):
        d, h = [r["call_wall_ms"] for r in runs[dev]], [r["call_wall_ms"] for r in runs[host]]
        md, mh = sum(d) / len(d), sum(h) / len(h)
        res["lift_" + name] = {"device_call_wall_ms": d, "host_call_wall_ms": h, "device_mean": md, "host_mean": mh, "device_faster_by_ms": mh - md,
                               "device_wins": mh - md > max(max(d) - min(d), max(h) - min(h))}
    q = [r["reg_kernels_ms"] for r in runs["q"]]
    res["registration_pinhole_full"] = {"reg_kernels_ms": q, "mean": sum(q) / len(q)}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
