"""A Kannala-Brandt sequence through the tracker's host bookkeeping without a GPU: tests/native/camera_track_host.cpp runs the CPU tracker made of the stage
functions of csrc/gf_track_host.hpp (the oracle's LK, circle and corner primitives in the place of the kernels) with a pinhole, with a Kannala-Brandt camera whose
pairs are picked from per-row tables as the lift kernel leaves them, and with the same camera lifted on the host; it demands ids, track counts, pixel coordinates,
depths and predictions bit for bit equal in all three, under the address and undefined-behaviour sanitizers.  Here its reported pairs are held to the 60-digit
formulas of tests/golden/make_camera_golden.py at the fixture's bars, and its velocities to ptsVelocity (feature_tracker.cpp:810-847) recomputed from those pairs."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np

import roi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, RANDOMS = 5, 512
W, H, MAX_CNT, MIN_DIST = RR.SIZES[2]


def test_kannala_brandt_sequence_on_the_cpu_tracker(tmp_path):
    exe, frames, dump = tmp_path / "camera_track_host", tmp_path / "frames.bin", tmp_path / "obs.bin"
    flags = [f for f in RR._makefile_flags() if f not in ("-O3", "-fPIC")]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-O1", "-g", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "camera_track_host.cpp"),
                           os.path.join(ROOT, "oracle", "tracker_oracle.cpp")])
    rng = np.random.default_rng(9)
    with open(frames, "wb") as f:
        f.write(np.array([W, H, FRAMES, RANDOMS], np.int32).tobytes())
        f.write(np.stack(RR.frames(W, H, n=FRAMES, seed=0)).astype(np.uint8).tobytes())
        f.write(np.stack([RR.depth(k, W, H) for k in range(FRAMES)]).tobytes())
        f.write(RR.region("A", W, H).tobytes())
        for _ in range(FRAMES):
            f.write(np.concatenate([rng.random(RANDOMS), rng.random(RANDOMS), rng.normal(0, 1, RANDOMS)]).astype(np.float64).tobytes())
    out = subprocess.run([str(exe), str(frames), str(MAX_CNT), str(MIN_DIST), str(dump)], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout
    proj = [float.fromhex(x) for x in [l for l in out.stdout.splitlines() if l.startswith("camera ")][0].split()[1:]]
    dist = [-0.9, 0.35, -0.05, 0.0025]

    import mpmath as mp
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_camera_golden as G
    mp.mp.dps = 15      # the generator sets its own precision when imported
    eps_d = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "camera_models.json.gz")).read())["eps_d"]
    raw = open(dump, "rb").read()
    at, prev, prev_t, seen, worst, several = 0, None, None, 0, 0.0, 0
    for k in range(FRAMES):
        n = int(np.frombuffer(raw, np.int32, 1, at)[0]); t = float(np.frombuffer(raw, np.float64, 1, at + 4)[0]); at += 12
        rec = np.frombuffer(raw, np.dtype([("id", "<i4"), ("v", "<f8", 8)]), n, at); at += n * 68
        ids, v = rec["id"], rec["v"]
        assert n > 0 and (v[:, 0:2] == v[:, 0:2].astype(np.float32)).all() and (v[:, 2] == 1).all()
        un = v[:, 0:2].astype(np.float32)
        with mp.workdps(60):
            for i in range(n):
                P, rho, theta, nroots = G.kb_lift(proj, dist, float(v[i, 3]), float(v[i, 4]))
                several += nroots > 1
                if abs(P[2]) / mp.sqrt(P[0] ** 2 + P[1] ** 2 + P[2] ** 2) < 0.05:
                    continue
                for j in range(2):
                    exact = P[j] / P[2]
                    hi = float(exact)
                    half_ulp = float(np.ldexp(0.5, int(np.floor(np.log2(max(abs(hi), float(np.finfo(np.float32).tiny))))) - 23))
                    err, bar = float(abs(mp.mpf(float(un[i, j])) - exact)), half_ulp + eps_d * max(1.0, abs(hi))
                    worst = max(worst, err / bar)
                    assert err <= bar, "frame %d, feature %d: pair[%d] = %r, the formulas give %r: off by %.3g, bar %.3g" % (k, ids[i], j, float(un[i, j]), hi, err, bar)
                    seen += 1
        want = np.zeros((n, 2), np.float32)
        if prev is not None:
            dt = np.float64(t) - np.float64(prev_t)
            for i in range(n):
                if int(ids[i]) in prev:
                    want[i] = ((un[i] - prev[int(ids[i])]).astype(np.float64) / dt).astype(np.float32)
        assert np.array_equal(v[:, 5:7].astype(np.float32).view(np.uint32), want.view(np.uint32)) and (v[:, 5:7] == v[:, 5:7].astype(np.float32)).all(), "frame %d: velocities" % k
        prev, prev_t = {int(f): un[i] for i, f in enumerate(ids)}, t
    assert at == len(raw) and seen > 2 * FRAMES * MAX_CNT * 0.9 and several > 0
    print("pairs within %.3g of their bar (%d compared, %d features where the polynomial has several roots)" % (worst, seen, several))
