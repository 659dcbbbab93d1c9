// gf_featsweep.hpp — the arithmetic of one feature track in the two per-feature sweeps of the measurement side:
//   FeatureManager::triangulateWithDepth   feature_manager.cpp:726-799   (depth of a track from its depth-camera observations, cross-checked between frames)
//   Estimator::movingConsistencyCheckW     estimator.cpp:3955-3995 with reprojectionError / reprojectionError3D :3899-3919
// One source for the estimator's host loops (gf_estimator.hip) and the batched kernels (gf_featsweep.hip); both compile it without contraction, so decisions and
// depths are bit-identical.  Obs gives the track's k-th observation: point(k), the normalised point, and depth(k), the depth camera's reading.  Rs / Ps are the
// window's poses as flat tables of 9 / 3 doubles per frame.  Which tracks are swept, and what is recorded about them, stays with the callers.
#pragma once
#include "gf_dmath.hpp"

namespace gfd {

// the track's n observations start at frame s; false: no pair of frames agrees, depth and flag stay as they are
template <class Obs> GFD bool track_depth_from_camera(const Obs& obs, int n, int s, const double* Rs, const double* Ps, V3 tic, const M3& ric, double depth_threshold,
                                                      double init_depth, double& estimated_depth, int& estimate_flag) {
    double depth_sum = 0.0; unsigned cnt = 0;
    const M3 Rs_s = arr9(Rs + 9 * s);
    const V3 tr = arr3(Ps + 3 * s) + Rs_s * tic; const M3 Rr = Rs_s * ric;
    for (int i = 0; i < n; i++) {
        const M3 Rsi = arr9(Rs + 9 * (s + i));
        const V3 t0 = arr3(Ps + 3 * (s + i)) + Rsi * tic; const M3 R0 = Rsi * ric;
        const double d = obs.depth(i);
        if (d < 0.1 || d > depth_threshold) continue;
        const V3 point0 = obs.point(i) * d;
        const V3 t2r = transpose(Rr) * (t0 - tr); const M3 R2r = transpose(Rr) * R0;
        for (int j = 0; j < n; j++) {
            if (i == j) continue;
            const M3 Rsj = arr9(Rs + 9 * (s + j));
            const V3 t1 = arr3(Ps + 3 * (s + j)) + Rsj * tic; const M3 R1 = Rsj * ric;
            const V3 t20 = transpose(R0) * (t1 - t0); const M3 R20 = transpose(R0) * R1;
            const V3 pp = transpose(R20) * point0 - transpose(R20) * t20;
            const V3 pj = obs.point(j);
            const double rx = pj.x - pp.x / pp.z, ry = pj.y - pp.y / pp.z;
            if (sqrt(rx * rx + ry * ry) < 10.0 / 460) { const V3 pr = R2r * point0 + t2r; depth_sum += pr.z; cnt++; }
        }
    }
    if (cnt == 0) return false;
    const double e = depth_sum / cnt;
    estimated_depth = e < 0.1 ? init_depth : e; estimate_flag = e < 0.1 ? 0 : 1;
    return true;
}

// the track's n >= 2 observations start at frame wi, where it has the depth `depth`; true: its mean reprojection error over the later frames marks it as moving
template <class Obs> GFD bool track_is_moving(const Obs& obs, int n, int wi, const double* Rs, const double* Ps, V3 tic, const M3& ric, double depth, double focal_length) {
    const M3 Ri = arr9(Rs + 9 * wi); const V3 Pi = arr3(Ps + 3 * wi);
    const V3 uvi = obs.point(0);
    double err = 0, err3D = 0; int errCnt = 0;
    for (int k = 1; k < n; k++) {
        const int wj = wi + k;
        const M3 Rj = arr9(Rs + 9 * wj); const V3 Pj = arr3(Ps + 3 * wj);
        const V3 uvj = obs.point(k);
        {   // reprojectionError
            const V3 pts_w = Ri * (ric * (uvi * depth) + tic) + Pi;
            const V3 pts_cj = transpose(ric) * (transpose(Rj) * (pts_w - Pj) - tic);
            const double rx = pts_cj.x / pts_cj.z - uvj.x, ry = pts_cj.y / pts_cj.z - uvj.y;
            err += sqrt(rx * rx + ry * ry);
        }
        {   // reprojectionError3D
            const V3 pts_w = Ri * (ric * (uvi * depth) + tic) + Pi;
            const V3 pts_cj = transpose(ric) * (transpose(Rj) * (pts_w - Pj) - tic);
            err3D += sqrt(sqn(pts_cj - uvj)) / depth;
        }
        errCnt++;
    }
    return errCnt > 0 && (focal_length * err / errCnt > 10 || err3D / errCnt > 2.0);
}

}  // namespace gfd
