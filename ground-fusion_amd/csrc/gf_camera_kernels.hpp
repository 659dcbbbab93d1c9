// gf_camera_kernels.hpp — liftProjective of camodocal's five camera models on the device (undistortedPts, feature_tracker.cpp:797-808): the formulas are
// gf_camera_models.hpp, one source with the host.  One thread per point.  A block of one wavefront takes a (list entry, set, chunk of 64 points) triple, so the
// camera and the branch on its model are wavefront-uniform: the entry's camera is read with scalar loads through an index every lane shares, as cvt_mixed_kernel
// reads its frame entry, and the turning table of a Kannala-Brandt camera, the eight coefficients of a PINHOLE_FULL one and the 11 doubles of a SCARAMUZZA
// one stay in scalar registers.  No LDS, no scratch ("Camera models", has the register counts).
#pragma once
#include <hip/hip_runtime.h>

#include "gf_camera_models.hpp"

namespace gfcam {

constexpr int kLiftThreads = 64;   // one wavefront: no wavefront spans two entries
__global__ __launch_bounds__(kLiftThreads) void camera_lift_kernel(const LiftArgs A) {
    const unsigned chunks = gridDim.x / (unsigned)A.n_sets, s = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const LiftSet S = A.set[s < (unsigned)kLiftSets ? s : 0];
    const Camera* cams = S.cams ? S.cams : A.cams;
    const int* cam_of = S.cams ? S.cam_of : A.cam_of;
    for (int b = blockIdx.y; b < A.batch; b += gridDim.y) {
        const int q = cam_of ? cam_of[b] : b;
        if (q < 0) continue;
        const Camera& cam = cams[q];
        size_t at; int n;
        if (A.first) { at = (size_t)A.first[b]; n = A.first[b + 1] - A.first[b]; }
        else { at = (size_t)b * A.cap; n = S.n ? min(S.n[b], A.cap) : 0; }
        for (int i = (int)(chunk * kLiftThreads + threadIdx.x); i < n; i += (int)(chunks * kLiftThreads)) {
            const Pair p = S.pts[at + i];
            double P[3]; Pair o;
            lift_pair(cam, (double)p.x, (double)p.y, P, o.x, o.y);
            S.un[at + i] = o;
            if (S.rays) { double* r = S.rays + 3 * (at + i); r[0] = P[0]; r[1] = P[1]; r[2] = P[2]; }
        }
    }
}

// chunks per set for entries of at most max_n points, and the grid
inline dim3 lift_grid(int max_n, int n_sets, int batch) {
    const unsigned chunks = (unsigned)((max_n > 0 ? max_n : 1) + kLiftThreads - 1) / kLiftThreads;
    return dim3(chunks * (unsigned)n_sets, (unsigned)(batch < 65535 ? batch : 65535));
}

}  // namespace gfcam
