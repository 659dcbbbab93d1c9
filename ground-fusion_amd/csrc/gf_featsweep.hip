// gf_featsweep.hip — the per-feature sweeps of the measurement side for many windows at once on the device:
//   FeatureManager::triangulateWithDepth   feature_manager.cpp:726-799   (depth of a track from its depth-camera observations, cross-checked between frames)
//   Estimator::movingConsistencyCheckW     estimator.cpp:3955-3995 with reprojectionError / reprojectionError3D :3899-3919
// One thread per feature.  The arithmetic of a track is gf_featsweep.hpp, the source the estimator's host loops (gf_estimator.hip) compile too, both without
// contraction: decisions and depths are bit-identical to the host's.
// Building blocks with their own C-ABI; the estimator keeps these sweeps on its host threads (0.03 ms of one core per frame, and a device launch
// would need one more rendezvous of the group's threads).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/groundfusion_hip.h"
#include "gf_featsweep.hpp"
#include "gf_hip_own.hpp"

using namespace gfd;

namespace {
struct SweepArgs {
    int B, W, F;
    const double *Rs, *Ps, *tic, *ric;          // per window: (W+1) x 9, (W+1) x 3, 3, 9
    const int *first_feature, *start_frame, *first_obs;
    const double* obs;                          // per observation: x, y, z of the normalised point, depth-camera depth
    double* estimated_depth; int* estimate_flag; int* remove;
    double depth_threshold, init_depth, focal_length;
    const double* par;                          // per window: depth_threshold, init_depth, focal_length (the windows of estimators that differ in them); null: the three above
};
struct FlatObs {   // a track's rows of the [x, y, z, depth] table
    const double* p;
    GFD V3 point(int k) const { return arr3(p + 4 * (size_t)k); }
    GFD double depth(int k) const { return p[4 * (size_t)k + 3]; }
};
__device__ int window_of(const int* first_feature, int B, int f) {   // largest b with first_feature[b] <= f
    int lo = 0, hi = B - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first_feature[mid] <= f) lo = mid; else hi = mid - 1; }
    return lo;
}

__global__ void __launch_bounds__(128) triangulate_with_depth_kernel(SweepArgs A) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.F) return;
    const int b = window_of(A.first_feature, A.B, f);
    const int o0 = A.first_obs[f], n = A.first_obs[f + 1] - o0, s = A.start_frame[f];
    if (n < 4) return;
    if (A.estimated_depth[f] > 0) return;
    double e; int flag;
    const double depth_threshold = A.par ? A.par[3 * b] : A.depth_threshold, init_depth = A.par ? A.par[3 * b + 1] : A.init_depth;
    if (!track_depth_from_camera(FlatObs{A.obs + 4 * (size_t)o0}, n, s, A.Rs + (size_t)b * (A.W + 1) * 9, A.Ps + (size_t)b * (A.W + 1) * 3, arr3(A.tic + 3 * b), arr9(A.ric + 9 * b),
                                 depth_threshold, init_depth, e, flag)) return;
    A.estimated_depth[f] = e; A.estimate_flag[f] = flag;
}

__global__ void __launch_bounds__(128) moving_consistency_kernel(SweepArgs A) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.F) return;
    A.remove[f] = 0;
    const int b = window_of(A.first_feature, A.B, f);
    const int o0 = A.first_obs[f], n = A.first_obs[f + 1] - o0, wi = A.start_frame[f];
    if (!(n >= 2 && wi < A.W - 2)) return;
    const double depth = A.estimated_depth[f];
    if (depth < 0) return;
    if (track_is_moving(FlatObs{A.obs + 4 * (size_t)o0}, n, wi, A.Rs + (size_t)b * (A.W + 1) * 9, A.Ps + (size_t)b * (A.W + 1) * 3, arr3(A.tic + 3 * b), arr9(A.ric + 9 * b), depth,
                        A.par ? A.par[3 * b + 2] : A.focal_length)) A.remove[f] = 1;
}

// grown on demand, at least 64 elements at a time
template <class T> int fit64(gf::DevBuf<T>& b, size_t n) {
    if (n > b.n) HIPCHK(b.fit(std::max(n, (size_t)64)));
    return GF_OK;
}
}  // namespace

struct gf_featsweep {
    gf::Stream stream;
    gf::Event ev0, ev1;
    gf::DevBuf<double> Rs, Ps, tic, ric, obs, depth;
    gf::DevBuf<double> par; std::vector<double> h_par;   // allocated by the first *_each call; the host copy lives until the call's stream is synchronised
    gf::DevBuf<int> first_feature, start_frame, first_obs, flag, remove;
    double kernel_ms = 0; long long launches = 0, features = 0;
};

static int upload_common(gf_featsweep* h, SweepArgs& A, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                         const int* start_frame, const int* first_obs, const double* obs, const double* estimated_depth) {
    const int F = first_feature[B];
    if (F < 0 || (F > 0 && (!start_frame || !first_obs || !obs))) return gf::set_err(GF_ERR_INVALID, "%d features listed but start_frame / first_obs / obs is null", F);
    const size_t O = F > 0 ? (size_t)first_obs[F] : 0;
    for (int b = 0; b < B; b++) if (first_feature[b + 1] < first_feature[b]) return gf::set_err(GF_ERR_INVALID, "first_feature must not decrease");
    for (int f = 0; f < F; f++) {
        const int n = first_obs[f + 1] - first_obs[f];
        if (n < 0 || start_frame[f] < 0 || start_frame[f] + n > W + 1) return gf::set_err(GF_ERR_INVALID, "feature %d: %d observations from frame %d do not fit a window of %d frames", f, n, start_frame[f], W + 1);
    }
    if (int rc = fit64(h->Rs, (size_t)B * (W + 1) * 9)) return rc;
    if (int rc = fit64(h->Ps, (size_t)B * (W + 1) * 3)) return rc;
    if (int rc = fit64(h->tic, (size_t)B * 3)) return rc;
    if (int rc = fit64(h->ric, (size_t)B * 9)) return rc;
    if (int rc = fit64(h->obs, O * 4)) return rc;
    if (int rc = fit64(h->depth, F)) return rc;
    if (int rc = fit64(h->first_feature, B + 1)) return rc;
    if (int rc = fit64(h->start_frame, F)) return rc;
    if (int rc = fit64(h->first_obs, F + 1)) return rc;
    if (int rc = fit64(h->flag, F)) return rc;
    if (int rc = fit64(h->remove, F)) return rc;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(h->Rs.p, Rs, sizeof(double) * B * (W + 1) * 9, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->Ps.p, Ps, sizeof(double) * B * (W + 1) * 3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->tic.p, tic, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->ric.p, ric, sizeof(double) * B * 9, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->first_feature.p, first_feature, sizeof(int) * (B + 1), hipMemcpyHostToDevice, s));
    if (F > 0) {
        HIPCHK(hipMemcpyAsync(h->obs.p, obs, sizeof(double) * O * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->depth.p, estimated_depth, sizeof(double) * F, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->start_frame.p, start_frame, sizeof(int) * F, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->first_obs.p, first_obs, sizeof(int) * (F + 1), hipMemcpyHostToDevice, s));
    }
    A.B = B; A.W = W; A.F = F;
    A.Rs = h->Rs.p; A.Ps = h->Ps.p; A.tic = h->tic.p; A.ric = h->ric.p; A.first_feature = h->first_feature.p; A.start_frame = h->start_frame.p; A.first_obs = h->first_obs.p;
    A.obs = h->obs.p; A.estimated_depth = h->depth.p; A.estimate_flag = h->flag.p; A.remove = h->remove.p;
    return GF_OK;
}
// the windows' own depth_threshold / init_depth / focal_length (a null array leaves its column 0: the kernel that is launched does not read it)
static int upload_par(gf_featsweep* h, SweepArgs& A, int B, const double* depth_threshold, const double* init_depth, const double* focal_length) {
    if (int rc = fit64(h->par, (size_t)B * 3)) return rc;
    std::vector<double>& par = h->h_par;
    par.assign((size_t)B * 3, 0.0);
    for (int b = 0; b < B; b++) {
        if (depth_threshold) par[3 * b] = depth_threshold[b];
        if (init_depth) par[3 * b + 1] = init_depth[b];
        if (focal_length) par[3 * b + 2] = focal_length[b];
    }
    HIPCHK(hipMemcpyAsync(h->par.p, par.data(), sizeof(double) * B * 3, hipMemcpyHostToDevice, h->stream));
    A.par = h->par.p;
    return GF_OK;
}

static int triangulate_with_depth_run(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                      const int* start_frame, const int* first_obs, const double* obs, double depth_threshold, double init_depth,
                                      const double* depth_threshold_each, const double* init_depth_each, double* estimated_depth, int* estimate_flag) {
    if (!h || B < 1 || W < 1 || !Rs || !Ps || !tic || !ric || !first_feature || !first_obs || !estimated_depth || !estimate_flag) return gf::set_err(GF_ERR_INVALID, "bad argument");
    SweepArgs A{};
    if (int rc = upload_common(h, A, B, W, Rs, Ps, tic, ric, first_feature, start_frame, first_obs, obs, estimated_depth)) return rc;
    if (A.F == 0) return GF_OK;
    A.depth_threshold = depth_threshold; A.init_depth = init_depth;
    if (depth_threshold_each) if (int rc = upload_par(h, A, B, depth_threshold_each, init_depth_each, nullptr)) return rc;
    HIPCHK(hipMemcpyAsync(h->flag.p, estimate_flag, sizeof(int) * A.F, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    triangulate_with_depth_kernel<<<dim3((A.F + 127) / 128), 128, 0, h->stream>>>(A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(estimated_depth, h->depth.p, sizeof(double) * A.F, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(estimate_flag, h->flag.p, sizeof(int) * A.F, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->kernel_ms += ms;
    h->launches++; h->features += A.F;
    return GF_OK;
}
static int moving_consistency_run(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                  const int* start_frame, const int* first_obs, const double* obs, const double* estimated_depth, double focal_length,
                                  const double* focal_length_each, int* remove) {
    if (!h || B < 1 || W < 1 || !Rs || !Ps || !tic || !ric || !first_feature || !first_obs || !estimated_depth || !remove) return gf::set_err(GF_ERR_INVALID, "bad argument");
    SweepArgs A{};
    if (int rc = upload_common(h, A, B, W, Rs, Ps, tic, ric, first_feature, start_frame, first_obs, obs, estimated_depth)) return rc;
    if (A.F == 0) return GF_OK;
    A.focal_length = focal_length;
    if (focal_length_each) if (int rc = upload_par(h, A, B, nullptr, nullptr, focal_length_each)) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    moving_consistency_kernel<<<dim3((A.F + 127) / 128), 128, 0, h->stream>>>(A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(remove, h->remove.p, sizeof(int) * A.F, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->kernel_ms += ms;
    h->launches++; h->features += A.F;
    return GF_OK;
}

extern "C" {
int gf_featsweep_create(gf_featsweep** out) {
    if (!out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::require_device()) return rc;
    std::unique_ptr<gf_featsweep> h(new gf_featsweep());
    HIPCHK(hipStreamCreate(&h->stream.s)); HIPCHK(hipEventCreate(&h->ev0.e)); HIPCHK(hipEventCreate(&h->ev1.e));
    *out = h.release();
    return GF_OK;
}
int gf_featsweep_destroy(gf_featsweep* h) { delete h; return GF_OK; }
int gf_triangulate_with_depth_batch(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                    const int* start_frame, const int* first_obs, const double* obs, double depth_threshold, double init_depth, double* estimated_depth,
                                    int* estimate_flag) {
    return triangulate_with_depth_run(h, B, W, Rs, Ps, tic, ric, first_feature, start_frame, first_obs, obs, depth_threshold, init_depth, nullptr, nullptr, estimated_depth, estimate_flag);
}
int gf_triangulate_with_depth_batch_each(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                         const int* start_frame, const int* first_obs, const double* obs, const double* depth_threshold, const double* init_depth,
                                         double* estimated_depth, int* estimate_flag) {
    if (!depth_threshold || !init_depth) return gf::set_err(GF_ERR_INVALID, "depth_threshold / init_depth: one value per window expected, got a null array");
    return triangulate_with_depth_run(h, B, W, Rs, Ps, tic, ric, first_feature, start_frame, first_obs, obs, 0.0, 0.0, depth_threshold, init_depth, estimated_depth, estimate_flag);
}
int gf_moving_consistency_batch(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                const int* start_frame, const int* first_obs, const double* obs, const double* estimated_depth, double focal_length, int* remove) {
    return moving_consistency_run(h, B, W, Rs, Ps, tic, ric, first_feature, start_frame, first_obs, obs, estimated_depth, focal_length, nullptr, remove);
}
int gf_moving_consistency_batch_each(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                     const int* start_frame, const int* first_obs, const double* obs, const double* estimated_depth, const double* focal_length, int* remove) {
    if (!focal_length) return gf::set_err(GF_ERR_INVALID, "focal_length: one value per window expected, got a null array");
    return moving_consistency_run(h, B, W, Rs, Ps, tic, ric, first_feature, start_frame, first_obs, obs, estimated_depth, 0.0, focal_length, remove);
}
int gf_featsweep_stats(gf_featsweep* h, long long* launches, long long* features, double* kernel_ms) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (launches) *launches = h->launches;
    if (features) *features = h->features;
    if (kernel_ms) *kernel_ms = h->kernel_ms;
    return GF_OK;
}
}  // extern "C"
