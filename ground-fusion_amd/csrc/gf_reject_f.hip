// gf_reject_f.hip — rejectWithF (feature_tracker.cpp:711-743) behind the C-ABI: reject_f_kernel (gf_reject_f_kernels.hpp) on batches of sets of virtual-pixel
// pairs.  The definition: gf_reject_f.hpp.  Used by the tracker (gf_tracker_set_seq_reject_f) and exported as building blocks.
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_hip_own.hpp"
#include "gf_reject_f_kernels.hpp"
#include "gf_reject_f_stage.hpp"

static_assert(GF_REJECT_F_MAX_PAIRS == gfrf::kMaxCandidates && GF_REJECT_F_HYPOTHESES == gfrf::kHypotheses, "the public header restates the definition's constants");
static_assert(sizeof(gf_reject_f_result) == sizeof(gfrf::Result), "gf_reject_f_result is gfrf::Result field for field");

namespace gf {

int reject_f_fit(RejectFStage& s, size_t jobs) {
    if (jobs <= s.cap) return GF_OK;
    DevBuf<uint8_t> d; PinBuf<uint8_t> h; DevBuf<gfrf::Result> dr; PinBuf<gfrf::Result> hr;   // into locals first: a failed allocation changes nothing
    HIPCHK(d.alloc(jobs * sizeof(gfrf::Job))); HIPCHK(h.alloc(jobs * sizeof(gfrf::Job)));
    HIPCHK(dr.alloc(jobs)); HIPCHK(hr.alloc(jobs));
    s.d_jobs = std::move(d); s.h_jobs = std::move(h); s.d_res = std::move(dr); s.h_res = std::move(hr); s.cap = jobs;
    return GF_OK;
}

void reject_f_job(RejectFStage& s, int i, const gfcam::Camera* cam, const void* d_prev, const void* d_cur, const gfrf::Cand* d_pairs, uint8_t* d_status, int n,
                  int width, int height, double f_threshold, double focal, uint32_t seed) {
    gfrf::Job& j = reinterpret_cast<gfrf::Job*>(s.h_jobs.p)[i];
    j.head.prev = static_cast<const gfcam::Pair*>(d_prev); j.head.cur = static_cast<const gfcam::Pair*>(d_cur); j.head.pairs = d_pairs;
    j.head.status = d_status; j.head.result = s.d_res.p + i;
    j.head.tt = f_threshold * f_threshold; j.head.focal = focal;
    j.head.n = n; j.head.width = width; j.head.height = height; j.head.lift = cam ? 1 : 0;
    j.head.seed = seed; j.head.pad_ = 0;
    if (cam) j.cam = *cam;
}

int reject_f_launch(RejectFStage& s, int n, hipStream_t stream, hipEvent_t before, hipEvent_t after) {
    if (n < 1) return GF_OK;
    if ((size_t)n > s.cap) return set_err(GF_ERR_INVALID, "reject_f: %d entries in a table of %zu", n, s.cap);
    const gfrf::Job* jobs = reinterpret_cast<const gfrf::Job*>(s.h_jobs.p);
    for (int i = 0; i < n; i++)
        if (jobs[i].head.n < 0 || jobs[i].head.n > gfrf::kMaxCandidates) return set_err(GF_ERR_CAPACITY, "reject_f: entry %d has %d rows (at most %d)", i, jobs[i].head.n, gfrf::kMaxCandidates);
    HIPCHK(hipMemcpyAsync(s.d_jobs.p, s.h_jobs.p, (size_t)n * sizeof(gfrf::Job), hipMemcpyHostToDevice, stream));
    if (before) HIPCHK(hipEventRecord(before, stream));
    gfrf::reject_f_kernel<<<dim3((unsigned)(n < 65535 ? n : 65535)), gfrf::kThreads, 0, stream>>>(reinterpret_cast<const gfrf::Job*>(s.d_jobs.p), n);
    HIPCHK(hipGetLastError());
    if (after) HIPCHK(hipEventRecord(after, stream));
    HIPCHK(hipMemcpyAsync(s.h_res.p, s.d_res.p, (size_t)n * sizeof(gfrf::Result), hipMemcpyDeviceToHost, stream));
    return GF_OK;
}

// what the batch calls refuse before anything is copied or launched
static int reject_f_batch_check(const char* who, int n, const int* first, const void* pairs, const double* f_threshold, const unsigned* seed, const void* status) {
    if (!first || !f_threshold || !seed) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    if (n < 1) return set_err(GF_ERR_INVALID, "%s: %d sets (must be >= 1)", who, n);
    if (first[0] != 0) return set_err(GF_ERR_INVALID, "%s: first[0] is %d, not 0", who, first[0]);
    for (int b = 0; b < n; b++) {
        const int m = first[b + 1] - first[b];
        if (m < 0) return set_err(GF_ERR_INVALID, "%s: first[%d] = %d is below first[%d] = %d", who, b + 1, first[b + 1], b, first[b]);
        if (m > gfrf::kMaxCandidates) return set_err(GF_ERR_CAPACITY, "%s: set %d holds %d pairs (at most %d)", who, b, m, gfrf::kMaxCandidates);
        char msg[160];
        if (!gfrf::check_cfg(f_threshold[b], 0.0, msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: set %d: %s", who, b, msg);
    }
    if (first[n] > 0 && (!pairs || !status)) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    return GF_OK;
}

}  // namespace gf

extern "C" {

int gf_reject_f_batch_host(int n, const int* first, const float* pairs, const double* f_threshold, const unsigned* seed, uint8_t* status, gf_reject_f_result* results) {
    if (int rc = gf::reject_f_batch_check("reject_f_host", n, first, pairs, f_threshold, seed, status)) return rc;
    std::vector<gfrf::Cand> cand(gfrf::kMaxCandidates);
    std::vector<int> row_of(gfrf::kMaxCandidates);
    for (int b = 0; b < n; b++) {
        const int m = first[b + 1] - first[b];
        uint8_t* st = status + first[b];
        for (int i = 0; i < m; i++) st[i] = 1;
        const gfrf::Result r = gfrf::reject(reinterpret_cast<const gfrf::Cand*>(pairs) + first[b], st, m, f_threshold[b], seed[b], cand.data(), row_of.data());
        if (results) results[b] = gf_reject_f_result{r.m, r.rejected, r.winner, r.inliers};
    }
    return GF_OK;
}

int gf_reject_f_batch_device(int n, const int* first, const float* d_pairs, const double* f_threshold, const unsigned* seed, uint8_t* d_status, gf_reject_f_result* results,
                             void* stream) {
    if (int rc = gf::reject_f_batch_check("reject_f", n, first, d_pairs, f_threshold, seed, d_status)) return rc;
    if (int rc = gf::require_device()) return rc;
    // the staging of the building block: one per process, grow-only, never released
    static std::mutex lock;
    static gf::RejectFStage* const stage = new gf::RejectFStage();
    std::lock_guard<std::mutex> hold(lock);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((size_t)n > stage->cap) HIPCHK(hipDeviceSynchronize());   // an earlier call on another stream may still use the table that goes
    if (int rc = gf::reject_f_fit(*stage, (size_t)n)) return rc;
    if (first[n] > 0) HIPCHK(hipMemsetAsync(d_status, 1, (size_t)first[n], s));
    for (int b = 0; b < n; b++)
        gf::reject_f_job(*stage, b, nullptr, nullptr, nullptr, reinterpret_cast<const gfrf::Cand*>(d_pairs) + first[b], d_status + first[b], first[b + 1] - first[b], 0, 0,
                         f_threshold[b], gfrf::kFocal, seed[b]);
    if (int rc = gf::reject_f_launch(*stage, n, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));   // the tables above are the call's own
    if (results) for (int b = 0; b < n; b++) { const gfrf::Result& r = stage->h_res.p[b]; results[b] = gf_reject_f_result{r.m, r.rejected, r.winner, r.inliers}; }
    return GF_OK;
}

int gf_reject_f_batch(int n, const int* first, const float* pairs, const double* f_threshold, const unsigned* seed, uint8_t* status, gf_reject_f_result* results) {
    if (int rc = gf::reject_f_batch_check("reject_f", n, first, pairs, f_threshold, seed, status)) return rc;
    if (int rc = gf::require_device()) return rc;
    const size_t rows = (size_t)first[n];
    if (rows == 0) { if (results) for (int b = 0; b < n; b++) results[b] = gf_reject_f_result{0, 0, -1, 0}; return GF_OK; }
    gf::DevBuf<float> d_pairs; gf::DevBuf<uint8_t> d_status;
    HIPCHK(d_pairs.fit(4 * rows)); HIPCHK(d_status.fit(rows));
    HIPCHK(hipMemcpy(d_pairs.p, pairs, 4 * rows * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = gf_reject_f_batch_device(n, first, d_pairs.p, f_threshold, seed, d_status.p, results, nullptr)) return rc;
    HIPCHK(hipMemcpy(status, d_status.p, rows, hipMemcpyDeviceToHost));
    return GF_OK;
}

// The stage on PIXEL rows with a camera each: what the tracker's launch does (lift = 1), as a building block
static int reject_f_pixels_check(const char* who, int n, const int* first, const gf_camera_model_ex* cams, const int* wh, const float* prev_uv, const float* cur_uv,
                                 const double* f_threshold, const double* focal_length, const unsigned* seed, const uint8_t* status, std::vector<gfcam::Camera>& prepared) {
    if (int rc = gf::reject_f_batch_check(who, n, first, prev_uv, f_threshold, seed, status)) return rc;
    if (!cams || !wh || !focal_length || (first[n] > 0 && !cur_uv)) return gf::set_err(GF_ERR_INVALID, "%s: null argument", who);
    prepared.resize(n);
    for (int b = 0; b < n; b++) {
        char msg[320];
        if (!gfcam::prepare(cams[b], prepared[b], msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "%s: set %d: camera: %s", who, b, msg);
        if (!gfrf::check_cfg(f_threshold[b], focal_length[b], msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "%s: set %d: %s", who, b, msg);
        if (wh[2 * b] < 1 || wh[2 * b + 1] < 1) return gf::set_err(GF_ERR_INVALID, "%s: set %d: size %d x %d", who, b, wh[2 * b], wh[2 * b + 1]);
    }
    return GF_OK;
}

int gf_reject_f_pixels_batch_host(int n, const int* first, const gf_camera_model_ex* cams, const int* wh, const float* prev_uv, const float* cur_uv, const double* f_threshold,
                                  const double* focal_length, const unsigned* seed, uint8_t* status, gf_reject_f_result* results) {
    std::vector<gfcam::Camera> cam;
    if (int rc = reject_f_pixels_check("reject_f_pixels_host", n, first, cams, wh, prev_uv, cur_uv, f_threshold, focal_length, seed, status, cam)) return rc;
    std::vector<gfrf::Cand> pairs(gfrf::kMaxCandidates), cand(gfrf::kMaxCandidates);
    std::vector<int> row_of(gfrf::kMaxCandidates);
    for (int b = 0; b < n; b++) {
        const int m = first[b + 1] - first[b];
        const double focal = focal_length[b] == 0.0 ? gfrf::kFocal : focal_length[b];
        uint8_t* st = status + first[b];
        for (int i = 0; i < m; i++) {
            const float* p = prev_uv + 2 * (size_t)(first[b] + i); const float* q = cur_uv + 2 * (size_t)(first[b] + i);
            double P[3];
            gfcam::lift(cam[b], (double)q[0], (double)q[1], P);
            pairs[i].bx = gfrf::virtual_pixel(focal, P[0], P[2], wh[2 * b]); pairs[i].by = gfrf::virtual_pixel(focal, P[1], P[2], wh[2 * b + 1]);
            gfcam::lift(cam[b], (double)p[0], (double)p[1], P);
            pairs[i].ax = gfrf::virtual_pixel(focal, P[0], P[2], wh[2 * b]); pairs[i].ay = gfrf::virtual_pixel(focal, P[1], P[2], wh[2 * b + 1]);
            st[i] = 1;
        }
        const gfrf::Result r = gfrf::reject(pairs.data(), st, m, f_threshold[b], seed[b], cand.data(), row_of.data());
        if (results) results[b] = gf_reject_f_result{r.m, r.rejected, r.winner, r.inliers};
    }
    return GF_OK;
}

int gf_reject_f_pixels_batch(int n, const int* first, const gf_camera_model_ex* cams, const int* wh, const float* prev_uv, const float* cur_uv, const double* f_threshold,
                             const double* focal_length, const unsigned* seed, uint8_t* status, gf_reject_f_result* results) {
    std::vector<gfcam::Camera> cam;
    if (int rc = reject_f_pixels_check("reject_f_pixels", n, first, cams, wh, prev_uv, cur_uv, f_threshold, focal_length, seed, status, cam)) return rc;
    if (int rc = gf::require_device()) return rc;
    const size_t rows = (size_t)first[n];
    if (rows == 0) { if (results) for (int b = 0; b < n; b++) results[b] = gf_reject_f_result{0, 0, -1, 0}; return GF_OK; }
    gf::DevBuf<float> d_prev, d_cur; gf::DevBuf<uint8_t> d_status;
    gf::RejectFStage stage;   // the call's own
    HIPCHK(d_prev.fit(2 * rows)); HIPCHK(d_cur.fit(2 * rows)); HIPCHK(d_status.fit(rows));
    if (int rc = gf::reject_f_fit(stage, (size_t)n)) return rc;
    HIPCHK(hipMemcpy(d_prev.p, prev_uv, 2 * rows * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cur.p, cur_uv, 2 * rows * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_status.p, 1, rows));
    for (int b = 0; b < n; b++)
        gf::reject_f_job(stage, b, &cam[b], d_prev.p + 2 * (size_t)first[b], d_cur.p + 2 * (size_t)first[b], nullptr, d_status.p + first[b], first[b + 1] - first[b], wh[2 * b], wh[2 * b + 1],
                         f_threshold[b], focal_length[b] == 0.0 ? gfrf::kFocal : focal_length[b], seed[b]);
    if (int rc = gf::reject_f_launch(stage, n, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    if (results) for (int b = 0; b < n; b++) { const gfrf::Result& r = stage.h_res.p[b]; results[b] = gf_reject_f_result{r.m, r.rejected, r.winner, r.inliers}; }
    HIPCHK(hipMemcpy(status, d_status.p, rows, hipMemcpyDeviceToHost));
    return GF_OK;
}

}  // extern "C"
