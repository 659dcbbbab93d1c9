// gf_stereo_depth.hip — the stereo depth behind the C-ABI: stereo_depth_kernel (gf_stereo_depth_kernels.hpp) on batches of sets of matched pixel pairs, and the
// same sets through the shared function on the host.  The definition: gf_stereo_depth.hpp.  Used by the tracker (gf_tracker_set_seq_stereo_depth) and exported
// as building blocks.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_hip_own.hpp"
#include "gf_stereo_depth_kernels.hpp"

static_assert(GF_STEREO_DEPTH_NO_MATCH == gfsd::kNoMatch && GF_STEREO_DEPTH_LIFT == gfsd::kLift && GF_STEREO_DEPTH_PARALLAX == gfsd::kParallax && GF_STEREO_DEPTH_BEHIND == gfsd::kBehind &&
              GF_STEREO_DEPTH_EPIPOLAR == gfsd::kEpipolar && GF_STEREO_DEPTH_RANGE == gfsd::kRange && GF_STEREO_DEPTH_OK == gfsd::kOk, "the public header restates the definition's reason codes");

namespace gf {

// one launch for the `A.count` positions of A, none of which has more than max_n points
int stereo_depth_launch(const gfsd::Args& A, int max_n, hipStream_t stream) {
    if (A.count < 1 || max_n < 1) return GF_OK;
    gfsd::stereo_depth_kernel<<<gfsd::grid_of(max_n, A.count), gfsd::kThreads, 0, stream>>>(A);
    HIPCHK(hipGetLastError());
    return GF_OK;
}

// what the batch calls refuse before anything is copied or launched; the checked sets into `out`, the longest set into *max_n
static int stereo_depth_batch_check(const char* who, int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                                    const void* left_uv, const void* right_uv, const void* status, const void* depth_mm, const void* why, std::vector<gfsd::Entry>& out, int* max_n) {
    if (!first || !left || !right || !cfg) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    if (n < 1) return set_err(GF_ERR_INVALID, "%s: %d sets (must be >= 1)", who, n);
    if (first[0] != 0) return set_err(GF_ERR_INVALID, "%s: first[0] is %d, not 0", who, first[0]);
    out.resize(n);
    *max_n = 0;
    for (int b = 0; b < n; b++) {
        if (first[b + 1] < first[b]) return set_err(GF_ERR_INVALID, "%s: first[%d] = %d is below first[%d] = %d", who, b + 1, first[b + 1], b, first[b]);
        *max_n = std::max(*max_n, first[b + 1] - first[b]);
        char msg[320];
        gfsd::Entry& e = out[b];
        e = gfsd::Entry{};
        if (!gfcam::prepare(left[b], e.left, msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: set %d: left camera: %s", who, b, msg);
        if (!gfcam::prepare(right[b], e.right, msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: set %d: right camera: %s", who, b, msg);
        if (!gfsd::check(cfg[b], msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: set %d: %s", who, b, msg);
        e.rig = gfsd::rig_of(cfg[b]);
        e.on = 1;
    }
    if (first[n] > 0 && (!left_uv || !right_uv || !status || !depth_mm || !why)) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    return GF_OK;
}

}  // namespace gf

extern "C" {

int gf_stereo_depth_batch_host(int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                               const float* left_uv, const float* right_uv, const uint8_t* status, uint16_t* depth_mm, uint8_t* why) {
    std::vector<gfsd::Entry> sets;
    int max_n = 0;
    if (int rc = gf::stereo_depth_batch_check("stereo_depth_host", n, first, left, right, cfg, left_uv, right_uv, status, depth_mm, why, sets, &max_n)) return rc;
    for (int b = 0; b < n; b++)
        for (int i = first[b]; i < first[b + 1]; i++) {
            const gfsd::Depth d = gfsd::depth_of(sets[b].left, sets[b].right, sets[b].rig, left_uv[2 * (size_t)i], left_uv[2 * (size_t)i + 1], right_uv[2 * (size_t)i], right_uv[2 * (size_t)i + 1], status[i]);
            depth_mm[i] = d.mm; why[i] = d.why;
        }
    return GF_OK;
}

int gf_stereo_depth_batch_device(int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                                 const float* d_left_uv, const float* d_right_uv, const uint8_t* d_status, uint16_t* d_depth_mm, uint8_t* d_why, void* stream) {
    std::vector<gfsd::Entry> sets;
    int max_n = 0;
    if (int rc = gf::stereo_depth_batch_check("stereo_depth", n, first, left, right, cfg, d_left_uv, d_right_uv, d_status, d_depth_mm, d_why, sets, &max_n)) return rc;
    if (first[n] == 0) return GF_OK;
    if (int rc = gf::require_device()) return rc;
    const size_t set_bytes = (size_t)n * sizeof(gfsd::Entry), first_bytes = ((size_t)n + 1) * sizeof(int);
    gf::DevBuf<uint8_t> d_tab;
    HIPCHK(d_tab.fit(set_bytes + first_bytes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipMemcpyAsync(d_tab.p, sets.data(), set_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tab.p + set_bytes, first, first_bytes, hipMemcpyHostToDevice, s));
    gfsd::Args A{};
    A.entries = reinterpret_cast<const gfsd::Entry*>(d_tab.p); A.entry_of = nullptr; A.first = reinterpret_cast<const int*>(d_tab.p + set_bytes);
    A.cap = 0; A.count = n;
    A.left_pts = reinterpret_cast<const gfcam::Pair*>(d_left_uv); A.right_pts = reinterpret_cast<const gfcam::Pair*>(d_right_uv); A.status = d_status;
    A.depth_mm = d_depth_mm; A.why = d_why;
    if (int rc = gf::stereo_depth_launch(A, max_n, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));   // the tables above are the call's own
    return GF_OK;
}

int gf_stereo_depth_batch(int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                          const float* left_uv, const float* right_uv, const uint8_t* status, uint16_t* depth_mm, uint8_t* why) {
    std::vector<gfsd::Entry> sets;
    int max_n = 0;
    if (int rc = gf::stereo_depth_batch_check("stereo_depth", n, first, left, right, cfg, left_uv, right_uv, status, depth_mm, why, sets, &max_n)) return rc;
    const size_t rows = (size_t)first[n];
    if (rows == 0) return GF_OK;
    if (int rc = gf::require_device()) return rc;
    gf::DevBuf<float> d_l, d_r; gf::DevBuf<uint8_t> d_st, d_why; gf::DevBuf<uint16_t> d_mm;
    HIPCHK(d_l.fit(2 * rows)); HIPCHK(d_r.fit(2 * rows)); HIPCHK(d_st.fit(rows)); HIPCHK(d_why.fit(rows)); HIPCHK(d_mm.fit(rows));
    HIPCHK(hipMemcpy(d_l.p, left_uv, 2 * rows * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_r.p, right_uv, 2 * rows * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_st.p, status, rows, hipMemcpyHostToDevice));
    if (int rc = gf_stereo_depth_batch_device(n, first, left, right, cfg, d_l.p, d_r.p, d_st.p, d_mm.p, d_why.p, nullptr)) return rc;
    HIPCHK(hipMemcpy(depth_mm, d_mm.p, rows * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(why, d_why.p, rows, hipMemcpyDeviceToHost));
    return GF_OK;
}

}  // extern "C"
