// gf_camera.hip — camodocal's PINHOLE, MEI, KANNALA_BRANDT, PINHOLE_FULL and SCARAMUZZA cameras behind the C-ABI (the last two through the _ex calls alone): liftProjective on batches of points through camera_lift_kernel
// (gf_camera_kernels.hpp; undistortedPts, feature_tracker.cpp:797-808) and spaceToPlane on the host (setPrediction, :1006-1027).  The formulas and what a setter
// refuses: gf_camera_models.hpp.  Used by the tracker (gf_tracker_set_seq_camera) and exported as building blocks.
#include <hip/hip_runtime.h>
#include <climits>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_camera_kernels.hpp"
#include "gf_hip_own.hpp"

namespace gf {

// one launch for the entries of A, none of which has more than max_n points per set
int camera_lift_launch(const gfcam::LiftArgs& A, int max_n, hipStream_t stream) {
    if (A.batch < 1 || max_n < 1) return GF_OK;
    gfcam::camera_lift_kernel<<<gfcam::lift_grid(max_n, A.n_sets, A.batch), gfcam::kLiftThreads, 0, stream>>>(A);
    HIPCHK(hipGetLastError());
    return GF_OK;
}

// cams / first of the batch calls: every camera checked into `out`, the offsets from 0 and not decreasing; *max_n: the longest entry
template <class Model>   // gf_camera_model, which holds models 0-2, or gf_camera_model_ex
static int camera_batch_check(const char* who, const Model* cams, int batch, const int* first, std::vector<gfcam::Camera>& out, int* max_n) {
    if (!cams || !first) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    if (batch < 1) return set_err(GF_ERR_INVALID, "%s: batch %d (must be >= 1)", who, batch);
    if (first[0] != 0) return set_err(GF_ERR_INVALID, "%s: first[0] is %d, not 0", who, first[0]);
    out.resize(batch);
    *max_n = 0;
    for (int b = 0; b < batch; b++) {
        if (first[b + 1] < first[b]) return set_err(GF_ERR_INVALID, "%s: first[%d] = %d is below first[%d] = %d", who, b + 1, first[b + 1], b, first[b]);
        *max_n = std::max(*max_n, first[b + 1] - first[b]);
        char msg[320];
        if (!gfcam::prepare(cams[b], out[b], msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: camera %d: %s", who, b, msg);
    }
    return GF_OK;
}

}  // namespace gf

template <class Model>
static int camera_lift_batch_device(const Model* cams, int batch, const int* first, const float* d_uv, double* d_rays, float* d_un, void* stream) {
    std::vector<gfcam::Camera> prepared;
    int max_n = 0;
    if (int rc = gf::camera_batch_check("camera_lift", cams, batch, first, prepared, &max_n)) return rc;
    if (first[batch] == 0) return GF_OK;
    if (!d_uv || !d_un) return gf::set_err(GF_ERR_INVALID, "camera_lift: null argument");
    if (int rc = gf::require_device()) return rc;
    const size_t cam_bytes = (size_t)batch * sizeof(gfcam::Camera), first_bytes = ((size_t)batch + 1) * sizeof(int);
    gf::DevBuf<uint8_t> d_tab;
    HIPCHK(d_tab.fit(cam_bytes + first_bytes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipMemcpyAsync(d_tab.p, prepared.data(), cam_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tab.p + cam_bytes, first, first_bytes, hipMemcpyHostToDevice, s));
    gfcam::LiftArgs A{};
    A.cams = reinterpret_cast<const gfcam::Camera*>(d_tab.p); A.cam_of = nullptr; A.first = reinterpret_cast<const int*>(d_tab.p + cam_bytes);
    A.cap = 0; A.batch = batch; A.n_sets = 1;
    A.set[0] = gfcam::LiftSet{reinterpret_cast<const gfcam::Pair*>(d_uv), nullptr, reinterpret_cast<gfcam::Pair*>(d_un), d_rays};
    if (int rc = gf::camera_lift_launch(A, max_n, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));   // the tables above are the call's own
    return GF_OK;
}

template <class Model>
static int camera_lift_batch(const Model* cams, int batch, const int* first, const float* uv, double* rays, float* un) {
    std::vector<gfcam::Camera> prepared;
    int max_n = 0;
    if (int rc = gf::camera_batch_check("camera_lift", cams, batch, first, prepared, &max_n)) return rc;
    const size_t n = (size_t)first[batch];
    if (n == 0) return GF_OK;
    if (!uv || !un) return gf::set_err(GF_ERR_INVALID, "camera_lift: null argument");
    if (int rc = gf::require_device()) return rc;
    gf::DevBuf<float> d_uv, d_un; gf::DevBuf<double> d_rays;
    HIPCHK(d_uv.fit(2 * n)); HIPCHK(d_un.fit(2 * n));
    if (rays) HIPCHK(d_rays.fit(3 * n));
    HIPCHK(hipMemcpy(d_uv.p, uv, 2 * n * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = camera_lift_batch_device(cams, batch, first, d_uv.p, rays ? d_rays.p : nullptr, d_un.p, nullptr)) return rc;
    HIPCHK(hipMemcpy(un, d_un.p, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (rays) HIPCHK(hipMemcpy(rays, d_rays.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    return GF_OK;
}

template <class Model>
static int camera_project_batch(const Model* cams, int batch, const int* first, const double* xyz, double* uv) {
    std::vector<gfcam::Camera> prepared;
    int max_n = 0;
    if (int rc = gf::camera_batch_check("camera_project", cams, batch, first, prepared, &max_n)) return rc;
    if (first[batch] == 0) return GF_OK;
    if (!xyz || !uv) return gf::set_err(GF_ERR_INVALID, "camera_project: null argument");
    for (int b = 0; b < batch; b++)
        for (int i = first[b]; i < first[b + 1]; i++) gfcam::space_to_plane(prepared[b], xyz + 3 * (size_t)i, uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
    return GF_OK;
}

extern "C" {

int gf_camera_lift_batch_device(const gf_camera_model* cams, int batch, const int* first, const float* d_uv, double* d_rays, float* d_un, void* stream) {
    return camera_lift_batch_device(cams, batch, first, d_uv, d_rays, d_un, stream);
}
int gf_camera_lift_batch_device_ex(const gf_camera_model_ex* cams, int batch, const int* first, const float* d_uv, double* d_rays, float* d_un, void* stream) {
    return camera_lift_batch_device(cams, batch, first, d_uv, d_rays, d_un, stream);
}
int gf_camera_lift_batch(const gf_camera_model* cams, int batch, const int* first, const float* uv, double* rays, float* un) {
    return camera_lift_batch(cams, batch, first, uv, rays, un);
}
int gf_camera_lift_batch_ex(const gf_camera_model_ex* cams, int batch, const int* first, const float* uv, double* rays, float* un) {
    return camera_lift_batch(cams, batch, first, uv, rays, un);
}
int gf_camera_project_batch(const gf_camera_model* cams, int batch, const int* first, const double* xyz, double* uv) {
    return camera_project_batch(cams, batch, first, xyz, uv);
}
int gf_camera_project_batch_ex(const gf_camera_model_ex* cams, int batch, const int* first, const double* xyz, double* uv) {
    return camera_project_batch(cams, batch, first, xyz, uv);
}

}  // extern "C"
