// gf_depth_reg.hip — raw depth registered to the colour camera behind the C-ABI: depth_scatter_kernel and depth_finish_kernel (gf_depth_reg_kernels.hpp) on
// batches of frames of any sizes.  The definition and what a setter refuses: gf_depth_reg.hpp.  Used by the tracker (gf_tracker_set_seq_depth_reg) and exported
// as building blocks.
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_depth_reg_kernels.hpp"
#include "gf_depth_reg_stage.hpp"
#include "gf_hip_own.hpp"

namespace gf {

int depth_reg_fit(DepthRegStage& s, size_t jobs, size_t zwords) {
    if (jobs > s.d_jobs.n) {   // into locals first: a failed allocation changes nothing
        DevBuf<gfdreg::Job> d; PinBuf<gfdreg::Job> h;
        HIPCHK(d.alloc(jobs)); HIPCHK(h.alloc(jobs));
        s.d_jobs = std::move(d); s.h_jobs = std::move(h);
    }
    if (zwords > s.z.n) {
        DevBuf<uint32_t> z;
        HIPCHK(z.fit(zwords));
        s.z = std::move(z); s.primed = false;
    }
    return GF_OK;
}

// The n jobs of s.h_jobs: down, scatter, finish, all on `stream`.  The caller keeps h_jobs as it is until the stream has passed the copy.
int depth_reg_launch(DepthRegStage& s, int n, hipStream_t stream, hipEvent_t before, hipEvent_t after) {
    if (n < 1) return GF_OK;
    size_t scatter_items = 0, finish_items = 0;
    bool full = false;   // an entry with a PINHOLE_FULL colour camera: the scatter kernel's other instance, still one launch
    for (int i = 0; i < n; i++) {
        const gfdreg::Job& j = s.h_jobs.p[i];
        full |= j.p.model == GF_CAMERA_PINHOLE_FULL;
        scatter_items = std::max(scatter_items, (size_t)j.wd * j.hd);
        finish_items = std::max(finish_items, gfdreg::zwords_of(j.wc, j.hc) / 8);
        if (j.zoff + gfdreg::zwords_of(j.wc, j.hc) > s.z.n || (j.zoff & 7)) return set_err(GF_ERR_INVALID, "depth_register: entry %d leaves the z-buffer", i);
    }
    if (!s.primed) HIPCHK(hipMemsetAsync(s.z.p, 0xff, s.z.n * sizeof(uint32_t), stream));   // a new buffer, or a call that did not get as far as its finish kernel
    s.primed = false;
    HIPCHK(hipMemcpyAsync(s.d_jobs.p, s.h_jobs.p, (size_t)n * sizeof(gfdreg::Job), hipMemcpyHostToDevice, stream));
    if (before) HIPCHK(hipEventRecord(before, stream));
    if (full) gfdreg::depth_scatter_kernel<true><<<gfdreg::reg_grid(scatter_items, n), gfdreg::kThreads, 0, stream>>>(s.d_jobs.p, s.z.p, n);
    else gfdreg::depth_scatter_kernel<false><<<gfdreg::reg_grid(scatter_items, n), gfdreg::kThreads, 0, stream>>>(s.d_jobs.p, s.z.p, n);
    HIPCHK(hipGetLastError());
    gfdreg::depth_finish_kernel<<<gfdreg::reg_grid(finish_items, n), gfdreg::kThreads, 0, stream>>>(s.d_jobs.p, s.z.p, n);
    HIPCHK(hipGetLastError());
    if (after) HIPCHK(hipEventRecord(after, stream));
    s.primed = true;   // behind the finish kernel every word holds kUntouched again
    return GF_OK;
}

// the colour camera of an entry as either struct carries it; gf_camera_model holds no PINHOLE_FULL
static const double* full_tail(const gf_camera_model&) { return nullptr; }
static const double* full_tail(const gf_camera_model_ex& c) { return c.model == GF_CAMERA_PINHOLE_FULL ? c.dist + 4 : nullptr; }
static const char* colour_models(const gf_camera_model&) { return "a GF_CAMERA_PINHOLE only"; }
static const char* colour_models(const gf_camera_model_ex&) { return "a GF_CAMERA_PINHOLE or GF_CAMERA_PINHOLE_FULL only"; }

// what the batch calls refuse before anything is copied or launched; params: map()'s doubles of every entry
template <class Model>
static int depth_reg_batch_check(const char* who, const gf_frame_ref* src, const gf_depth_reg* reg, const Model* colour, const int* colour_wh, const gf_frame_ref* dst, int batch,
                                 std::vector<gfdreg::Params>& params) {
    if (!src || !reg || !colour || !colour_wh || !dst) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    if (batch < 1) return set_err(GF_ERR_INVALID, "%s: batch %d (must be >= 1)", who, batch);
    params.resize(batch);
    for (int b = 0; b < batch; b++) {
        char msg[320];
        if (!gfdreg::check(reg[b], msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: entry %d: %s", who, b, msg);
        gfcam::Camera cam;
        if (!gfcam::prepare(colour[b], cam, msg, sizeof msg)) return set_err(GF_ERR_INVALID, "%s: entry %d: colour camera: %s", who, b, msg);
        if (colour[b].model != GF_CAMERA_PINHOLE && !full_tail(colour[b]))
            return set_err(GF_ERR_INVALID, "%s: entry %d: the colour camera is %s; depth is registered to %s", who, b, gfcam::model_name(colour[b].model), colour_models(colour[b]));
        const int wc = colour_wh[2 * b], hc = colour_wh[2 * b + 1];
        if (wc < gfdreg::kMinSize || wc > gfdreg::kMaxSize || hc < gfdreg::kMinSize || hc > gfdreg::kMaxSize)
            return set_err(GF_ERR_INVALID, "%s: entry %d: colour size %d x %d is outside %d .. %d", who, b, wc, hc, gfdreg::kMinSize, gfdreg::kMaxSize);
        gfref::Verdict v = gfref::check(src[b], (size_t)reg[b].width * 2, true, false);
        if (v != gfref::kOk) return set_err(GF_ERR_INVALID, "%s: raw depth frame of entry %d: %s (data %p, pitch %zu bytes, a row is %zu bytes)", who, b, gfref::verdict_text(v), src[b].data, src[b].pitch, (size_t)reg[b].width * 2);
        v = gfref::check(dst[b], (size_t)wc * 2, true, false);
        if (v != gfref::kOk) return set_err(GF_ERR_INVALID, "%s: registered frame of entry %d: %s (data %p, pitch %zu bytes, a row is %zu bytes)", who, b, gfref::verdict_text(v), dst[b].data, dst[b].pitch, (size_t)wc * 2);
        params[b] = gfdreg::params_of(reg[b], colour[b].proj, colour[b].dist, full_tail(colour[b]));
    }
    return GF_OK;
}

}  // namespace gf

template <class Model>
static int depth_register_batch_device(const gf_frame_ref* d_src, const gf_depth_reg* reg, const Model* colour, const int* colour_wh, const gf_frame_ref* d_dst, int batch, void* stream) {
    std::vector<gfdreg::Params> params;
    if (int rc = gf::depth_reg_batch_check("depth_register", d_src, reg, colour, colour_wh, d_dst, batch, params)) return rc;
    if (int rc = gf::require_device()) return rc;
    // the staging of the building block: one per process, grow-only, never released (the z-buffer keeps its priming from call to call)
    static std::mutex lock;
    static gf::DepthRegStage* const stage = new gf::DepthRegStage();
    std::lock_guard<std::mutex> hold(lock);
    size_t zwords = 0;
    for (int b = 0; b < batch; b++) zwords += gfdreg::zwords_of(colour_wh[2 * b], colour_wh[2 * b + 1]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (zwords > stage->z.n) HIPCHK(hipDeviceSynchronize());   // an earlier call on another stream may still use the buffer that goes
    if (int rc = gf::depth_reg_fit(*stage, (size_t)batch, zwords)) return rc;
    size_t zoff = 0;
    for (int b = 0; b < batch; b++) {
        gfdreg::Job& j = stage->h_jobs.p[b];
        j.src = static_cast<const uint8_t*>(d_src[b].data); j.src_pitch = d_src[b].pitch;
        j.dst = static_cast<uint8_t*>(const_cast<void*>(d_dst[b].data)); j.dst_pitch = d_dst[b].pitch;
        j.zoff = zoff;
        j.wd = reg[b].width; j.hd = reg[b].height; j.wc = colour_wh[2 * b]; j.hc = colour_wh[2 * b + 1];
        j.p = params[b];
        zoff += gfdreg::zwords_of(j.wc, j.hc);
    }
    if (int rc = gf::depth_reg_launch(*stage, batch, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));   // the table above is the call's own
    return GF_OK;
}

template <class Model>
static int depth_register_batch(const gf_frame_ref* src, const gf_depth_reg* reg, const Model* colour, const int* colour_wh, const gf_frame_ref* dst, int batch) {
    std::vector<gfdreg::Params> params;
    if (int rc = gf::depth_reg_batch_check("depth_register", src, reg, colour, colour_wh, dst, batch, params)) return rc;
    if (int rc = gf::require_device()) return rc;
    // tight device frames: every source, then every destination
    std::vector<gf_frame_ref> d_src(batch), d_dst(batch);
    size_t bytes = 0;
    for (int b = 0; b < batch; b++) bytes += ((size_t)reg[b].width * reg[b].height * 2 + 15) & ~(size_t)15;
    const size_t dst_at = bytes;
    for (int b = 0; b < batch; b++) bytes += ((size_t)colour_wh[2 * b] * colour_wh[2 * b + 1] * 2 + 15) & ~(size_t)15;
    gf::DevBuf<uint8_t> d;
    HIPCHK(d.fit(bytes));
    size_t at = 0, to = dst_at;
    for (int b = 0; b < batch; b++) {
        const size_t row = (size_t)reg[b].width * 2, out_row = (size_t)colour_wh[2 * b] * 2;
        d_src[b] = gf_frame_ref{d.p + at, row};
        d_dst[b] = gf_frame_ref{d.p + to, out_row};
        HIPCHK(hipMemcpy2D(d.p + at, row, src[b].data, src[b].pitch, row, reg[b].height, hipMemcpyHostToDevice));
        at += (row * reg[b].height + 15) & ~(size_t)15;
        to += (out_row * colour_wh[2 * b + 1] + 15) & ~(size_t)15;
    }
    if (int rc = depth_register_batch_device(d_src.data(), reg, colour, colour_wh, d_dst.data(), batch, nullptr)) return rc;
    for (int b = 0; b < batch; b++) {
        const size_t out_row = (size_t)colour_wh[2 * b] * 2;
        HIPCHK(hipMemcpy2D(const_cast<void*>(dst[b].data), dst[b].pitch, d_dst[b].data, out_row, out_row, colour_wh[2 * b + 1], hipMemcpyDeviceToHost));
    }
    return GF_OK;
}

extern "C" {

int gf_depth_register_batch_device(const gf_frame_ref* d_src, const gf_depth_reg* reg, const gf_camera_model* colour, const int* colour_wh, const gf_frame_ref* d_dst, int batch, void* stream) {
    return depth_register_batch_device(d_src, reg, colour, colour_wh, d_dst, batch, stream);
}
int gf_depth_register_batch_device_ex(const gf_frame_ref* d_src, const gf_depth_reg* reg, const gf_camera_model_ex* colour, const int* colour_wh, const gf_frame_ref* d_dst, int batch, void* stream) {
    return depth_register_batch_device(d_src, reg, colour, colour_wh, d_dst, batch, stream);
}
int gf_depth_register_batch(const gf_frame_ref* src, const gf_depth_reg* reg, const gf_camera_model* colour, const int* colour_wh, const gf_frame_ref* dst, int batch) {
    return depth_register_batch(src, reg, colour, colour_wh, dst, batch);
}
int gf_depth_register_batch_ex(const gf_frame_ref* src, const gf_depth_reg* reg, const gf_camera_model_ex* colour, const int* colour_wh, const gf_frame_ref* dst, int batch) {
    return depth_register_batch(src, reg, colour, colour_wh, dst, batch);
}

}  // extern "C"
