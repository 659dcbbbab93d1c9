// gf_clahe.hip — cv::createCLAHE(clipLimit, Size(tiles_x, tiles_y))->apply(img, img) on batches of u8 frames (the EQUALIZE step of the reference's node,
// rosNodeTest.cpp:256-261, ahead of trackImage).  Kernels: gf_clahe_kernels.hpp.  Used by the tracker (gf_tracker_cfg.equalize) and exported as its own C-ABI.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>

#include "../../include/groundfusion_hip.h"
#include "gf_clahe_kernels.hpp"
#include "gf_hip_own.hpp"

#pragma clang fp contract(off)   // as -ffp-contract=off (build.py): a fused multiply-add changes the interpolated bits

namespace gf {

// the tile geometry, clip limit and scales of CLAHE_Impl::apply (clahe.cpp), or GF_ERR_INVALID
static int clahe_geom(int w, int h, double clip_limit, int tiles_x, int tiles_y, gfclahe::Geom& g) {
    if (tiles_x < 1 || tiles_y < 1 || w <= tiles_x || h <= tiles_y)
        return set_err(GF_ERR_INVALID, "clahe: %dx%d frames with a %dx%d tile grid (needs width > tiles_x >= 1 and height > tiles_y >= 1)", w, h, tiles_x, tiles_y);
    if (!(clip_limit >= 0.0) || !std::isfinite(clip_limit)) return set_err(GF_ERR_INVALID, "clahe: clip limit %g (needs a finite value >= 0)", clip_limit);
    g.w = w; g.h = h; g.tx = tiles_x; g.ty = tiles_y;
    if (w % tiles_x == 0 && h % tiles_y == 0) { g.tw = w / tiles_x; g.th = h / tiles_y; }
    else { g.tw = (w + tiles_x - w % tiles_x) / tiles_x; g.th = (h + tiles_y - h % tiles_y) / tiles_y; }   // copyMakeBorder(.., 0, ty - h % ty, 0, tx - w % tx, REFLECT_101)
    const int area = g.tw * g.th;
    g.use_clip = clip_limit > 0.0;
    g.clip = 0;
    if (g.use_clip) g.clip = std::max((int)(clip_limit * area / 256), 1);
    g.lut_scale = 255.0f / area;
    g.inv_tw = 1.0f / g.tw;
    g.inv_th = 1.0f / g.th;
    return GF_OK;
}

size_t clahe_lut_bytes(int batch, int tiles_x, int tiles_y) { return (size_t)batch * tiles_x * tiles_y * 256; }

// d_lut: clahe_lut_bytes(batch, tiles_x, tiles_y) bytes of the caller's scratch
// d_refs == nullptr: d_src holds `batch` tight frames back to back.  Otherwise (the table form) d_src is not read and frame b lies at d_refs[b] (device-readable
// gf_frame_ref, checked by the caller): the vector forms follow the sizes and d_dst here, and each block falls back to bytes when its own frame's pointer or
// pitch misses their alignment.
static int clahe_launch_any(const uint8_t* d_src, const gf_frame_ref* d_refs, uint8_t* d_dst, uint8_t* d_lut, int batch, int w, int h, double clip_limit, int tiles_x, int tiles_y, hipStream_t stream) {
    using namespace gfclahe;
    Geom g;
    if (int rc = clahe_geom(w, h, clip_limit, tiles_x, tiles_y, g)) return rc;
    if (batch < 1 || batch > 65535) return set_err(GF_ERR_INVALID, "clahe: batch %d (1 .. 65535)", batch);
    const int vec4 = !(w & 3) && !(g.tw & 3) && (d_refs || !(reinterpret_cast<uintptr_t>(d_src) & 3));
    if (d_refs) clahe_lut_refs_kernel<<<dim3(g.tx * g.ty, batch), kThreads, 0, stream>>>(d_refs, d_lut, g, vec4);
    else clahe_lut_kernel<<<dim3(g.tx * g.ty, batch), kThreads, 0, stream>>>(d_src, d_lut, g, vec4);
    // bands: about a thousand workgroups in all, 8 .. 64 rows each, and at most 32 KB of LUT rows in LDS
    const int want_bands = std::max(1, (1024 + batch - 1) / batch);
    int band = std::min(64, std::max(8, (h + want_bands - 1) / want_bands));
    const size_t plane = (size_t)g.tx * 256;
    auto rows_for = [&](int bnd) { return std::min(g.ty, (bnd - 1) / g.th + 4); };   // tile rows a band of bnd rows can touch (+1 for float rounding)
    while (band > 1 && rows_for(band) * plane > 32 * 1024) band >>= 1;
    const bool lds = rows_for(band) * plane <= 64 * 1024;
    const int lds_rows = rows_for(band);
    const size_t lds_bytes = lds ? lds_rows * plane : 0;
    const dim3 grid((h + band - 1) / band, batch);
    const bool v16 = !(w & 15) && !(((d_refs ? 0 : reinterpret_cast<uintptr_t>(d_src)) | reinterpret_cast<uintptr_t>(d_dst)) & 15);
    if (d_refs) {
        if (v16 && lds) clahe_apply_refs_kernel<true, true><<<grid, kThreads, lds_bytes, stream>>>(d_refs, d_dst, d_lut, g, band, lds_rows);
        else if (lds) clahe_apply_refs_kernel<false, true><<<grid, kThreads, lds_bytes, stream>>>(d_refs, d_dst, d_lut, g, band, lds_rows);
        else if (v16) clahe_apply_refs_kernel<true, false><<<grid, kThreads, 0, stream>>>(d_refs, d_dst, d_lut, g, band, lds_rows);
        else clahe_apply_refs_kernel<false, false><<<grid, kThreads, 0, stream>>>(d_refs, d_dst, d_lut, g, band, lds_rows);
    }
    else if (v16 && lds) clahe_apply_kernel<true, true><<<grid, kThreads, lds_bytes, stream>>>(d_src, d_dst, d_lut, g, band, lds_rows);
    else if (lds) clahe_apply_kernel<false, true><<<grid, kThreads, lds_bytes, stream>>>(d_src, d_dst, d_lut, g, band, lds_rows);
    else if (v16) clahe_apply_kernel<true, false><<<grid, kThreads, 0, stream>>>(d_src, d_dst, d_lut, g, band, lds_rows);
    else clahe_apply_kernel<false, false><<<grid, kThreads, 0, stream>>>(d_src, d_dst, d_lut, g, band, lds_rows);
    HIPCHK(hipGetLastError());
    return GF_OK;
}
int clahe_launch(const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_lut, int batch, int w, int h, double clip_limit, int tiles_x, int tiles_y, hipStream_t stream) {
    return clahe_launch_any(d_src, nullptr, d_dst, d_lut, batch, w, h, clip_limit, tiles_x, tiles_y, stream);
}
int clahe_launch_refs(const gf_frame_ref* d_refs, uint8_t* d_dst, uint8_t* d_lut, int batch, int w, int h, double clip_limit, int tiles_x, int tiles_y, hipStream_t stream) {
    return clahe_launch_any(nullptr, d_refs, d_dst, d_lut, batch, w, h, clip_limit, tiles_x, tiles_y, stream);
}

}  // namespace gf

extern "C" {

int gf_clahe_batch_device(const void* d_src, void* d_dst, int batch, int width, int height, double clip_limit, int tiles_x, int tiles_y, void* stream) {
    if (!d_src || !d_dst) return gf::set_err(GF_ERR_INVALID, "null argument");
    gfclahe::Geom g;
    if (int rc = gf::clahe_geom(width, height, clip_limit, tiles_x, tiles_y, g)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // the LUTs live from the first launch to the second only: stream-ordered scratch keeps the call asynchronous
    uint8_t* lut = nullptr;
    HIPCHK(hipMallocAsync((void**)&lut, gf::clahe_lut_bytes(batch, tiles_x, tiles_y), s));
    const int rc = gf::clahe_launch(static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), lut, batch, width, height, clip_limit, tiles_x, tiles_y, s);
    const hipError_t e = hipFreeAsync(lut, s);
    if (rc) return rc;
    HIPCHK(e);
    return GF_OK;
}

int gf_clahe_batch(const uint8_t* src, uint8_t* dst, int batch, int width, int height, double clip_limit, int tiles_x, int tiles_y) {
    if (!src || !dst) return gf::set_err(GF_ERR_INVALID, "null argument");
    gfclahe::Geom g;
    if (int rc = gf::clahe_geom(width, height, clip_limit, tiles_x, tiles_y, g)) return rc;
    if (batch < 1) return gf::set_err(GF_ERR_INVALID, "clahe: batch %d", batch);
    if (int rc = gf::require_device()) return rc;
    const size_t bytes = (size_t)batch * width * height;
    gf::DevBuf<uint8_t> d;
    HIPCHK(d.fit(bytes));
    HIPCHK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    if (int rc = gf_clahe_batch_device(d.p, d.p, batch, width, height, clip_limit, tiles_x, tiles_y, nullptr)) return rc;
    HIPCHK(hipMemcpy(dst, d.p, bytes, hipMemcpyDeviceToHost));
    return GF_OK;
}

}  // extern "C"
