// gf_cvt.hip — cv_bridge::toCvCopy(img_msg, MONO8) on batches of colour, Bayer, YUV 4:2:2, 16-bit and u8 frames on the device (getImageFromMsg, rosNodeTest.cpp:238-254: the step of the reference's
// node ahead of CLAHE and trackImage).  Kernels: gf_cvt_kernels.hpp; arithmetic and channel layouts: gf_pixfmt.hpp, shared with the host decoder.  Used by the
// tracker (gf_tracker_cfg.pixel_format) and exported as its own C-ABI.
#include <hip/hip_runtime.h>
#include <climits>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/groundfusion_hip.h"
#include "gf_cvt_kernels.hpp"
#include "gf_hip_own.hpp"

namespace gf {

// format, sizes and pitch of a conversion, or GF_ERR_INVALID
static int cvt_check(size_t src_pitch, int format, int batch, int w, int h) {
    if (!gfpix::valid(format)) return set_err(GF_ERR_INVALID, "cvt_gray: unknown pixel format %d (GF_PIX_MONO8 .. GF_PIX_BGRA8, GF_PIX_BAYER_RGGB8 .. GF_PIX_MONO16)", format);
    if (batch < 1 || w < 1 || h < 1) return set_err(GF_ERR_INVALID, "cvt_gray: %d frames of %dx%d (all must be >= 1)", batch, w, h);
    if (w < gfpix::min_side(format) || h < gfpix::min_side(format)) return set_err(GF_ERR_INVALID, "cvt_gray: a Bayer frame of %dx%d has no interior pixel (width and height must be >= 3)", w, h);
    if ((long long)w * h > INT_MAX) return set_err(GF_ERR_INVALID, "cvt_gray: %dx%d frames have more than 2^31 - 1 pixels", w, h);
    if (src_pitch < (size_t)w * gfpix::channels(format)) return set_err(GF_ERR_INVALID, "cvt_gray: a pitch of %zu bytes is shorter than a row of %d pixels of %d bytes", src_pitch, w, gfpix::channels(format));
    return GF_OK;
}

// bytes from the first the conversion reads to behind the last: the last row ends with its pixels, not with its padding
static size_t cvt_src_bytes(size_t src_pitch, int format, int batch, int w, int h) { return ((size_t)batch * h - 1) * src_pitch + (size_t)w * gfpix::channels(format); }

template <int CH> static void cvt_launch_ch(const uint8_t* d_src, size_t src_pitch, int red_at, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream) {
    using namespace gfcvt;
    const unsigned gy = (unsigned)std::min(batch, 65535);
    const bool dwords = !((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst) | src_pitch | (size_t)w) & 3);
    auto blocks = [&](int per_row) { return (unsigned)(((size_t)per_row * h + kThreads - 1) / kThreads); };
    if (dwords && !(w & 15)) cvt_gray_vec_kernel<CH, 16><<<dim3(blocks(w / 16), gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, red_at);
    else if (dwords) cvt_gray_vec_kernel<CH, 4><<<dim3(blocks(w / 4), gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, red_at);
    else cvt_gray_byte_kernel<CH><<<dim3(blocks(w), gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, red_at);
}

// YUV 4:2:2 and MONO16 (two bytes per pixel) and Bayer: form and grid from gfcvt::raw_plan
template <bool M16> static void cvt_launch_pair(const uint8_t* d_src, size_t src_pitch, int luma_at, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream) {
    using namespace gfcvt;
    const RawPlan pl = raw_plan(false, d_src, src_pitch, d_dst, batch, w, h);
    if (pl.form == 16) cvt_pair_vec_kernel<M16, 16><<<dim3(pl.gx, pl.gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, luma_at);
    else if (pl.form == 4) cvt_pair_vec_kernel<M16, 4><<<dim3(pl.gx, pl.gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, luma_at);
    else cvt_pair_byte_kernel<M16><<<dim3(pl.gx, pl.gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, luma_at);
}
static void cvt_launch_bayer(const uint8_t* d_src, size_t src_pitch, int format, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream) {
    using namespace gfcvt;
    const RawPlan pl = raw_plan(true, d_src, src_pitch, d_dst, batch, w, h);
    const int gf = gfpix::bayer_green_first(format), br = gfpix::bayer_blue_row0(format);
    if (pl.form == 4) cvt_bayer_vec_kernel<<<dim3(pl.gx, pl.gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, gf, br);
    else cvt_bayer_byte_kernel<<<dim3(pl.gx, pl.gy), kThreads, 0, stream>>>(d_src, src_pitch, d_dst, batch, w, h, gf, br);
}

// `batch` frames of h rows, src_pitch bytes apart, in `format` -> tight h x w u8 frames; the ranges must not overlap (the callers see to it)
int cvt_launch(const uint8_t* d_src, size_t src_pitch, int format, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream) {
    if (int rc = cvt_check(src_pitch, format, batch, w, h)) return rc;
    const int ch = gfpix::channels(format), red_at = gfpix::red_at(format);
    if (gfpix::is_bayer(format)) cvt_launch_bayer(d_src, src_pitch, format, d_dst, batch, w, h, stream);
    else if (format == GF_PIX_MONO16) cvt_launch_pair<true>(d_src, src_pitch, 0, d_dst, batch, w, h, stream);
    else if (ch == 2) cvt_launch_pair<false>(d_src, src_pitch, gfpix::luma_at(format), d_dst, batch, w, h, stream);
    else if (ch == 1) cvt_launch_ch<1>(d_src, src_pitch, red_at, d_dst, batch, w, h, stream);
    else if (ch == 3) cvt_launch_ch<3>(d_src, src_pitch, red_at, d_dst, batch, w, h, stream);
    else cvt_launch_ch<4>(d_src, src_pitch, red_at, d_dst, batch, w, h, stream);
    HIPCHK(hipGetLastError());
    return GF_OK;
}

// The same conversion with the frames where the caller keeps them: d_refs[b] (device-readable, [batch]) names frame b, h_refs is the same table as the host reads
// it (the caller has checked its entries: gfref::check).  Each frame takes the form its own pointer and pitch allow; the launch of a form is left out when no
// frame of the call takes it.  *n_bytes (optional): the frames that took a byte form although the size has a dword form.
int cvt_launch_refs(const gf_frame_ref* d_refs, const gf_frame_ref* h_refs, int format, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream, int* n_bytes) {
    using namespace gfcvt;
    if (int rc = cvt_check((size_t)w * gfpix::channels(format), format, batch, w, h)) return rc;
    const int ch = gfpix::channels(format), red_at = gfpix::red_at(format);
    const bool bayer = gfpix::is_bayer(format);
    const bool dst_dwords = !((reinterpret_cast<uintptr_t>(d_dst) | (size_t)w) & 3) && (!bayer || w >= 8);   // the part of raw_dwords() that is not the frame's
    int n_dw = 0;
    for (int b = 0; b < batch; b++) n_dw += gfref::form(reinterpret_cast<uintptr_t>(h_refs[b].data), h_refs[b].pitch) >= 4 ? 1 : 0;
    if (!dst_dwords) n_dw = 0;
    const int n_by = batch - n_dw;
    if (n_bytes) *n_bytes = dst_dwords ? n_by : 0;
    const int byte_want = dst_dwords ? 0 : -1;
    const unsigned gy = (unsigned)std::min(batch, 65535);
    const int npx = bayer ? 4 : !(w & 15) ? 16 : 4;
    const dim3 gv(bayer ? raw_blocks((size_t)w / 4, ((size_t)h + kBayerBand - 1) / kBayerBand) : raw_blocks((size_t)w / npx, (size_t)h), gy), gb(raw_blocks((size_t)w, (size_t)h), gy);
    auto gray = [&](auto chc) {
        constexpr int CH = decltype(chc)::value;
        if (n_dw && npx == 16) cvt_gray_vec_refs_kernel<CH, 16><<<gv, kThreads, 0, stream>>>(d_refs, 1, d_dst, batch, w, h, red_at);
        else if (n_dw) cvt_gray_vec_refs_kernel<CH, 4><<<gv, kThreads, 0, stream>>>(d_refs, 1, d_dst, batch, w, h, red_at);
        if (n_by) cvt_gray_byte_refs_kernel<CH><<<gb, kThreads, 0, stream>>>(d_refs, byte_want, d_dst, batch, w, h, red_at);
    };
    auto pair = [&](auto m16c, int luma_at) {
        constexpr bool M16 = decltype(m16c)::value;
        if (n_dw && npx == 16) cvt_pair_vec_refs_kernel<M16, 16><<<gv, kThreads, 0, stream>>>(d_refs, 1, d_dst, batch, w, h, luma_at);
        else if (n_dw) cvt_pair_vec_refs_kernel<M16, 4><<<gv, kThreads, 0, stream>>>(d_refs, 1, d_dst, batch, w, h, luma_at);
        if (n_by) cvt_pair_byte_refs_kernel<M16><<<gb, kThreads, 0, stream>>>(d_refs, byte_want, d_dst, batch, w, h, luma_at);
    };
    if (bayer) {
        const int gf = gfpix::bayer_green_first(format), br = gfpix::bayer_blue_row0(format);
        if (n_dw) cvt_bayer_vec_refs_kernel<<<gv, kThreads, 0, stream>>>(d_refs, 1, d_dst, batch, w, h, gf, br);
        if (n_by) cvt_bayer_byte_refs_kernel<<<gb, kThreads, 0, stream>>>(d_refs, byte_want, d_dst, batch, w, h, gf, br);
    } else if (format == GF_PIX_MONO16) pair(std::true_type{}, 0);
    else if (ch == 2) pair(std::false_type{}, gfpix::luma_at(format));
    else if (ch == 1) gray(std::integral_constant<int, 1>{});
    else if (ch == 3) gray(std::integral_constant<int, 3>{});
    else gray(std::integral_constant<int, 4>{});
    HIPCHK(hipGetLastError());
    return GF_OK;
}

// One format per frame (gf_cvt_kernels.hpp, cvt_mixed_kernel): frame b lies at d_refs[b] in d_formats[b] and goes to the tight frame b of d_dst; an entry that is
// no GF_PIX_* is skipped.  h_refs / h_formats: the same tables as the host reads them (the tracker's page-locked ones), or null where the host cannot read them
// (gf_cvt_gray_mixed_device).  With them the grid is the largest any listed frame needs, a call without a frame to convert launches nothing and the Bayer part
// is launched only where a Bayer frame is listed; without them the grid is that of the widest form of the size (narrower frames take several turns) and both
// parts are launched.  Two launches at the most, whatever the formats and however long the list: the streaming formats keep the registers and the occupancy of
// their homogeneous kernels, which the Bayer stencil would cost them ("Formats per sequence").
int cvt_launch_mixed(const gf_frame_ref* d_refs, const int* d_formats, const gf_frame_ref* h_refs, const int* h_formats, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream) {
    using namespace gfcvt;
    if (batch < 1 || w < 1 || h < 1) return set_err(GF_ERR_INVALID, "cvt_gray_mixed: %d frames of %dx%d (all must be >= 1)", batch, w, h);
    if ((long long)w * h > INT_MAX) return set_err(GF_ERR_INVALID, "cvt_gray_mixed: %dx%d frames have more than 2^31 - 1 pixels", w, h);
    const int dst_dwords = !((reinterpret_cast<uintptr_t>(d_dst) | (size_t)w) & 3) ? 1 : 0;
    unsigned gx_stream = 0, gx_bayer = 0;
    if (h_refs && h_formats) {
        for (int b = 0; b < batch; b++) {
            const int f = h_formats[b];
            if (!gfpix::valid(f)) continue;
            const unsigned need = mixed_blocks(f, mixed_form(f, h_refs[b].data, h_refs[b].pitch, dst_dwords, w), w, h);
            if (gfpix::is_bayer(f)) gx_bayer = std::max(gx_bayer, need); else gx_stream = std::max(gx_stream, need);
        }
    } else {
        gx_stream = mixed_blocks(GF_PIX_MONO8, dst_dwords ? ((w & 15) ? 4 : 16) : 1, w, h);
        if (w >= 3 && h >= 3) gx_bayer = mixed_blocks(GF_PIX_BAYER_RGGB8, dst_dwords && w >= 8 ? 4 : 1, w, h);
    }
    const unsigned gy = (unsigned)std::min(batch, 65535);
    if (gx_stream) cvt_mixed_kernel<1><<<dim3(gx_stream, gy), kThreads, 0, stream>>>(d_refs, d_formats, d_dst, batch, w, h, dst_dwords);
    if (gx_bayer) cvt_mixed_kernel<2><<<dim3(gx_bayer, gy), kThreads, 0, stream>>>(d_refs, d_formats, d_dst, batch, w, h, dst_dwords);
    HIPCHK(hipGetLastError());
    return GF_OK;
}

}  // namespace gf

extern "C" {

int gf_cvt_gray_batch_device(const void* d_src, size_t src_pitch, int format, void* d_dst, int batch, int width, int height, void* stream) {
    if (!d_src || !d_dst) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::cvt_check(src_pitch, format, batch, width, height)) return rc;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), s1 = s0 + gf::cvt_src_bytes(src_pitch, format, batch, width, height);
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(d_dst), d1 = d0 + (size_t)batch * width * height;
    const bool same_tight_mono = format == GF_PIX_MONO8 && s0 == d0 && src_pitch == (size_t)width;   // every lane writes back what it read
    if (s0 < d1 && d0 < s1 && !same_tight_mono)
        return gf::set_err(GF_ERR_INVALID, "cvt_gray: source and destination overlap (the conversion shrinks the frames: a lane would read what another has written)");
    return gf::cvt_launch(static_cast<const uint8_t*>(d_src), src_pitch, format, static_cast<uint8_t*>(d_dst), batch, width, height, static_cast<hipStream_t>(stream));
}

int gf_cvt_gray_batch(const uint8_t* src, size_t src_pitch, int format, uint8_t* dst, int batch, int width, int height) {
    if (!src || !dst) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::cvt_check(src_pitch, format, batch, width, height)) return rc;
    const size_t in = gf::cvt_src_bytes(src_pitch, format, batch, width, height), out = (size_t)batch * width * height;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    if (format != GF_PIX_MONO8 && s0 < d0 + out && d0 < s0 + in) return gf::set_err(GF_ERR_INVALID, "cvt_gray: source and destination overlap");
    if (int rc = gf::require_device()) return rc;
    gf::DevBuf<uint8_t> d_in, d_out;
    HIPCHK(d_in.fit(in)); HIPCHK(d_out.fit(out));
    HIPCHK(hipMemcpy(d_in.p, src, in, hipMemcpyHostToDevice));
    if (int rc = gf_cvt_gray_batch_device(d_in.p, src_pitch, format, d_out.p, batch, width, height, nullptr)) return rc;
    HIPCHK(hipMemcpy(dst, d_out.p, out, hipMemcpyDeviceToHost));
    return GF_OK;
}

int gf_cvt_gray_mixed_device(const gf_frame_ref* d_refs, const int* d_formats, void* d_dst, int batch, int width, int height, void* stream) {
    if (!d_refs || !d_formats || !d_dst) return gf::set_err(GF_ERR_INVALID, "cvt_gray_mixed: null argument");
    return gf::cvt_launch_mixed(d_refs, d_formats, nullptr, nullptr, static_cast<uint8_t*>(d_dst), batch, width, height, static_cast<hipStream_t>(stream));
}

int gf_cvt_gray_mixed(const uint8_t* const* src, const size_t* pitch, const int* format, uint8_t* dst, int batch, int width, int height) {
    if (!src || !pitch || !format || !dst) return gf::set_err(GF_ERR_INVALID, "cvt_gray_mixed: null argument");
    if (batch < 1 || width < 1 || height < 1) return gf::set_err(GF_ERR_INVALID, "cvt_gray_mixed: %d frames of %dx%d (all must be >= 1)", batch, width, height);
    const size_t px = (size_t)width * height, out = (size_t)batch * px;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst);
    std::vector<size_t> at(batch), bytes(batch);
    size_t in = 0;
    for (int b = 0; b < batch; b++) {   // everything gf_cvt_gray_batch refuses, per frame
        if (!src[b]) return gf::set_err(GF_ERR_INVALID, "cvt_gray_mixed: frame %d: null source", b);
        if (gf::cvt_check(pitch[b], format[b], 1, width, height)) return gf::set_err(GF_ERR_INVALID, "cvt_gray_mixed: frame %d: %s", b, std::string(gf_last_error()).c_str());
        bytes[b] = gf::cvt_src_bytes(pitch[b], format[b], 1, width, height);
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(src[b]);
        if (s0 < d0 + out && d0 < s0 + bytes[b]) return gf::set_err(GF_ERR_INVALID, "cvt_gray_mixed: frame %d: source and destination overlap", b);
        at[b] = ((in + 15) & ~(size_t)15) + (s0 & 15);   // the device copy keeps the host pointer's phase: the frame takes the form it would take where it lies
        in = at[b] + bytes[b];
    }
    if (int rc = gf::require_device()) return rc;
    gf::DevBuf<uint8_t> d_in, d_out, d_tab;
    const size_t tab = (size_t)batch * (sizeof(gf_frame_ref) + sizeof(int));
    HIPCHK(d_in.fit(in)); HIPCHK(d_out.fit(out)); HIPCHK(d_tab.fit(tab));
    std::vector<uint8_t> h_tab(tab);
    gf_frame_ref* refs = reinterpret_cast<gf_frame_ref*>(h_tab.data());
    int* fmts = reinterpret_cast<int*>(refs + batch);
    for (int b = 0; b < batch; b++) {
        HIPCHK(hipMemcpy(d_in.p + at[b], src[b], bytes[b], hipMemcpyHostToDevice));
        refs[b] = gf_frame_ref{d_in.p + at[b], pitch[b]};
        fmts[b] = format[b];
    }
    HIPCHK(hipMemcpy(d_tab.p, h_tab.data(), tab, hipMemcpyHostToDevice));
    const gf_frame_ref* d_refs = reinterpret_cast<const gf_frame_ref*>(d_tab.p);
    if (int rc = gf::cvt_launch_mixed(d_refs, reinterpret_cast<const int*>(d_refs + batch), refs, fmts, d_out.p, batch, width, height, nullptr)) return rc;
    HIPCHK(hipMemcpy(dst, d_out.p, out, hipMemcpyDeviceToHost));
    return GF_OK;
}

}  // extern "C"
