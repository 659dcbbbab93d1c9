// gf_seq_format.hpp — the pixel format and the equalise switch a sequence of a tracker handle may have of its own (gf_tracker_seq_format,
// include/groundfusion_hip.h): what the reference's node does per camera ahead of trackImage, cv_bridge::toCvCopy(msg, MONO8) and the CLAHE of getImageFromMsg
// (rosNodeTest.cpp:238-261).  Plain C++, no HIP types: the limits the setter checks and the plan of a call -- where each listed frame lies, which stage reads
// what, where it writes -- in one place that the setter, the track calls and a stand-alone host program (tests/native/seq_format_host.cpp) share.
//
// The front of a frame has three stages, each reading what the one before it left: conversion to MONO8, equalisation, pyramid.  Per list position i:
//   converted  iff the sequence's format is not GF_PIX_MONO8: from the caller's frame into slot i of the conversion buffer ([batch] tight frames)
//   equalised  iff its switch is on: from the conversion slot, or from the caller's frame where nothing was converted, into slot eq_index[i] of the equalisation
//              buffer; the equalised positions are numbered 0 .. n_eq - 1 in list order, because the CLAHE launch walks a dense table and owns one set of LUTs per entry
//   pyramid    reads the slot the last stage wrote, or the caller's frame itself for a MONO8 sequence without equalisation: that frame is not copied
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_pixfmt.hpp"

namespace gfseqfmt {

constexpr int kClaheTiles = 8;   // cv::createCLAHE() defaults (rosNodeTest.cpp:258): a frame must be wider and higher than the grid

// the handle's own values: what a sequence that was never set runs with
inline gf_tracker_seq_format of_handle(const gf_tracker_cfg& c) {
    gf_tracker_seq_format f{};
    f.pixel_format = c.pixel_format; f.equalize = c.equalize; f.host_stride = 0;
    return f;
}

inline size_t row_bytes(int w, int format) { return (size_t)w * (size_t)gfpix::channels(format); }
inline size_t frame_bytes(int w, int h, int format) { return row_bytes(w, format) * (size_t)h; }

// True if a sequence of a w x h handle can have `f`; otherwise a message that names the field.
inline bool fits(int w, int h, const gf_tracker_seq_format& f, char* msg, size_t n) {
    if (!gfpix::valid(f.pixel_format)) { snprintf(msg, n, "gf_tracker_seq_format.pixel_format must be one of GF_PIX_MONO8 (0) .. GF_PIX_BGRA8 (4) or GF_PIX_BAYER_RGGB8 (8) .. GF_PIX_MONO16 (14), got %d", f.pixel_format); return false; }
    if (w < gfpix::min_side(f.pixel_format) || h < gfpix::min_side(f.pixel_format)) { snprintf(msg, n, "gf_tracker_seq_format.pixel_format %d: a Bayer frame of %dx%d has no interior pixel (width and height must be >= 3)", f.pixel_format, w, h); return false; }
    if (f.equalize != 0 && f.equalize != 1) { snprintf(msg, n, "gf_tracker_seq_format.equalize must be 0 or 1, got %d", f.equalize); return false; }
    if (f.equalize && (w <= kClaheTiles || h <= kClaheTiles)) { snprintf(msg, n, "gf_tracker_seq_format.equalize: a frame of %dx%d is not larger than the %d x %d grid", w, h, kClaheTiles, kClaheTiles); return false; }
    if (f.host_stride < 0) { snprintf(msg, n, "gf_tracker_seq_format.host_stride must be >= 0, got %d", f.host_stride); return false; }
    if (f.host_stride && (size_t)f.host_stride < row_bytes(w, f.pixel_format)) { snprintf(msg, n, "gf_tracker_seq_format.host_stride %d is shorter than a row of %d pixels of %d bytes", f.host_stride, w, gfpix::channels(f.pixel_format)); return false; }
    return true;
}

// the row step of a sequence's host frames on a call with `call_stride`
inline long long host_stride(const gf_tracker_seq_format& f, int call_stride) { return f.host_stride ? f.host_stride : call_stride; }

// The plan of one call.  Everything is indexed by the list position i unless it says otherwise; the vectors keep their capacity from call to call.
struct Plan {
    int count = 0;
    bool homogeneous = true;          // every listed sequence runs with the handle's own format and switch: the call takes the code path of a handle without settings
    int n_cvt = 0, n_eq = 0;          // listed sequences that are converted / equalised
    size_t total_bytes = 0;           // of the listed frames back to back
    std::vector<int> format, equalize;
    std::vector<size_t> bytes, offset;      // of frame i, and where it starts in a tight device block or in the staging buffer: the sum of the frames before it
    std::vector<int> cvt_format;            // what the conversion kernel reads for entry i: the format, or -1 (skip: MONO8 needs none); the slot is i
    std::vector<int> eq_index;              // the slot of the equalisation buffer and the LUTs, or -1
    std::vector<gf_frame_ref> cvt_src;      // [count]: the caller's frame (data = null on a skipped entry)
    std::vector<gf_frame_ref> eq_src;       // [n_eq], by eq_index
    std::vector<gf_frame_ref> pyr_src;      // [count]
};

// formats, sizes and slots of the listed sequences; fmt[seq]: what is in force for each sequence of the handle, own: the handle's own values
inline void plan_list(Plan& p, const gf_tracker_seq_format* fmt, const gf_tracker_seq_format& own, int count, const int* seq, int w, int h) {
    p.count = count; p.homogeneous = true; p.n_cvt = p.n_eq = 0; p.total_bytes = 0;
    p.format.resize(count); p.equalize.resize(count); p.bytes.resize(count); p.offset.resize(count); p.cvt_format.resize(count); p.eq_index.resize(count);
    for (int i = 0; i < count; i++) {
        const gf_tracker_seq_format& f = fmt[seq[i]];
        p.format[i] = f.pixel_format; p.equalize[i] = f.equalize;
        if (f.pixel_format != own.pixel_format || f.equalize != own.equalize) p.homogeneous = false;
        p.bytes[i] = frame_bytes(w, h, f.pixel_format);
        p.offset[i] = p.total_bytes;
        p.total_bytes += p.bytes[i];
        p.cvt_format[i] = f.pixel_format != GF_PIX_MONO8 ? f.pixel_format : -1;
        if (p.cvt_format[i] >= 0) p.n_cvt++;
        p.eq_index[i] = f.equalize ? p.n_eq++ : -1;
    }
}

// the frames of a tight block at `base` as one pointer and pitch each (frames[count])
inline void tight_frames(const Plan& p, const void* base, int w, gf_frame_ref* frames) {
    for (int i = 0; i < p.count; i++) frames[i] = gf_frame_ref{static_cast<const uint8_t*>(base) + p.offset[i], row_bytes(w, p.format[i])};
}

// what each stage reads: frames[i] is where the caller's frame of position i lies; cvt_buf / eq_buf: the handle's [batch] tight MONO8 frames
inline void plan_sources(Plan& p, const gf_frame_ref* frames, const void* cvt_buf, const void* eq_buf, int w, int h) {
    const size_t px = (size_t)w * h;
    p.cvt_src.resize(p.count); p.pyr_src.resize(p.count); p.eq_src.resize(p.n_eq);
    for (int i = 0; i < p.count; i++) {
        gf_frame_ref cur = frames[i];
        if (p.cvt_format[i] >= 0) { p.cvt_src[i] = cur; cur = gf_frame_ref{static_cast<const uint8_t*>(cvt_buf) + (size_t)i * px, (size_t)w}; }
        else p.cvt_src[i] = gf_frame_ref{nullptr, 0};
        if (p.eq_index[i] >= 0) { p.eq_src[p.eq_index[i]] = cur; cur = gf_frame_ref{static_cast<const uint8_t*>(eq_buf) + (size_t)p.eq_index[i] * px, (size_t)w}; }
        p.pyr_src[i] = cur;
    }
}

}  // namespace gfseqfmt
