// gf_roi.hpp — the region of interest of a tracker sequence as the detector reads it: one bit per pixel, in the geometry of detect_strip_kernel's strips.
// A sequence's table is [band = y / kRows][x] 32-bit words, bit r of a word = pixel (x, band * kRows + r) is allowed; bits of rows past the image are 0.
// A lane of a strip owns one column of one band, so its whole share of the region is one word, and the 64 lanes of a wavefront load 64 neighbouring words.
// One source for the host setter (gf_tracker_set_roi packs on the host), the packing kernel of the device setter (roi_pack_kernel, gf_detect_kernels.hpp) and
// setMask's test of a tracked point (set_mask_host): both setters leave the same bits because they run the same function.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/groundfusion_hip.h"   // gf_box

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GF_ROI_HD __host__ __device__ __forceinline__
#else
#define GF_ROI_HD inline
#endif

namespace gfroi {

constexpr int kRows = 30;   // rows per band = rows per strip of the detector (kDS_R, gf_detect_kernels.hpp, which asserts the two are one number)
static_assert(kRows >= 1 && kRows <= 32, "one bit per row of a band in a 32-bit word");

GF_ROI_HD int bands(int h) { return (h + kRows - 1) / kRows; }
GF_ROI_HD size_t words(int w, int h) { return (size_t)bands(h) * (size_t)w; }          // words of one sequence's table
GF_ROI_HD size_t word_at(int w, int band, int x) { return (size_t)band * (size_t)w + (size_t)x; }
GF_ROI_HD int rows_of_band(int h, int band) { const int n = h - band * kRows; return n < kRows ? n : kRows; }   // the last band may be short

// The word of column x of one band: col points at pixel (x, band * kRows) of a byte image whose rows lie `stride` bytes apart, nrows = rows_of_band().
// Non-zero = allowed (the mask convention of OpenCV and of goodFeaturesToTrack).
GF_ROI_HD uint32_t pack_word(const uint8_t* col, size_t stride, int nrows) {
    uint32_t w = 0;
    for (int r = 0; r < nrows; r++) w |= (uint32_t)(col[(size_t)r * stride] != 0) << r;
    return w;
}

// One thread of the packing grid (roi_pack_kernel; the host setter loops over the same function): the word of column x of band `band` of the h x w byte image
// `mask`, rows `stride` bytes apart, into a sequence's table.  Reads mask[(band * kRows + r) * stride + x] for r < rows_of_band(): rows < h and columns < w only,
// for every band < bands(h); threads with x >= w (the tail of the last block) do nothing.
GF_ROI_HD void pack_thread(const uint8_t* mask, size_t stride, int w, int h, int band, int x, uint32_t* table) {
    if (x >= w) return;
    table[word_at(w, band, x)] = pack_word(mask + (size_t)band * kRows * stride + x, stride, rows_of_band(h, band));
}

// `mask.at<uchar>(y, x) != 0` on a packed table
GF_ROI_HD bool allowed(const uint32_t* table, int w, int x, int y) {
    const int band = y / kRows;
    return (table[word_at(w, band, x)] >> (y - band * kRows)) & 1u;
}

// ---- exclusion boxes (gf_box, gf_tracker_set_boxes_some; DESIGN.md section 4, "Exclusion boxes").  A sequence's region in force is
//   R_eff = R_base AND NOT union(boxes),
// a box excluding the pixels xmin <= x <= xmax && ymin <= y <= ymax of the frame.  Any int32_t is a coordinate: a box is clipped to the frame (band) by comparisons
// before anything is added or subtracted, so INT32_MIN / INT32_MAX corners overflow nothing, and a box with xmin > xmax or ymin > ymax clips to nothing.
// One copy for the composing kernel (roi_boxes_kernel, gf_detect_kernels.hpp), gf_tracker_get_roi, setMask's walk and tests/native/roi_boxes_host.cpp.

// The rows of band `band` of an h-row frame that the box covers, as bits of the band's words: the same for every column of the band.
GF_ROI_HD uint32_t box_rows(const gf_box& b, int h, int band) {
    const int y0 = band * kRows, y1 = y0 + rows_of_band(h, band) - 1;   // the band's first and last row, inside the frame
    const int lo = b.ymin > y0 ? b.ymin : y0, hi = b.ymax < y1 ? b.ymax : y1;
    if (lo > hi) return 0;
    const int n = hi - lo + 1;   // 1 .. kRows
    return (n >= 32 ? ~0u : (1u << n) - 1u) << (lo - y0);
}
// The columns of a w-column frame that the box covers: x0 .. x1; false: none
GF_ROI_HD bool box_cols(const gf_box& b, int w, int& x0, int& x1) {
    x0 = b.xmin > 0 ? b.xmin : 0;
    x1 = b.xmax < w - 1 ? b.xmax : w - 1;
    return x0 <= x1;
}
// The bits of the word of (band, x) that the list excludes
GF_ROI_HD uint32_t covered_word(const gf_box* boxes, int n, int w, int h, int band, int x) {
    uint32_t covered = 0;
    for (int i = 0; i < n; i++) {
        int x0, x1;
        if (box_cols(boxes[i], w, x0, x1) && x >= x0 && x <= x1) covered |= box_rows(boxes[i], h, band);
    }
    return covered;
}
// The table word of (band, x) under a box list: the base table's word (all ones for a sequence without a base region) minus what the boxes cover
GF_ROI_HD uint32_t compose_word(uint32_t base_word, uint32_t covered) { return base_word & ~covered; }
GF_ROI_HD uint32_t box_word(uint32_t base_word, const gf_box* boxes, int n, int w, int h, int band, int x) {
    return compose_word(base_word, covered_word(boxes, n, w, h, band, x));
}
// `R_eff.at<uchar>(y, x) != 0` for a pixel of the frame without a composed table: the base table (null: all allowed) and the list
GF_ROI_HD bool allowed(const uint32_t* base_table_or_null, const gf_box* boxes, int n, int w, int x, int y) {
    if (base_table_or_null && !allowed(base_table_or_null, w, x, y)) return false;
    for (int i = 0; i < n; i++)
        if (x >= boxes[i].xmin && x <= boxes[i].xmax && y >= boxes[i].ymin && y <= boxes[i].ymax) return false;
    return true;
}

}  // namespace gfroi
