// gf_roi.hpp — the region of interest of a tracker sequence as the detector reads it: one bit per pixel, in the geometry of detect_strip_kernel's strips.
// A sequence's table is [band = y / kRows][x] 32-bit words, bit r of a word = pixel (x, band * kRows + r) is allowed; bits of rows past the image are 0.
// A lane of a strip owns one column of one band, so its whole share of the region is one word, and the 64 lanes of a wavefront load 64 neighbouring words.
// One source for the host setter (gf_tracker_set_roi packs on the host), the packing kernel of the device setter (roi_pack_kernel, gf_detect_kernels.hpp) and
// setMask's test of a tracked point (set_mask_host): both setters leave the same bits because they run the same function.
#pragma once
#include <stddef.h>
#include <stdint.h>

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

}  // namespace gfroi
