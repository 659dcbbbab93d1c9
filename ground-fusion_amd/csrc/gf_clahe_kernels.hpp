// gf_clahe_kernels.hpp — contrast-limited adaptive histogram equalisation of u8 frames (cv::CLAHE::apply on CV_8UC1, OpenCV 4.2 modules/imgproc/src/clahe.cpp:
// CLAHE_CalcLut_Body + CLAHE_Interpolation_Body, scalar path), batched over contiguous frames.  Included by gf_clahe.hip only.
//
// Two launches per call:
//   clahe_lut_kernel    one workgroup per (tile, frame): histogram of the tile in LDS (one sub-histogram per wavefront), clip + redistribution, prefix sum,
//                       u8 LUT of 256 entries to lut[frame][tile].
//   clahe_apply_kernel  one workgroup per (band of rows, frame): the band's LUT tile rows staged in LDS, bilinear blend of the four tile LUTs around each pixel.
// Every float expression below is written in the order the OpenCV scalar code evaluates it; the translation unit is compiled with -ffp-contract=off (build.py),
// so nothing is fused and the results are the same bits.
// Inside the tracker a "frame" is a position in the call's sequence list (gf_lk_kernels.hpp): source frames, equalised frames and LUTs all belong to the call and
// none of them is kept per sequence, so both passes run over the first `count` frames of their buffers and need no table to find them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gf_frame_ref.hpp"

namespace gfclahe {

constexpr int kThreads = 256;   // = the number of histogram bins: thread t owns bin t in the clip and the scan

struct Geom {
    int w, h;            // frame size (the pixels that are equalised)
    int tx, ty;          // tile grid
    int tw, th;          // tile size (of the padded frame when the grid does not divide it)
    int clip;            // clip limit in pixels per bin; used when use_clip
    int use_clip;        // clipLimit > 0
    float lut_scale;     // 255.0f / (tw * th)
    float inv_tw, inv_th;  // 1.0f / tw, 1.0f / th (the interpolation multiplies by them, as OpenCV does)
};

// BORDER_REFLECT_101 on the right / bottom only (the padded frame extends the image there and nowhere else); p < 2n - 1 is guaranteed by w > tx, h > ty
__device__ __forceinline__ int reflect_hi(int p, int n) { return p < n ? p : 2 * (n - 1) - p; }

__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// vec4: w % 4 == 0, tw % 4 == 0 and src 4-byte aligned (every in-image quad is then one aligned u32)
// REFS (both passes): false -- the source frames are tight and back to back from src; true -- src is the call's table of gf_frame_ref (gfref::frame_at), and a
// frame whose pointer or pitch misses the alignment of the vector form is read byte by byte, block by block.  The LUTs and the equalised frames are the
// caller's tight buffers either way.
template <bool REFS>
__device__ __forceinline__ void clahe_lut_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ lut, const Geom& g, int vec4, unsigned (*hist)[256], int* red) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int tile = blockIdx.x, b = blockIdx.y;
    for (int k = 0; k < kThreads / 64; k++) hist[k][t] = 0;
    __syncthreads();
    const int X0 = (tile % g.tx) * g.tw, Y0 = (tile / g.tx) * g.th;
    const gfref::Frame fr = gfref::frame_at<REFS>(src, (size_t)g.w * g.h, (size_t)g.w, b);
    const uint8_t* f = fr.data;
    if (REFS) vec4 = vec4 && gfref::form(reinterpret_cast<uintptr_t>(fr.data), fr.pitch) >= 4;
    unsigned* hw = hist[wave];
    const int qw = (g.tw + 3) >> 2, n = qw * g.th;
    for (int i = t; i < n; i += kThreads) {
        const int r = i / qw, q = i - r * qw;
        const uint8_t* row = REFS ? f + (size_t)reflect_hi(Y0 + r, g.h) * fr.pitch : f + (size_t)reflect_hi(Y0 + r, g.h) * g.w;
        const int x0 = X0 + 4 * q;
        if (vec4 && x0 + 3 < g.w && 4 * q + 3 < g.tw) {
            const unsigned v = *reinterpret_cast<const unsigned*>(row + x0);
            atomicAdd(&hw[v & 255], 1u); atomicAdd(&hw[(v >> 8) & 255], 1u); atomicAdd(&hw[(v >> 16) & 255], 1u); atomicAdd(&hw[v >> 24], 1u);
        } else {
            for (int k = 0; k < 4; k++)
                if (4 * q + k < g.tw) atomicAdd(&hw[row[reflect_hi(x0 + k, g.w)]], 1u);
        }
    }
    __syncthreads();
    int c = 0;
    for (int k = 0; k < kThreads / 64; k++) c += (int)hist[k][t];
    if (g.use_clip) {
        // clahe.cpp: cut every bin at clipLimit, add excess / 256 to every bin, then +1 to bins 0, step, 2 step, ... while the residual lasts
        const int excess = c > g.clip ? c - g.clip : 0;
        c -= excess;
        const int ws = wave_sum(excess);
        if (lane == 0) red[wave] = ws;
        __syncthreads();
        int clipped = 0;
        for (int k = 0; k < kThreads / 64; k++) clipped += red[k];
        const int batch = clipped / 256, residual = clipped - batch * 256;
        c += batch;
        if (residual != 0) {
            const int step = max(256 / residual, 1);
            if (t % step == 0 && t / step < residual) c++;
        }
        __syncthreads();   // red[] is reused by the scan
    }
    // inclusive prefix sum over the 256 bins: within each wavefront, then the wavefront totals
    int s = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(s, o, 64);
        if (lane >= o) s += u;
    }
    if (lane == 63) red[wave] = s;
    __syncthreads();
    for (int k = 0; k < wave; k++) s += red[k];
    // saturate_cast<uchar>(sum * lutScale): int * float is a float, cvRound rounds half to even
    const int v = __float2int_rn((float)s * g.lut_scale);
    lut[((size_t)b * g.tx * g.ty + tile) * 256 + t] = (uint8_t)min(max(v, 0), 255);
}
__global__ __launch_bounds__(kThreads) void clahe_lut_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ lut, Geom g, int vec4) {
    __shared__ unsigned hist[kThreads / 64][256];
    __shared__ int red[kThreads / 64];
    clahe_lut_body<false>(src, lut, g, vec4, hist, red);
}
__global__ __launch_bounds__(kThreads) void clahe_lut_refs_kernel(const gf_frame_ref* __restrict__ refs, uint8_t* __restrict__ lut, Geom g, int vec4) {
    __shared__ unsigned hist[kThreads / 64][256];
    __shared__ int red[kThreads / 64];
    clahe_lut_body<true>(reinterpret_cast<const uint8_t*>(refs), lut, g, vec4, hist, red);
}

struct RowLut {   // what one row needs: the two tile-row LUT planes and the row weights
    const uint8_t *p1, *p2;
    float ya, ya1;
};

__device__ __forceinline__ int tile_row_of(int y, const Geom& g) { return (int)floorf((float)y * g.inv_th - 0.5f); }

// lut_rows: first tile row held by L and how many (bounds of the staged window); L points at that first row
__device__ __forceinline__ RowLut row_lut(int y, const Geom& g, const uint8_t* L, int row0, int nrows) {
    const float tyf = (float)y * g.inv_th - 0.5f;
    const int ty1 = (int)floorf(tyf);
    RowLut R;
    R.ya = tyf - (float)ty1;
    R.ya1 = 1.0f - R.ya;
    const int a = min(max(max(ty1, 0) - row0, 0), nrows - 1), c = min(max(min(ty1 + 1, g.ty - 1) - row0, 0), nrows - 1);
    R.p1 = L + (size_t)a * g.tx * 256;
    R.p2 = L + (size_t)c * g.tx * 256;
    return R;
}

__device__ __forceinline__ uint8_t clahe_px(const RowLut& R, int x, int v, const Geom& g) {
    const float txf = (float)x * g.inv_tw - 0.5f;
    const int tx1 = (int)floorf(txf);
    const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
    const int i1 = min(max(tx1, 0), g.tx - 1) * 256 + v, i2 = min(tx1 + 1, g.tx - 1) * 256 + v;
    const float res = ((float)R.p1[i1] * xa1 + (float)R.p1[i2] * xa) * R.ya1 + ((float)R.p2[i1] * xa1 + (float)R.p2[i2] * xa) * R.ya;
    return (uint8_t)min(max(__float2int_rn(res), 0), 255);
}

// kVec16: w % 16 == 0 and src / dst 16-byte aligned: 16 pixels per load and store.  kLds: the band's tile rows of LUTs (at most lds_rows of them) go to LDS first;
// otherwise the LUTs are read from global memory (grids too wide for LDS).  src == dst is allowed: every pixel is read and written by the same thread.
template <bool kVec16, bool kLds, bool REFS>
__device__ __forceinline__ void clahe_apply_body(const uint8_t* src, uint8_t* dst, const uint8_t* __restrict__ lut, const Geom& g, int band, int lds_rows) {
    extern __shared__ __align__(16) uint8_t slut[];
    const int b = blockIdx.y, y0 = blockIdx.x * band, y1 = min(y0 + band, g.h);
    const size_t plane = (size_t)g.tx * 256;
    const uint8_t* flut = lut + (size_t)b * g.ty * plane;
    int row0 = 0, nrows = g.ty;
    const uint8_t* L = flut;
    if (kLds) {
        row0 = max(tile_row_of(y0, g), 0);
        const int last = min(tile_row_of(y1 - 1, g) + 1, g.ty - 1);
        nrows = min(last - row0 + 1, lds_rows);
        const uint4* s4 = reinterpret_cast<const uint4*>(flut + row0 * plane);
        uint4* d4 = reinterpret_cast<uint4*>(slut);
        const int n16 = (int)(nrows * plane / 16);
        for (int i = threadIdx.x; i < n16; i += kThreads) d4[i] = s4[i];
        __syncthreads();
        L = slut;
    }
    const size_t fo = (size_t)b * g.w * g.h;
    const gfref::Frame fr = gfref::frame_at<REFS>(src, (size_t)g.w * g.h, (size_t)g.w, b);   // the source frame; the destination stays dst + fo, rows g.w apart
    if (kVec16 && (!REFS || gfref::form(reinterpret_cast<uintptr_t>(fr.data), fr.pitch) == 16)) {
        const int upr = g.w >> 4, n = (y1 - y0) * upr;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int r = i / upr, u = i - r * upr, y = y0 + r;
            const RowLut R = row_lut(y, g, L, row0, nrows);
            const size_t o = fo + (size_t)y * g.w + 16 * u;
            uint4 v = *reinterpret_cast<const uint4*>(REFS ? fr.data + (size_t)y * fr.pitch + 16 * u : src + o);
            unsigned* w = reinterpret_cast<unsigned*>(&v);
            for (int k = 0; k < 4; k++) {
                unsigned in = w[k], out = 0;
                for (int j = 0; j < 4; j++) out |= (unsigned)clahe_px(R, 16 * u + 4 * k + j, (in >> (8 * j)) & 255, g) << (8 * j);
                w[k] = out;
            }
            *reinterpret_cast<uint4*>(dst + o) = v;
        }
    } else {
        const int n = (y1 - y0) * g.w;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int r = i / g.w, x = i - r * g.w, y = y0 + r;
            const RowLut R = row_lut(y, g, L, row0, nrows);
            const size_t o = fo + (size_t)y * g.w + x;
            dst[o] = clahe_px(R, x, REFS ? fr.data[(size_t)y * fr.pitch + x] : src[o], g);
        }
    }
}
template <bool kVec16, bool kLds>
__global__ __launch_bounds__(kThreads) void clahe_apply_kernel(const uint8_t* src, uint8_t* dst, const uint8_t* __restrict__ lut, Geom g, int band, int lds_rows) {
    clahe_apply_body<kVec16, kLds, false>(src, dst, lut, g, band, lds_rows);
}
template <bool kVec16, bool kLds>
__global__ __launch_bounds__(kThreads) void clahe_apply_refs_kernel(const gf_frame_ref* refs, uint8_t* dst, const uint8_t* __restrict__ lut, Geom g, int band, int lds_rows) {
    clahe_apply_body<kVec16, kLds, true>(reinterpret_cast<const uint8_t*>(refs), dst, lut, g, band, lds_rows);
}

}  // namespace gfclahe
