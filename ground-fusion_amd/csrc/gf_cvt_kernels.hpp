// gf_cvt_kernels.hpp — colour -> MONO8 on batches of u8 frames: cv_bridge::toCvCopy(msg, MONO8) of getImageFromMsg (rosNodeTest.cpp:238-254), the arithmetic
// of gf_pixfmt.hpp.  Included by gf_cvt.hip only.
//
// A pure stream: CH bytes in, one byte out per pixel, nothing is read twice.
//   cvt_gray_vec_kernel<CH, NPX>  a lane takes NPX (4 or 16) consecutive pixels of a row: NPX * CH / 4 source dwords in, NPX / 4 dwords out; consecutive lanes take
//                                 consecutive pieces of a row, so a wavefront reads one contiguous span and writes one.  Needs every row base of source and
//                                 destination on a 4-byte boundary (both pointers, the pitch and the width multiples of 4) and NPX | width.
//   cvt_gray_byte_kernel<CH>      one pixel per lane, byte loads and a byte store: any pointer, any pitch, any width.
// blockIdx.y walks the frames (strided, for batches beyond the grid limit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_pixfmt.hpp"

namespace gfcvt {

constexpr int kThreads = 256;

template <int N> struct __attribute__((packed, aligned(4))) Dwords { uint32_t v[N]; };   // N dwords on a 4-byte boundary: one load / store instruction of that width

// pixel j (0 .. NPX-1) of a piece held as little-endian dwords: byte k of the piece is (v[k >> 2] >> 8 (k & 3)) & 255; all indices are compile-time after unrolling
template <int CH, int NPX> __device__ __forceinline__ unsigned byte_of(const Dwords<NPX * CH / 4>& s, int k) { return (s.v[k >> 2] >> (8 * (k & 3))) & 255u; }

template <int CH, int NPX>
__global__ __launch_bounds__(kThreads) void cvt_gray_vec_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    const int per_row = w / NPX;
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;   // piece of the frame; the host keeps per_row * h below 2^31
    if (p >= (unsigned)per_row * (unsigned)h) return;
    const int y = p / per_row, xp = p - y * per_row;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const Dwords<NPX * CH / 4> s = *reinterpret_cast<const Dwords<NPX * CH / 4>*>(src + ((size_t)b * h + y) * src_pitch + (size_t)xp * (NPX * CH));
        Dwords<NPX / 4> o;
#pragma unroll
        for (int q = 0; q < NPX / 4; q++) {
            unsigned out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = (4 * q + j) * CH;
                unsigned g;
                if (CH == 1) g = byte_of<CH, NPX>(s, k);
                else {
                    const unsigned c0 = byte_of<CH, NPX>(s, k), c1 = byte_of<CH, NPX>(s, k + 1), c2 = byte_of<CH, NPX>(s, k + 2);
                    g = gfpix::gray(red_at ? c2 : c0, c1, red_at ? c0 : c2);
                }
                out |= g << (8 * j);
            }
            o.v[q] = out;
        }
        *reinterpret_cast<Dwords<NPX / 4>*>(dst + ((size_t)b * h + y) * w + (size_t)xp * NPX) = o;
    }
}

template <int CH>
__global__ __launch_bounds__(kThreads) void cvt_gray_byte_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;   // pixel of the frame; the host keeps w * h below 2^31
    if (p >= (unsigned)w * (unsigned)h) return;
    const int y = p / w, x = p - y * w;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const uint8_t* s = src + ((size_t)b * h + y) * src_pitch + (size_t)x * CH;
        dst[((size_t)b * h + y) * w + x] = CH == 1 ? s[0] : gfpix::gray(s[red_at], s[1], s[2 - red_at]);
    }
}

}  // namespace gfcvt
