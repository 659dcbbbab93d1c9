// gf_depth_reg_kernels.hpp — raw depth registered to the colour camera on the device: the definition is gf_depth_reg.hpp, one source with the host.  Two
// launches per call, whatever the number of entries and whatever their sizes:
//   depth_scatter_kernel  a block belongs to one list entry (blockIdx.y) and reads the entry's Job -- source, pitch, sizes, the 25 doubles of the two cameras and
//                         the pose -- with scalar loads through an index every lane shares, as cvt_mixed_kernel and camera_lift_kernel read theirs.  Lanes take
//                         adjacent depth pixels of a row, so the atomics of a wavefront instruction fall on adjacent words: a lane pair reads one dword where
//                         the frame's pointer and pitch are multiples of 4 (gfref::form) and each lane takes its half, a u16 per lane otherwise (pointer and
//                         pitch are even, so a count never straddles).  A contributing lane applies gfdreg::scatter_pixel with an
//                         unsigned 32-bit atomic minimum per covered colour pixel into the entry's rows of the z-buffer, which hold 0xFFFFFFFF.  A minimum does
//                         not depend on the order of arrival: the result is the same bits from run to run, and there is no floating-point atomic.
//   depth_finish_kernel   eight words of a z-buffer row per lane (the rows start on 32 bytes): narrowed to u16, 0 where nothing arrived, written as one 16-byte
//                         piece where the destination's pointer and pitch are multiples of 16 and the eight lie inside the row, as u16s otherwise; the words
//                         are primed again for the next call, so there is no clear pass.  Bytes of a destination row beyond wc x 2 are never written.
// No LDS, no scratch ("Depth registration", has the register counts).
#pragma once
#include <hip/hip_runtime.h>

#include "gf_depth_reg.hpp"
#include "gf_frame_ref.hpp"

namespace gfdreg {

constexpr int kThreads = 256;

// the first N dwords of entry b, the same for the whole block: saying so keeps them, and every address derived from them, in scalar registers (gfref::entry)
template <int N> __device__ __forceinline__ Job job_at(const Job* __restrict__ jobs, unsigned b) {
    static_assert(N * 4 <= (int)sizeof(Job), "a Job has that many dwords");
    const uint32_t* p = reinterpret_cast<const uint32_t*>(jobs + b);
    union { Job j; uint32_t w[sizeof(Job) / 4]; } u;
#pragma unroll
    for (int i = 0; i < N; i++) u.w[i] = __builtin_amdgcn_readfirstlane(p[i]);
    return u.j;
}
constexpr int kJobHeadDwords = (5 * 8 + 4 * 4) / 4;   // all but the doubles
constexpr int kJobDwords = sizeof(Job) / 4, kJobPinholeDwords = kJobHeadDwords + 2 * kPinholeDoubles;   // everything / all a PINHOLE entry has

// FULL: the call lists a PINHOLE_FULL colour camera; every entry then reads its whole Job and branches on its model, the same for the whole block.  Without, the
// kernel is the one it was before that model: it reads the 25 doubles of a PINHOLE entry and holds no branch.
template <bool FULL> __global__ __launch_bounds__(kThreads) void depth_scatter_kernel(const Job* __restrict__ jobs, uint32_t* __restrict__ zbuf, int batch) {
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const Job j = job_at<FULL ? kJobDwords : kJobPinholeDwords>(jobs, b);
        const bool dwords = gfref::form(reinterpret_cast<uintptr_t>(j.src), j.src_pitch) >= 4;
        const unsigned per_row = (unsigned)j.wd, items = per_row * (unsigned)j.hd;   // <= 4096 x 4096
        uint32_t* z = zbuf + j.zoff;
        const size_t zs = zstride_of(j.wc);
        const auto min_into = [](uint32_t* w, uint32_t v) { atomicMin(w, v); };
        for (unsigned idx = blockIdx.x * kThreads + threadIdx.x; idx < items; idx += gridDim.x * kThreads) {
            const unsigned y = idx / per_row, x = idx - y * per_row;
            const uint8_t* row = j.src + (size_t)y * j.src_pitch;
            uint16_t d;
            if (dwords && (x | 1u) < per_row) d = (uint16_t)(*reinterpret_cast<const uint32_t*>(row + 4 * (size_t)(x >> 1)) >> (16 * (x & 1u)));   // the dword its neighbour lane reads too
            else d = *reinterpret_cast<const uint16_t*>(row + 2 * (size_t)x);                    // the last count of an odd width: the dword would leave the row
            scatter_pixel<FULL>(j.p, j.wc, j.hc, (int)x, (int)y, d, z, zs, min_into);
        }
    }
}

__global__ __launch_bounds__(kThreads) void depth_finish_kernel(const Job* __restrict__ jobs, uint32_t* __restrict__ zbuf, int batch) {
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const Job j = job_at<kJobHeadDwords>(jobs, b);
        const size_t zs = zstride_of(j.wc);
        const unsigned groups = (unsigned)(zs / 8), items = groups * (unsigned)j.hc;
        const bool wide = gfref::form(reinterpret_cast<uintptr_t>(j.dst), j.dst_pitch) == 16;
        uint32_t* z = zbuf + j.zoff;
        for (unsigned idx = blockIdx.x * kThreads + threadIdx.x; idx < items; idx += gridDim.x * kThreads) {
            const unsigned v = idx / groups, g = idx - v * groups;
            uint4* zp = reinterpret_cast<uint4*>(z + (size_t)v * zs + 8 * (size_t)g);
            const uint4 lo = zp[0], hi = zp[1];
            const uint4 prime = make_uint4(kUntouched, kUntouched, kUntouched, kUntouched);
            zp[0] = prime; zp[1] = prime;
            const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            const int x = 8 * (int)g;
            uint8_t* out = j.dst + (size_t)v * j.dst_pitch + 2 * (size_t)x;
            if (wide && x + 8 <= j.wc) {
                uint4 o;
                o.x = (uint32_t)narrow(w[0]) | ((uint32_t)narrow(w[1]) << 16); o.y = (uint32_t)narrow(w[2]) | ((uint32_t)narrow(w[3]) << 16);
                o.z = (uint32_t)narrow(w[4]) | ((uint32_t)narrow(w[5]) << 16); o.w = (uint32_t)narrow(w[6]) | ((uint32_t)narrow(w[7]) << 16);
                *reinterpret_cast<uint4*>(out) = o;
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) if (x + i < j.wc) reinterpret_cast<uint16_t*>(out)[i] = narrow(w[i]);
            }
        }
    }
}

// the grid of either kernel for entries of at most max_items lane items
inline dim3 reg_grid(size_t max_items, int batch) {
    const size_t blocks = (max_items + kThreads - 1) / kThreads;
    return dim3((unsigned)(blocks < 1 ? 1 : blocks > 65535 ? 65535 : blocks), (unsigned)(batch < 65535 ? batch : 65535));
}

}  // namespace gfdreg
