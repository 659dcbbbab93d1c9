// gf_stereo_depth_kernels.hpp — gfx950 device code of the stereo depth (gf_stereo_depth.hpp is the definition, one source with the host): the depth each
// left-to-right match of a call determines, in ONE launch behind stereo_lk_sized_kernel on the same stream.  camera_lift_kernel's shape: a block of one wavefront
// takes a (list position, chunk of 64 points) pair, one point per lane, so the position's two cameras, its rig and its gates are read through an index every
// lane shares and stay in scalar registers, and the branches on the two models are wavefront-uniform.  No LDS, no scratch, plain vector stores (DESIGN.md
// section 4, "Stereo depth", has the register counts).  It is a kernel of its own on purpose: the two lifts need about as many VGPRs as camera_lift_kernel,
// which neither the stereo kernel (68 VGPRs, 7 waves per SIMD) nor camera_lift_kernel's other callers should pay for.
#pragma once
#include <hip/hip_runtime.h>

#include "gf_stereo_depth.hpp"

namespace gfsd {

constexpr int kThreads = 64;   // one wavefront: no wavefront spans two positions
__global__ __launch_bounds__(kThreads) void stereo_depth_kernel(const Args A) {
    const int chunks = (int)gridDim.x, chunk = (int)blockIdx.x;
    for (int b = blockIdx.y; b < A.count; b += gridDim.y) {
        const int q = A.entry_of ? A.entry_of[b] : b;
        if (q < 0) continue;                    // a mono position, or a stereo one handed no right frame
        const Entry& e = A.entries[q];
        if (!e.on) continue;                    // a stereo position without the switch
        size_t at; int n, nt = 0;
        if (A.first) { at = (size_t)A.first[b]; n = A.first[b + 1] - A.first[b]; }
        else {   // the row as stereo_lk_body counts it: the sum never passes the row, whatever the tables hold
            at = (size_t)b * A.cap;
            nt = min(max(A.n_tracked[b], 0), A.cap);
            n = nt + min(max(A.n_new[b], 0), A.cap - nt);
        }
        for (int i = chunk * kThreads + (int)threadIdx.x; i < n; i += chunks * kThreads) {
            gfcam::Pair l;
            if (A.first) l = A.left_pts[at + i];
            else if (i < nt) l = A.lk_pts[at + min(max(A.row[at + i], 0), A.cap - 1)];
            else l = A.new_pts[at + (i - nt)];
            const gfcam::Pair r = A.right_pts[at + i];
            const Depth d = depth_of(e.left, e.right, e.rig, l.x, l.y, r.x, r.y, A.status[at + i]);
            A.depth_mm[at + i] = d.mm;
            A.why[at + i] = d.why;
        }
    }
}

// chunks per position for positions of at most max_n points, and the grid
inline dim3 grid_of(int max_n, int count) {
    const unsigned chunks = (unsigned)((max_n > 0 ? max_n : 1) + kThreads - 1) / kThreads;
    return dim3(chunks, (unsigned)(count < 65535 ? count : 65535));
}

}  // namespace gfsd
