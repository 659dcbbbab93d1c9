// gf_stereo_kernels.hpp — gfx950 device code of the stereo branch of FeatureTracker::trackImage (feature_tracker.cpp:259-303, kept there as VINS-Fusion wrote
// it, commented out): forward LK from the current left frame to the right frame on all of cur_pts, and with FLOW_BACK the reverse pass and the 0.5 px test.
//   cv::calcOpticalFlowPyrLK(cur_img, rightImg, cur_pts, cur_right_pts, status, err, cv::Size(21, 21), 3);                      (:273)
//   cv::calcOpticalFlowPyrLK(rightImg, cur_img, cur_right_pts, reverseLeftPts, statusRightLeft, err, cv::Size(21, 21), 3);      (:277)
//   status = status && statusRightLeft && inBorder(cur_right_pts[i]) && distance(cur_pts[i], reverseLeftPts[i]) <= 0.5          (:280)
// Both passes are lk_solve of gf_lk_kernels.hpp, unchanged: window 21 x 21, maxLevel 3, 30 iterations / 0.01, no initial flow.  The reverse pass is NOT the
// one-level pass from an initial flow that the temporal reverse check runs (:141): it starts from scratch with every level, as the call above says.
// One wavefront per point, whatever GF_LK_POINTS says (the multi-point forms serve the temporal launch alone).
#pragma once
#include "gf_lk_kernels.hpp"

namespace gf {

// One launch serves every stereo sequence of a call.  Every table is indexed by the list position i (grid.y); right_of[i] < 0: position i has no right frame in
// this call (a mono sequence, or a stereo one handed a null right entry) and its blocks leave at once, writing nothing but a count of 0 (n_points).
// A point's source is a gather: cur_pts of a sequence is its tracked survivors in setMask's order followed by the new corners.  The survivors are rows of the
// temporal launch's output table, named by `row` (uploaded with setMask's hand-over, SeqState::lk_row); the corners lie in the selection's output table, and
// their number is read where the selection left it.  Point k of the sequence: k < n_tracked[i] ? lk_pts[row[k]] : new_pts[k - n_tracked[i]].
struct StereoLkArgs {
    const uint8_t* left;        // the left pyramids, slot_bytes apart
    const int* left_of;         // [count] pyramid of the current left frame (the call's cur_of)
    const uint8_t* right;       // the right pyramids, slot_bytes apart
    const int* right_of;        // [count] pyramid of the right frame, or -1
    int cap;                    // row length of every point table below
    const int* n_tracked;       // [count]
    const int* row;             // [count][cap]
    const float2* lk_pts;       // [count][cap]
    const int* n_new;           // [count]
    const float2* new_pts;      // [count][cap]
    const uint8_t* flow_back_of;   // [count] FLOW_BACK of the sequence at each position
    float2* right_pts;          // [count][cap] out: cur_right_pts before the reduction
    uint8_t* status;            // [count][cap] out: the status the reduction reads (:280, or the forward status alone without FLOW_BACK)
    uint8_t* fwd_status;        // [count][cap] out: the forward pass alone
    int* n_points;              // [count] out, or null: how many points of the row were written (0 for a position without a right frame): what a lift behind this kernel reads
};

// grid.x = ceil(cap / 4) blocks of 4 wavefronts, grid.y = list position.  G: the geometry of the position's frames (both eyes have the sequence's size).
__device__ __forceinline__ void stereo_lk_body(const PyrGeom& G, const size_t slot_bytes, const StereoLkArgs& A, uint8_t* tiles) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int i = blockIdx.x * 4 + wave;
    const int rgt = list_entry(A.right_of, b);
    const int nt = rgt < 0 ? 0 : min(max(list_entry(A.n_tracked, b), 0), A.cap);
    const int nn = rgt < 0 ? 0 : min(max(list_entry(A.n_new, b), 0), A.cap - nt);   // the sum never passes the row, whatever the tables hold
    if (i == 0 && lane == 0 && A.n_points) A.n_points[b] = nt + nn;
    if (i >= nt + nn) return;
    const int flow_back = __builtin_amdgcn_readfirstlane((int)A.flow_back_of[b]);
    uint8_t* tile = tiles + wave * kTileBytes;
    const size_t at = (size_t)b * A.cap;
    float2 pp;
    if (i < nt) {
        const int r = uni(A.row[at + i]);
        pp = A.lk_pts[at + min(max(r, 0), A.cap - 1)];
    } else pp = A.new_pts[at + (i - nt)];
    pp.x = unif(pp.x); pp.y = unif(pp.y);
    const uint8_t* L = A.left + (size_t)list_entry(A.left_of, b) * slot_bytes;
    const uint8_t* R = A.right + (size_t)rgt * slot_bytes;
    unsigned n_levels = 0, n_iters = 0;
    const int top = min(3, G.nlevels - 1);
    float cx = 0.f, cy = 0.f;
    const int fwd = lk_solve(G, LkImages{L, R}, pp.x, pp.y, cx, cy, top, false, tile, lane, n_levels, n_iters);
    int st = fwd;
    if (flow_back && fwd) {   // a point whose forward pass failed fails the conjunction whatever the reverse pass would say
        float rx = 0.f, ry = 0.f;
        const int rev = lk_solve(G, LkImages{R, L}, cx, cy, rx, ry, top, false, tile, lane, n_levels, n_iters);
        const double ddx = (double)(pp.x - rx), ddy = (double)(pp.y - ry);   // distance(): float differences, the norm in double, as lk_track_body's
        const LevelGeom g0 = G.lv[0];
        const int bx = __float2int_rn(cx), by = __float2int_rn(cy);          // inBorder (:14-20): cvRound, BORDER_SIZE 1
        const bool in = 1 <= bx && bx < g0.w - 1 && 1 <= by && by < g0.h - 1;
        st = (rev && in && sqrt(ddx * ddx + ddy * ddy) <= 0.5) ? 1 : 0;
    }
    if (lane == 0) {
        A.right_pts[at + i] = make_float2(cx, cy);
        A.status[at + i] = (uint8_t)st;
        A.fwd_status[at + i] = (uint8_t)fwd;
    }
}

// The geometry of a block's list position is a row of a table of sizes (SizeRow, as lk_track_sized_kernel reads it); the distance between two pyramids is the caller's.
__global__ void __launch_bounds__(256, 7) stereo_lk_sized_kernel(const SizeRow* __restrict__ rows, const uint8_t* __restrict__ size_of, size_t slot_bytes, StereoLkArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4 * kTileBytes];
    stereo_lk_body(size_row(rows, size_of, blockIdx.y).G, slot_bytes, A, tiles);
}

}  // namespace gf
