// gf_reject_f_kernels.hpp — rejectWithF on the device (feature_tracker.cpp:711-743): the definition is gf_reject_f.hpp, one source with the host.  One launch
// for every listed set, a block of 256 threads per set (the entry's Job read through a block-uniform index, as camera_lift_kernel and depth_scatter_kernel
// read theirs):
//   compact   the rows with status 1 are lifted to virtual pixels (or taken as given, the building block) and the finite ones packed into LDS in row order by
//             ballot and popcount, 16 bytes a candidate, with the row each came from
//   model     8 lanes per hypothesis, 32 hypotheses per pass, 16 passes.  Lane 0 of a group draws; every lane normalises (the sums run in the definition's
//             order, so they are not split) and builds ONE row of the 8 x 9 system in LDS; an elimination step is a row-local search, three shuffles among the
//             group's lanes and a row-local update; lane 0 back-substitutes and denormalises into LDS
//   score     the group's lanes walk the candidates in LDS eight apart with F in registers; counts are integers, so their sum has no order
//   result    (count, h) reduced block-wide through LDS; the block rewrites the status bytes of the winner's outliers with per-lane (vector) byte stores
// 45216 bytes of LDS (three blocks of a CU by LDS); 210 VGPRs hold it to two blocks per CU.  No scratch ("rejectWithF", has the register counts).
#pragma once
#include <hip/hip_runtime.h>

#include "gf_camera_models.hpp"
#include "gf_reject_f.hpp"

namespace gfrf {

constexpr int kThreads = 256, kLanes = 8, kGroups = kThreads / kLanes, kPasses = kHypotheses / kGroups, kWaves = kThreads / 64;
static_assert(kLanes == kSample && kPasses * kGroups == kHypotheses, "a lane per row of the system, whole passes");

// One set.  lift != 0 (the tracker): prev / cur are rows of pixel points, lifted with cam to virtual pixels.  lift == 0 (the building block): pairs holds the
// virtual pixels.  n <= kMaxCandidates rows.
struct JobHead {
    const gfcam::Pair* prev; const gfcam::Pair* cur; const Cand* pairs;
    uint8_t* status; Result* result;
    double tt, focal;      // F_threshold squared; FOCAL_LENGTH
    int32_t n, width, height, lift;
    uint32_t seed, pad_;
};
struct Job { JobHead head; gfcam::Camera cam; };
constexpr int kJobHeadDwords = sizeof(JobHead) / 4;

// the head of entry b, the same for the whole block: saying so keeps it, and every address derived from it, in scalar registers
__device__ __forceinline__ JobHead job_head(const Job* __restrict__ jobs, unsigned b) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(jobs + b);
    union { JobHead j; uint32_t w[kJobHeadDwords]; } u;
#pragma unroll
    for (int i = 0; i < kJobHeadDwords; i++) u.w[i] = __builtin_amdgcn_readfirstlane(p[i]);
    return u.j;
}

__global__ __launch_bounds__(kThreads) void reject_f_kernel(const Job* __restrict__ jobs, int n_jobs) {
    __shared__ Cand s_cand[kMaxCandidates];
    __shared__ uint16_t s_row[kMaxCandidates];
    __shared__ double s_A[kGroups][kSample * 9];
    __shared__ double s_x[kGroups][9], s_F[kGroups][9], s_bestF[kGroups][9];
    __shared__ int s_idx[kGroups][kSample];
    __shared__ int s_ok[kGroups];
    __shared__ int s_cnt[2][kWaves];
    __shared__ unsigned long long s_key[kGroups];
    const int tid = (int)threadIdx.x, g = tid / kLanes, l = tid % kLanes, wave = tid / 64, lane = tid % 64;
    for (unsigned b = blockIdx.x; b < (unsigned)n_jobs; b += gridDim.x) {
        const JobHead j = job_head(jobs, b);
        const gfcam::Camera& cam = jobs[b].cam;
        const int n = j.n < kMaxCandidates ? j.n : kMaxCandidates;
        // ---- compact
        int m = 0, bad = 0;
        for (int base = 0; base < n; base += kThreads) {
            const int i = base + tid;
            bool take = false, drop = false;
            Cand c{0.f, 0.f, 0.f, 0.f};
            if (i < n && j.status[i]) {
                if (j.lift) {
                    const gfcam::Pair p = j.prev[i], q = j.cur[i];
                    double P[3];
                    gfcam::lift(cam, (double)q.x, (double)q.y, P);
                    c.bx = virtual_pixel(j.focal, P[0], P[2], j.width); c.by = virtual_pixel(j.focal, P[1], P[2], j.height);
                    gfcam::lift(cam, (double)p.x, (double)p.y, P);
                    c.ax = virtual_pixel(j.focal, P[0], P[2], j.width); c.ay = virtual_pixel(j.focal, P[1], P[2], j.height);
                } else c = j.pairs[i];
                take = finite_cand(c); drop = !take;
            }
            if (drop) j.status[i] = 0;
            const unsigned long long bt = __ballot(take), bd = __ballot(drop);
            if (lane == 0) { s_cnt[0][wave] = __popcll(bt); s_cnt[1][wave] = __popcll(bd); }
            __syncthreads();
            int at = m;
#pragma unroll
            for (int w = 0; w < kWaves; w++) { if (w < wave) at += s_cnt[0][w]; m += s_cnt[0][w]; bad += s_cnt[1][w]; }
            if (take) { const int k = at + __popcll(bt & ((1ull << lane) - 1ull)); s_cand[k] = c; s_row[k] = (uint16_t)i; }
            __syncthreads();
        }
        if (m < kSample) {
            if (tid == 0) *j.result = Result{m, bad, -1, 0};
            continue;
        }
        // ---- hypotheses
        int best_count = 0, best_h = -1;
        for (int pass = 0; pass < kPasses; pass++) {
            const int h = pass * kGroups + g;
            if (l == 0) {
                int* idx = s_idx[g];
#pragma unroll
                for (int k = 0; k < kSample; k++) idx[k] = 0;   // a void hypothesis still reads eight candidates
                s_ok[g] = draw_sample(j.seed, h, m, idx) ? 1 : 0;
            }
            __syncthreads();
            bool ok = s_ok[g] != 0;
            double cax, cay, sa, cbx, cby, sb;
            {
                double ax[kSample], ay[kSample], bx[kSample], by[kSample];
#pragma unroll
                for (int k = 0; k < kSample; k++) { const Cand c = s_cand[s_idx[g][k]]; ax[k] = (double)c.ax; ay[k] = (double)c.ay; bx[k] = (double)c.bx; by[k] = (double)c.by; }
                ok = hartley(ax, ay, cax, cay, sa) && ok;
                ok = hartley(bx, by, cbx, cby, sb) && ok;
            }
            double* A = s_A[g];
            {
                const Cand c = s_cand[s_idx[g][l]];
                system_row(((double)c.ax - cax) * sa, ((double)c.ay - cay) * sa, ((double)c.bx - cbx) * sb, ((double)c.by - cby) * sb, A + 9 * l);
            }
            uint32_t row_used = 0, col_used = 0, prow = 0, pcol = 0;
            for (int i = 0; i < kSample; i++) {
                __syncthreads();   // the rows as the step before left them
                double v = -2.0; int pc = 0, pr = l;
                if (!((row_used >> l) & 1U)) row_best(A + 9 * l, col_used, v, pc);
#pragma unroll
                for (int d = 1; d < kLanes; d <<= 1) {
                    const double ov = __shfl_xor(v, d, kLanes);
                    const int oc = __shfl_xor(pc, d, kLanes), orow = __shfl_xor(pr, d, kLanes);
                    if (ov > v || (ov == v && orow < pr)) { v = ov; pc = oc; pr = orow; }
                }
                ok = ok && v >= kPivotMin;
                row_used |= 1U << pr; col_used |= 1U << pc; prow |= (uint32_t)pr << (4 * i); pcol |= (uint32_t)pc << (4 * i);
                if (!((row_used >> l) & 1U)) row_eliminate(A + 9 * l, A + 9 * pr, pc, col_used);
            }
            __syncthreads();
            if (l == 0) {
                back_substitute(A, prow, pcol, col_used, s_x[g]);
                denormalise(s_x[g], cax, cay, sa, cbx, cby, sb, s_F[g]);
            }
            __syncthreads();
            // ---- score
            double F[9];
#pragma unroll
            for (int c = 0; c < 9; c++) F[c] = s_F[g][c];
            int count = 0;
            for (int k = l; k < m; k += kLanes) count += inlier(F, s_cand[k], j.tt) ? 1 : 0;
#pragma unroll
            for (int d = 1; d < kLanes; d <<= 1) count += __shfl_xor(count, d, kLanes);
            if (ok && count >= kSample && count > best_count) {   // h grows with the pass: within a group the smaller h keeps a tie
                best_count = count; best_h = h;
                if (l == 0) {
#pragma unroll
                    for (int c = 0; c < 9; c++) s_bestF[g][c] = F[c];
                }
            }
        }
        // ---- the winner: most inliers, then the smaller h
        if (l == 0) s_key[g] = best_h < 0 ? 0ull : ((unsigned long long)best_count << 32) | (unsigned)(kHypotheses - best_h);
        __syncthreads();
        unsigned long long key = 0; int gwin = 0;
        for (int k = 0; k < kGroups; k++) { const unsigned long long o = s_key[k]; if (o > key) { key = o; gwin = k; } }
        if (key == 0ull) {
            if (tid == 0) *j.result = Result{m, bad, -1, 0};
            __syncthreads();
            continue;
        }
        double F[9];
#pragma unroll
        for (int c = 0; c < 9; c++) F[c] = s_bestF[gwin][c];
        int rejected = 0;
        for (int base = 0; base < m; base += kThreads) {
            const int k = base + tid;
            const bool out = k < m && !inlier(F, s_cand[k], j.tt);
            if (out) j.status[s_row[k]] = 0;
            rejected += __popcll(__ballot(out));
        }
        if (lane == 0) s_cnt[0][wave] = rejected;
        __syncthreads();
        if (tid == 0) {
            int r = bad;
            for (int w = 0; w < kWaves; w++) r += s_cnt[0][w];
            *j.result = Result{m, r, kHypotheses - (int)(unsigned)(key & 0xffffffffull), (int)(key >> 32)};
        }
        __syncthreads();
    }
}

}  // namespace gfrf
