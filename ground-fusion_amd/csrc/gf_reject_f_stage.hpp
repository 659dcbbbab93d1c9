// gf_reject_f_stage.hpp — what a launch of rejectWithF (gf_reject_f.hip) works in: the table of a call's jobs and of their results.  One per tracker handle that
// uses the feature (obtained by its first gf_tracker_set_seq_reject_f) and one for the building blocks.  No kernel in here: gf_tracker.hip fills jobs without
// holding the kernel.
#pragma once
#include "gf_camera_models.hpp"
#include "gf_hip_own.hpp"
#include "gf_reject_f.hpp"

namespace gfrf {
struct Job;   // gf_reject_f_kernels.hpp
}

namespace gf {

struct RejectFStage {
    DevBuf<uint8_t> d_jobs; PinBuf<uint8_t> h_jobs;   // gfrf::Job entries: filled in h_jobs by the caller (reject_f_job), carried down by reject_f_launch
    DevBuf<gfrf::Result> d_res; PinBuf<gfrf::Result> h_res;   // entry i's result: up behind the kernel
    size_t cap = 0;                                   // entries there is room for
};
// room for `jobs` entries; grows, never shrinks.  GF_ERR_HIP with nothing changed if an allocation fails.
int reject_f_fit(RejectFStage& s, size_t jobs);
// entry i of the call.  cam (the tracker): prev / cur are device rows of n pixel points each, lifted with *cam into virtual pixels of a width x height frame;
// null (the building block): d_pairs holds n rows of virtual pixels.  d_status: the n status bytes, rewritten in place.
void reject_f_job(RejectFStage& s, int i, const gfcam::Camera* cam, const void* d_prev, const void* d_cur, const gfrf::Cand* d_pairs, uint8_t* d_status, int n,
                  int width, int height, double f_threshold, double focal, uint32_t seed);
// entries [0, n): the table down, one launch of reject_f_kernel, the results up, all on `stream`; returns when they are enqueued.  before / after (may be
// null): recorded around the kernel.
int reject_f_launch(RejectFStage& s, int n, hipStream_t stream, hipEvent_t before = nullptr, hipEvent_t after = nullptr);

}  // namespace gf
