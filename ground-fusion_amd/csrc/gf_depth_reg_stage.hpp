// gf_depth_reg_stage.hpp — what a launch of the depth registration (gf_depth_reg.hip) works in: the z-buffer and the table of a call's jobs.  One per tracker
// handle that uses the feature (obtained by its first gf_tracker_set_seq_depth_reg) and one for the building blocks.
#pragma once
#include "gf_depth_reg.hpp"
#include "gf_hip_own.hpp"

namespace gf {

struct DepthRegStage {
    DevBuf<uint32_t> z;                // one word per colour pixel of every entry of a call, rows padded to eight words
    DevBuf<gfdreg::Job> d_jobs; PinBuf<gfdreg::Job> h_jobs;   // the call's entries: filled in h_jobs by the caller, carried down by depth_reg_launch
    bool primed = false;               // every word of z holds gfdreg::kUntouched
};
// room for `jobs` entries and `zwords` words; grows, never shrinks.  GF_ERR_HIP with nothing changed if an allocation fails.
int depth_reg_fit(DepthRegStage& s, size_t jobs, size_t zwords);
// h_jobs[0 .. n): copy, scatter kernel, finish kernel on `stream`; returns when they are launched.  before / after (may be null): recorded around the two kernels.
int depth_reg_launch(DepthRegStage& s, int n, hipStream_t stream, hipEvent_t before = nullptr, hipEvent_t after = nullptr);

}  // namespace gf
