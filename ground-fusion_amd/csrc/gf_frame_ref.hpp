// gf_frame_ref.hpp — frames the caller keeps on the device, handed over as one {pointer of row 0, bytes from row to row} per listed sequence (gf_frame_ref,
// gf_tracker_track_some_device_refs / _track_batch_device_refs / gf_tracker_set_roi_some_device_refs).  One source for the three things host and device share:
// what an entry must satisfy (check), which load form a frame gets (form), and how a block reads its entry (entry).
// The table of a call is [count] by list position, like cur_of (gf_lk_kernels.hpp), and travels the same way: page-locked, read by the first kernel of the call
// over the bus, one wave-uniform load per block.  Only the first kernel that reads the caller's memory sees it; everything behind reads the handle's own tight
// buffers.  Nothing behind an entry is ever written.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/groundfusion_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GF_REF_HD __host__ __device__ __forceinline__
#else
#define GF_REF_HD inline
#endif

namespace gfref {

// The widest piece a frame may be loaded in: 16 bytes when its first row and its pitch (and with them every row) are multiples of 16, 4 when they are multiples
// of 4, single bytes otherwise.  A block-uniform decision from the frame's own entry: one launch may mix all three.
GF_REF_HD int form(uintptr_t data, size_t pitch) {
    const uintptr_t m = data | (uintptr_t)pitch;
    return !(m & 15) ? 16 : !(m & 3) ? 4 : 1;
}
// whether a frame misses the widest form of its first reader (`widest`: 16 for the pyramid and CLAHE, 4 for the conversion kernels, whose vector form needs
// dword-aligned rows only): what gf_tracker_stats.frames_unaligned counts
GF_REF_HD bool unaligned(uintptr_t data, size_t pitch, int widest) { return form(data, pitch) < widest; }

// What is refused (GF_ERR_INVALID, naming the list position) before anything is copied, launched or changed.
enum Verdict { kOk = 0, kNullData, kShortPitch, kOddDepth };
// row_bytes: width x bytes per pixel.  u16: a depth frame (pointer and pitch must be even).  may_be_null: the depth entry of a sequence whose depth_cam is 0.
GF_REF_HD Verdict check(const gf_frame_ref& r, size_t row_bytes, bool u16, bool may_be_null) {
    if (!r.data) return may_be_null ? kOk : kNullData;
    if (r.pitch < row_bytes) return kShortPitch;
    if (u16 && ((reinterpret_cast<uintptr_t>(r.data) | (uintptr_t)r.pitch) & 1)) return kOddDepth;
    return kOk;
}
inline const char* verdict_text(Verdict v) {
    return v == kNullData ? "null data pointer" : v == kShortPitch ? "pitch shorter than a row" : v == kOddDepth ? "depth pointer or pitch is odd" : "ok";
}

struct Frame { const uint8_t* data; size_t pitch; };

#if defined(__HIPCC__) || defined(__HIP__)
// The entry of list position i, the same for the whole block: saying so keeps base and pitch, and every row address derived from them, in scalar registers
// (list_entry, gf_lk_kernels.hpp).
__device__ __forceinline__ Frame entry(const gf_frame_ref* __restrict__ table, unsigned i) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(table + i);
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(p[0]), d1 = __builtin_amdgcn_readfirstlane(p[1]);
    const uint32_t p0 = __builtin_amdgcn_readfirstlane(p[2]), p1 = __builtin_amdgcn_readfirstlane(p[3]);
    Frame f;
    f.data = reinterpret_cast<const uint8_t*>(((uint64_t)d1 << 32) | d0);
    f.pitch = (size_t)(((uint64_t)p1 << 32) | p0);
    return f;
}
// Where the frames of a launch lie.  REFS = false: `count` frames back to back from `raw`, seq_stride bytes apart, rows `stride` bytes apart (the tight entry
// points and the handle's own buffers; the code of before).  REFS = true: `raw` is the call's table of gf_frame_ref and the two numbers are not read.
template <bool REFS> __device__ __forceinline__ Frame frame_at(const uint8_t* __restrict__ raw, size_t seq_stride, size_t stride, unsigned i) {
    if (REFS) return entry(reinterpret_cast<const gf_frame_ref*>(raw), i);
    Frame f;
    f.data = raw + i * seq_stride;
    f.pitch = stride;
    return f;
}
// one u16 of the depth frame of list position i (a single lane asks: no scalar broadcast needed); a null entry (a sequence without a depth camera) reads as 0
template <bool REFS> __device__ __forceinline__ uint16_t depth_at(const uint16_t* __restrict__ depth, size_t seq_stride, int stride, unsigned i, int y, int x) {
    if (REFS) {
        const gf_frame_ref r = reinterpret_cast<const gf_frame_ref*>(depth)[i];
        if (!r.data) return 0;
        return *reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(r.data) + (size_t)y * r.pitch + 2 * (size_t)x);
    }
    return depth[i * seq_stride + (size_t)y * stride + x];
}
#endif

}  // namespace gfref
