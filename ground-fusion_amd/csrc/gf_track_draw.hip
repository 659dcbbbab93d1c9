// gf_track_draw.hip — the track image (gf_track_draw.hpp; FeatureTracker::drawTrack / getTrackImage, feature_tracker.cpp:849-905, :1047) on the device: the launch
// the tracker uses (gf_tracker_track_image_some_device, gf_tracker.hip) and the building block on host buffers, gf_draw_track_batch.  Kernel: gf_track_draw_kernels.hpp.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_hip_own.hpp"
#include "gf_track_draw_kernels.hpp"

namespace gf {

// `count` frames of w x h pixels, one per entry of d_jobs (device memory), in one launch on `stream`
int draw_track_launch(const gfdraw::DrawJob* d_jobs, int count, int w, int h, hipStream_t stream) {
    using namespace gfdraw;
    if (count < 1 || count > 65535) return set_err(GF_ERR_INVALID, "track image: %d frames in one launch (1 .. 65535)", count);
    if (w < 1 || h < 1) return set_err(GF_ERR_INVALID, "track image: %dx%d frames", w, h);
    const long long tiles = (long long)((w + kTileW - 1) / kTileW) * ((h + kTileH - 1) / kTileH);
    if (tiles > 0x7fffffffLL) return set_err(GF_ERR_INVALID, "track image: %dx%d frames", w, h);
    draw_track_kernel<<<dim3((unsigned)tiles, count), kDrawThreads, 0, stream>>>(d_jobs, w, h);
    HIPCHK(hipGetLastError());
    return GF_OK;
}

}  // namespace gf

static int draw_track_host_buffers(const uint8_t* gray, size_t gray_pitch, int batch, int width, int height, const int* n, const float* cur_xy, const int* track_cnt,
                                   const float* prev_xy, const uint8_t* has_prev, int cap, uint8_t* dst, size_t dst_pitch, const int* n_boxes, const gf_box* boxes, int box_cap);

extern "C" {

// Copies in, renders with the tracker's kernel, copies out; synchronous.  The device copies of `gray` and `dst` take the host pointers' alignment (address & 15),
// so a caller chooses the load and store forms by where its arrays start.  Both buffers are read and written from their first byte to the last byte of their last
// row and no further -- (batch x height - 1) x pitch + a row -- so either may be a crop of a wider image; `dst` travels both ways over that span, so bytes of
// it that are no pixel come back as they were.
int gf_draw_track_batch(const uint8_t* gray, size_t gray_pitch, int batch, int width, int height, const int* n, const float* cur_xy, const int* track_cnt,
                        const float* prev_xy, const uint8_t* has_prev, int cap, uint8_t* dst, size_t dst_pitch) {
    return draw_track_host_buffers(gray, gray_pitch, batch, width, height, n, cur_xy, track_cnt, prev_xy, has_prev, cap, dst, dst_pitch, nullptr, nullptr, 0);
}
// The same with the frames of frame b's n_boxes[b] <= box_cap boxes, row b of the [batch][box_cap] table, behind its dots and strokes (drawTrackbox, :960-975)
int gf_draw_track_boxes_batch(const uint8_t* gray, size_t gray_pitch, int batch, int width, int height, const int* n, const float* cur_xy, const int* track_cnt,
                              const float* prev_xy, const uint8_t* has_prev, int cap, uint8_t* dst, size_t dst_pitch, const int* n_boxes, const gf_box* boxes, int box_cap) {
    if (!n_boxes || box_cap < 0) return gf::set_err(GF_ERR_INVALID, "track image: null table of box counts or a box capacity of %d", box_cap);
    return draw_track_host_buffers(gray, gray_pitch, batch, width, height, n, cur_xy, track_cnt, prev_xy, has_prev, cap, dst, dst_pitch, n_boxes, boxes, box_cap);
}

}  // extern "C"

static int draw_track_host_buffers(const uint8_t* gray, size_t gray_pitch, int batch, int width, int height, const int* n, const float* cur_xy, const int* track_cnt,
                                   const float* prev_xy, const uint8_t* has_prev, int cap, uint8_t* dst, size_t dst_pitch, const int* n_boxes, const gf_box* boxes, int box_cap) {
    using namespace gfdraw;
    if (!gray || !dst || !n) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (batch < 1 || width < 1 || height < 1 || cap < 0) return gf::set_err(GF_ERR_INVALID, "track image: batch %d of %dx%d frames, capacity %d", batch, width, height, cap);
    if (gray_pitch < (size_t)width || dst_pitch < 3 * (size_t)width) return gf::set_err(GF_ERR_INVALID, "track image: a pitch is shorter than a row of %d pixels", width);
    const size_t room = list_capacity((size_t)cap) + (size_t)box_cap;   // primitives of one frame
    std::vector<Prim> lists((size_t)batch * room);
    std::vector<int> count(batch);
    for (int b = 0; b < batch; b++) {
        if (n[b] < 0 || n[b] > cap) return gf::set_err(GF_ERR_INVALID, "track image: frame %d lists %d features, capacity %d", b, n[b], cap);
        if (n[b] > 0 && (!cur_xy || !track_cnt)) return gf::set_err(GF_ERR_INVALID, "null argument");
        char msg[160];
        const size_t at = (size_t)b * cap;
        count[b] = build_list(n[b], cur_xy + 2 * at, track_cnt + at, prev_xy ? prev_xy + 2 * at : nullptr, has_prev ? has_prev + at : nullptr,
                              lists.data() + (size_t)b * room, msg, sizeof msg);
        if (count[b] < 0) return gf::set_err(GF_ERR_INVALID, "track image: frame %d: %s", b, msg);
        if (n_boxes) {
            if (n_boxes[b] < 0 || n_boxes[b] > box_cap || (n_boxes[b] > 0 && !boxes)) return gf::set_err(GF_ERR_INVALID, "track image: frame %d lists %d boxes, capacity %d", b, n_boxes[b], box_cap);
            count[b] += append_frames(boxes ? boxes + (size_t)b * box_cap : nullptr, n_boxes[b], lists.data() + (size_t)b * room + count[b]);
        }
    }
    if (int rc = gf::require_device()) return rc;
    constexpr size_t kGuard = 64;   // bytes on either side of the destination that must come back as they were put
    const size_t rows = (size_t)batch * height;   // the last row of a buffer ends with its pixels, not with its pitch
    const size_t gray_bytes = (rows - 1) * gray_pitch + (size_t)width, dst_bytes = (rows - 1) * dst_pitch + 3 * (size_t)width;
    const size_t gray_phase = reinterpret_cast<uintptr_t>(gray) & 15, dst_phase = reinterpret_cast<uintptr_t>(dst) & 15;
    gf::DevBuf<uint8_t> d_gray, d_dst; gf::DevBuf<Prim> d_lists; gf::DevBuf<DrawJob> d_jobs;
    HIPCHK(d_gray.fit(gray_bytes + 16)); HIPCHK(d_dst.fit(dst_bytes + 2 * kGuard + 16)); HIPCHK(d_lists.fit(lists.size() + 1)); HIPCHK(d_jobs.fit(batch));
    uint8_t* g0 = d_gray.p + gray_phase;
    uint8_t* o0 = d_dst.p + kGuard + dst_phase;
    std::vector<uint8_t> guard(2 * kGuard + 16, 0xa5), back(2 * kGuard + 16);
    HIPCHK(hipMemcpy(g0, gray, gray_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_dst.p, guard.data(), kGuard + dst_phase, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o0, dst, dst_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o0 + dst_bytes, guard.data(), kGuard, hipMemcpyHostToDevice));
    if (!lists.empty()) HIPCHK(hipMemcpy(d_lists.p, lists.data(), lists.size() * sizeof(Prim), hipMemcpyHostToDevice));
    std::vector<DrawJob> jobs(batch);
    for (int b = 0; b < batch; b++)
        jobs[b] = DrawJob{g0 + (size_t)b * height * gray_pitch, gray_pitch, o0 + (size_t)b * height * dst_pitch, dst_pitch, d_lists.p + (size_t)b * room, count[b], 0};
    HIPCHK(hipMemcpy(d_jobs.p, jobs.data(), jobs.size() * sizeof(DrawJob), hipMemcpyHostToDevice));
    if (int rc = gf::draw_track_launch(d_jobs.p, batch, width, height, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(back.data(), d_dst.p, kGuard + dst_phase, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(back.data() + kGuard + dst_phase, o0 + dst_bytes, kGuard, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < 2 * kGuard + dst_phase; k++)
        if (back[k] != 0xa5) return gf::set_err(GF_ERR_HIP, "track image: a byte %s the destination was written", k < kGuard + dst_phase ? "in front of" : "behind");
    HIPCHK(hipMemcpy(dst, o0, dst_bytes, hipMemcpyDeviceToHost));
    return GF_OK;
}
