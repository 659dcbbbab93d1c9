// gf_seq_cfg.hpp — the parameters a sequence of a tracker handle may have of its own (gf_tracker_seq_cfg, include/groundfusion_hip.h): what the reference keeps
// per FeatureTracker object (MAX_CNT, MIN_DIST, FLOW_BACK, depth_cam, m_camera).  Plain C++, no device code: the limits a setter checks and the table of
// setMask's circle that the host walk and the detector both read, in one place, so that a stand-alone host program can run them (tests/native/seq_cfg_host.hip).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>

#include "../../include/groundfusion_hip.h"

namespace gf {

constexpr int kMaxRadius = 128;  // largest MIN_DIST supported by the disk table

struct DiskTable { short hw[kMaxRadius + 1]; int radius; };  // half-width of row |dy| of OpenCV's filled midpoint circle

inline void make_disk_table(int radius, DiskTable& T) {  // drawing.cpp Circle(): union of the h-lines per row offset
    T.radius = radius;
    for (int i = 0; i <= kMaxRadius; i++) T.hw[i] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        T.hw[dy] = std::max<short>(T.hw[dy], (short)dx);
        T.hw[dx] = std::max<short>(T.hw[dx], (short)dy);
        dy++; err += plus; plus += 2;
        int mask = (err <= 0) - 1;
        err -= minus & mask; dx += mask; minus -= mask & 2;
    }
}

namespace gfseq {

// the handle's own values: what a sequence that was never set runs with
inline gf_tracker_seq_cfg of_handle(const gf_tracker_cfg& c) {
    gf_tracker_seq_cfg s{};
    s.max_cnt = c.max_cnt; s.min_dist = c.min_dist; s.flow_back = c.flow_back; s.depth_cam = c.depth_cam;
    s.fx = c.fx; s.fy = c.fy; s.cx = c.cx; s.cy = c.cy; s.k1 = c.k1; s.k2 = c.k2; s.p1 = c.p1; s.p2 = c.p2;
    return s;
}

// The handle's cfg is the capacity: its max_cnt sized the point arrays, its min_dist the selection grid and the sort area.  True if `c` fits; otherwise a
// message that names the field.
inline bool fits(const gf_tracker_cfg& cap, const gf_tracker_seq_cfg& c, char* msg, size_t n) {
    if (c.max_cnt < 1 || c.max_cnt > cap.max_cnt) { snprintf(msg, n, "gf_tracker_seq_cfg.max_cnt %d outside 1 .. %d (the handle's max_cnt sized the point arrays)", c.max_cnt, cap.max_cnt); return false; }
    if (c.min_dist < cap.min_dist || c.min_dist > kMaxRadius) { snprintf(msg, n, "gf_tracker_seq_cfg.min_dist %d outside %d .. %d (the handle's min_dist sized the selection grid)", c.min_dist, cap.min_dist, kMaxRadius); return false; }
    if (c.flow_back != 0 && c.flow_back != 1) { snprintf(msg, n, "gf_tracker_seq_cfg.flow_back must be 0 or 1, got %d", c.flow_back); return false; }
    if (c.depth_cam != 0 && c.depth_cam != 1) { snprintf(msg, n, "gf_tracker_seq_cfg.depth_cam must be 0 or 1, got %d", c.depth_cam); return false; }
    if (!(c.fx > 0.0)) { snprintf(msg, n, "gf_tracker_seq_cfg.fx must be > 0, got %g", c.fx); return false; }
    if (!(c.fy > 0.0)) { snprintf(msg, n, "gf_tracker_seq_cfg.fy must be > 0, got %g", c.fy); return false; }
    return true;
}

}  // namespace gfseq
}  // namespace gf
