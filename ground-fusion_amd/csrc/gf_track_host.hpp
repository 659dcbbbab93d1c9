// gf_track_host.hpp — the host bookkeeping of ONE tracker sequence: what FeatureTracker (vins_estimator/src/featureTracker/feature_tracker.{h,cpp}) keeps in C++
// around its image calls -- ids, track_cnt, n_id, the id -> point maps of the velocities, setMask's std::sort + greedy keep, the camera model, setPrediction and
// removeOutliers -- and the per-sequence stages of a frame between the kernels of gf_tracker.hip.  Plain C++17 on host memory, no HIP header: the part of the
// front end that must equal oracle/tracker_oracle.cpp's Tracker bit for bit builds into a stand-alone CPU program (tests/native/track_host.cpp) as it builds into
// the library.  A stage works on one list position's rows of the hand-over tables, given by pointer; gf_tracker.hip owns the tables, the pool and the counters.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "gf_camera_models.hpp"
#include "gf_stereo_depth.hpp"
#include "gf_reject_f.hpp"
#include "gf_roi.hpp"
#include "gf_seq_cfg.hpp"
#include "gf_track_draw.hpp"

namespace gf {

struct P2f { float x, y; };   // a point, in SeqState and in the rows of the hand-over tables (the device side's float2)
struct P2i { int x, y; };     // a circle centre of setMask (the device side's int2)

struct SeqState {  // per-sequence FeatureTracker members (feature_tracker.h:76-98)
    std::vector<P2f> prev_pts, cur_pts, predict_pts, prev_un_pts, cur_un_pts, pts_velocity;
    std::vector<int> ids, track_cnt;
    std::vector<uint16_t> cur_depth;
    // the row of LK's tables each point of cur_pts came from, through the reduction by status and setMask's sort: where a lift that ran on the device left the
    // point's pair (after_detect).  Kept for the sequences that need it (after_lk's keep_rows), empty otherwise
    std::vector<int> lk_row;
    // cur_un_pts_map / prev_un_pts_map (feature_tracker.h:89): id -> point, kept as id-sorted vectors (ids are unique)
    std::vector<std::pair<int, P2f>> cur_un_pts_map, prev_un_pts_map;
    std::vector<int> grid_head, grid_next;  // scratch of set_mask_host
    double cur_time = 0, prev_time = 0;
    int n_id = 0;
    int frames = 0;   // frames the sequence has taken since gf_tracker_create / gf_tracker_reset_seq, the one in progress included: rejectWithF's draws depend on it
    bool hasPrediction = false;
    bool started = false;   // the sequence has taken a frame since gf_tracker_create / gf_tracker_reset_seq: its parameters are fixed (gf_tracker_set_seq_cfg)
    int slot = 1;   // which of the sequence's two pyramids holds its newest frame; flipped when the sequence takes a frame, and only then (the first frame goes to 0)
    // SHOW_TRACK (gf_tracker_set_show_track; drawTrack, feature_tracker.cpp:304-305, :849-905).  Nothing below is touched while the switch is off.
    // draw_from: prevLeftPtsMap for the features LK carried into the frame being taken -- id -> the point it was tracked from, id-sorted; written by after_lk ahead
    // of setMask, which reorders the features but not prev_pts.  draw_list: the primitives of the newest frame (record_track), valid while draw_have; the picture
    // of the moment trackImage returned, which setPrediction / removeOutliers do not change.  draw_sent: the list is on the device as it is here.
    bool show_track = false, draw_have = false, draw_sent = false;
    std::vector<std::pair<int, P2f>> draw_from;
    std::vector<gfdraw::Prim> draw_list;
    std::string draw_why;   // why the builder refused the newest frame's list (then draw_have is false); empty otherwise
    // The stereo branch (feature_tracker.cpp:259-303; stereo_stage below): the right-hand members of feature_tracker.h:85-89.  Nothing here is touched by a
    // sequence without a right camera, or by a frame that comes without a right image.
    std::vector<int> ids_right;
    std::vector<P2f> cur_right_pts, cur_un_right_pts, right_pts_velocity;
    std::vector<std::pair<int, P2f>> cur_un_right_pts_map, prev_un_right_pts_map;
};

static inline int cvRoundf(float v) { return (int)lrintf(v); }

// camodocal PinholeCamera (camera_models/src/camera_models/PinholeCamera.cc:450-510, :520-542, :646-662) on the camera fields of a sequence's parameters: the
// formulas are gf_camera_models.hpp, shared with the other models and with the device
inline void distortion(const gf_tracker_seq_cfg& c, double x, double y, double& dx, double& dy) { gfcam::distortion(c.k1, c.k2, c.p1, c.p2, x, y, dx, dy); }
inline bool no_distortion(const gf_tracker_seq_cfg& c) { return gfcam::no_distortion(c.k1, c.k2, c.p1, c.p2); }
inline void lift_projective(const gf_tracker_seq_cfg& c, double u, double v, double& X, double& Y) { gfcam::undistort(c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, u, v, X, Y); }
inline void space_to_plane(const gf_tracker_seq_cfg& c, const double* P, double& u, double& v) {
    gfcam::distort_to_plane(c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, P[0] / P[2], P[1] / P[2], u, v);
}

template <class V> inline void reduce_vector(std::vector<V>& v, const uint8_t* st) {  // feature_tracker.cpp:30-46
    int j = 0;
    for (int i = 0; i < (int)v.size(); i++) if (st[i]) v[j++] = v[i];
    v.resize(j);
}

// setMask (feature_tracker.cpp:56-83): std::sort by track count (same comparator, same libstdc++ algorithm as
// the reference) and greedy keep of points not covered by an earlier kept point's filled circle.
// roi: the sequence's region of interest (gf_roi.hpp) or null.  With one, the walk starts from `mask = R` instead of an all-255 image: a point whose rounded pixel
// is excluded fails `mask.at(pt) == 255` like a covered one -- not kept, no circle, gone from ids / track_cnt / cur_pts.
// boxes, n_boxes: the sequence's exclusion boxes (gf_box); the walk then starts from R_eff = R AND NOT union(boxes), tested per point against the base table and
// the list (gfroi::allowed): no table is composed on the host.
// T: the circle of the sequence's min_dist.  width, height: the frame's.
inline void set_mask_host(int width, int height, SeqState& s, const DiskTable& T, const uint32_t* roi, P2i* centers, int& n_centers, const gf_box* boxes = nullptr,
                          int n_boxes = 0) {
    struct E { int cnt; P2f pt; int id; uint16_t depth; int row; };
    static thread_local std::vector<E> v;
    v.clear();
    const bool rows = s.lk_row.size() == s.cur_pts.size();   // a sequence that keeps no rows (after_lk) gets none back
    for (size_t i = 0; i < s.cur_pts.size(); i++) v.push_back({s.track_cnt[i], s.cur_pts[i], s.ids[i], s.cur_depth[i], rows ? s.lk_row[i] : -1});
    std::sort(v.begin(), v.end(), [](const E& a, const E& b) { return a.cnt > b.cnt; });
    s.cur_pts.clear(); s.ids.clear(); s.track_cnt.clear(); s.cur_depth.clear(); s.lk_row.clear();
    n_centers = 0;
    // `mask.at(pt) == 255` <=> pt is inside no earlier kept point's filled circle; circles reach at most `radius`
    // pixels, so only centres in the 3x3 neighbourhood of radius-sized cells can cover pt.
    const int cell = std::max(T.radius, 1);
    const int gw = width / cell + 1, gh = height / cell + 1;
    s.grid_head.assign((size_t)gw * gh, -1);
    s.grid_next.clear();
    for (auto& it : v) {
        const int x = cvRoundf(it.pt.x), y = cvRoundf(it.pt.y);
        if ((roi || n_boxes > 0) && !gfroi::allowed(roi, boxes, n_boxes, width, x, y)) continue;   // tracked points are inside the image (inBorder, feature_tracker.cpp:14-20)
        const int cx = x / cell, cy = y / cell;
        bool covered = false;
        for (int yy = std::max(cy - 1, 0); yy <= std::min(cy + 1, gh - 1) && !covered; yy++)
            for (int xx = std::max(cx - 1, 0); xx <= std::min(cx + 1, gw - 1) && !covered; xx++)
                for (int k = s.grid_head[(size_t)yy * gw + xx]; k >= 0; k = s.grid_next[k]) {
                    const int dy = std::abs(y - centers[k].y), dx = std::abs(x - centers[k].x);
                    if (dy <= T.radius && dx <= T.hw[dy]) { covered = true; break; }
                }
        if (!covered) {
            s.cur_pts.push_back(it.pt); s.ids.push_back(it.id); s.track_cnt.push_back(it.cnt); s.cur_depth.push_back(it.depth);
            if (rows) s.lk_row.push_back(it.row);
            centers[n_centers] = P2i{x, y};
            s.grid_next.push_back(s.grid_head[(size_t)cy * gw + cx]);
            s.grid_head[(size_t)cy * gw + cx] = n_centers++;
        }
    }
}

// ptsVelocity (feature_tracker.cpp:810-847) on any of the tracker's lists: cur_map is rebuilt from ids and pts, the velocities are taken against prev_map over dt
inline void pts_velocity_of(const std::vector<int>& ids, const std::vector<P2f>& pts, std::vector<std::pair<int, P2f>>& cur_map,
                            const std::vector<std::pair<int, P2f>>& prev_map, double dt, std::vector<P2f>& vel) {
    const size_t n = ids.size();
    vel.resize(n);
    cur_map.resize(n);
    for (size_t i = 0; i < n; i++) cur_map[i] = {ids[i], pts[i]};
    std::sort(cur_map.begin(), cur_map.end(), [](const std::pair<int, P2f>& a, const std::pair<int, P2f>& b) { return a.first < b.first; });
    if (!prev_map.empty()) {
        for (size_t i = 0; i < n; i++) {
            const int id = ids[i];
            auto it = std::lower_bound(prev_map.begin(), prev_map.end(), id, [](const std::pair<int, P2f>& a, int v) { return a.first < v; });
            if (it != prev_map.end() && it->first == id) {
                const double vx = (pts[i].x - it->second.x) / dt, vy = (pts[i].y - it->second.y) / dt;
                vel[i] = {(float)vx, (float)vy};
            } else vel[i] = {0.f, 0.f};
        }
    } else for (size_t i = 0; i < n; i++) vel[i] = {0.f, 0.f};
}
inline void pts_velocity(SeqState& s) { pts_velocity_of(s.ids, s.cur_un_pts, s.cur_un_pts_map, s.prev_un_pts_map, s.cur_time - s.prev_time, s.pts_velocity); }

// cam: the sequence's camera where it is no pinhole (gf_tracker_set_seq_camera); null: the pinhole of par
inline void set_prediction(SeqState& s, const gf_tracker_seq_cfg& par, const int* ids, const double* xyz, int n, const gfcam::Camera* cam = nullptr) {  // feature_tracker.cpp:1006-1027
    s.hasPrediction = true;
    s.predict_pts.clear();
    std::map<int, const double*> m;
    for (int i = 0; i < n; i++) m[ids[i]] = xyz + 3 * i;
    for (size_t i = 0; i < s.ids.size(); i++) {
        auto it = m.find(s.ids[i]);
        if (it != m.end()) {
            double u, v;
            if (cam) gfcam::space_to_plane(*cam, it->second, u, v); else space_to_plane(par, it->second, u, v);
            s.predict_pts.push_back({(float)u, (float)v});
        }
        else s.predict_pts.push_back(s.prev_pts[i]);
    }
}

inline void remove_outliers(SeqState& s, const int* ids, int n) {  // feature_tracker.cpp:1029-1045
    std::set<int> rm(ids, ids + n);
    std::vector<uint8_t> st;
    for (size_t i = 0; i < s.ids.size(); i++) st.push_back(rm.count(s.ids[i]) ? 0 : 1);
    reduce_vector(s.prev_pts, st.data()); reduce_vector(s.ids, st.data()); reduce_vector(s.track_cnt, st.data());
}

// ---- the stages of one frame of one sequence, in the order a call runs them.  b is the sequence's position in the call's list; every *_row is row b of a table.

// The sequence takes a frame stamped t.  Returns the pyramid slot (0 or 1) the frame goes to; s.slot itself moves when the frame is done (after_detect).
inline int begin_frame(SeqState& s, double t) {
    s.cur_time = t; s.cur_pts.clear(); s.cur_depth.clear(); s.lk_row.clear();
    s.started = true;
    s.frames++;
    return s.slot ^ 1;
}

// Before LK (feature_tracker.cpp:113-122): the tracked points into prev_row, the prediction, if the sequence has one, into init_row, their number into *n_pts.
// *has_pts: LK has work for the sequence; *predicted: in the form that starts from init_row.  GF_OK, or a refusal with its text in msg; `seq` only names the
// sequence there.
inline int stage_points(const SeqState& s, int seq, int cap, P2f* prev_row, P2f* init_row, int* n_pts, bool* has_pts, bool* predicted, char* msg, size_t msg_len) {
    const int n = (int)s.prev_pts.size();
    *n_pts = n; *has_pts = n > 0; *predicted = false;
    if (n > cap) { snprintf(msg, msg_len, "sequence %d holds %d points > capacity %d", seq, n, cap); return GF_ERR_CAPACITY; }
    for (int k = 0; k < n; k++) prev_row[k] = s.prev_pts[k];
    if (n == 0 || !s.hasPrediction) return GF_OK;
    if ((int)s.predict_pts.size() != n) {
        snprintf(msg, msg_len, "sequence %d: prediction holds %d points but %d are tracked (call removeOutliers before setPrediction, estimator.cpp:1134-1135)", seq, (int)s.predict_pts.size(), n);
        return GF_ERR_INVALID;
    }
    for (int k = 0; k < n; k++) init_row[k] = s.predict_pts[k];
    *predicted = true;
    return GF_OK;
}

// feature_tracker.cpp:124-132: fewer than 10 forward successes of a predicted sequence -> LK again with 3 levels from scratch.  fwd_status_row: the forward pass alone.
inline bool prediction_failed(const SeqState& s, const uint8_t* fwd_status_row, int n_pts) {
    if (!s.hasPrediction || n_pts == 0) return false;
    int succ = 0;
    for (int k = 0; k < n_pts; k++) succ += fwd_status_row[k] ? 1 : 0;
    return succ < 10;
}

// What LK left for the sequence.  depth_out: the kernels' depth samples, or null on the entry points that hand in host depth images: there `host_depth` is the
// sequence's image, rows of host_dstride pixels, sampled here (null: the sequence has no depth camera or the call no depth; every sample is 0).
struct LkRows {
    const P2f* cur_pts; const uint8_t* status; const uint16_t* depth_out; const unsigned* counters;   // counters: [cap][2] level passes, iterations
    const uint16_t* host_depth; int host_dstride;
};
struct LkTally { long long level_passes = 0, iterations = 0, points = 0, tracked = 0; };   // what the sequence adds to gf_tracker_stats

// rejectWithF on the host (feature_tracker.cpp:711-743; gf_reject_f.hpp) for one sequence, at the reference's place: on the points LK kept, ahead of track_cnt++
// and setMask.  status: the sequence's row of status bytes, rewritten in place as the kernel rewrites it on the device.  ran / result: what the stage left.
struct RejectFHost {
    gfcam::Camera cam; uint8_t* status;
    double f_threshold, focal; uint32_t seed;
    bool ran; gfrf::Result result;
};
// The virtual pixels of row i (:722-729): previous and current point lifted with the sequence's camera
inline gfrf::Cand virtual_pair(const gfcam::Camera& cam, double focal, int width, int height, P2f prev, P2f cur) {
    gfrf::Cand c; double P[3];
    gfcam::lift(cam, (double)cur.x, (double)cur.y, P);
    c.bx = gfrf::virtual_pixel(focal, P[0], P[2], width); c.by = gfrf::virtual_pixel(focal, P[1], P[2], height);
    gfcam::lift(cam, (double)prev.x, (double)prev.y, P);
    c.ax = gfrf::virtual_pixel(focal, P[0], P[2], width); c.ay = gfrf::virtual_pixel(focal, P[1], P[2], height);
    return c;
}
inline void reject_f_host(const SeqState& s, int width, int height, const P2f* cur_row, RejectFHost& rf) {
    const int n = (int)s.prev_pts.size();
    rf.ran = false;
    if (n < gfrf::kSample) return;   // as the device form: no job
    static thread_local std::vector<gfrf::Cand> pairs, cand;
    static thread_local std::vector<int> row_of;
    pairs.resize(n); cand.resize(n); row_of.resize(n);
    for (int i = 0; i < n; i++) pairs[i] = rf.status[i] ? virtual_pair(rf.cam, rf.focal, width, height, s.prev_pts[i], cur_row[i]) : gfrf::Cand{0.f, 0.f, 0.f, 0.f};
    rf.result = gfrf::reject(pairs.data(), rf.status, n, rf.f_threshold, rf.seed, cand.data(), row_of.data());
    rf.ran = true;
}

// After LK (feature_tracker.cpp:170-186): the reduction by status, track_cnt++, setMask and the number of corners the sequence wants.
// T: the circle of par.min_dist; roi: the sequence's region of interest or null; centers_row / *n_centers: setMask's kept points for the detector;
// boxes, n_boxes: the sequence's exclusion boxes, as set_mask_host takes them.  keep_rows: the sequence's pairs come from a lift on the device (after_detect's
// un_lk): every kept point carries the row of LK's table it came from (SeqState::lk_row).  rf: rejectWithF runs here (RejectFHost; null: it is off, or ran on the
// device and the status bytes arrive already changed).
inline LkTally after_lk(SeqState& s, const gf_tracker_seq_cfg& par, int width, int height, const DiskTable& T, const uint32_t* roi, const LkRows& r,
                        P2i* centers_row, int* n_centers, int* want, const gf_box* boxes = nullptr, int n_boxes = 0, bool keep_rows = false, RejectFHost* rf = nullptr) {
    LkTally tally;
    const int n = (int)s.prev_pts.size();
    if (rf) reject_f_host(s, width, height, r.cur_pts, *rf);   // rf->status is r.status: the reduction below reads what the stage left
    if (n > 0) {
        const uint8_t* st = r.status;
        s.cur_pts.resize(n); s.cur_depth.resize(n);
        if (keep_rows) { s.lk_row.resize(n); for (int i = 0; i < n; i++) s.lk_row[i] = i; }
        for (int i = 0; i < n; i++) {
            const P2f c = r.cur_pts[i];
            s.cur_pts[i] = c;
            if (r.host_depth) { const int ry = (int)std::round((double)c.y), rx = (int)std::round((double)c.x); s.cur_depth[i] = st[i] ? r.host_depth[(size_t)ry * r.host_dstride + rx] : (uint16_t)0; }   // st: inside the image (post checks)
            else if (!r.depth_out) s.cur_depth[i] = 0;
            else s.cur_depth[i] = r.depth_out[i];
            tally.level_passes += r.counters[2 * i];
            tally.iterations += r.counters[2 * i + 1];
        }
        tally.points = n;
        reduce_vector(s.prev_pts, st); reduce_vector(s.cur_pts, st); reduce_vector(s.ids, st); reduce_vector(s.track_cnt, st);
        reduce_vector(s.cur_depth, st);
        if (keep_rows) reduce_vector(s.lk_row, st);
        tally.tracked = (long long)s.cur_pts.size();
    }
    if (s.show_track) {   // the arrows' far ends, while prev_pts and ids still go by the same index
        s.draw_from.clear();
        if (n > 0) for (size_t i = 0; i < s.ids.size(); i++) s.draw_from.push_back({s.ids[i], s.prev_pts[i]});
        std::sort(s.draw_from.begin(), s.draw_from.end(), [](const std::pair<int, P2f>& a, const std::pair<int, P2f>& b) { return a.first < b.first; });
    }
    for (auto& c : s.track_cnt) c++;
    int nc = 0;   // counted here and stored once: the tables are page-locked memory that neighbouring sequences' threads write too
    set_mask_host(width, height, s, T, roi, centers_row, nc, boxes, n_boxes);
    *n_centers = nc;
    *want = par.max_cnt - (int)s.cur_pts.size();
    return tally;
}

// What the detection left for the sequence: out_n corners (0 for a sequence that wanted none).  out_depth / host_depth as in LkRows.
struct DetectRows {
    const P2f* out_pts; const uint16_t* out_depth; int out_n;
    const uint16_t* host_depth; int host_dstride;
};
struct Packed { int written; int overflow; };   // observations written; or overflow >= 0: that many features did not fit cap_out, none written

// What the stereo kernel left for the sequence (gf_stereo_kernels.hpp), by position in cur_pts -- the tracked survivors in setMask's order, then the new corners:
// the right point of every one and the status the reduction reads (:280; the forward status alone without FLOW_BACK).  cam: the right camera.  un_right: the
// pairs a lift on the device left for the same rows, or null: the right camera's lift runs here, per kept point.
struct StereoRows { const P2f* right_pts; const uint8_t* status; const gfcam::Camera* cam; const P2f* un_right; };
// What a sequence whose left observations carry the depth its matches determine (gf_stereo_depth.hpp) brings to after_detect, with or without a right frame.
// depth_mm / why: what stereo_depth_kernel left for the frame, by position in cur_pts; both null: left (the left camera as the kernel would read it) and rig are
// set and the host computes.  right_obs: the camera_id 1 observations are still emitted.  census (may be null): [gfsd::kReasons] counts by reason, added to.
struct StereoDepthRows { const uint16_t* depth_mm; const uint8_t* why; const gfcam::Camera* left; const gfsd::Rig* rig; bool right_obs; long long* census; };

// The stereo branch of trackImage (feature_tracker.cpp:259-303) behind undistortedPts and ptsVelocity of the left (:210-211) and ahead of the roll-over (:307-312),
// for a frame that came with a right image: the right-hand lists are cleared (:261-265); if cur_pts is not empty, ids_right = ids, cur_right_pts and ids_right are
// reduced by the status (:286-288; the left lists are not touched), the kept points are lifted through the right camera (:298) and their velocities taken against
// the map of the last frame that ran the stage, over this frame's cur_time - prev_time (:299); then prev_un_right_pts_map = cur_un_right_pts_map (:302), also where
// cur_pts was empty.
// sd (gf_tracker_set_seq_stereo_depth): the depth each match determines goes into cur_depth, where a depth camera's sample travels -- read from the kernel's rows,
// or computed here by the same function (GF_STEREO_DEPTH_HOST=1) from the points the kernel would have gathered -- ahead of everything else: the left lists are
// not reduced by the stage, so position i of the rows is feature i.
inline void stereo_stage(SeqState& s, const StereoRows& r, const StereoDepthRows* sd = nullptr) {
    if (sd) {
        const size_t m = s.cur_pts.size();
        s.cur_depth.resize(m);
        for (size_t i = 0; i < m; i++) {
            gfsd::Depth d;
            if (sd->depth_mm) d = gfsd::Depth{sd->depth_mm[i], sd->why[i]};
            else d = gfsd::depth_of(*sd->left, *r.cam, *sd->rig, s.cur_pts[i].x, s.cur_pts[i].y, r.right_pts[i].x, r.right_pts[i].y, r.status[i]);
            s.cur_depth[i] = d.mm;
            if (sd->census) sd->census[d.why < gfsd::kReasons ? d.why : 0]++;
        }
    }
    s.ids_right.clear(); s.cur_right_pts.clear(); s.cur_un_right_pts.clear(); s.right_pts_velocity.clear(); s.cur_un_right_pts_map.clear();
    const size_t n = s.cur_pts.size();
    if (n > 0) {
        for (size_t i = 0; i < n; i++) {
            if (!r.status[i]) continue;
            s.ids_right.push_back(s.ids[i]); s.cur_right_pts.push_back(r.right_pts[i]);
            if (r.un_right) s.cur_un_right_pts.push_back(r.un_right[i]);
            else { double P[3]; P2f o; gfcam::lift_pair(*r.cam, (double)r.right_pts[i].x, (double)r.right_pts[i].y, P, o.x, o.y); s.cur_un_right_pts.push_back(o); }
        }
        pts_velocity_of(s.ids_right, s.cur_un_right_pts, s.cur_un_right_pts_map, s.prev_un_right_pts_map, s.cur_time - s.prev_time, s.right_pts_velocity);
    }
    s.prev_un_right_pts_map = s.cur_un_right_pts_map;
}

// After the detection (feature_tracker.cpp:85-93, 210-211, 322-368): addPoints, undistortedPts, ptsVelocity, the roll-over of prev_* and of the pyramid slot,
// and the featureFrame into out[0 .. cap_out).  have_depth: the call came with depth images.
// cam: the sequence's camera where it is no pinhole (gf_tracker_set_seq_camera); null: the pinhole of par, lifted here as ever.  un_lk / un_out: the pairs a
// lift on the device left for the rows of LK's table and of the detection's (a tracked point picks its own by the row it came from, a new corner by position);
// both null: the model's lift runs here, per point.
// stereo: the frame came with a right image for a sequence that has a right camera (stereo_stage runs at its place, and one observation per entry of ids_right
// follows the left ones: camera_id 1, the right point's pair, pixel and velocity, and the mono loop's -2.4 in the eighth field; the reference's second left
// observation, which would read the right image as depth (:344-368), is not reproduced); null: the stage is skipped and the right-hand state stays as it is.
// sd: the sequence's left observations carry the depth its matches determine (StereoDepthRows): the eighth field is the depth-camera expression on cur_depth,
// 0 for every feature of a frame without a right image; without right_obs the camera_id 1 observations are not emitted and do not count against cap_out.
inline Packed after_detect(SeqState& s, const gf_tracker_seq_cfg& par, const DetectRows& r, bool have_depth, gf_feature_obs* out, int cap_out,
                           const gfcam::Camera* cam = nullptr, const P2f* un_lk = nullptr, const P2f* un_out = nullptr, const StereoRows* stereo = nullptr,
                           const StereoDepthRows* sd = nullptr) {
    const size_t n_tracked = s.cur_pts.size();
    for (int i = 0; i < r.out_n; i++) {
        const P2f p = r.out_pts[i];
        s.cur_pts.push_back(p); s.ids.push_back(s.n_id++); s.track_cnt.push_back(1);
        s.cur_depth.push_back(r.host_depth ? r.host_depth[(size_t)(int)p.y * r.host_dstride + (int)p.x] : !r.out_depth ? (uint16_t)0 : r.out_depth[i]);   // corners sit on pixel centres
    }
    s.cur_un_pts.clear();
    if (!cam) for (auto& p : s.cur_pts) { double X, Y; lift_projective(par, (double)p.x, (double)p.y, X, Y); s.cur_un_pts.push_back({(float)(X / 1.0), (float)(Y / 1.0)}); }
    else if (un_lk && un_out) for (size_t i = 0; i < s.cur_pts.size(); i++) s.cur_un_pts.push_back(i < n_tracked ? un_lk[s.lk_row[i]] : un_out[i - n_tracked]);
    else for (auto& p : s.cur_pts) { double P[3]; P2f o; gfcam::lift_pair(*cam, (double)p.x, (double)p.y, P, o.x, o.y); s.cur_un_pts.push_back(o); }
    pts_velocity(s);
    if (stereo) stereo_stage(s, *stereo, sd);
    else if (sd) s.cur_depth.assign(s.cur_pts.size(), (uint16_t)0);   // no right image: no match determines a depth
    s.prev_pts = s.cur_pts; s.prev_un_pts = s.cur_un_pts; s.prev_un_pts_map.swap(s.cur_un_pts_map); s.prev_time = s.cur_time;
    s.hasPrediction = false;
    s.slot ^= 1;   // the pyramid written in this call is the sequence's previous frame from here on
    const int n = (int)s.ids.size();
    // depth_cam set but no depth image: neither packing loop of the reference runs (feature_tracker.cpp:320 `depth_cam == 0`, :344 `!_img1.empty()`):
    // the returned featureFrame is empty, the tracker state has advanced all the same
    if (par.depth_cam && !have_depth) return {0, -1};
    const int n_right = stereo && (!sd || sd->right_obs) ? (int)s.ids_right.size() : 0;
    if (n + n_right > cap_out) return {0, n + n_right};   // the overflow rule holds for the sum
    for (int i = 0; i < n_right; i++) {
        gf_feature_obs* o = out + n + i;
        o->id = s.ids_right[i]; o->camera_id = 1;
        o->v[0] = s.cur_un_right_pts[i].x; o->v[1] = s.cur_un_right_pts[i].y; o->v[2] = 1; o->v[3] = s.cur_right_pts[i].x; o->v[4] = s.cur_right_pts[i].y;
        o->v[5] = s.right_pts_velocity[i].x; o->v[6] = s.right_pts_velocity[i].y;
        o->v[7] = -2.4;
    }
    for (int i = 0; i < n; i++) {
        gf_feature_obs* o = out + i;
        o->id = s.ids[i]; o->camera_id = 0;
        o->v[0] = s.cur_un_pts[i].x; o->v[1] = s.cur_un_pts[i].y; o->v[2] = 1; o->v[3] = s.cur_pts[i].x; o->v[4] = s.cur_pts[i].y;
        o->v[5] = s.pts_velocity[i].x; o->v[6] = s.pts_velocity[i].y;
        o->v[7] = par.depth_cam || sd ? (double)(int)s.cur_depth[i] / 1000 : -2.4;
    }
    return {n + n_right, -1};
}

// After after_detect, for a sequence whose show_track is on (drawTrack, feature_tracker.cpp:849-905): the frame's primitive list from what the frame left -- a dot
// per feature at its current point, coloured by track_cnt, and an arrow for every feature whose id was in the previous frame, back to the point LK tracked it from
// (draw_from; a newly detected corner has none).  False if the builder refuses a point; the sequence then has no picture and keeps the reason in draw_why.
// boxes, n_boxes: the exclusion boxes in force for the frame; their frames follow all dots and strokes (drawTrackbox, feature_tracker.cpp:960-975).  Its yellow
// dots for the features inside a box (:982-987) have no counterpart: no kept feature lies inside a box.
inline bool record_track(SeqState& s, const gf_box* boxes = nullptr, int n_boxes = 0) {
    const size_t n = s.ids.size();
    static thread_local std::vector<float> cur, prev;
    static thread_local std::vector<uint8_t> has;
    cur.resize(2 * n); prev.assign(2 * n, 0.f); has.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        cur[2 * i] = s.prev_pts[i].x; cur[2 * i + 1] = s.prev_pts[i].y;   // after the roll-over prev_pts holds the frame's points
        auto it = std::lower_bound(s.draw_from.begin(), s.draw_from.end(), s.ids[i], [](const std::pair<int, P2f>& a, int v) { return a.first < v; });
        if (it != s.draw_from.end() && it->first == s.ids[i]) { has[i] = 1; prev[2 * i] = it->second.x; prev[2 * i + 1] = it->second.y; }
    }
    s.draw_list.resize(gfdraw::list_capacity(n) + (size_t)n_boxes);
    char msg[160] = "";
    int m = gfdraw::build_list((int)n, cur.data(), s.track_cnt.data(), prev.data(), has.data(), s.draw_list.data(), msg, sizeof msg);
    if (m >= 0 && n_boxes > 0) m += gfdraw::append_frames(boxes, n_boxes, s.draw_list.data() + m);
    s.draw_sent = false;
    s.draw_have = m >= 0;
    s.draw_list.resize(m >= 0 ? (size_t)m : 0);
    s.draw_why = m >= 0 ? "" : msg;
    return s.draw_have;
}

}  // namespace gf
