// TEST INFRASTRUCTURE: the target of the region-of-interest tests (tests/test_roi_host.py, tests/test_roi_gpu.py).
//
// oracle/ has no mask parameter and is not to change, and a Python restatement would not reproduce std::sort's order among equal track counts, which decides
// both setMask's greedy keep and the order of the output.  So this translation unit includes the oracle's tracker unchanged, derives from gfo::Tracker and
// restates trackImage (feature_tracker.cpp:103-372) in full -- prediction branch and `< 10` fallback included -- with exactly two differences:
//   * setMask() starts from the region of interest R (in {0, 255}) instead of an all-255 image (feature_tracker.cpp:58; VINS-Mono: fisheye_mask.clone()),
//   * goodFeaturesToTrack therefore sees R minus the circles (it is handed the mask setMask left, as in the reference).
// It counts the tracks setMask drops because their pixel lies outside R.  Without a region every line is the base class's.  setPrediction / removeOutliers /
// state come from the base class.  Built by tests/roi_ref.py with the flags of oracle/Makefile, never linked into the product.
#include "../oracle/tracker_oracle.cpp"

namespace {

struct RoiTracker : gfo::Tracker {
    std::vector<uint8_t> roi;   // row x col, 0 / 255; empty: none
    int roi_w = 0, roi_h = 0;
    long long dropped_outside = 0;

    void setMaskRoi() {  // FT:56-83 with `mask = R`
        const bool has = !roi.empty();
        if (has) mask = roi; else mask.assign((size_t)row * col, 255);
        struct E { int cnt; gfo::P2f pt; int id; };
        std::vector<E> v;
        for (size_t i = 0; i < cur_pts.size(); i++) v.push_back({track_cnt[i], cur_pts[i], ids[i]});
        std::sort(v.begin(), v.end(), [](const E& a, const E& b) { return a.cnt > b.cnt; });
        cur_pts.clear(); ids.clear(); track_cnt.clear();
        for (auto& it : v) {
            int x = gfo::cvRoundf(it.pt.x), y = gfo::cvRoundf(it.pt.y);
            if (mask[(size_t)y * col + x] == 255) {
                cur_pts.push_back(it.pt); ids.push_back(it.id); track_cnt.push_back(it.cnt);
                gfo::fill_circle(mask.data(), col, row, col, x, y, cfg.min_dist, 0);
            } else if (has && roi[(size_t)y * col + x] == 0) dropped_outside++;
        }
    }

    int trackImageRoi(double t, const uint8_t* img, int w, int h, int stride, const uint16_t* depth, int dstride, int* out_ids, double* out_obs, int cap) {
        using namespace gfo;
        if (!roi.empty() && (roi_w != w || roi_h != h)) return -1;
        cur_time = t; row = h; col = w;
        cur_img.resize((size_t)w * h);
        for (int y = 0; y < h; y++) memcpy(&cur_img[(size_t)y * w], img + (size_t)y * stride, w);
        cur_pts.clear();
        if (!prev_pts.empty()) {
            std::vector<uint8_t> status(prev_pts.size(), 0);
            if (hasPrediction) {  // FT:118-133
                cur_pts = predict_pts;
                calc_optical_flow_pyr_lk(prev_img.data(), cur_img.data(), w, h, w, prev_pts.data(), cur_pts.data(), status.data(), (int)prev_pts.size(), 1, 30, 0.01, true, &lk_iters);
                int succ = 0;
                for (auto s : status) if (s) succ++;
                if (succ < 10)
                    calc_optical_flow_pyr_lk(prev_img.data(), cur_img.data(), w, h, w, prev_pts.data(), cur_pts.data(), status.data(), (int)prev_pts.size(), 3, 30, 0.01, false, &lk_iters);
            } else {
                cur_pts.assign(prev_pts.size(), P2f{0, 0});
                calc_optical_flow_pyr_lk(prev_img.data(), cur_img.data(), w, h, w, prev_pts.data(), cur_pts.data(), status.data(), (int)prev_pts.size(), 3, 30, 0.01, false, &lk_iters);
            }
            if (cfg.flow_back) {  // FT:138-153
                std::vector<uint8_t> rstatus(prev_pts.size(), 0);
                std::vector<P2f> rpts = prev_pts;
                calc_optical_flow_pyr_lk(cur_img.data(), prev_img.data(), w, h, w, cur_pts.data(), rpts.data(), rstatus.data(), (int)prev_pts.size(), 1, 30, 0.01, true, &lk_iters);
                for (size_t i = 0; i < status.size(); i++) {
                    const double dx = (double)(prev_pts[i].x - rpts[i].x), dy = (double)(prev_pts[i].y - rpts[i].y);  // FT:22-28 (float difference -> double)
                    status[i] = (status[i] && rstatus[i] && std::sqrt(dx * dx + dy * dy) <= 0.5) ? 1 : 0;
                }
            }
            for (int i = 0; i < (int)cur_pts.size(); i++) {  // FT:155-168
                if (status[i] && !inBorder(cur_pts[i])) status[i] = 0;
                int p_u = (int)cur_pts[i].x, p_v = (int)cur_pts[i].y;
                float grey = 0.f;
                if (p_u >= 0 && p_u < row && p_v >= 0 && p_v < col) grey = cur_img[(size_t)p_u * col + p_v];
                if (status[i] && grey > 250) status[i] = 0;
            }
            reduceVector(prev_pts, status); reduceVector(cur_pts, status); reduceVector(ids, status); reduceVector(track_cnt, status);
        }
        for (auto& n : track_cnt) n++;  // FT:178
        setMaskRoi();                   // FT:186, the first difference
        int n_max_cnt = cfg.max_cnt - (int)cur_pts.size();
        if (n_max_cnt > 0)
            good_features_to_track(cur_img.data(), w, h, w, n_pts, n_max_cnt, 0.01, (double)cfg.min_dist, mask.data(), w);  // FT:198, the second: this mask began as R
        else n_pts.clear();
        for (auto& p : n_pts) { cur_pts.push_back(p); ids.push_back(n_id++); track_cnt.push_back(1); }  // FT:85-93
        cur_un_pts = undistortedPts(cur_pts);                                                            // FT:210
        pts_velocity = ptsVelocity(ids, cur_un_pts, cur_un_pts_map, prev_un_pts_map);                    // FT:211
        prev_img = cur_img; prev_pts = cur_pts; prev_un_pts = cur_un_pts; prev_un_pts_map = cur_un_pts_map;
        prev_time = cur_time; hasPrediction = false;
        int n = (int)ids.size();
        if (cfg.depth_cam && !depth) return 0;   // FT:320 / FT:344: empty featureFrame
        for (int i = 0; i < n && i < cap; i++) {  // FT:322-368
            double* o = out_obs + (size_t)i * 8;
            out_ids[i] = ids[i];
            o[0] = cur_un_pts[i].x; o[1] = cur_un_pts[i].y; o[2] = 1; o[3] = cur_pts[i].x; o[4] = cur_pts[i].y;
            o[5] = pts_velocity[i].x; o[6] = pts_velocity[i].y;
            if (cfg.depth_cam && depth) {
                long ry = lround((double)cur_pts[i].y), rx = lround((double)cur_pts[i].x);
                double d = (int)depth[(size_t)ry * dstride + rx];
                o[7] = d / 1000;
            } else o[7] = -2.4;
        }
        return n;
    }
};

}  // namespace

extern "C" {
void* roiref_create(const gfo_tracker_cfg* cfg) { RoiTracker* t = new RoiTracker(); t->cfg = *cfg; return t; }
void roiref_destroy(void* h) { delete (RoiTracker*)h; }
// mask: h x w bytes, non-zero = allowed (stored as 0 / 255); NULL clears
void roiref_set_roi(void* h, const uint8_t* mask, int w, int hh) {
    RoiTracker* t = (RoiTracker*)h;
    t->roi.clear(); t->roi_w = w; t->roi_h = hh;
    if (mask) { t->roi.resize((size_t)w * hh); for (size_t i = 0; i < t->roi.size(); i++) t->roi[i] = mask[i] ? 255 : 0; }
}
int roiref_track(void* h, double t, const uint8_t* img, int w, int hh, int stride, const uint16_t* depth, int dstride, int* out_ids, double* out_obs, int cap) {
    return ((RoiTracker*)h)->trackImageRoi(t, img, w, hh, stride, depth, dstride, out_ids, out_obs, cap);
}
long long roiref_dropped_outside(void* h) { return ((RoiTracker*)h)->dropped_outside; }
// the base class's members, through the base class's own functions
void roiref_set_prediction(void* h, const int* ids, const double* xyz, int n) { ((RoiTracker*)h)->setPrediction(ids, xyz, n); }
void roiref_remove_outliers(void* h, const int* ids, int n) { ((RoiTracker*)h)->removeOutliers(ids, n); }
int roiref_state(void* h, int* ids, int* track_cnt, float* prev_pts, int cap) { return gfo_tracker_state((gfo::Tracker*)(RoiTracker*)h, ids, track_cnt, prev_pts, cap); }
}
