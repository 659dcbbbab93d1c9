// Stand-alone host program for ground-fusion_amd/csrc/gf_track_host.hpp: a CPU tracker made of the library's own per-sequence stage functions, with the oracle's
// primitives standing in for the kernels, next to the oracle's Tracker (gfo_tracker_*) on the same frames -- with roi=1, and only then, next to the tracker with
// a region of interest of tests/roi_tracker_ref.cpp (roiref_*) instead.  After every frame ids, the eight observation values (as uint64), n_out and the ids /
// track_cnt / prev_pts state must be equal bit for bit.  No HIP call is made; tests/test_track_host.py writes the frames, builds this file together with
// tests/roi_tracker_ref.cpp (which includes oracle/tracker_oracle.cpp) under the address and undefined-behaviour sanitizers, and runs one case per call:
//   track_host FILE max_cnt min_dist [flow_back=0|1] [feedback=1] [distort=1] [depth_cam=0|1] [depth=none|kernel|host] [roi=1] [two=1]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_track_host.hpp"
#include "../../oracle/gf_oracle.h"

extern "C" {   // tests/roi_tracker_ref.cpp
void* roiref_create(const gfo_tracker_cfg* cfg);
void roiref_destroy(void* h);
void roiref_set_roi(void* h, const uint8_t* mask, int w, int hh);
int roiref_track(void* h, double t, const uint8_t* img, int w, int hh, int stride, const uint16_t* depth, int dstride, int* out_ids, double* out_obs, int cap);
long long roiref_dropped_outside(void* h);
void roiref_set_prediction(void* h, const int* ids, const double* xyz, int n);
void roiref_remove_outliers(void* h, const int* ids, int n);
int roiref_state(void* h, int* ids, int* track_cnt, float* prev_pts, int cap);
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// The yardstick of one sequence: the oracle's own Tracker, or with a region (which the oracle does not have) tests/roi_tracker_ref.cpp's.
struct Oracle {
    void* h; const bool roi;
    Oracle(const gfo_tracker_cfg& c, bool with_region) : h(with_region ? roiref_create(&c) : gfo_tracker_create(&c)), roi(with_region) {}
    ~Oracle() { if (roi) roiref_destroy(h); else gfo_tracker_destroy(h); }
    Oracle(const Oracle&) = delete;
    int track(double t, const uint8_t* img, int w, int hh, const uint16_t* depth, int* ids, double* obs, int cap) {
        return roi ? roiref_track(h, t, img, w, hh, w, depth, w, ids, obs, cap) : gfo_tracker_track(h, t, img, w, hh, w, depth, w, ids, obs, cap);
    }
    void set_prediction(const int* ids, const double* xyz, int n) { if (roi) roiref_set_prediction(h, ids, xyz, n); else gfo_tracker_set_prediction(h, ids, xyz, n); }
    void remove_outliers(const int* ids, int n) { if (roi) roiref_remove_outliers(h, ids, n); else gfo_tracker_remove_outliers(h, ids, n); }
    int state(int* ids, int* cnt, float* pts, int cap) { return roi ? roiref_state(h, ids, cnt, pts, cap) : gfo_tracker_state(h, ids, cnt, pts, cap); }
    long long dropped_outside() { return roi ? roiref_dropped_outside(h) : 0; }
};

enum DepthMode { kNoDepth, kKernelDepth, kHostDepth };   // none; sampled "in the kernels" into the depth rows; the host image handed to the stages

struct Frames {   // what the pytest wrote: int32 w, h, n, r; n gray frames; n depth frames; the region (w x h, 0 / 255); n x 3 x r doubles (uniform, uniform, normal)
    int w = 0, h = 0, n = 0, r = 0;
    std::vector<uint8_t> gray, region;
    std::vector<uint16_t> depth;
    std::vector<double> rnd;
    const uint8_t* img(int k) const { return gray.data() + (size_t)k * w * h; }
    const uint16_t* dimg(int k) const { return depth.data() + (size_t)k * w * h; }
    const double* random(int k, int which) const { return rnd.data() + ((size_t)k * 3 + which) * r; }
};

static bool read_frames(const char* path, Frames& F) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int hd[4];
    bool ok = fread(hd, sizeof(int), 4, f) == 4;
    if (ok) {
        F.w = hd[0]; F.h = hd[1]; F.n = hd[2]; F.r = hd[3];
        const size_t px = (size_t)F.w * F.h;
        F.gray.resize(px * F.n); F.depth.resize(px * F.n); F.region.resize(px); F.rnd.resize((size_t)F.n * 3 * F.r);
        ok = fread(F.gray.data(), 1, F.gray.size(), f) == F.gray.size() && fread(F.depth.data(), 2, F.depth.size(), f) == F.depth.size() &&
             fread(F.region.data(), 1, px, f) == px && fread(F.rnd.data(), 8, F.rnd.size(), f) == F.rnd.size();
    }
    fclose(f);
    return ok;
}

// One sequence of the library's bookkeeping with the hand-over tables of one list position, and the oracle's kernels-to-be around it.
struct CpuSeq {
    gf::SeqState s;
    gf_tracker_seq_cfg par{};
    gf::DiskTable T;
    int w = 0, h = 0, cap = 0;
    std::vector<uint32_t> roi_words;   // gf_roi.hpp's table of the region, as gf_tracker_set_roi packs it; empty: none
    std::vector<uint8_t> roi_mask, prev_img, mask;
    std::vector<gf::P2f> prev_row, init_row, cur_row, out_pts;
    std::vector<gf::P2i> centers;
    std::vector<uint8_t> status, fwd_status;
    std::vector<uint16_t> depth_out, out_depth;
    std::vector<unsigned> counters;
    long long fallbacks = 0, covered = 0, want_passes = 0, want_iters = 0;   // want_*: what LkTally must add up to in this frame

    void create(const gf_tracker_seq_cfg& c, int width, int height) {
        par = c; w = width; h = height; cap = (c.max_cnt + 3) & ~3;
        gf::make_disk_table(c.min_dist, T);
        prev_row.resize(cap); init_row.resize(cap); cur_row.resize(cap); out_pts.resize(cap); centers.resize(cap);
        status.resize(cap); fwd_status.resize(cap); depth_out.resize(cap); out_depth.resize(cap); counters.assign(2 * (size_t)cap, 0);
    }
    void set_roi(const uint8_t* m) {
        roi_mask.assign(m, m + (size_t)w * h);
        roi_words.assign(gfroi::words(w, h), 0);
        for (int band = 0; band < gfroi::bands(h); band++)
            for (int x = 0; x < w; x++) gfroi::pack_thread(m, (size_t)w, w, h, band, x, roi_words.data());
    }

    // what one LK launch leaves in the tables (lk_track_body, gf_lk_kernels.hpp): forward pass, LkBatchArgs::flow_back, LkBatchArgs::post_checks, the depth sample
    void lk(const uint8_t* img, const uint16_t* kdepth, int n, int levels, bool use_init, bool redo = false) {
        float* next = &cur_row[0].x;
        for (int i = 0; i < n; i++) cur_row[i] = use_init ? init_row[i] : gf::P2f{0.f, 0.f};
        gfo_lk(prev_img.data(), img, w, h, &prev_row[0].x, next, fwd_status.data(), n, levels, 30, 0.01, use_init ? 1 : 0, nullptr);
        for (int i = 0; i < n; i++) status[i] = fwd_status[i];
        if (par.flow_back) {   // reverse LK + 0.5 px check (feature_tracker.cpp:138-153)
            std::vector<gf::P2f> rpts(prev_row.begin(), prev_row.begin() + n);
            std::vector<uint8_t> rst(n, 0);
            gfo_lk(img, prev_img.data(), w, h, next, &rpts[0].x, rst.data(), n, 1, 30, 0.01, 1, nullptr);
            for (int i = 0; i < n; i++) {
                const double dx = (double)(prev_row[i].x - rpts[i].x), dy = (double)(prev_row[i].y - rpts[i].y);
                status[i] = (status[i] && rst[i] && std::sqrt(dx * dx + dy * dy) <= 0.5) ? 1 : 0;
            }
        }
        for (int i = 0; i < n; i++) {   // inBorder and the brightness test with x as the row (feature_tracker.cpp:155-168)
            const float cx = cur_row[i].x, cy = cur_row[i].y;
            const int bx = gf::cvRoundf(cx), by = gf::cvRoundf(cy);
            if (status[i] && !(1 <= bx && bx < w - 1 && 1 <= by && by < h - 1)) status[i] = 0;
            const int p_u = (int)cx, p_v = (int)cy;
            int grey = 0;
            if (status[i] && p_u >= 0 && p_u < h && p_v >= 0 && p_v < w) grey = img[(size_t)p_u * w + p_v];
            if (grey > 250) status[i] = 0;
            const unsigned passes = 3u * i + levels, iters = 5u * i + 1;   // a pattern in the place of the kernel's counts; a redone sequence keeps both passes' (redo_fallback)
            counters[2 * i] = redo ? counters[2 * i] + passes : passes; counters[2 * i + 1] = redo ? counters[2 * i + 1] + iters : iters;
            want_passes += passes; want_iters += iters;
            depth_out[i] = status[i] && kdepth ? kdepth[(size_t)(int)std::round((double)cy) * w + (int)std::round((double)cx)] : (uint16_t)0;
        }
    }

    // one frame through the stages of gf_track_host.hpp in track_core's order; returns n_out
    int track(double t, const uint8_t* img, const uint16_t* depth, DepthMode mode, gf_feature_obs* out, int cap_out) {
        const uint16_t* kdepth = mode == kKernelDepth ? depth : nullptr;
        const uint16_t* hdepth = mode == kHostDepth && par.depth_cam ? depth : nullptr;   // FrameInput::host_image
        const int slot = s.slot;
        CHECK(gf::begin_frame(s, t) == (slot ^ 1), "begin_frame names the wrong pyramid");
        int n = 0;
        bool has = false, pred = false;
        char msg[256];
        const int rc = gf::stage_points(s, 0, cap, prev_row.data(), init_row.data(), &n, &has, &pred, msg, sizeof msg);
        CHECK(rc == GF_OK, "stage_points: %s", msg);
        if (rc != GF_OK) return -1;
        want_passes = want_iters = 0;
        if (has) {
            lk(img, kdepth, n, pred ? 1 : 3, pred);
            if (gf::prediction_failed(s, fwd_status.data(), n)) { fallbacks++; lk(img, kdepth, n, 3, false, true); }
        }
        int nc = 0, want = 0, alive = 0;
        for (int i = 0; has && i < n; i++) alive += status[i];
        const gf::LkRows lr{cur_row.data(), status.data(), mode == kHostDepth ? nullptr : depth_out.data(), counters.data(), hdepth, w};
        const gf::LkTally tally = gf::after_lk(s, par, w, h, T, roi_words.empty() ? nullptr : roi_words.data(), lr, centers.data(), &nc, &want);
        CHECK(tally.points == (has ? n : 0), "after_lk counted %lld points of %d", tally.points, n);
        CHECK(tally.level_passes == want_passes && tally.iterations == want_iters, "after_lk summed %lld level passes and %lld iterations, the rows hold %lld and %lld", tally.level_passes, tally.iterations, want_passes, want_iters);
        CHECK(tally.tracked == alive, "after_lk: %lld tracked, the status row keeps %d", tally.tracked, alive);
        if (roi_words.empty()) covered += tally.tracked - nc;   // what setMask's walk dropped under an earlier point's circle
        int out_n = 0;
        if (want > 0) {   // the detector's mask -- the region or all-255, minus the circles -- and the selection
            if (roi_mask.empty()) mask.assign((size_t)w * h, 255); else mask = roi_mask;
            for (int k = 0; k < nc; k++) gfo_fill_circle(mask.data(), w, h, centers[k].x, centers[k].y, par.min_dist, 0);
            std::vector<float> corners(2 * (size_t)want);
            out_n = gfo_good_features(img, w, h, corners.data(), want, 0.01, (double)par.min_dist, mask.data());
            CHECK(out_n <= want && out_n <= cap, "%d corners for %d wanted", out_n, want);
            for (int i = 0; i < out_n; i++) {
                out_pts[i] = {corners[2 * i], corners[2 * i + 1]};
                out_depth[i] = kdepth ? kdepth[(size_t)(int)corners[2 * i + 1] * w + (int)corners[2 * i]] : (uint16_t)0;
            }
        }
        const gf::DetectRows dr{out_pts.data(), mode == kHostDepth ? nullptr : out_depth.data(), out_n, hdepth, w};
        const gf::Packed p = gf::after_detect(s, par, dr, mode != kNoDepth, out, cap_out);
        CHECK(p.overflow < 0, "%d features overflow the output", p.overflow);
        CHECK(s.slot == (slot ^ 1), "the pyramid slot did not flip");
        prev_img.assign(img, img + (size_t)w * h);
        return p.written;
    }
};

struct Options { int flow_back = 1, feedback = 0, distort = 0, depth_cam = 1, roi = 0, two = 0; DepthMode depth = kKernelDepth; };

// set_prediction / remove_outliers between frames, as _feedback of tests/test_roi_host.py drives them: 5 % of the reported ids are removed, 70 % of the rest get a
// prediction near their pixel -- far from it behind frame 3, so that most fail and the `< 10` branch runs.  The oracle gets the same calls.
static void feedback(const Frames& F, int k, CpuSeq& c, Oracle& oracle, const int* ids_out, int n_out) {
    const double* u1 = F.random(k, 0), * u2 = F.random(k, 1), * nrm = F.random(k, 2);
    std::vector<int> rm, sel;
    for (int i = 0; i < n_out; i++) if (u1[i % F.r] < 0.05) rm.push_back(ids_out[i]);
    gf::remove_outliers(c.s, rm.data(), (int)rm.size());
    oracle.remove_outliers(rm.data(), (int)rm.size());
    const double noise = k == 3 ? 200.0 : 1.0;
    std::vector<double> xyz;
    for (size_t i = 0; i < c.s.ids.size(); i++) {
        if (!(u2[i % F.r] < 0.7)) continue;
        const double u = c.s.prev_pts[i].x + noise * nrm[(2 * i) % F.r], v = c.s.prev_pts[i].y + noise * nrm[(2 * i + 1) % F.r];
        sel.push_back(c.s.ids[i]);
        xyz.push_back((u - c.par.cx) / c.par.fx * 2.0); xyz.push_back((v - c.par.cy) / c.par.fy * 2.0); xyz.push_back(2.0);
    }
    gf::set_prediction(c.s, c.par, sel.data(), xyz.data(), (int)sel.size());
    oracle.set_prediction(sel.data(), xyz.data(), (int)sel.size());
}

// one sequence against its oracle, frame by frame
struct Runner {
    const Frames& F; const Options& o; gf_tracker_seq_cfg par; std::string name; double t0;
    CpuSeq c;
    Oracle oracle;
    static constexpr int cap = 4096;
    std::vector<gf_feature_obs> obs = std::vector<gf_feature_obs>(cap);
    std::vector<int> oids = std::vector<int>(cap), ocnt = std::vector<int>(cap), prev_ids;
    std::vector<double> oobs = std::vector<double>((size_t)cap * 8);
    std::vector<float> opts = std::vector<float>((size_t)cap * 2);
    int fewest = 1 << 30;   // ids carried over from one frame to the next

    Runner(const Frames& F_, const Options& o_, const gf_tracker_seq_cfg& p, const char* n, double t)
        : F(F_), o(o_), par(p), name(n), t0(t),
          oracle(gfo_tracker_cfg{p.max_cnt, p.min_dist, p.flow_back, p.depth_cam, p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.p1, p.p2}, o_.roi != 0) {
        c.create(par, F.w, F.h);
        if (o.roi) { c.set_roi(F.region.data()); roiref_set_roi(oracle.h, F.region.data(), F.w, F.h); }
    }
    void step(int k) {
        const char* nm = name.c_str();
        const double t = t0 + 0.0666 * k;
        const uint16_t* depth = o.depth == kNoDepth ? nullptr : F.dimg(k);
        const int n = c.track(t, F.img(k), depth, o.depth, obs.data(), cap);
        const int on = oracle.track(t, F.img(k), F.w, F.h, depth, oids.data(), oobs.data(), cap);
        CHECK(n == on, "%s frame %d: n_out %d, the oracle's %d", nm, k, n, on);
        for (int i = 0; i < n && i < on; i++) {
            CHECK(obs[i].id == oids[i] && obs[i].camera_id == 0, "%s frame %d: id %d at %d, the oracle's %d", nm, k, obs[i].id, i, oids[i]);
            CHECK(memcmp(obs[i].v, &oobs[(size_t)i * 8], 8 * sizeof(uint64_t)) == 0, "%s frame %d: observation %d differs", nm, k, i);
        }
        const int sn = oracle.state(oids.data(), ocnt.data(), opts.data(), cap);
        CHECK(sn == (int)c.s.ids.size() && c.s.track_cnt.size() == c.s.ids.size() && c.s.prev_pts.size() == c.s.ids.size(), "%s frame %d: %zu ids, the oracle's %d", nm, k, c.s.ids.size(), sn);
        for (int i = 0; i < sn && i < (int)c.s.ids.size(); i++)
            CHECK(c.s.ids[i] == oids[i] && c.s.track_cnt[i] == ocnt[i] && memcmp(&c.s.prev_pts[i], &opts[2 * (size_t)i], 8) == 0, "%s frame %d: state differs at %d", nm, k, i);
        if (k > 0) { int carried = 0; for (int id : c.s.ids) for (int p : prev_ids) carried += id == p; fewest = std::min(fewest, carried); }
        prev_ids = c.s.ids;
        if (o.feedback) feedback(F, k, c, oracle, oids.data(), sn);   // the state's ids: the reported ones, also where depth_cam without an image leaves the frame empty
    }
    void finish() {   // the inputs are alive: a dead sequence would pass everything above
        const char* nm = name.c_str();
        printf("%s: fewest ids carried over %d of %d, setMask dropped %lld covered points, the region %lld tracks, %lld fallbacks\n", nm, fewest, par.max_cnt, c.covered,
               oracle.dropped_outside(), c.fallbacks);
        CHECK(3 * fewest >= par.max_cnt, "%s: only %d of %d ids carried over", nm, fewest, par.max_cnt);
        if (o.roi) CHECK(oracle.dropped_outside() >= 1, "%s: the region dropped no track", nm);
        else CHECK(c.covered >= 1, "%s: setMask dropped no covered point", nm);
        if (o.feedback) CHECK(c.fallbacks >= 1, "%s: the `< 10` branch was never taken", nm);
    }
};

int main(int argc, char** argv) {
    if (argc < 5) { printf("usage: track_host FILE max_cnt min_dist [key=value ...]\n"); return 2; }
    Frames F;
    if (!read_frames(argv[1], F)) { printf("cannot read %s\n", argv[1]); return 2; }
    Options o;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        const std::string key = a.substr(0, a.find('=')), val = a.substr(a.find('=') + 1);
        if (key == "flow_back") o.flow_back = atoi(val.c_str());
        else if (key == "feedback") o.feedback = atoi(val.c_str());
        else if (key == "distort") o.distort = atoi(val.c_str());
        else if (key == "depth_cam") o.depth_cam = atoi(val.c_str());
        else if (key == "roi") o.roi = atoi(val.c_str());
        else if (key == "two") o.two = atoi(val.c_str());
        else if (key == "depth") o.depth = val == "none" ? kNoDepth : val == "host" ? kHostDepth : kKernelDepth;
        else { printf("unknown option %s\n", a.c_str()); return 2; }
    }
    gf_tracker_seq_cfg par{atoi(argv[2]), atoi(argv[3]), o.flow_back, o.depth_cam, 603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656, 0, 0, 0, 0};
    if (o.distort) {   // tests/test_tracker_gpu.py, test_track_image_with_lens_distortion (config/realsense/idc_cam.yaml)
        par.fx = 6.2097277909374247e+02; par.fy = 6.2212293397677581e+02; par.cx = 3.1175896455154810e+02; par.cy = 2.4718077836114819e+02;
        par.k1 = 1.4865749308203452e-01; par.k2 = -4.6815685578576460e-01; par.p1 = 1.6205585303208318e-03; par.p2 = -8.9101576735577930e-03;
    }
    gf_tracker_seq_cfg other = par;   // two=1: a second sequence with parameters of its own through the same functions, in turn with the first as a call walks its list
    other.max_cnt = par.max_cnt * 3 / 4; other.min_dist = par.min_dist + 2; other.flow_back = !par.flow_back;
    Runner a(F, o, par, "sequence 0", 0.0), b(F, o, o.two ? other : par, "sequence 1", 100.0);   // without two=1 the second one stays idle
    for (int k = 0; k < F.n; k++) { a.step(k); if (o.two) b.step(k); }
    a.finish();
    if (o.two) b.finish();
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
