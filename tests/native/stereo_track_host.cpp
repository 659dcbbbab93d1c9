// Stand-alone host program for the stereo stage of ground-fusion_amd/csrc/gf_track_host.hpp (stereo_stage, after_detect's right-hand packing): a CPU tracker made of
// the library's own per-sequence stage functions, with the oracle's LK, circle and corner primitives standing in for the kernels -- the temporal pass as
// lk_track_body runs it, the left-to-right pass as stereo_lk_body (gf_stereo_kernels.hpp) runs it.  No HIP call is made.  It writes what every frame left --
// n_out or the overflow, every observation, the left state and the right-hand state -- to a file; tests/test_stereo_track_host.py writes the frames, builds this
// file with oracle/tracker_oracle.cpp under the address and undefined-behaviour sanitizers, and holds the file to the restatement of tests/stereo_ref.py bit for bit.
//   stereo_track_host FRAMES OUT max_cnt min_dist flow_back fx fy cx cy k1 k2 p1 p2 [remove=K] [reset=K] [short=K]
// FRAMES: int32 w, h, n; n left frames; n right frames; n bytes: 1 = the frame comes with its right image.  The twelve numbers after OUT: the sequence's
// parameters and the right camera (a PINHOLE).  remove=K: removeOutliers of every id with id % 7 == 3 behind frame K; reset=K: gf_tracker_reset_seq's effect ahead
// of frame K; short=K: frame K is first packed into an output one short of what it needs (the stage functions run on a copy of the state).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_track_host.hpp"
#include "../../oracle/gf_oracle.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Frames {
    int w = 0, h = 0, n = 0;
    std::vector<uint8_t> left, right, has_right;
    const uint8_t* L(int k) const { return left.data() + (size_t)k * w * h; }
    const uint8_t* R(int k) const { return has_right[k] ? right.data() + (size_t)k * w * h : nullptr; }
};

static bool read_frames(const char* path, Frames& F) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int hd[3];
    bool ok = fread(hd, sizeof(int), 3, f) == 3;
    if (ok) {
        F.w = hd[0]; F.h = hd[1]; F.n = hd[2];
        const size_t px = (size_t)F.w * F.h;
        F.left.resize(px * F.n); F.right.resize(px * F.n); F.has_right.resize(F.n);
        ok = fread(F.left.data(), 1, F.left.size(), f) == F.left.size() && fread(F.right.data(), 1, F.right.size(), f) == F.right.size() &&
             fread(F.has_right.data(), 1, F.has_right.size(), f) == F.has_right.size();
    }
    fclose(f);
    return ok;
}

// One sequence of the library's bookkeeping with the hand-over tables of one list position, and the oracle's kernels-to-be around it.
struct CpuSeq {
    gf::SeqState s;
    gf_tracker_seq_cfg par{};
    gfcam::Camera right_cam{};
    gf::DiskTable T;
    int w = 0, h = 0, cap = 0;
    std::vector<uint8_t> prev_img, mask;
    std::vector<gf::P2f> prev_row, init_row, cur_row, out_pts, right_row;
    std::vector<gf::P2i> centers;
    std::vector<uint8_t> status, fwd_status, right_status;
    std::vector<uint16_t> depth_out;
    std::vector<unsigned> counters;

    void create(const gf_tracker_seq_cfg& c, const gfcam::Camera& rc, int width, int height) {
        par = c; right_cam = rc; w = width; h = height; cap = (c.max_cnt + 3) & ~3;
        gf::make_disk_table(c.min_dist, T);
        prev_row.resize(cap); init_row.resize(cap); cur_row.resize(cap); out_pts.resize(cap); right_row.resize(cap); centers.resize(cap);
        status.resize(cap); fwd_status.resize(cap); right_status.resize(cap); depth_out.assign(cap, 0); counters.assign(2 * (size_t)cap, 0);
    }

    // what one temporal LK launch leaves in the tables (lk_track_body, gf_lk_kernels.hpp)
    void lk(const uint8_t* img, int n) {
        float* next = &cur_row[0].x;
        for (int i = 0; i < n; i++) cur_row[i] = gf::P2f{0.f, 0.f};
        gfo_lk(prev_img.data(), img, w, h, &prev_row[0].x, next, fwd_status.data(), n, 3, 30, 0.01, 0, nullptr);
        for (int i = 0; i < n; i++) status[i] = fwd_status[i];
        if (par.flow_back) {
            std::vector<gf::P2f> rpts(prev_row.begin(), prev_row.begin() + n);
            std::vector<uint8_t> rst(n, 0);
            gfo_lk(img, prev_img.data(), w, h, next, &rpts[0].x, rst.data(), n, 1, 30, 0.01, 1, nullptr);
            for (int i = 0; i < n; i++) {
                const double dx = (double)(prev_row[i].x - rpts[i].x), dy = (double)(prev_row[i].y - rpts[i].y);
                status[i] = (status[i] && rst[i] && std::sqrt(dx * dx + dy * dy) <= 0.5) ? 1 : 0;
            }
        }
        for (int i = 0; i < n; i++) {
            const float cx = cur_row[i].x, cy = cur_row[i].y;
            const int bx = gf::cvRoundf(cx), by = gf::cvRoundf(cy);
            if (status[i] && !(1 <= bx && bx < w - 1 && 1 <= by && by < h - 1)) status[i] = 0;
            const int p_u = (int)cx, p_v = (int)cy;
            int grey = 0;
            if (status[i] && p_u >= 0 && p_u < h && p_v >= 0 && p_v < w) grey = img[(size_t)p_u * w + p_v];
            if (grey > 250) status[i] = 0;
        }
    }

    // what the stereo launch leaves (stereo_lk_body): the points gathered from LK's rows (SeqState::lk_row) and the selection's table, both passes from scratch with
    // every level, the conjunction of feature_tracker.cpp:280
    void stereo_lk(const uint8_t* left, const uint8_t* right, int n_tracked, int n_new) {
        const int n = n_tracked + n_new;
        std::vector<gf::P2f> src(n), back(n, gf::P2f{0.f, 0.f});
        for (int i = 0; i < n; i++) src[i] = i < n_tracked ? cur_row[s.lk_row[i]] : out_pts[i - n_tracked];
        for (int i = 0; i < n; i++) CHECK(i >= n_tracked || memcmp(&src[i], &s.cur_pts[i], sizeof(gf::P2f)) == 0,"the gather of tracked point %d is not cur_pts[%d]", i, i);
        std::vector<uint8_t> fwd(n, 0), rev(n, 0);
        for (int i = 0; i < n; i++) right_row[i] = gf::P2f{0.f, 0.f};
        if (n == 0) return;
        gfo_lk(left, right, w, h, &src[0].x, &right_row[0].x, fwd.data(), n, 3, 30, 0.01, 0, nullptr);
        for (int i = 0; i < n; i++) right_status[i] = fwd[i];
        if (!par.flow_back) return;
        gfo_lk(right, left, w, h, &right_row[0].x, &back[0].x, rev.data(), n, 3, 30, 0.01, 0, nullptr);
        for (int i = 0; i < n; i++) {
            const double dx = (double)(src[i].x - back[i].x), dy = (double)(src[i].y - back[i].y);
            const int bx = gf::cvRoundf(right_row[i].x), by = gf::cvRoundf(right_row[i].y);
            const bool in = 1 <= bx && bx < w - 1 && 1 <= by && by < h - 1;
            right_status[i] = (fwd[i] && rev[i] && in && std::sqrt(dx * dx + dy * dy) <= 0.5) ? 1 : 0;
        }
    }

    // one frame through the stages of gf_track_host.hpp in track_core's order.  right: the right image or null.  cap_out < 0: one short of what the frame needs
    gf::Packed track(double t, const uint8_t* img, const uint8_t* right, gf_feature_obs* out, int cap_out) {
        (void)gf::begin_frame(s, t);
        int n = 0;
        bool has = false, pred = false;
        char msg[256];
        const int rc = gf::stage_points(s, 0, cap, prev_row.data(), init_row.data(), &n, &has, &pred, msg, sizeof msg);
        CHECK(rc == GF_OK && !pred, "stage_points: %s", msg);
        if (has) lk(img, n);
        int nc = 0, want = 0;
        const gf::LkRows lr{cur_row.data(), status.data(), depth_out.data(), counters.data(), nullptr, w};
        (void)gf::after_lk(s, par, w, h, T, nullptr, lr, centers.data(), &nc, &want, nullptr, 0, /*keep_rows*/ true);
        const int n_tracked = (int)s.cur_pts.size();
        CHECK((int)s.lk_row.size() == n_tracked, "after_lk kept %zu rows for %d points", s.lk_row.size(), n_tracked);
        int out_n = 0;
        if (want > 0) {
            mask.assign((size_t)w * h, 255);
            for (int k = 0; k < nc; k++) gfo_fill_circle(mask.data(), w, h, centers[k].x, centers[k].y, par.min_dist, 0);
            std::vector<float> corners(2 * (size_t)want);
            out_n = gfo_good_features(img, w, h, corners.data(), want, 0.01, (double)par.min_dist, mask.data());
            CHECK(out_n <= want && out_n <= cap, "%d corners for %d wanted", out_n, want);
            for (int i = 0; i < out_n; i++) out_pts[i] = {corners[2 * i], corners[2 * i + 1]};
        }
        if (right) stereo_lk(img, right, n_tracked, out_n);
        const gf::DetectRows dr{out_pts.data(), nullptr, out_n, nullptr, w};
        const gf::StereoRows sr{right_row.data(), right_status.data(), &right_cam, nullptr};
        gf::Packed p;
        if (cap_out < 0) {   // first into an output one short, on a copy of the state: nothing may be written, and the overflow names the sum
            gf::SeqState copy = s;
            std::vector<gf_feature_obs> small(4096);
            const gf::Packed full = gf::after_detect(copy, par, dr, false, small.data(), 4096, nullptr, nullptr, nullptr, right ? &sr : nullptr);
            copy = s;
            memset(small.data(), 0x5a, small.size() * sizeof(gf_feature_obs));
            const gf::Packed shortp = gf::after_detect(copy, par, dr, false, small.data(), full.written - 1, nullptr, nullptr, nullptr, right ? &sr : nullptr);
            CHECK(shortp.written == 0 && shortp.overflow == full.written, "an output of %d for %d observations: written %d, overflow %d", full.written - 1, full.written, shortp.written, shortp.overflow);
            bool clean = true;
            for (size_t i = 0; i < small.size() * sizeof(gf_feature_obs); i++) clean = clean && reinterpret_cast<const uint8_t*>(small.data())[i] == 0x5a;
            CHECK(clean, "an overflowing frame wrote observations");
            printf("short output: %d observations refused in %d\n", full.written, full.written - 1);
            cap_out = 4096;
        }
        p = gf::after_detect(s, par, dr, false, out, cap_out, nullptr, nullptr, nullptr, right ? &sr : nullptr);
        prev_img.assign(img, img + (size_t)w * h);
        return p;
    }
};

template <class T> static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
static void put_int(FILE* f, int v) { fwrite(&v, sizeof v, 1, f); }

int main(int argc, char** argv) {
    if (argc < 14) { printf("usage: stereo_track_host FRAMES OUT max_cnt min_dist flow_back fx fy cx cy k1 k2 p1 p2 [remove=K] [reset=K] [short=K]\n"); return 2; }
    Frames F;
    if (!read_frames(argv[1], F)) { printf("cannot read %s\n", argv[1]); return 2; }
    int remove_at = -1, reset_at = -1, short_at = -1;
    for (int i = 14; i < argc; i++) {
        const std::string a = argv[i];
        const std::string key = a.substr(0, a.find('=')), val = a.substr(a.find('=') + 1);
        if (key == "remove") remove_at = atoi(val.c_str());
        else if (key == "reset") reset_at = atoi(val.c_str());
        else if (key == "short") short_at = atoi(val.c_str());
        else { printf("unknown option %s\n", a.c_str()); return 2; }
    }
    const gf_tracker_seq_cfg par{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), 0, 603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656, 0, 0, 0, 0};
    gf_camera_model rm{};
    rm.model = GF_CAMERA_PINHOLE;
    for (int i = 0; i < 4; i++) { rm.proj[i] = atof(argv[6 + i]); rm.dist[i] = atof(argv[10 + i]); }
    gfcam::Camera rc{};
    char msg[320];
    if (!gfcam::prepare(rm, rc, msg, sizeof msg)) { printf("right camera: %s\n", msg); return 2; }
    CpuSeq c;
    c.create(par, rc, F.w, F.h);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { printf("cannot write %s\n", argv[2]); return 2; }
    std::vector<gf_feature_obs> obs(4096);
    for (int k = 0; k < F.n; k++) {
        if (k == reset_at) c.s = gf::SeqState{};   // gf_tracker_reset_seq: a fresh state; the right-hand members go with it
        const gf::Packed p = c.track(0.0666 * k + 0.001 * k * k, F.L(k), F.R(k), obs.data(), k == short_at ? -1 : 4096);
        CHECK(p.overflow < 0, "frame %d: %d observations overflow the output", k, p.overflow);
        put_int(out, p.written);
        for (int i = 0; i < p.written; i++) { put_int(out, obs[i].id); put_int(out, obs[i].camera_id); put(out, obs[i].v, 8); }
        const gf::SeqState& s = c.s;
        put_int(out, (int)s.ids.size()); put(out, s.ids.data(), s.ids.size()); put(out, s.track_cnt.data(), s.track_cnt.size()); put(out, s.prev_pts.data(), s.prev_pts.size());
        put_int(out, (int)s.ids_right.size()); put(out, s.ids_right.data(), s.ids_right.size()); put(out, s.cur_right_pts.data(), s.cur_right_pts.size());
        put_int(out, (int)s.prev_un_right_pts_map.size());
        for (const auto& e : s.prev_un_right_pts_map) { put_int(out, e.first); put(out, &e.second, 1); }
        if (k == remove_at) {
            std::vector<int> rm_ids;
            for (int id : s.ids) if (id % 7 == 3) rm_ids.push_back(id);
            gf::remove_outliers(c.s, rm_ids.data(), (int)rm_ids.size());
            printf("removeOutliers behind frame %d: %zu ids\n", k, rm_ids.size());
        }
    }
    fclose(out);
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
