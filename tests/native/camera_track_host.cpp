// Stand-alone host program for the camera models in the tracker's host bookkeeping (ground-fusion_amd/csrc/gf_track_host.hpp): the CPU tracker that
// tests/native/track_host.cpp is made of -- the library's per-sequence stage functions with the oracle's LK, circle and corner primitives in the place of the
// kernels -- run three times on the same frames:
//   pinhole      no camera: the host lift of ever
//   tables       a Kannala-Brandt camera whose pairs come from two tables filled for EVERY row of LK's points and of the new corners, as the lift kernel leaves
//                them, so that a tracked point has to find its own through the reduction by status and setMask's sort
//   host         the same camera lifted per point in after_detect (GF_CAMERA_LIFT_HOST)
// Between frames every run drops the same ids and gets predictions for the same float pixel targets, each through its own model's space_to_plane.
// Ids, track counts, pixel coordinates and depths must be equal bit for bit in all three; pairs and velocities of `tables` and `host` likewise (one header, one
// machine).  The observations of `tables` go to OUT for tests/test_camera_track_host.py, which holds them to the 60-digit formulas:
//   camera_track_host FRAMES max_cnt min_dist OUT      FRAMES as tests/test_track_host.py writes it
//   OUT: per frame  int32 n, double t, n x (int32 id, 8 doubles)
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

struct Frames {   // int32 w, h, n, r; n gray frames; n depth frames; a region (not used here); n x 3 x r doubles (uniform, uniform, normal)
    int w = 0, h = 0, n = 0, r = 0;
    std::vector<uint8_t> gray;
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
        std::vector<uint8_t> region(px);
        F.gray.resize(px * F.n); F.depth.resize(px * F.n); F.rnd.resize((size_t)F.n * 3 * F.r);
        ok = fread(F.gray.data(), 1, F.gray.size(), f) == F.gray.size() && fread(F.depth.data(), 2, F.depth.size(), f) == F.depth.size() &&
             fread(region.data(), 1, px, f) == px && fread(F.rnd.data(), 8, F.rnd.size(), f) == F.rnd.size();
    }
    fclose(f);
    return ok;
}

enum Mode { kPinhole, kTables, kHostLift };

struct CpuSeq {   // one sequence through the stages of gf_track_host.hpp in track_core's order (tests/native/track_host.cpp has the annotated original)
    gf::SeqState s;
    gf_tracker_seq_cfg par{};
    gf::DiskTable T;
    Mode mode = kPinhole;
    gfcam::Camera cam{};
    int w = 0, h = 0, cap = 0;
    long long fallbacks = 0, moved = 0;   // moved: tracked points that left the row LK had them in
    std::vector<uint8_t> prev_img, mask, status, fwd_status;
    std::vector<gf::P2f> prev_row, init_row, cur_row, out_pts, un_lk, un_out;
    std::vector<gf::P2i> centers;
    std::vector<uint16_t> depth_out, out_depth;
    std::vector<unsigned> counters;

    void create(const gf_tracker_seq_cfg& c, int width, int height, Mode m, const gfcam::Camera& camera) {
        par = c; w = width; h = height; cap = (c.max_cnt + 3) & ~3; mode = m; cam = camera;
        gf::make_disk_table(c.min_dist, T);
        prev_row.resize(cap); init_row.resize(cap); cur_row.resize(cap); out_pts.resize(cap); un_lk.resize(cap); un_out.resize(cap); centers.resize(cap);
        status.resize(cap); fwd_status.resize(cap); depth_out.resize(cap); out_depth.resize(cap); counters.assign(2 * (size_t)cap, 0);
    }
    void lk(const uint8_t* img, const uint16_t* kdepth, int n, int levels, bool use_init) {
        float* next = &cur_row[0].x;
        for (int i = 0; i < n; i++) cur_row[i] = use_init ? init_row[i] : gf::P2f{0.f, 0.f};
        gfo_lk(prev_img.data(), img, w, h, &prev_row[0].x, next, fwd_status.data(), n, levels, 30, 0.01, use_init ? 1 : 0, nullptr);
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
            counters[2 * i] = 1; counters[2 * i + 1] = 1;
            depth_out[i] = status[i] && kdepth ? kdepth[(size_t)(int)std::round((double)cy) * w + (int)std::round((double)cx)] : (uint16_t)0;
        }
    }
    int track(double t, const uint8_t* img, const uint16_t* depth, gf_feature_obs* out, int cap_out) {
        (void)gf::begin_frame(s, t);
        int n = 0;
        bool has = false, pred = false;
        char msg[256];
        const int rc = gf::stage_points(s, 0, cap, prev_row.data(), init_row.data(), &n, &has, &pred, msg, sizeof msg);
        CHECK(rc == GF_OK, "stage_points: %s", msg);
        if (rc != GF_OK) return -1;
        if (has) {
            lk(img, depth, n, pred ? 1 : 3, pred);
            if (gf::prediction_failed(s, fwd_status.data(), n)) { fallbacks++; lk(img, depth, n, 3, false); }
        }
        // what the lift kernel leaves for LK's table: a pair for every row, tracked or not (a lost point's coordinates are anything; the lift has a bound)
        if (mode == kTables) for (int i = 0; i < n; i++) { double P[3]; gfcam::lift_pair(cam, (double)cur_row[i].x, (double)cur_row[i].y, P, un_lk[i].x, un_lk[i].y); }
        int nc = 0, want = 0;
        const gf::LkRows lr{cur_row.data(), status.data(), depth_out.data(), counters.data(), nullptr, w};
        (void)gf::after_lk(s, par, w, h, T, nullptr, lr, centers.data(), &nc, &want, nullptr, 0, mode == kTables);
        for (size_t i = 0; i < s.lk_row.size(); i++) moved += s.lk_row[i] != (int)i;
        CHECK(s.lk_row.size() == (mode == kTables ? s.cur_pts.size() : 0), "after_lk left %zu rows for %zu points", s.lk_row.size(), s.cur_pts.size());
        for (size_t i = 0; i < s.lk_row.size() && i < s.cur_pts.size(); i++)
            CHECK(s.lk_row[i] >= 0 && s.lk_row[i] < n && memcmp(&cur_row[s.lk_row[i]], &s.cur_pts[i], sizeof(gf::P2f)) == 0, "point %zu does not lie in the row it names", i);
        int out_n = 0;
        if (want > 0) {
            mask.assign((size_t)w * h, 255);
            for (int k = 0; k < nc; k++) gfo_fill_circle(mask.data(), w, h, centers[k].x, centers[k].y, par.min_dist, 0);
            std::vector<float> corners(2 * (size_t)want);
            out_n = gfo_good_features(img, w, h, corners.data(), want, 0.01, (double)par.min_dist, mask.data());
            for (int i = 0; i < out_n; i++) {
                out_pts[i] = {corners[2 * i], corners[2 * i + 1]};
                out_depth[i] = depth ? depth[(size_t)(int)corners[2 * i + 1] * w + (int)corners[2 * i]] : (uint16_t)0;
                if (mode == kTables) { double P[3]; gfcam::lift_pair(cam, (double)out_pts[i].x, (double)out_pts[i].y, P, un_out[i].x, un_out[i].y); }
            }
        }
        const gf::DetectRows dr{out_pts.data(), out_depth.data(), out_n, nullptr, w};
        const gf::Packed p = mode == kPinhole ? gf::after_detect(s, par, dr, depth != nullptr, out, cap_out)
                           : mode == kTables  ? gf::after_detect(s, par, dr, depth != nullptr, out, cap_out, &cam, un_lk.data(), un_out.data())
                                              : gf::after_detect(s, par, dr, depth != nullptr, out, cap_out, &cam);
        CHECK(p.overflow < 0, "%d features overflow the output", p.overflow);
        prev_img.assign(img, img + (size_t)w * h);
        return p.written;
    }
};

int main(int argc, char** argv) {
    if (argc < 5) { printf("usage: camera_track_host FRAMES max_cnt min_dist OUT\n"); return 2; }
    Frames F;
    if (!read_frames(argv[1], F)) { printf("cannot read %s\n", argv[1]); return 2; }
    FILE* dump = fopen(argv[4], "wb");
    if (!dump) { printf("cannot write %s\n", argv[4]); return 2; }
    const gf_tracker_seq_cfg par{atoi(argv[2]), atoi(argv[3]), 1, 1, 0.9 * F.w, 0.9 * F.w, 0.5 * F.w + 0.25, 0.5 * F.h - 0.25, 0.05, -0.01, 1e-3, -5e-4};
    gf_camera_model m;   // the `wiggle` polynomial of the fixture, scaled so that one root, three roots and the jump to the last segment all lie inside the frame
    memset(&m, 0, sizeof m);
    m.model = GF_CAMERA_KANNALA_BRANDT;
    m.proj[0] = 0.45 * F.w; m.proj[1] = 0.45 * F.w + 0.75; m.proj[2] = 0.5 * F.w + 0.5; m.proj[3] = 0.5 * F.h + 0.25;
    m.dist[0] = -0.9; m.dist[1] = 0.35; m.dist[2] = -0.05; m.dist[3] = 0.0025;
    gfcam::Camera cam;
    char msg[320];
    if (!gfcam::prepare(m, cam, msg, sizeof msg)) { printf("camera refused: %s\n", msg); return 2; }
    printf("camera %a %a %a %a\n", m.proj[0], m.proj[1], m.proj[2], m.proj[3]);
    CpuSeq run[3];
    const Mode modes[3] = {kPinhole, kTables, kHostLift};
    for (int i = 0; i < 3; i++) run[i].create(par, F.w, F.h, modes[i], cam);
    const int cap = 4096;
    std::vector<gf_feature_obs> obs[3] = {std::vector<gf_feature_obs>(cap), std::vector<gf_feature_obs>(cap), std::vector<gf_feature_obs>(cap)};
    long long carried = 0, predicted = 0;
    std::vector<int> prev_ids;
    for (int k = 0; k < F.n; k++) {
        const double t = 0.0666 * k;
        int n[3];
        for (int i = 0; i < 3; i++) n[i] = run[i].track(t, F.img(k), F.dimg(k), obs[i].data(), cap);
        CHECK(n[0] == n[1] && n[0] == n[2] && n[0] > 0, "frame %d: n_out %d, %d, %d", k, n[0], n[1], n[2]);
        for (int j = 0; j < n[0] && j < n[1] && j < n[2]; j++) {
            const gf_feature_obs &a = obs[0][j], &b = obs[1][j], &c = obs[2][j];
            CHECK(a.id == b.id && a.id == c.id, "frame %d: ids %d, %d, %d at %d", k, a.id, b.id, c.id, j);
            CHECK(memcmp(&a.v[2], &b.v[2], 24) == 0 && memcmp(&a.v[2], &c.v[2], 24) == 0 && memcmp(&a.v[7], &b.v[7], 8) == 0 && memcmp(&a.v[7], &c.v[7], 8) == 0,
                  "frame %d: pixel coordinates or depth of feature %d differ between the models", k, j);
            CHECK(memcmp(b.v, c.v, sizeof b.v) == 0, "frame %d: the pairs picked from the tables and the pairs lifted in place differ at feature %d", k, j);
        }
        for (int i = 1; i < 3; i++) {
            const gf::SeqState &a = run[0].s, &b = run[i].s;
            CHECK(a.ids == b.ids && a.track_cnt == b.track_cnt && a.prev_pts.size() == b.prev_pts.size() &&
                  memcmp(a.prev_pts.data(), b.prev_pts.data(), a.prev_pts.size() * sizeof(gf::P2f)) == 0, "frame %d: the state of run %d differs from the pinhole run's", k, i);
        }
        for (int id : run[0].s.ids) for (int p : prev_ids) carried += id == p;
        prev_ids = run[0].s.ids;
        const int32_t nn = n[1];
        fwrite(&nn, 4, 1, dump); fwrite(&t, 8, 1, dump);
        for (int j = 0; j < n[1]; j++) { const int32_t id = obs[1][j].id; fwrite(&id, 4, 1, dump); fwrite(obs[1][j].v, 8, 8, dump); }
        // feedback: 5 % of the ids removed, 70 % of the rest predicted at a float pixel near their own -- far from it behind frame 3, so that the `< 10` branch runs
        const double* u1 = F.random(k, 0), * u2 = F.random(k, 1), * nrm = F.random(k, 2);
        std::vector<int> rm, sel;
        for (size_t i = 0; i < run[0].s.ids.size(); i++) if (u1[i % F.r] < 0.05) rm.push_back(run[0].s.ids[i]);
        for (int i = 0; i < 3; i++) gf::remove_outliers(run[i].s, rm.data(), (int)rm.size());
        const double noise = k == 3 ? 200.0 : 1.0;
        std::vector<double> xyz_pin, xyz_cam;
        for (size_t i = 0; i < run[0].s.ids.size(); i++) {
            if (!(u2[i % F.r] < 0.7)) continue;
            const float u = (float)(run[0].s.prev_pts[i].x + noise * nrm[(2 * i) % F.r]), v = (float)(run[0].s.prev_pts[i].y + noise * nrm[(2 * i + 1) % F.r]);
            double X, Y, P[3], bu, bv;
            gf::lift_projective(par, (double)u, (double)v, X, Y);   // the pinhole's own inverse: its projection lands on the float pixel again
            gfcam::lift(cam, (double)u, (double)v, P);
            gfcam::space_to_plane(cam, P, bu, bv);
            double pu, pv;
            const double R[3] = {X * 2.0, Y * 2.0, 2.0};
            gf::space_to_plane(par, R, pu, pv);
            if ((float)bu != u || (float)bv != v || (float)pu != u || (float)pv != v) continue;   // a target in the several-roots band of the polynomial, or outside the convergence of the fixed point
            sel.push_back(run[0].s.ids[i]);
            xyz_pin.insert(xyz_pin.end(), R, R + 3);
            for (int j = 0; j < 3; j++) xyz_cam.push_back(P[j] * 1.5);
        }
        predicted += (long long)sel.size();
        gf::set_prediction(run[0].s, par, sel.data(), xyz_pin.data(), (int)sel.size());
        for (int i = 1; i < 3; i++) gf::set_prediction(run[i].s, par, sel.data(), xyz_cam.data(), (int)sel.size(), &cam);
        for (int i = 1; i < 3; i++)
            CHECK(run[i].s.predict_pts.size() == run[0].s.predict_pts.size() &&
                  memcmp(run[i].s.predict_pts.data(), run[0].s.predict_pts.data(), run[0].s.predict_pts.size() * sizeof(gf::P2f)) == 0, "frame %d: predictions of run %d differ", k, i);
    }
    fclose(dump);
    printf("ids carried over %lld, predictions %lld, tracked points that left their row %lld, fallbacks %lld\n", carried, predicted, run[1].moved, run[1].fallbacks);
    CHECK(carried >= 2LL * par.max_cnt, "only %lld ids were carried from frame to frame", carried);
    CHECK(run[1].moved >= 10, "only %lld tracked points left the row LK had them in: the row index is not exercised", run[1].moved);
    CHECK(predicted >= 20, "only %lld predictions went through the model's space_to_plane", predicted);
    CHECK(run[0].fallbacks == run[1].fallbacks && run[0].fallbacks == run[2].fallbacks, "the `< 10` branch ran %lld, %lld, %lld times", run[0].fallbacks, run[1].fallbacks, run[2].fallbacks);
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
