// rejectWithF in the host stage (after_lk, csrc/gf_track_host.hpp) on the CPU tracker of tests/native/track_host.cpp (included below, its main renamed).  Two
// sequences take the same frames through the same stages around the oracle's LK and corner primitives:
//   on      the switch on: after_lk runs gfrf::reject at the reference's place (feature_tracker.cpp:170-186), lifting through gfcam::lift
//   edited  the switch off, fed a status row edited between LK and after_lk: the virtual pixels restated here with the pinhole's own lift_projective, the edit by
//           gfrf::reject, and every edit written to DUMP_FILE, where tests/test_reject_f_track_host.py holds it to the numpy restatement
// After every frame observations (all eight fields), ids and state must be equal bit for bit.  Before frame 3 both get a prediction that fails, so the stage also
// runs behind the three-level fallback.  Built under the address and undefined-behaviour sanitizers:
//   reject_f_track_host FRAMES_FILE max_cnt min_dist f_threshold seed DUMP_FILE
// DUMP_FILE: per edit int32 n, uint32 frame seed, double threshold, n x 4 floats, n status bytes before, n after, 4 int32 result.
#define main track_host_main
#include "track_host.cpp"
#undef main

struct RfSeq : CpuSeq {
    long long rejected = 0, runs = 0;
    // CpuSeq::track with the stage: rf_on -> inside after_lk; dump -> the status row edited ahead of an after_lk that has the switch off
    int track_rf(double t, const uint8_t* img, bool rf_on, double thr, uint32_t seed, FILE* dump, gf_feature_obs* out, int cap_out) {
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
            lk(img, nullptr, n, pred ? 1 : 3, pred);
            if (gf::prediction_failed(s, fwd_status.data(), n)) { fallbacks++; lk(img, nullptr, n, 3, false, true); }
        }
        const uint32_t fseed = gfrf::frame_seed(seed, (uint32_t)s.frames);
        gf::RejectFHost rf{};
        if (rf_on) {
            CHECK(gfcam::prepare(gfcam::pinhole_of(par), rf.cam, msg, sizeof msg), "the pinhole was refused: %s", msg);
            rf.status = status.data(); rf.f_threshold = thr; rf.focal = gfrf::kFocal; rf.seed = fseed;
        } else if (dump && n >= gfrf::kSample) {
            std::vector<gfrf::Cand> pairs(n), cand(n);
            std::vector<int> row_of(n);
            for (int i = 0; i < n; i++) {   // :722-729 with the pinhole's liftProjective, whose z is 1
                double X, Y;
                gf::lift_projective(par, (double)cur_row[i].x, (double)cur_row[i].y, X, Y);
                pairs[i].bx = (float)(460.0 * X / 1.0 + w / 2.0); pairs[i].by = (float)(460.0 * Y / 1.0 + h / 2.0);
                gf::lift_projective(par, (double)s.prev_pts[i].x, (double)s.prev_pts[i].y, X, Y);
                pairs[i].ax = (float)(460.0 * X / 1.0 + w / 2.0); pairs[i].ay = (float)(460.0 * Y / 1.0 + h / 2.0);
            }
            const std::vector<uint8_t> before(status.begin(), status.begin() + n);
            const gfrf::Result r = gfrf::reject(pairs.data(), status.data(), n, thr, fseed, cand.data(), row_of.data());
            const int32_t nn = n, res[4] = {r.m, r.rejected, r.winner, r.inliers};
            fwrite(&nn, 4, 1, dump); fwrite(&fseed, 4, 1, dump); fwrite(&thr, 8, 1, dump); fwrite(pairs.data(), 16, n, dump);
            fwrite(before.data(), 1, n, dump); fwrite(status.data(), 1, n, dump); fwrite(res, 4, 4, dump);
            rejected += r.rejected; runs++;
        }
        int nc = 0, want = 0;
        const gf::LkRows lr{cur_row.data(), status.data(), nullptr, counters.data(), nullptr, w};
        const gf::LkTally tally = gf::after_lk(s, par, w, h, T, nullptr, lr, centers.data(), &nc, &want, nullptr, 0, false, rf_on ? &rf : nullptr);
        if (rf_on && rf.ran) { rejected += rf.result.rejected; runs++; }
        int alive = 0;
        for (int i = 0; has && i < n; i++) alive += status[i];
        CHECK(tally.tracked == alive && tally.points == (has ? n : 0), "after_lk: %lld tracked of %lld, the status row keeps %d of %d", tally.tracked, tally.points, alive, n);
        int out_n = 0;
        if (want > 0) {
            mask.assign((size_t)w * h, 255);
            for (int k = 0; k < nc; k++) gfo_fill_circle(mask.data(), w, h, centers[k].x, centers[k].y, par.min_dist, 0);
            std::vector<float> corners(2 * (size_t)want);
            out_n = gfo_good_features(img, w, h, corners.data(), want, 0.01, (double)par.min_dist, mask.data());
            for (int i = 0; i < out_n; i++) { out_pts[i] = {corners[2 * i], corners[2 * i + 1]}; out_depth[i] = 0; }
        }
        const gf::DetectRows dr{out_pts.data(), out_depth.data(), out_n, nullptr, w};
        const gf::Packed p = gf::after_detect(s, par, dr, false, out, cap_out);
        CHECK(p.overflow < 0, "%d features overflow the output", p.overflow);
        prev_img.assign(img, img + (size_t)w * h);
        return p.written;
    }
};

// a prediction far outside the frame for every tracked point: fewer than 10 forward successes, the `< 10` branch
static void bad_prediction(RfSeq& c) {
    std::vector<int> ids = c.s.ids;
    std::vector<double> xyz;
    for (size_t i = 0; i < ids.size(); i++) {
        const double u = c.s.prev_pts[i].x + 400.0, v = c.s.prev_pts[i].y + 400.0;
        xyz.push_back((u - c.par.cx) / c.par.fx * 2.0); xyz.push_back((v - c.par.cy) / c.par.fy * 2.0); xyz.push_back(2.0);
    }
    gf::set_prediction(c.s, c.par, ids.data(), xyz.data(), (int)ids.size());
}

int main(int argc, char** argv) {
    if (argc != 7) { printf("usage: reject_f_track_host FRAMES_FILE max_cnt min_dist f_threshold seed DUMP_FILE\n"); return 2; }
    Frames F;
    if (!read_frames(argv[1], F)) { printf("cannot read %s\n", argv[1]); return 2; }
    FILE* dump = fopen(argv[6], "wb");
    if (!dump) { printf("cannot write %s\n", argv[6]); return 2; }
    const double thr = atof(argv[4]);
    const uint32_t seed = (uint32_t)strtoul(argv[5], nullptr, 10);
    // the camera of a 160 x 120 stream: wt_cam's pinhole scaled by four, with a little distortion so that the lift iterates
    const gf_tracker_seq_cfg par{atoi(argv[2]), atoi(argv[3]), 1, 0, 150.98889160156250, 150.78144836425781, 81.021453857421875, 58.180759429931641, 0.05, -0.02, 0.001, -0.002};
    RfSeq on, edited;
    on.create(par, F.w, F.h); edited.create(par, F.w, F.h);
    const int cap = 4096;
    std::vector<gf_feature_obs> a(cap), b(cap);
    for (int k = 0; k < F.n; k++) {
        if (k == 3) { bad_prediction(on); bad_prediction(edited); }
        const double t = 0.0666 * k;
        const int na = on.track_rf(t, F.img(k), true, thr, seed, nullptr, a.data(), cap);
        const int nb = edited.track_rf(t, F.img(k), false, thr, seed, dump, b.data(), cap);
        CHECK(na == nb, "frame %d: n_out %d with the stage, %d with the edited status", k, na, nb);
        for (int i = 0; i < na && i < nb; i++)
            CHECK(a[i].id == b[i].id && a[i].camera_id == b[i].camera_id && memcmp(a[i].v, b[i].v, sizeof a[i].v) == 0, "frame %d: observation %d differs", k, i);
        CHECK(on.s.ids == edited.s.ids && on.s.track_cnt == edited.s.track_cnt && on.s.prev_pts.size() == edited.s.prev_pts.size() &&
              memcmp(on.s.prev_pts.data(), edited.s.prev_pts.data(), on.s.prev_pts.size() * sizeof(gf::P2f)) == 0, "frame %d: the state differs", k);
        CHECK(on.rejected == edited.rejected && on.runs == edited.runs, "frame %d: %lld rejected in %lld runs with the stage, %lld in %lld edits", k, on.rejected, on.runs, edited.rejected, edited.runs);
        printf("frame %d: %d features, %lld rejected so far\n", k, na, on.rejected);
    }
    fclose(dump);
    printf("rejected %lld in %lld runs, %lld fallbacks\n", on.rejected, on.runs, on.fallbacks);
    CHECK(on.rejected > 0, "the stream has no rejection");
    CHECK(on.fallbacks >= 1 && on.fallbacks == edited.fallbacks, "the `< 10` branch was never taken");
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
