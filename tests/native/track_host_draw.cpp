// Stand-alone host program for the recording stage of the track image (gf::record_track and the draw_from snapshot of gf::after_lk, csrc/gf_track_host.hpp): the
// CPU tracker of tests/native/track_host.cpp -- included as it is, its main set aside -- takes frames with SHOW_TRACK on, and after every frame this program
// prints the state before the call, the state after it and the recorded primitive list.  tests/test_track_host_draw.py builds the list those states imply with
// tests/track_draw_ref.py and compares.  No HIP call is made.
//   track_host_draw FILE max_cnt min_dist on_at=K [feedback=1]     SHOW_TRACK goes on before frame K; feedback: removeOutliers / setPrediction between frames
// (That the stages are the oracle's tracker is track_host.cpp's own business; here they only have to run.)
#define main track_host_main
#include "track_host.cpp"
#undef main

static void print_list(const gf::SeqState& s) {
    for (const gfdraw::Prim& p : s.draw_list) printf("prim %d %d %d %d %d %d %d\n", p.ux, p.uy, p.vx, p.vy, (int)p.stroke, (int)p.c0, (int)p.c2);
}

int main(int argc, char** argv) {
    if (argc < 5) { printf("usage: track_host_draw FILE max_cnt min_dist on_at=K [feedback=1]\n"); return 2; }
    Frames F;
    if (!read_frames(argv[1], F)) { printf("cannot read %s\n", argv[1]); return 2; }
    int on_at = 0, with_feedback = 0;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        const std::string key = a.substr(0, a.find('=')), val = a.substr(a.find('=') + 1);
        if (key == "on_at") on_at = atoi(val.c_str());
        else if (key == "feedback") with_feedback = atoi(val.c_str());
        else { printf("unknown option %s\n", a.c_str()); return 2; }
    }
    const gf_tracker_seq_cfg par{atoi(argv[2]), atoi(argv[3]), 1, 0, 603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656, 0, 0, 0, 0};
    CpuSeq c;
    c.create(par, F.w, F.h);
    gf::SeqState& s = c.s;
    std::vector<gf_feature_obs> obs(4096);
    for (int k = 0; k < F.n; k++) {
        if (k == on_at) s.show_track = true;
        printf("frame %d show %d\n", k, s.show_track ? 1 : 0);
        for (size_t i = 0; i < s.ids.size(); i++) printf("before %d %.9g %.9g\n", s.ids[i], (double)s.prev_pts[i].x, (double)s.prev_pts[i].y);
        const int n = c.track(0.0666 * k, F.img(k), nullptr, kNoDepth, obs.data(), (int)obs.size());
        CHECK(n == (int)s.ids.size(), "frame %d: %d observations for %zu features", k, n, s.ids.size());
        if (s.show_track) {   // as book_after_detect does behind after_detect
            CHECK(gf::record_track(s) && s.draw_why.empty(), "frame %d: record_track refused: %s", k, s.draw_why.c_str());
            CHECK(s.draw_have && !s.draw_sent, "frame %d: the list is not marked as new", k);
        } else CHECK(!s.draw_have && s.draw_list.empty() && s.draw_from.empty(), "frame %d: something was recorded with the switch off", k);
        for (size_t i = 0; i < s.ids.size(); i++) printf("after %d %d %.9g %.9g\n", s.ids[i], s.track_cnt[i], (double)s.prev_pts[i].x, (double)s.prev_pts[i].y);
        print_list(s);
        if (with_feedback) {   // removeOutliers on every seventh id, a prediction on its own pixel for every second of the rest: the recorded picture stays
            const std::vector<gfdraw::Prim> kept = s.draw_list;
            std::vector<int> rm, sel; std::vector<double> xyz;
            for (size_t i = 0; i < s.ids.size(); i += 7) rm.push_back(s.ids[i]);
            gf::remove_outliers(s, rm.data(), (int)rm.size());
            for (size_t i = 0; i < s.ids.size(); i += 2) {
                sel.push_back(s.ids[i]);
                xyz.push_back(((double)s.prev_pts[i].x - par.cx) / par.fx * 2.0); xyz.push_back(((double)s.prev_pts[i].y - par.cy) / par.fy * 2.0); xyz.push_back(2.0);
            }
            gf::set_prediction(s, par, sel.data(), xyz.data(), (int)sel.size());
            CHECK(kept.size() == s.draw_list.size() && (kept.empty() || !memcmp(kept.data(), s.draw_list.data(), kept.size() * sizeof(gfdraw::Prim))), "frame %d: the feedback calls changed the recorded list", k);
            printf("removed %zu\n", rm.size());
        }
    }
    {   // a list the builder refuses: no picture, and the reason is kept for the caller
        gf::SeqState bad;
        bad.show_track = true;
        bad.ids = {7}; bad.track_cnt = {1}; bad.prev_pts = {gf::P2f{std::nanf(""), 3.f}};
        CHECK(!gf::record_track(bad) && !bad.draw_have && bad.draw_list.empty() && bad.draw_why.find("not finite") != std::string::npos, "a refused list: '%s'", bad.draw_why.c_str());
        bad.prev_pts = {gf::P2f{4.f, 3.f}};
        CHECK(gf::record_track(bad) && bad.draw_have && bad.draw_list.size() == 1 && bad.draw_why.empty(), "the next good list clears the reason");
    }
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
