// A frame size per sequence on the CPU tracker of tests/native/track_host.cpp (included below, its main renamed): the stage functions of gf_track_host.hpp take a
// sequence's own width and height, as track_core hands them over once a sequence has a size of its own (gf_tracker_set_seq_size; `row`, `col` of
// feature_tracker.cpp:108-109).  Two sequences advance in turn as a call walks its list, a small one and a 640-wide neighbour, each against the oracle's Tracker on
// frames of its own size: ids, observations, n_out and state bit for bit after every frame.  Then one point at x = 100: out of border for the small sequence,
// whose frame ends at its own width, and kept by the neighbour.  Built by tests/test_seq_size_track_host.py under the address and undefined-behaviour sanitizers:
//   seq_size_track_host SMALL_FILE small_max_cnt small_min_dist LARGE_FILE large_max_cnt large_min_dist
#define main track_host_main
#include "track_host.cpp"
#undef main

// the sequence with nothing but one tracked point, id 0, at (x, y) of its first frame, taking that frame again; true if the point is still tracked afterwards
static bool keeps_point(const Frames& F, gf_tracker_seq_cfg par, float x, float y) {
    CpuSeq c;
    par.depth_cam = 0;   // no depth image is handed in: with a depth camera the frame would be reported empty
    c.create(par, F.w, F.h);
    c.prev_img.assign(F.img(0), F.img(0) + (size_t)F.w * F.h);
    c.s.prev_pts = {gf::P2f{x, y}}; c.s.ids = {0}; c.s.track_cnt = {1}; c.s.n_id = 1; c.s.started = true; c.s.slot = 0;
    std::vector<gf_feature_obs> obs(4096);
    const int n = c.track(1.0, F.img(0), nullptr, kNoDepth, obs.data(), 4096);
    CHECK(n > 0, "the %d x %d sequence reported nothing", F.w, F.h);
    for (size_t i = 0; i < c.s.ids.size(); i++) {
        CHECK(c.s.prev_pts[i].x >= 0 && c.s.prev_pts[i].x < F.w && c.s.prev_pts[i].y >= 0 && c.s.prev_pts[i].y < F.h, "a feature of the %d x %d sequence lies at (%g, %g)", F.w, F.h,
              c.s.prev_pts[i].x, c.s.prev_pts[i].y);
        if (c.s.ids[i] == 0) return true;
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 7) { printf("usage: seq_size_track_host SMALL_FILE max_cnt min_dist LARGE_FILE max_cnt min_dist\n"); return 2; }
    Frames S, L;
    if (!read_frames(argv[1], S) || !read_frames(argv[4], L)) { printf("cannot read the frames\n"); return 2; }
    CHECK(S.w < 100 && L.w > 101 && S.h <= L.h, "the small frames are %d x %d, the large ones %d x %d", S.w, S.h, L.w, L.h);
    Options o;
    o.flow_back = 1; o.depth_cam = 1; o.depth = kHostDepth;   // the host samples each sequence's depth image with that image's own row step
    const gf_tracker_seq_cfg small{atoi(argv[2]), atoi(argv[3]), 1, 1, 603.95556640625, 603.1257934570312, 324.0858154296875, 232.72303771972656, 0, 0, 0, 0};
    gf_tracker_seq_cfg large = small;
    large.max_cnt = atoi(argv[5]); large.min_dist = atoi(argv[6]);
    Runner a(S, o, small, "small sequence", 0.0), b(L, o, large, "large sequence", 100.0);
    for (int k = 0; k < S.n && k < L.n; k++) { a.step(k); b.step(k); }
    printf("small: fewest ids carried over %d of %d; large: %d of %d\n", a.fewest, small.max_cnt, b.fewest, large.max_cnt);
    CHECK(a.fewest >= 1 && 3 * b.fewest >= large.max_cnt, "the sequences are not alive");
    for (size_t i = 0; i < a.c.s.prev_pts.size(); i++) CHECK(a.c.s.prev_pts[i].x < S.w && a.c.s.prev_pts[i].y < S.h, "the small sequence holds a point outside its frame");
    const bool in_small = keeps_point(S, small, 100.f, 20.f), in_large = keeps_point(L, large, 100.f, 20.f);
    printf("the point at x = 100: %s by the %d-wide sequence, %s by the %d-wide one\n", in_small ? "kept" : "dropped", S.w, in_large ? "kept" : "dropped", L.w);
    CHECK(!in_small, "a point at x = 100 survived in a frame %d wide", S.w);
    CHECK(in_large, "the %d-wide neighbour lost the point at x = 100", L.w);
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
