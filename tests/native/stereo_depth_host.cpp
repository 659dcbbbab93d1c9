// stereo_depth_host.cpp — csrc/gf_stereo_depth.hpp on the CPU, stand-alone: the header the kernel, the tracker's host stage and the building blocks compile, with
// a main of its own, so that tests/test_stereo_depth_host.py can build it plain and under the address and undefined-behaviour sanitizers and hold it bit for bit
// against the numpy restatement of tests/stereo_depth_ref.py, through files.
//   stereo_depth_host run CASE OUT   CASE: three lines -- the left camera, the right camera (model, proj[4], dist[8], xi, poly[5], inv_poly[20], affine[5]) and the
//                                    configuration (enable, right_obs, R[9], t[3], min_parallax, max_epipolar, min_depth, max_depth) -- then n and n lines
//                                    "ul vl ur vr status"; every real number as strtod reads it (hex floats, nan).  OUT: n lines "depth_mm why"; the census
//                                    by reason goes to stdout.
//   stereo_depth_host check          configurations on stdin, one per line as above; per line "ok" or the message of gfsd::check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_stereo_depth.hpp"

static bool real(FILE* f, double& v) {
    char tok[128];
    if (fscanf(f, "%127s", tok) != 1) return false;
    char* end = nullptr;
    v = strtod(tok, &end);
    return end && *end == 0;
}
static bool whole(FILE* f, int& v) { return fscanf(f, "%d", &v) == 1; }

static bool read_camera(FILE* f, gf_camera_model_ex& m) {
    m = gf_camera_model_ex{};
    if (!whole(f, m.model)) return false;
    for (double& v : m.proj) if (!real(f, v)) return false;
    for (double& v : m.dist) if (!real(f, v)) return false;
    if (!real(f, m.xi)) return false;
    for (double& v : m.poly) if (!real(f, v)) return false;
    for (double& v : m.inv_poly) if (!real(f, v)) return false;
    for (double& v : m.affine) if (!real(f, v)) return false;
    return true;
}
static bool read_cfg(FILE* f, gf_stereo_depth_cfg& c) {
    c = gf_stereo_depth_cfg{};
    if (!whole(f, c.enable) || !whole(f, c.right_obs)) return false;
    for (double& v : c.R) if (!real(f, v)) return false;
    for (double& v : c.t) if (!real(f, v)) return false;
    return real(f, c.min_parallax) && real(f, c.max_epipolar) && real(f, c.min_depth) && real(f, c.max_depth);
}

static int run(const char* case_path, const char* out_path) {
    FILE* f = fopen(case_path, "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", case_path); return 2; }
    gf_camera_model_ex lm, rm; gf_stereo_depth_cfg cfg; int n = 0;
    if (!read_camera(f, lm) || !read_camera(f, rm) || !read_cfg(f, cfg) || !whole(f, n) || n < 0) { fprintf(stderr, "%s: malformed head\n", case_path); return 2; }
    char msg[320];
    gfcam::Camera left, right;
    if (!gfcam::prepare(lm, left, msg, sizeof msg)) { fprintf(stderr, "left camera: %s\n", msg); return 3; }
    if (!gfcam::prepare(rm, right, msg, sizeof msg)) { fprintf(stderr, "right camera: %s\n", msg); return 3; }
    if (!gfsd::check(cfg, msg, sizeof msg)) { fprintf(stderr, "configuration: %s\n", msg); return 3; }
    const gfsd::Rig rig = gfsd::rig_of(cfg);
    std::vector<gfsd::Depth> out((size_t)n);
    long long census[gfsd::kReasons] = {0};
    for (int i = 0; i < n; i++) {
        double p[4]; int st = 0;
        for (double& v : p) if (!real(f, v)) { fprintf(stderr, "%s: malformed point %d\n", case_path, i); return 2; }
        if (!whole(f, st)) { fprintf(stderr, "%s: malformed point %d\n", case_path, i); return 2; }
        out[(size_t)i] = gfsd::depth_of(left, right, rig, (float)p[0], (float)p[1], (float)p[2], (float)p[3], (uint8_t)st);
        census[out[(size_t)i].why]++;
    }
    fclose(f);
    FILE* o = fopen(out_path, "w");
    if (!o) { fprintf(stderr, "cannot write %s\n", out_path); return 2; }
    for (const gfsd::Depth& d : out) fprintf(o, "%u %u\n", (unsigned)d.mm, (unsigned)d.why);
    fclose(o);
    printf("census");
    for (int k = 0; k < gfsd::kReasons; k++) printf(" %lld", census[k]);
    printf("\n");
    return 0;
}

static int check() {
    for (;;) {
        gf_stereo_depth_cfg cfg;
        if (!read_cfg(stdin, cfg)) break;
        char msg[320];
        puts(gfsd::check(cfg, msg, sizeof msg) ? "ok" : msg);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    fprintf(stderr, "usage: %s run CASE OUT | check\n", argv[0]);
    return 2;
}
