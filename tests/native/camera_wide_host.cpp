// Stand-alone host program for the PINHOLE_FULL and SCARAMUZZA models of ground-fusion_amd/csrc/gf_camera_models.hpp and for the PINHOLE_FULL projection of
// csrc/gf_depth_reg.hpp, on the CPU, against tests/golden/camera_models_wide.json.gz.  tests/test_camera_wide_host.py writes the fixture as lines of hex floats,
// builds this file plain and under the address and undefined-behaviour sanitizers and runs both:  camera_wide_host FILE
//   bar B                                                             four times the numpy double route's largest deviation from 60 digits (SCARAMUZZA projection)
//   case NAME MODEL proj[4] dist[8] xi poly[5] inv_poly[20] affine[5]
//   pt U V ray_d[3] un_d[2] px_d[2] HAS_RAY60 ray60[3 x (hi lo)] HAS_PX60 px60[2 x (hi lo)]
// Bars (the issue's): both lifts, their float pairs and PINHOLE_FULL's projection give the BITS of the numpy float64 route wherever that is finite, and are not
// finite where it is not; SCARAMUZZA's projection, which goes through atan2, lies within `bar` x max(1, |pixel|) of the 60-digit value.  The deviation of the
// rays from their 60-digit values is printed, not asserted.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_camera_models.hpp"
#include "../../ground-fusion_amd/csrc/gf_depth_reg.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Point { double u, v, ray_d[3], un_d[2], px_d[2]; int has_ray60, has_px60; double ray60[3][2], px60[2][2]; };
struct Case { std::string name; gf_camera_model_ex m; std::vector<Point> pts; };

static bool same(double got, double want) {   // the bits where `want` is finite (either zero), not finite where it is not
    if (!std::isfinite(want)) return !std::isfinite(got);
    return memcmp(&got, &want, 8) == 0 || (got == 0.0 && want == 0.0 && std::signbit(got) == std::signbit(want));
}
static bool same_f(float got, double want) {
    if (!std::isfinite(want)) return !std::isfinite(got);
    const float w = (float)want;
    return memcmp(&got, &w, 4) == 0;
}
static double err(double got, const double* hilo) { return std::fabs((got - hilo[0]) - hilo[1]); }
static double scale(const double* hilo) { return std::fmax(1.0, std::fabs(hilo[0])); }

static bool read_fixture(const char* path, double& bar, std::vector<Case>& cases) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    static char line[16384];
    while (fgets(line, sizeof line, f)) {
        std::vector<std::string> tok;
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        auto num = [&](size_t i) { return strtod(tok.at(i).c_str(), nullptr); };
        if (tok[0] == "bar") bar = num(1);
        else if (tok[0] == "case") {
            Case c; c.name = tok.at(1);
            memset(&c.m, 0, sizeof c.m);
            c.m.model = atoi(tok.at(2).c_str());
            size_t at = 3;
            for (int i = 0; i < 4; i++) c.m.proj[i] = num(at++);
            for (int i = 0; i < 8; i++) c.m.dist[i] = num(at++);
            c.m.xi = num(at++);
            for (int i = 0; i < 5; i++) c.m.poly[i] = num(at++);
            for (int i = 0; i < 20; i++) c.m.inv_poly[i] = num(at++);
            for (int i = 0; i < 5; i++) c.m.affine[i] = num(at++);
            cases.push_back(c);
        } else if (tok[0] == "pt") {
            Point p{};
            size_t at = 1;
            p.u = num(at++); p.v = num(at++);
            for (int i = 0; i < 3; i++) p.ray_d[i] = num(at++);
            for (int i = 0; i < 2; i++) p.un_d[i] = num(at++);
            for (int i = 0; i < 2; i++) p.px_d[i] = num(at++);
            p.has_ray60 = atoi(tok.at(at++).c_str());
            for (int i = 0; i < 3; i++) { p.ray60[i][0] = num(at++); p.ray60[i][1] = num(at++); }
            p.has_px60 = atoi(tok.at(at++).c_str());
            for (int i = 0; i < 2; i++) { p.px60[i][0] = num(at++); p.px60[i][1] = num(at++); }
            cases.back().pts.push_back(p);
        }
    }
    fclose(f);
    return !cases.empty() && bar > 0;
}

static void check_fixture(double bar, const std::vector<Case>& cases) {
    for (const Case& c : cases) {
        gfcam::Camera cam;
        char msg[320] = "";
        const bool ok = gfcam::prepare(c.m, cam, msg, sizeof msg);
        CHECK(ok, "%s: refused: %s", c.name.c_str(), msg);
        if (!ok) continue;
        double worst_ray60 = 0, worst_px = 0;
        int non_finite = 0;
        for (const Point& p : c.pts) {
            double P[3]; float x, y;
            gfcam::lift_pair(cam, p.u, p.v, P, x, y);
            for (int i = 0; i < 3; i++)
                CHECK(same(P[i], p.ray_d[i]), "%s (%.9g, %.9g): ray[%d] = %a, the double route of the reference gives %a", c.name.c_str(), p.u, p.v, i, P[i], p.ray_d[i]);
            CHECK(same_f(x, p.un_d[0]) && same_f(y, p.un_d[1]), "%s (%.9g, %.9g): pair (%a, %a), the double route of the reference gives (%a, %a)", c.name.c_str(), p.u, p.v,
                  (double)x, (double)y, p.un_d[0], p.un_d[1]);
            non_finite += !(std::isfinite(P[0]) && std::isfinite(P[1]) && std::isfinite(P[2]));
            if (p.has_ray60) for (int i = 0; i < 3; i++) worst_ray60 = std::fmax(worst_ray60, err(P[i], p.ray60[i]) / scale(p.ray60[i]));
            double u, v;
            gfcam::space_to_plane(cam, p.ray_d, u, v);   // of the fixture's doubles: the same input as the numpy route had
            if (c.m.model == GF_CAMERA_PINHOLE_FULL) {
                CHECK(same(u, p.px_d[0]) && same(v, p.px_d[1]), "%s (%.9g, %.9g): projection (%a, %a), the double route of the reference gives (%a, %a)", c.name.c_str(), p.u, p.v,
                      u, v, p.px_d[0], p.px_d[1]);
            } else {
                if (!std::isfinite(p.px_d[0]) || !std::isfinite(p.px_d[1])) CHECK(!std::isfinite(u) || !std::isfinite(v), "%s (%.9g, %.9g): a finite projection where the reference has none", c.name.c_str(), p.u, p.v);
                if (p.has_px60) {
                    const double got[2] = {u, v};
                    for (int i = 0; i < 2; i++) {
                        const double e = err(got[i], p.px60[i]) / scale(p.px60[i]);
                        worst_px = std::fmax(worst_px, e);
                        CHECK(e <= bar, "%s (%.9g, %.9g): projection[%d] = %.17g, 60 digits give %.17g: off by %.3g of the scale, bar %.3g", c.name.c_str(), p.u, p.v, i, got[i], p.px60[i][0], e, bar);
                    }
                }
            }
        }
        printf("%-20s %zu points, %d with a non-finite ray: the bits of the double route; rays within %.3g of 60 digits", c.name.c_str(), c.pts.size(), non_finite, worst_ray60);
        if (c.m.model == GF_CAMERA_SCARAMUZZA) printf("; projection within %.3g (bar %.3g)", worst_px, bar);
        printf("\n");
        if (c.m.model == GF_CAMERA_SCARAMUZZA) {   // a ray on the axis: norm == 0, 1 / 0, 0 * inf -- non-finite, as in the reference
            const double axis[3] = {0.0, 0.0, 1.0};
            double u, v;
            gfcam::space_to_plane(cam, axis, u, v);
            CHECK(!std::isfinite(u) && !std::isfinite(v), "%s: a ray on the axis projects to (%g, %g); the reference's 1 / norm makes it non-finite", c.name.c_str(), u, v);
        }
    }
}

// PINHOLE_FULL with all distortion zero and PINHOLE with all distortion zero are both (1 / f) u - c / f: the same bits
static void check_identity(const std::vector<Case>& cases) {
    for (const Case& c : cases) {
        if (c.name != "full_zero") continue;
        gf_camera_model pm{};
        pm.model = GF_CAMERA_PINHOLE;
        for (int i = 0; i < 4; i++) pm.proj[i] = c.m.proj[i];
        gfcam::Camera full, pin, wide_pin;
        char msg[320];
        CHECK(gfcam::prepare(c.m, full, msg, sizeof msg) && gfcam::prepare(pm, pin, msg, sizeof msg) && gfcam::prepare(gfcam::widen(pm), wide_pin, msg, sizeof msg), "refused: %s", msg);
        CHECK(memcmp(&pin, &wide_pin, sizeof pin) == 0, "a PINHOLE through the wide checker is not the camera the 80-byte checker makes");
        for (const Point& p : c.pts) {
            if (!std::isfinite(p.u) || !std::isfinite(p.v)) continue;
            double P[3], Q[3]; float a, b, x, y;
            gfcam::lift_pair(full, p.u, p.v, P, a, b);
            gfcam::lift_pair(pin, p.u, p.v, Q, x, y);
            CHECK(memcmp(P, Q, sizeof P) == 0 && memcmp(&a, &x, 4) == 0 && memcmp(&b, &y, 4) == 0, "full_zero (%.9g, %.9g): PINHOLE_FULL and PINHOLE differ in their bits", p.u, p.v);
            double u0, v0, u1, v1;
            const double R[3] = {0.3, -0.2, 1.7};
            gfcam::space_to_plane(full, R, u0, v0);
            gfcam::space_to_plane(pin, R, u1, v1);
            CHECK(std::fabs(u0 - u1) <= 1e-12 * std::fabs(u1) && std::fabs(v0 - v1) <= 1e-12 * std::fabs(v1), "full_zero: the projections differ: (%.17g, %.17g) and (%.17g, %.17g)", u0, v0, u1, v1);
        }
    }
}

static void refused(const gf_camera_model_ex& m, const char* names) {
    gfcam::Camera cam;
    char msg[320] = "";
    const bool ok = gfcam::prepare(m, cam, msg, sizeof msg);
    CHECK(!ok, "a model that must be refused for its %s was accepted", names);
    CHECK(strstr(msg, names) != nullptr, "the refusal does not name `%s`: %s", names, msg);
}
static void accepted(const gf_camera_model_ex& m, const char* what) {
    gfcam::Camera cam;
    char msg[320] = "";
    CHECK(gfcam::prepare(m, cam, msg, sizeof msg), "%s was refused: %s", what, msg);
}

static void check_refusals(const std::vector<Case>& cases) {
    const double nan = std::nan(""), inf = INFINITY;
    gf_camera_model_ex full{}, sca{};
    for (const Case& c : cases) { if (c.name == "full_kinect8") full = c.m; if (c.name == "sca_affine") sca = c.m; }
    accepted(full, "a valid PINHOLE_FULL camera"); accepted(sca, "a valid SCARAMUZZA camera");
    gf_camera_model_ex m = full;
    m.model = 5; refused(m, "model");
    m = full; m.model = -1; refused(m, "model");
    m = full; m.reserved = 1; refused(m, "reserved");
    m = sca; m.reserved = -3; refused(m, "reserved");
    static const char* const pn[4] = {"fx", "fy", "cx", "cy"};
    static const char* const dn[8] = {"k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"};
    for (int i = 0; i < 4; i++) { m = full; m.proj[i] = i & 1 ? inf : nan; refused(m, pn[i]); }
    for (int i = 0; i < 8; i++) { m = full; m.dist[i] = i & 1 ? -inf : nan; refused(m, dn[i]); }
    m = full; m.proj[0] = 0.0; refused(m, "fx");
    m = full; m.proj[1] = -504.75; refused(m, "fy");
    m = full; m.xi = nan; m.poly[0] = nan; m.inv_poly[19] = inf; m.affine[0] = nan; accepted(m, "a PINHOLE_FULL camera with non-finite fields it does not use");
    char name[32];
    for (int i = 0; i < 5; i++) { m = sca; m.poly[i] = nan; snprintf(name, sizeof name, "poly[%d]", i); refused(m, name); }
    for (int i = 0; i < 20; i++) { m = sca; m.inv_poly[i] = inf; snprintf(name, sizeof name, "inv_poly[%d]", i); refused(m, name); }
    static const char* const an[5] = {"ac", "ad", "ae", "cx", "cy"};
    for (int i = 0; i < 5; i++) { m = sca; m.affine[i] = nan; refused(m, an[i]); }
    m = sca; m.affine[0] = 0.5; m.affine[1] = 2.0; m.affine[2] = 0.25; refused(m, "ac - ad * ae");
    m = sca; m.affine[0] = 0.0; m.affine[1] = 0.0; refused(m, "ac - ad * ae");
    m = sca; for (int i = 0; i < 4; i++) m.proj[i] = nan; for (int i = 0; i < 8; i++) m.dist[i] = inf; m.xi = nan; accepted(m, "a SCARAMUZZA camera with non-finite fields it does not use");
    // models 0-2 through the wide checker: what the 80-byte checker refuses, and nothing for the fields gf_camera_model does not have
    gf_camera_model_ex mei{};
    mei.model = GF_CAMERA_MEI; mei.proj[0] = 500; mei.proj[1] = 500; mei.proj[2] = 320; mei.proj[3] = 240; mei.dist[0] = -0.1; mei.xi = 1.2;
    accepted(mei, "a valid MEI camera in the wide struct");
    m = mei; m.dist[4] = nan; m.dist[7] = inf; m.poly[2] = nan; m.affine[4] = nan; accepted(m, "a MEI camera with non-finite fields it does not use");
    m = mei; m.xi = -0.01; refused(m, "xi");
    m = mei; m.proj[0] = 0.0; refused(m, "gamma1");
    m = mei; m.dist[3] = nan; refused(m, "p2");
    m = mei; m.model = GF_CAMERA_KANNALA_BRANDT; m.dist[0] = 0.0; m.dist[1] = 0.0; m.dist[3] = 1e-4; refused(m, "k5");
    m = mei; m.model = GF_CAMERA_PINHOLE; m.proj[1] = -1.0; refused(m, "fy");
    // the 80-byte checker still refuses models 3 and 4, naming the model
    gf_camera_model old{};
    old.proj[0] = old.proj[1] = 500; old.proj[2] = 320; old.proj[3] = 240;
    for (int model = 3; model <= 4; model++) {
        old.model = model;
        gfcam::Camera cam;
        char msg[320] = "";
        CHECK(!gfcam::prepare(old, cam, msg, sizeof msg) && strstr(msg, "model"), "the 80-byte checker took model %d, or its refusal does not name the model: %s", model, msg);
    }
}

// a fixed bound on every loop: these return, whatever they return
static void check_termination(const std::vector<Case>& cases) {
    const double bad[] = {std::nan(""), INFINITY, -INFINITY, 1e30, -1e30, 1e300, 5e-324, 0.0};
    long long calls = 0;
    for (const Case& c : cases) {
        gfcam::Camera cam;
        char msg[320];
        if (!gfcam::prepare(c.m, cam, msg, sizeof msg)) continue;
        for (double u : bad) for (double v : bad) { double P[3]; float x, y; gfcam::lift_pair(cam, u, v, P, x, y); double a, b; gfcam::space_to_plane(cam, P, a, b); calls++; }
    }
    printf("termination: %lld lifts and projections of non-finite and huge coordinates returned\n", calls);
}

// ---- gfdreg::register_frame with a PINHOLE_FULL colour camera against a brute force that restates the definition: every colour pixel asks every depth pixel
struct BruteMap { bool front; double u, v, Pz; };
static BruteMap brute_map(const gf_depth_reg& r, const gf_camera_model_ex& c, double px, double py, double z) {
    const double X = (px - r.cx) / r.fx * z, Y = (py - r.cy) / r.fy * z;
    const double Px = ((r.R[0] * X + r.R[1] * Y) + r.R[2] * z) + r.T[0], Py = ((r.R[3] * X + r.R[4] * Y) + r.R[5] * z) + r.T[1], Pz = ((r.R[6] * X + r.R[7] * Y) + r.R[8] * z) + r.T[2];
    BruteMap m{Pz > 0.0, 0, 0, Pz};
    if (!m.front) return m;
    const double x = Px / Pz, y = Py / Pz;                                          // PinholeFullCamera.cc:628
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4], k4 = c.dist[5], k5 = c.dist[6], k6 = c.dist[7];
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2, a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;   // :770-775
    const double cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6, icdist2 = 1. / (1 + k4 * r2 + k5 * r4 + k6 * r6);                 // :776-777
    const double dx = x * cdist * icdist2 + p1 * a1 + p2 * a2 - x, dy = y * cdist * icdist2 + p1 * a3 + p2 * a1 - y;         // :779-780
    m.u = c.proj[0] * (x + dx) + c.proj[2]; m.v = c.proj[1] * (y + dy) + c.proj[3];                                         // :639, :643-644
    return m;
}
static void depth_case(const char* name, const gf_depth_reg& r, const gf_camera_model_ex& c, int wc, int hc, unsigned seed) {
    char msg[320];
    CHECK(gfdreg::check(r, msg, sizeof msg), "%s: registration refused: %s", name, msg);
    const int wd = r.width, hd = r.height;
    std::vector<uint16_t> src((size_t)wd * hd), dst((size_t)wc * hc, 0xABCD), want((size_t)wc * hc, 0);
    for (auto& d : src) { seed = seed * 1664525u + 1013904223u; d = (seed >> 28) == 0 ? 0 : (uint16_t)(600 + (seed >> 8) % 3000); }   // 0.6 .. 3.6 m, one in sixteen without a measurement
    std::vector<uint32_t> z(gfdreg::zwords_of(wc, hc), gfdreg::kUntouched);
    long long census[gfdreg::kWrites + 1] = {};
    const gfdreg::Params p = gfdreg::params_of(r, c.proj, c.dist, c.dist + 4);
    gfdreg::register_frame(p, src.data(), (size_t)wd * 2, wd, hd, dst.data(), (size_t)wc * 2, wc, hc, z.data(), census);
    for (uint32_t w : z) if (w != gfdreg::kUntouched) { CHECK(false, "%s: the z-buffer is not left primed", name); break; }
    long long covered = 0;
    for (int v = 0; v < hc; v++)
        for (int u = 0; u < wc; u++) {
            uint32_t best = 0;
            for (int y = 0; y < hd; y++)
                for (int x = 0; x < wd; x++) {
                    const uint16_t d = src[(size_t)y * wd + x];
                    if (!d) continue;
                    const double zz = (double)d * r.scale;
                    const BruteMap a = brute_map(r, c, x - 0.5, y - 0.5, zz), b = brute_map(r, c, x + 0.5, y + 0.5, zz), m = brute_map(r, c, x, y, zz);
                    if (!a.front || !b.front || !m.front) continue;
                    if (!std::isfinite(a.u) || !std::isfinite(a.v) || !std::isfinite(b.u) || !std::isfinite(b.v) || !std::isfinite(m.u) || !std::isfinite(m.v)) continue;
                    const double val = std::floor(m.Pz / 0.001 + 0.5);
                    if (!(val >= 1.0 && val <= 65535.0)) continue;
                    const double x0 = std::ceil(std::fmin(a.u, b.u)), x1 = std::ceil(std::fmax(a.u, b.u)) - 1.0, y0 = std::ceil(std::fmin(a.v, b.v)), y1 = std::ceil(std::fmax(a.v, b.v)) - 1.0;
                    if (x1 - x0 + 1.0 > 8.0 || y1 - y0 + 1.0 > 8.0) continue;
                    if ((double)u < x0 || (double)u > x1 || (double)v < y0 || (double)v > y1) continue;
                    if (!best || (uint32_t)val < best) best = (uint32_t)val;
                }
            want[(size_t)v * wc + u] = (uint16_t)best;
            covered += best != 0;
        }
    long long differ = 0;
    for (size_t i = 0; i < want.size(); i++) differ += want[i] != dst[i];
    CHECK(differ == 0, "%s: %lld of %zu colour pixels differ from the brute force", name, differ, want.size());
    CHECK(covered * 4 >= (long long)want.size() && census[gfdreg::kWrites] > 0, "%s: only %lld of %zu colour pixels are covered: the case shows nothing", name, covered, want.size());
    printf("depth registration %-14s %d x %d -> %d x %d: %lld colour pixels covered, %lld depth pixels write, the brute force agrees\n", name, wd, hd, wc, hc, covered, census[gfdreg::kWrites]);
}
static void check_depth_reg(const std::vector<Case>& cases) {
    gf_camera_model_ex full{};
    for (const Case& c : cases) if (c.name == "full_kinect8") full = c.m;
    // the colour camera at the sizes of the two cases: the fixture's coefficients, the intrinsics scaled to the frame
    gf_camera_model_ex a = full, b = full;
    a.proj[0] = 19.0; a.proj[1] = 19.5; a.proj[2] = 11.75; a.proj[3] = 8.25;
    b.proj[0] = 25.5; b.proj[1] = 25.0; b.proj[2] = 15.25; b.proj[3] = 11.5;
    gf_depth_reg ra{}, rb{};
    ra.width = 24; ra.height = 16; ra.fx = 19.0; ra.fy = 19.5; ra.cx = 11.75; ra.cy = 8.25; ra.scale = 0.001;
    ra.R[0] = ra.R[4] = ra.R[8] = 1.0;
    depth_case("same_pose", ra, a, 24, 16, 1u);
    rb.width = 20; rb.height = 14; rb.fx = 17.0; rb.fy = 17.25; rb.cx = 9.5; rb.cy = 6.75; rb.scale = 0.00025;
    const double t = 0.03, ct = std::cos(t), st = std::sin(t);   // a rotation about y and a baseline: the footprints grow to several colour pixels
    rb.R[0] = ct; rb.R[2] = st; rb.R[4] = 1.0; rb.R[6] = -st; rb.R[8] = ct;
    rb.T[0] = 0.015; rb.T[1] = -0.002; rb.T[2] = 0.001;
    depth_case("pose_upscaled", rb, b, 31, 23, 7u);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: camera_wide_host FILE\n"); return 2; }
    double bar = 0;
    std::vector<Case> cases;
    if (!read_fixture(argv[1], bar, cases)) { printf("cannot read %s\n", argv[1]); return 2; }
    check_fixture(bar, cases);
    check_identity(cases);
    check_refusals(cases);
    check_termination(cases);
    check_depth_reg(cases);
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
