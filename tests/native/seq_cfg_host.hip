// Stand-alone host program for ground-fusion_amd/csrc/gf_seq_cfg.hpp: the limits gf_tracker_set_seq_cfg checks and the table of setMask's circle that a
// sequence with its own min_dist gets.  No HIP call is made; tests/test_seq_cfg_host.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../ground-fusion_amd/csrc/gf_seq_cfg.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static gf_tracker_cfg handle_cfg() {
    gf_tracker_cfg c{};
    c.width = 640; c.height = 480; c.batch = 4; c.max_cnt = 500; c.min_dist = 12; c.flow_back = 1; c.depth_cam = 1;
    c.fx = 603.9; c.fy = 603.1; c.cx = 324.0; c.cy = 232.7; c.k1 = 0.1; c.k2 = -0.2; c.p1 = 0.001; c.p2 = -0.002;
    return c;
}

static void disk_tables() {
    for (int r = 0; r <= gf::kMaxRadius; r++) {
        struct { char before[64]; gf::DiskTable T; char after[64]; } g;
        memset(&g, 0x5a, sizeof g);
        gf::make_disk_table(r, g.T);
        const gf::DiskTable& T = g.T;
        bool guard = true;
        for (int i = 0; i < 64; i++) guard = guard && g.before[i] == 0x5a && g.after[i] == 0x5a;
        CHECK(guard, "radius %d: written outside the table", r);
        CHECK(T.radius == r && T.hw[0] == r, "radius %d: hw[0] = %d", r, T.hw[0]);
        for (int i = 0; i <= gf::kMaxRadius; i++) {
            if (i > r) { CHECK(T.hw[i] == -1, "radius %d: hw[%d] = %d past the radius", r, i, T.hw[i]); continue; }
            CHECK(T.hw[i] >= 0 && T.hw[i] <= r, "radius %d: hw[%d] = %d", r, i, T.hw[i]);
            if (i > 0) CHECK(T.hw[i] <= T.hw[i - 1], "radius %d: not monotone at %d", r, i);
            CHECK(std::fabs((double)T.hw[i] - std::sqrt((double)r * r - (double)i * i)) <= 1.0, "radius %d: hw[%d] = %d is no circle", r, i, T.hw[i]);
            // what the detector relies on: |dx| <= hw[|dy|]  <=>  |dy| <= hw[|dx|]
            for (int j = 0; j <= r; j++) CHECK((j <= T.hw[i]) == (i <= T.hw[j]), "radius %d: not symmetric at (%d, %d)", r, i, j);
        }
    }
    printf("disk tables 0 .. %d: ok\n", gf::kMaxRadius);
}

static void limits() {
    const gf_tracker_cfg cap = handle_cfg();
    const gf_tracker_seq_cfg own = gf::gfseq::of_handle(cap);
    char msg[256] = "";
    CHECK(own.max_cnt == 500 && own.min_dist == 12 && own.flow_back == 1 && own.depth_cam == 1 && own.fx == cap.fx && own.fy == cap.fy && own.cx == cap.cx &&
          own.cy == cap.cy && own.k1 == cap.k1 && own.k2 == cap.k2 && own.p1 == cap.p1 && own.p2 == cap.p2, "of_handle");
    CHECK(gf::gfseq::fits(cap, own, msg, sizeof msg), "the handle's own values: %s", msg);
    printf("the handle's own values: ok\n");
    struct Case { const char* field; bool ok; gf_tracker_seq_cfg c; };
    auto with = [&](auto set) { gf_tracker_seq_cfg c = own; set(c); return c; };
    const Case cases[] = {
        {"max_cnt", true, with([](auto& c) { c.max_cnt = 1; })}, {"max_cnt", false, with([](auto& c) { c.max_cnt = 0; })},
        {"max_cnt", true, with([](auto& c) { c.max_cnt = 500; })}, {"max_cnt", false, with([](auto& c) { c.max_cnt = 501; })},
        {"min_dist", true, with([](auto& c) { c.min_dist = 12; })}, {"min_dist", false, with([](auto& c) { c.min_dist = 11; })},
        {"min_dist", true, with([](auto& c) { c.min_dist = gf::kMaxRadius; })}, {"min_dist", false, with([](auto& c) { c.min_dist = gf::kMaxRadius + 1; })},
        {"flow_back", true, with([](auto& c) { c.flow_back = 0; })}, {"flow_back", false, with([](auto& c) { c.flow_back = 2; })}, {"flow_back", false, with([](auto& c) { c.flow_back = -1; })},
        {"depth_cam", true, with([](auto& c) { c.depth_cam = 0; })}, {"depth_cam", false, with([](auto& c) { c.depth_cam = 2; })}, {"depth_cam", false, with([](auto& c) { c.depth_cam = -1; })},
        {"fx", true, with([](auto& c) { c.fx = 1e-3; })}, {"fx", false, with([](auto& c) { c.fx = 0.0; })}, {"fx", false, with([](auto& c) { c.fx = -1.0; })}, {"fx", false, with([](auto& c) { c.fx = NAN; })},
        {"fy", true, with([](auto& c) { c.fy = 384.06; })}, {"fy", false, with([](auto& c) { c.fy = 0.0; })}, {"fy", false, with([](auto& c) { c.fy = NAN; })},
        {"cx", true, with([](auto& c) { c.cx = -5.0; c.cy = 1e4; c.k1 = c.k2 = c.p1 = c.p2 = 0.0; })},
    };
    int n = 0;
    for (const Case& k : cases) {
        char small[24];   // a short buffer: the message is cut, never written past
        msg[0] = 0;
        const bool ok = gf::gfseq::fits(cap, k.c, msg, sizeof msg);
        CHECK(ok == k.ok, "case %d (%s): fits() = %d", n, k.field, (int)ok);
        if (!k.ok) {
            char name[64];
            snprintf(name, sizeof name, "gf_tracker_seq_cfg.%s ", k.field);
            CHECK(strstr(msg, name) != nullptr, "case %d: the message does not name %s: %s", n, k.field, msg);
            CHECK(!gf::gfseq::fits(cap, k.c, small, sizeof small) && strlen(small) < sizeof small, "case %d: short buffer", n);
        }
        n++;
    }
    printf("%d limits: ok\n", n);
}

int main() {
    disk_tables();
    limits();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("all: ok\n");
    return 0;
}
