// Stand-alone host program over ground-fusion_amd/csrc/gf_track_draw.hpp, the code host and device share for the track image.  No HIP call is made.
//   track_draw_host selftest          the literals of the definition ("Track image"), the binning function against brute force, the refusals
//   track_draw_host render IN OUT     a whole frame on the CPU by the per-pixel function the kernel walks; tests/test_track_draw_host.py compares it with
//                                     tests/track_draw_ref.py byte for byte
// IN: int32 w, h, n; w * h gray bytes; n x (x, y) float32 current points; n int32 track_cnt; n x (x, y) float32 previous points; n bytes has_prev.
// OUT: h * w * 3 bytes.  Built plain and with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_track_draw.hpp"

using namespace gfdraw;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static std::vector<Prim> list_of(const std::vector<float>& cur, const std::vector<int>& cnt, const std::vector<float>& prev, const std::vector<uint8_t>& has, int* rc = nullptr) {
    std::vector<Prim> out(list_capacity(cnt.size()) + 1);
    char msg[160] = "";
    const int m = build_list((int)cnt.size(), cur.data(), cnt.data(), prev.empty() ? nullptr : prev.data(), has.empty() ? nullptr : has.data(), out.data(), msg, sizeof msg);
    if (rc) *rc = m;
    out.resize(m < 0 ? 0 : m);
    return out;
}

static int green_count(const std::vector<Prim>& l, int w, int h, int gx0 = 0, int gy0 = 0, int gx1 = -1, int gy1 = -1, bool* only_inside = nullptr) {
    int n = 0;
    if (only_inside) *only_inside = true;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            if (resolve(l.data(), (int)l.size(), x, y, 7) == (255u << 8)) {
                n++;
                if (only_inside && !(x >= gx0 && x <= gx1 && y >= gy0 && y <= gy1)) *only_inside = false;
            }
    return n;
}

static void selftest() {
    // the worked example: cur = (15, 10), prev = (5, 10); tips (6, 11) and (6, 9); green = x 4..16 x y 9..11 plus x 5..7 at y = 8 and y = 12: 45 pixels
    {
        std::vector<Prim> l = list_of({15, 10}, {1}, {5, 10}, {1});
        CHECK(l.size() == 4);
        CHECK(l[1].stroke && l[1].ux == 15 && l[1].uy == 10 && l[1].vx == 5 && l[1].vy == 10);
        CHECK(l[2].ux == 6 && l[2].uy == 11 && l[2].vx == 5 && l[2].vy == 10);
        CHECK(l[3].ux == 6 && l[3].uy == 9 && l[3].vx == 5 && l[3].vy == 10);
        int n = 0;
        for (int y = 0; y < 24; y++)
            for (int x = 0; x < 32; x++) {
                const bool want = (x >= 4 && x <= 16 && y >= 9 && y <= 11) || (x >= 5 && x <= 7 && (y == 8 || y == 12));
                const bool got = resolve(l.data(), 4, x, y, 7) == (255u << 8);
                CHECK(want == got);
                n += got;
            }
        CHECK(n == 45);
    }
    {   // cur == prev: three strokes of no length, the 3 x 3 block
        std::vector<Prim> l = list_of({9, 9}, {1}, {9, 9}, {1});
        bool inside = false;
        CHECK(green_count(l, 20, 20, 8, 8, 10, 10, &inside) == 9 && inside);
    }
    {   // one dot, nothing clipped: 81 pixels of (C0[k], 0, C2[k]); everything else grey
        std::vector<Prim> l = list_of({10, 10}, {3}, {}, {});
        int n = 0;
        for (int y = 0; y < 21; y++)
            for (int x = 0; x < 21; x++) {
                const uint32_t v = resolve(l.data(), 1, x, y, 9);
                if (v == (217u | (38u << 16))) { n++; CHECK((x - 10) * (x - 10) + (y - 10) * (y - 10) <= 25); }
                else CHECK(v == 0x090909u);
            }
        CHECK(n == 81);
    }
    {   // rounding of the centre: half to even
        std::vector<Prim> l = list_of({2.5f, 3.5f}, {1}, {}, {});
        CHECK(l[0].ux == 2 && l[0].uy == 4);
    }
    // both colour tables
    const int c0[21] = {255, 242, 230, 217, 204, 191, 178, 166, 153, 140, 128, 115, 102, 89, 77, 64, 51, 38, 25, 13, 0};
    const int c2[21] = {0, 13, 26, 38, 51, 64, 76, 89, 102, 115, 128, 140, 153, 166, 178, 191, 204, 217, 230, 242, 255};
    for (int k = 0; k <= 30; k++) {
        const Prim d = make_dot(0, 0, k);
        CHECK(d.c0 == c0[k < 20 ? k : 20] && d.c2 == c2[k < 20 ? k : 20] && !d.stroke);
        if (k <= 20) {   // the reference's expression, in the host's doubles
            const double len = std::min(1.0, 1.0 * k / 20);
            CHECK(lrint(255 * (1 - len)) == c0[k] && lrint(255 * len) == c2[k]);
        }
    }
    // the binning function for every tile of a frame, against brute force over all primitives: never missing from a tile it covers
    {
        const int w = 150, h = 70, tw = 64, th = 16;
        std::vector<float> cur, prev; std::vector<int> cnt; std::vector<uint8_t> has;
        unsigned s = 12345;
        auto rnd = [&](int lo, int hi) { s = s * 1664525u + 1013904223u; return lo + (int)((s >> 8) % (unsigned)(hi - lo + 1)); };
        for (int i = 0; i < 300; i++) {
            const int x = rnd(-10, w + 10), y = rnd(-10, h + 10);
            cur.push_back((float)x); cur.push_back((float)y);
            prev.push_back((float)(x + rnd(-40, 40))); prev.push_back((float)(y + rnd(-40, 40)));
            cnt.push_back(rnd(1, 25)); has.push_back(rnd(0, 3) != 0);
        }
        std::vector<Prim> l = list_of(cur, cnt, prev, has);
        long covered = 0, let_through = 0;
        for (int ty = 0; ty * th < h; ty++)
            for (int tx = 0; tx * tw < w; tx++) {
                const int x0 = tx * tw, y0 = ty * th, x1 = std::min(x0 + tw, w) - 1, y1 = std::min(y0 + th, h) - 1;
                for (const Prim& p : l) {
                    bool any = false;
                    for (int y = y0; y <= y1 && !any; y++) for (int x = x0; x <= x1 && !any; x++) any = covers(p, x, y);
                    const bool t = touches(p, x0, y0, x1, y1);
                    if (any) { covered++; CHECK(t); }
                    let_through += t;
                }
            }
        CHECK(covered > 500 && let_through < 4 * covered);   // the test saw work, and the box is no licence to pass everything
    }
    // the builder's refusals
    {
        int rc = 0;
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        list_of({nan, 1}, {1}, {}, {}, &rc); CHECK(rc == -1);
        list_of({1, inf}, {1}, {}, {}, &rc); CHECK(rc == -1);
        list_of({1048577.f, 1}, {1}, {}, {}, &rc); CHECK(rc == -1);
        list_of({1, -1048577.f}, {1}, {}, {}, &rc); CHECK(rc == -1);
        list_of({1048576.f, -1048576.f}, {1}, {}, {}, &rc); CHECK(rc == 1);
        list_of({1, 1}, {-1}, {}, {}, &rc); CHECK(rc == -1);
        list_of({1, 1}, {0}, {}, {}, &rc); CHECK(rc == 1);
        list_of({1, 1}, {1}, {nan, 0}, {1}, &rc); CHECK(rc == -1);
        list_of({1, 1}, {1}, {nan, 0}, {0}, &rc); CHECK(rc == 1);     // not read without an arrow
        list_of({1, 1}, {1}, {1048577.f, 0}, {1}, &rc); CHECK(rc == -1);
        // the longest arrow the builder takes: corner to corner of the range, every product inside int64
        std::vector<Prim> l = list_of({1048576.f, 1048576.f}, {1}, {-1048576.f, -1048576.f}, {1}, &rc);
        CHECK(rc == 4);
        CHECK(resolve(l.data(), 4, 0, 0, 1) == (255u << 8) && resolve(l.data(), 4, 1, 0, 1) == (255u << 8) && resolve(l.data(), 4, 3, 0, 1) == 0x010101u);
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "selftest")) {
        selftest();
        printf(fails ? "%d checks failed\n" : "ok\n", fails);
        return fails ? 1 : 0;
    }
    if (argc != 4 || strcmp(argv[1], "render")) { printf("usage: track_draw_host selftest | render IN OUT\n"); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
    int hdr[3];
    if (fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int w = hdr[0], h = hdr[1], n = hdr[2];
    std::vector<uint8_t> gray((size_t)w * h), has(n);
    std::vector<float> cur(2 * (size_t)n), prev(2 * (size_t)n);
    std::vector<int> cnt(n);
    bool ok = fread(gray.data(), 1, gray.size(), f) == gray.size();
    if (n > 0) {
        ok = ok && fread(cur.data(), sizeof(float), cur.size(), f) == cur.size() && fread(cnt.data(), sizeof(int), n, f) == (size_t)n;
        ok = ok && fread(prev.data(), sizeof(float), prev.size(), f) == prev.size() && fread(has.data(), 1, n, f) == (size_t)n;
    }
    fclose(f);
    if (!ok) { printf("short input\n"); return 2; }
    std::vector<Prim> list(list_capacity(n) + 1);
    char msg[160];
    const int m = build_list(n, cur.data(), cnt.data(), prev.data(), has.data(), list.data(), msg, sizeof msg);
    if (m < 0) { printf("refused: %s\n", msg); return 3; }
    std::vector<uint8_t> out((size_t)w * h * 3);
    render_host(gray.data(), (size_t)w, w, h, list.data(), m, out.data(), 3 * (size_t)w);
    FILE* o = fopen(argv[3], "wb");
    if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) return 2;
    fclose(o);
    return 0;
}
