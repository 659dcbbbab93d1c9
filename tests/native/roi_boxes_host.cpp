// Stand-alone host program for the exclusion boxes (csrc/gf_roi.hpp: box_rows / box_cols / covered_word / box_word and the point test allowed(base, boxes, ..);
// csrc/gf_track_draw.hpp: the frame primitive), built with the address and undefined-behaviour sanitizers by tests/test_roi_boxes_host.py.
//   usage: roi_boxes_host <file>
// The file (tests/test_roi_boxes_host.py writes it from tests/roi_boxes_ref.py): int32 w, h, n_lists; per list int32 n and n x (xmin, ymin, xmax, ymax); then the
// h x w byte masks of regions A and B.  For every list, without a base and with each region:
//   - the word function against a per-pixel rasterisation written out here (64-bit comparisons, no clipping);
//   - the point test against gfroi::allowed on the composed table, at every pixel;
//   - every box's frame primitive against the three inequalities in 64 bits on the box's own coordinates, around and far from the image, and `touches` never
//     false for a tile the frame covers a pixel of; a rendered picture shows the frame over dots and strokes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_roi.hpp"
#include "../../ground-fusion_amd/csrc/gf_track_draw.hpp"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static bool in_box(const gf_box& b, int64_t x, int64_t y) { return (int64_t)b.xmin <= x && x <= (int64_t)b.xmax && (int64_t)b.ymin <= y && y <= (int64_t)b.ymax; }

static bool frame_brute(const gf_box& b, int64_t x, int64_t y) {
    if (!(b.xmax > b.xmin && b.ymax > b.ymin)) return false;
    const int64_t X0 = b.xmin, X1 = (int64_t)b.xmax - 1, Y0 = b.ymin, Y1 = (int64_t)b.ymax - 1;
    return X0 - 2 <= x && x <= X1 + 2 && Y0 - 2 <= y && y <= Y1 + 2 && !(X0 + 2 < x && x < X1 - 2 && Y0 + 2 < y && y < Y1 - 2);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <file>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) return 2;
    const int w = hdr[0], h = hdr[1], n_lists = hdr[2];
    std::vector<std::vector<gf_box>> lists(n_lists);
    for (auto& l : lists) {
        int32_t n;
        if (fread(&n, 4, 1, f) != 1) return 2;
        l.resize(n);
        if (n && fread(l.data(), sizeof(gf_box), n, f) != (size_t)n) return 2;
    }
    std::vector<uint8_t> masks[2] = {std::vector<uint8_t>((size_t)w * h), std::vector<uint8_t>((size_t)w * h)};
    for (auto& m : masks) if (fread(m.data(), 1, m.size(), f) != m.size()) return 2;
    fclose(f);
    static_assert(sizeof(gf_box) == 16, "gf_box is four int32_t");

    const int bands = gfroi::bands(h);
    const size_t words = gfroi::words(w, h);
    long long pixels = 0, excluded = 0, frames = 0, frame_pixels = 0;
    for (int base = 0; base < 3; base++) {   // 0: none, 1: A, 2: B
        std::vector<uint32_t> base_table(words, ~0u);   // a sequence without a base region: all ones, as the handle's table holds them
        if (base) for (int band = 0; band < bands; band++) for (int x = 0; x < w; x++) gfroi::pack_thread(masks[base - 1].data(), (size_t)w, w, h, band, x, base_table.data());
        const uint32_t* base_or_null = base ? base_table.data() : nullptr;
        for (int li = 0; li < n_lists; li++) {
            const std::vector<gf_box>& l = lists[li];
            const gf_box* bx = l.empty() ? nullptr : l.data();
            const int n = (int)l.size();
            std::vector<uint8_t> brute((size_t)w * h);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    bool ok = !base || masks[base - 1][(size_t)y * w + x] != 0;
                    for (int i = 0; i < n; i++) if (in_box(l[i], x, y)) ok = false;
                    brute[(size_t)y * w + x] = ok;
                    pixels++; excluded += !ok;
                }
            std::vector<uint32_t> composed(words);
            for (int band = 0; band < bands; band++)
                for (int x = 0; x < w; x++) {
                    const uint32_t word = gfroi::box_word(base_table[gfroi::word_at(w, band, x)], bx, n, w, h, band, x);
                    composed[gfroi::word_at(w, band, x)] = word;
                    const int rows = gfroi::rows_of_band(h, band);
                    for (int r = 0; r < rows; r++)
                        CHECK(((word >> r) & 1u) == brute[(size_t)(band * gfroi::kRows + r) * w + x], "base %d list %d: word of band %d column %d, row %d", base, li, band, x, r);
                    if (base && rows < 32) CHECK((word >> rows) == 0, "base %d list %d: bits past the image in band %d column %d", base, li, band, x);
                    uint32_t by_box = 0;   // the row mask depends on the band alone: the same for every column a box covers
                    for (int i = 0; i < n; i++) { int x0, x1; if (gfroi::box_cols(l[i], w, x0, x1) && x >= x0 && x <= x1) by_box |= gfroi::box_rows(l[i], h, band); }
                    CHECK(by_box == gfroi::covered_word(bx, n, w, h, band, x), "base %d list %d: covered_word", base, li);
                }
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const bool a = gfroi::allowed(base_or_null, bx, n, w, x, y), t = gfroi::allowed(composed.data(), w, x, y);
                    CHECK(a == t && a == (bool)brute[(size_t)y * w + x], "base %d list %d: point test at (%d, %d): %d, table %d, brute %d", base, li, x, y, a, t, brute[(size_t)y * w + x]);
                }
        }
    }

    // ---- the frame primitive
    for (int li = 0; li < n_lists; li++)
        for (const gf_box& b : lists[li]) {
            gfdraw::Prim p{};
            const bool drawn = gfdraw::make_frame(b, p);
            CHECK(drawn == (b.xmax > b.xmin && b.ymax > b.ymin), "list %d: make_frame of an empty rectangle", li);
            if (!drawn) { for (int y = -8; y < h + 8; y++) for (int x = -8; x < w + 8; x++) CHECK(!frame_brute(b, x, y), "list %d: brute draws an empty rectangle", li); continue; }
            frames++;
            CHECK(p.stroke == gfdraw::kFrame && abs(p.ux) <= gfdraw::kMaxCoord && abs(p.uy) <= gfdraw::kMaxCoord && abs(p.vx) <= gfdraw::kMaxCoord && abs(p.vy) <= gfdraw::kMaxCoord, "list %d: a coordinate beyond kMaxCoord", li);
            for (int y = -8; y < h + 8; y++)
                for (int x = -8; x < w + 8; x++) {
                    const bool c = gfdraw::frame_covers(p, x, y);
                    CHECK(c == frame_brute(b, x, y) && c == gfdraw::covers(p, x, y), "list %d box (%d %d %d %d): frame at (%d, %d)", li, b.xmin, b.ymin, b.xmax, b.ymax, x, y);
                    frame_pixels += c;
                }
            // tiles of the kernel's size and odd ones: never culled while a pixel of them is covered
            for (int th : {16, 5, 1})
                for (int tw : {64, 7, 1})
                    for (int y0 = 0; y0 < h; y0 += th)
                        for (int x0 = 0; x0 < w; x0 += tw) {
                            const int x1 = (x0 + tw < w ? x0 + tw : w) - 1, y1 = (y0 + th < h ? y0 + th : h) - 1;
                            bool any = false;
                            for (int y = y0; y <= y1 && !any; y++) for (int x = x0; x <= x1 && !any; x++) any = frame_brute(b, x, y);
                            if (any) CHECK(gfdraw::touches(p, x0, y0, x1, y1), "list %d box (%d %d %d %d): touches misses tile %d..%d x %d..%d", li, b.xmin, b.ymin, b.xmax, b.ymax, x0, x1, y0, y1);
                        }
        }
    // a frame covers strokes and dots; a list without frames renders what it rendered
    {
        const int W = 48, H = 40;
        std::vector<uint8_t> gray((size_t)W * H, 90), with((size_t)W * H * 3), without(with.size());
        const gf_box b{10, 8, 30, 28};
        gfdraw::Prim list[4] = {gfdraw::make_dot(10, 8, 3), gfdraw::make_dot(20, 18, 25), gfdraw::make_stroke(2, 8, 40, 8), gfdraw::Prim{}};
        CHECK(gfdraw::make_frame(b, list[3]), "make_frame");
        gfdraw::render_host(gray.data(), W, W, H, list, 4, with.data(), 3 * (size_t)W);
        gfdraw::render_host(gray.data(), W, W, H, list, 3, without.data(), 3 * (size_t)W);
        int over = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const uint8_t* a = with.data() + 3 * ((size_t)y * W + x);
                const uint8_t* o = without.data() + 3 * ((size_t)y * W + x);
                if (frame_brute(b, x, y)) { CHECK(a[0] == 0 && a[1] == 128 && a[2] == 255, "the frame's colour at (%d, %d)", x, y); over += o[0] != 90 || o[1] != 90 || o[2] != 90; }
                else CHECK(a[0] == o[0] && a[1] == o[1] && a[2] == o[2], "a pixel outside the frame changed at (%d, %d)", x, y);
            }
        CHECK(over > 20, "the frame covered only %d pixels of dots and strokes", over);
    }
    printf("%d x %d: %d lists, %lld pixels tested, %lld excluded, %lld frames, %lld frame pixels\n", w, h, n_lists, pixels, excluded, frames, frame_pixels);
    CHECK(excluded > 0 && (frames > 0 || w * h < 40), "the lists exclude nothing or draw nothing");
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("all: ok\n");
    return 0;
}
