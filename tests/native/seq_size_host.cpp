// gf_seq_size.hpp as a stand-alone host program, built with -fsanitize=address,undefined: the limits gf_tracker_set_seq_size checks, the table of the sizes in
// force (the ninth distinct size), the pyramid geometry of a size, "the geometry fits the slot", and the plan of a call on a handle whose sequences have sizes of
// their own (feature_tracker.cpp:108-109 per sequence) -- lists of 1 .. 8 sizes in every order, checked here for what a plan must satisfy and printed as one
// digest per length, which tests/test_seq_size_host.py holds against its own restatement, and a few lists printed in full.  No HIP, no GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_seq_size.hpp"

namespace {

long failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 30) printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

// the sizes of tests/test_tracker_sizes_gpu.py's SIZES, in its order
const int kSizes[11][2] = {{640, 480}, {1280, 720}, {640, 160}, {640, 481}, {1920, 1080}, {2560, 1440}, {752, 480}, {320, 240}, {644, 481}, {64, 48}, {40, 36}};

bool refused(int W, int H, int w, int h, const char* field) {
    char msg[256] = "";
    return !gfsize::limits_ok(W, H, w, h, msg, sizeof msg) && strstr(msg, field) != nullptr;
}

void limits() {
    const long before = failures;
    char msg[256];
    CHECK(gfsize::limits_ok(644, 481, 644, 481, msg, sizeof msg) && gfsize::limits_ok(644, 481, 32, 32, msg, sizeof msg) && gfsize::limits_ok(644, 481, 40, 36, msg, sizeof msg));
    CHECK(refused(644, 481, 28, 480, "width") && refused(644, 481, 648, 480, "width") && refused(644, 481, 0, 480, "width") && refused(644, 481, -4, 480, "width"));
    CHECK(refused(644, 481, 640, 31, "height") && refused(644, 481, 640, 482, "height") && refused(644, 481, 640, 0, "height") && refused(644, 481, 640, -1, "height"));
    CHECK(refused(644, 481, 642, 480, "width") && refused(644, 481, 33, 33, "width") && refused(644, 481, 1 << 30, 480, "width"));
    // the table: row 0 is the handle's and stays; seven more distinct sizes; the ninth is refused; a size that is in force is shared; a freed row is taken again
    gfsize::Table t;
    t.init(2560, 1440, 12);
    CHECK(t.in_force() == 1 && t.find(3, 0, 0) == 0 && t.find(3, 2560, 1440) == 0);
    for (int k = 0; k < 7; k++) {
        const int r = t.find(k, 64 + 4 * k, 48 + k);
        CHECK(r == k + 1);
        t.move(k, r, 64 + 4 * k, 48 + k);
        CHECK(t.in_force() == k + 2 && t.row_of[k] == r && t.w[r] == 64 + 4 * k && t.h[r] == 48 + k);
    }
    CHECK(t.find(8, 400, 300) == -1 && t.in_force() == GF_MAX_SEQ_SIZES);          // the ninth
    CHECK(t.find(8, 64, 48) == 1 && t.find(8, 2560, 1440) == 0);                   // in force already
    t.move(8, 1, 64, 48);
    CHECK(t.users[1] == 2 && t.find(0, 400, 300) == -1);                           // sequence 0 shares its row now: it cannot retype it
    CHECK(t.find(1, 400, 300) == 2);                                               // sequence 1 is its row's only user: the row takes the new size
    t.move(1, 2, 400, 300);
    CHECK(t.w[2] == 400 && t.h[2] == 300 && t.users[2] == 1 && t.in_force() == GF_MAX_SEQ_SIZES);
    t.move(1, 0, 0, 0);                                                            // back to the handle's: row 2 is free
    CHECK(t.users[2] == 0 && t.in_force() == GF_MAX_SEQ_SIZES - 1 && t.row_of[1] == 0 && t.w[0] == 2560 && t.h[0] == 1440 && t.users[0] == 12 - 7);
    CHECK(t.find(9, 800, 600) == 2);
    int users = 0;
    for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) users += t.users[r];
    CHECK(users == 12);
    printf("limits: %s\n", failures == before ? "ok" : "FAILED");
}

void geometry() {
    const long before = failures;
    for (const auto& s : kSizes) {
        gfsize::Geom g;
        gfsize::build_geom(s[0], s[1], g);
        printf("geom %d %d %d %zu", s[0], s[1], g.nlevels, g.img_bytes);
        for (int l = 0; l < g.nlevels; l++) printf(" %d %d %d %d", g.lv[l].w, g.lv[l].h, g.lv[l].stride, g.lv[l].img_off);
        printf("\n");
        CHECK(g.nlevels >= 1 && g.nlevels <= gfsize::kMaxLevels && g.img_bytes % 256 == 0);
    }
    // every size fits the slot of every size that dominates it
    int pairs = 0;
    for (const auto& a : kSizes)
        for (const auto& b : kSizes)
            if (b[0] <= a[0] && b[1] <= a[1]) { CHECK(gfsize::fits_slot(b[0], b[1], a[0], a[1])); pairs++; }
    CHECK(!gfsize::fits_slot(1280, 720, 640, 480));
    // ... and every level of the smaller pyramid ends inside the larger slot, for every size the limits allow under a few handles
    for (const auto& a : kSizes) {
        gfsize::Geom slot;
        gfsize::build_geom(a[0], a[1], slot);
        for (int w = 32; w <= a[0]; w += (a[0] > 700 ? 92 : 4))
            for (int h = 32; h <= a[1]; h += (a[1] > 500 ? 37 : 3)) {
                gfsize::Geom g;
                gfsize::build_geom(w, h, g);
                const gfsize::Level& last = g.lv[g.nlevels - 1];
                const size_t end = (size_t)last.img_off - (size_t)gfsize::kPad * last.stride - gfsize::kPad + (size_t)(last.h + 2 * gfsize::kPad) * last.stride;
                CHECK(end <= g.img_bytes && g.img_bytes <= slot.img_bytes);
            }
    }
    printf("fits %d\n", pairs);
    printf("geometry: %s\n", failures == before ? "ok" : "FAILED");
}

// what every plan must satisfy, whatever the list
void check_plan(const gfsize::Plan& p, const gfsize::Table& t, int count, const int* seq, const int* bpp) {
    CHECK(p.count == count);
    size_t g_off = 0, d_off = 0, m_off = 0;
    bool sized = false;
    int mw = 0, mh = 0;
    for (int i = 0; i < count; i++) {
        const int r = t.row_of[seq[i]];
        CHECK(p.row[i] == r && p.w[i] == t.w[r] && p.h[i] == t.h[r]);
        CHECK(p.gray_off[i] == g_off && p.depth_off[i] == d_off && p.mask_off[i] == m_off);
        const size_t px = (size_t)t.w[r] * t.h[r];
        g_off += px * (bpp ? bpp[i] : 1); d_off += 2 * px; m_off += px;
        sized = sized || r != 0;
        mw = std::max(mw, t.w[r]); mh = std::max(mh, t.h[r]);
    }
    CHECK(p.gray_bytes == g_off && p.depth_bytes == d_off && p.mask_bytes == m_off && p.sized == sized && p.max_w == mw && p.max_h == mh);
    // the groups partition the list positions: each once, in list order inside its group, one row per group, groups in the order of their first member
    std::vector<int> seen(count, 0);
    int at = 0, prev_first = -1;
    CHECK(p.n_groups >= (count > 0 ? 1 : 0) && p.n_groups <= GF_MAX_SEQ_SIZES);
    for (int g = 0; g < p.n_groups; g++) {
        CHECK(p.group_first[g] == at && p.group_n[g] >= 1);
        for (int g2 = 0; g2 < g; g2++) CHECK(p.group_row[g2] != p.group_row[g]);
        for (int k = 0; k < p.group_n[g]; k++) {
            const int i = p.member[at + k];
            CHECK(i >= 0 && i < count && !seen[i] && p.row[i] == p.group_row[g]);
            if (i >= 0 && i < count) seen[i]++;
            if (k > 0) CHECK(i > p.member[at + k - 1]);
        }
        CHECK(p.member[at] > prev_first);
        prev_first = p.member[at];
        at += p.group_n[g];
    }
    CHECK(at == count);
}

unsigned long long digest = 0;
void mix(unsigned long long v) { digest = (digest ^ v) * 1099511628211ull; }
void mix_plan(const gfsize::Plan& p) {
    mix(p.count); mix(p.sized); mix(p.max_w); mix(p.max_h); mix(p.gray_bytes); mix(p.depth_bytes); mix(p.mask_bytes); mix(p.n_groups);
    for (int i = 0; i < p.count; i++) { mix(p.row[i]); mix(p.w[i]); mix(p.h[i]); mix(p.gray_off[i]); mix(p.depth_off[i]); mix(p.mask_off[i]); mix(p.member[i]); }
    for (int g = 0; g < p.n_groups; g++) { mix(p.group_row[g]); mix(p.group_first[g]); mix(p.group_n[g]); }
}
void print_plan(const char* name, const gfsize::Plan& p, int count, const int* seq) {
    printf("plan %s seq", name);
    for (int i = 0; i < count; i++) printf(" %d", seq[i]);
    printf(" | sized %d max %d %d bytes %zu %zu %zu | row", (int)p.sized, p.max_w, p.max_h, p.gray_bytes, p.depth_bytes, p.mask_bytes);
    for (int i = 0; i < count; i++) printf(" %d", p.row[i]);
    printf(" | off");
    for (int i = 0; i < count; i++) printf(" %zu %zu %zu", p.gray_off[i], p.depth_off[i], p.mask_off[i]);
    printf(" | groups");
    for (int g = 0; g < p.n_groups; g++) printf(" %d %d %d", p.group_row[g], p.group_first[g], p.group_n[g]);
    printf(" | member");
    for (int i = 0; i < count; i++) printf(" %d", p.member[i]);
    printf("\n");
}

// a handle of 2560 x 1440 with 10 sequences: sequence k (k >= 1) has kSizes[order[k]], sequence 0, 8 and 9 what the caller says
void orders() {
    const long before = failures;
    const int pick[8] = {5, 0, 1, 2, 8, 7, 9, 10};   // 2560 x 1440 (the handle's own), 640 x 480, 1280 x 720, 640 x 160, 644 x 481, 320 x 240, 64 x 48, 40 x 36
    gfsize::Plan p;
    long long calls = 0;
    for (int n = 1; n <= 8; n++) {
        gfsize::Table t;
        t.init(2560, 1440, 10);
        for (int k = 1; k < n; k++) { const int r = t.find(k, kSizes[pick[k]][0], kSizes[pick[k]][1]); CHECK(r == k); t.move(k, r, kSizes[pick[k]][0], kSizes[pick[k]][1]); }
        CHECK(t.in_force() == n);
        std::vector<int> seq(n);
        for (int k = 0; k < n; k++) seq[k] = k;
        digest = 14695981039346656037ull;
        long long perms = 0;
        do {
            gfsize::plan_list(p, t, n, seq.data());
            check_plan(p, t, n, seq.data(), nullptr);
            CHECK(p.n_groups == n && p.sized == (n > 1));   // every position a different size
            mix_plan(p);
            perms++; calls++;
        } while (std::next_permutation(seq.begin(), seq.end()));
        printf("orders %d %lld %llu\n", n, perms, digest);
    }
    printf("orders: %s (%lld plans)\n", failures == before ? "ok" : "FAILED", calls);
}

void lists() {
    const long before = failures;
    gfsize::Table t;
    t.init(644, 481, 8);
    const int own[8][2] = {{0, 0}, {640, 480}, {640, 160}, {320, 240}, {64, 48}, {40, 36}, {64, 48}, {64, 48}};
    for (int k = 1; k < 8; k++) { const int r = t.find(k, own[k][0], own[k][1]); CHECK(r > 0); t.move(k, r, own[k][0], own[k][1]); }
    CHECK(t.in_force() == 6 && t.row_of[4] == t.row_of[6] && t.row_of[6] == t.row_of[7]);
    gfsize::Plan p;
    struct L { const char* name; int n; int seq[8]; };
    const L cases[] = {
        {"all", 8, {0, 1, 2, 3, 4, 5, 6, 7}}, {"reverse", 8, {7, 6, 5, 4, 3, 2, 1, 0}}, {"two", 2, {5, 1}}, {"own_only", 1, {0}}, {"one_size", 3, {6, 4, 7}},
        {"small_small_large", 3, {4, 0, 7}}, {"different", 6, {3, 0, 5, 1, 4, 2}}, {"empty", 0, {0}},
    };
    for (const L& c : cases) {
        gfsize::plan_list(p, t, c.n, c.seq);
        check_plan(p, t, c.n, c.seq, nullptr);
        print_plan(c.name, p, c.n, c.seq);
    }
    gfsize::plan_list(p, t, 1, cases[3].seq);
    CHECK(!p.sized && p.n_groups == 1 && p.group_row[0] == 0);                    // the handle's own size alone: the call of a handle without sizes
    gfsize::plan_list(p, t, 3, cases[4].seq);
    CHECK(p.sized && p.n_groups == 1 && p.group_n[0] == 3 && p.member[0] == 0 && p.member[1] == 1 && p.member[2] == 2);
    const int bpp[3] = {3, 1, 2};                                                 // bytes per pixel of the gray frames: the offsets of the formats' rule
    gfsize::plan_list(p, t, 3, cases[5].seq, bpp);
    check_plan(p, t, 3, cases[5].seq, bpp);
    CHECK(p.gray_off[1] == 64u * 48 * 3 && p.gray_off[2] == 64u * 48 * 3 + 644u * 481 && p.gray_bytes == 64u * 48 * 3 + 644u * 481 + 64u * 48 * 2);
    // offsets past 2^32: 9 sequences of 16384 x 16384 u16 depth
    gfsize::Table big;
    big.init(16384, 16384, 9);
    std::vector<int> seq(9);
    for (int k = 0; k < 9; k++) seq[k] = k;
    gfsize::plan_list(p, big, 9, seq.data());
    check_plan(p, big, 9, seq.data(), nullptr);
    CHECK(p.depth_off[8] == 8ull * 16384 * 16384 * 2 && p.depth_off[8] == (1ull << 32) && p.depth_bytes == 9ull << 29 && p.gray_off[8] == 1ull << 31 && p.mask_bytes == 9ull << 28);
    printf("lists: %s\n", failures == before ? "ok" : "FAILED");
}

}  // namespace

int main() {
    limits();
    geometry();
    orders();
    lists();
    printf("all: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
