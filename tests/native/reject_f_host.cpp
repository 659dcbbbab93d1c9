// rejectWithF on the host (csrc/gf_reject_f.hpp) against the restatement of tests/reject_f_ref.py, byte for byte: a stand-alone program, built by
// tests/test_reject_f_host.py plain and under the address and undefined-behaviour sanitizers.
//   reject_f_host CASES_FILE
// CASES_FILE: int32 count, then per case int32 n, uint32 seed, double threshold, n x 4 floats, n status bytes in, n status bytes expected, 4 int32 (m, rejected,
// winner, inliers) expected.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_reject_f.hpp"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

template <class T> static bool get(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: reject_f_host CASES_FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t count = 0;
    if (!get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        int32_t n = 0, want_res[4]; uint32_t seed = 0; double thr = 0;
        if (!get(f, &n, 1) || !get(f, &seed, 1) || !get(f, &thr, 1) || n < 0 || n > gfrf::kMaxCandidates) { printf("case %d: bad header\n", k); return 2; }
        // exact-size buffers: a read or write one past the end is the sanitizer's to see
        std::vector<gfrf::Cand> pairs(n), cand(n);
        std::vector<uint8_t> st(n), want(n);
        std::vector<int> row_of(n);
        if (!get(f, reinterpret_cast<float*>(pairs.data()), 4 * (size_t)n) || !get(f, st.data(), n) || !get(f, want.data(), n) || !get(f, want_res, 4)) { printf("case %d: short file\n", k); return 2; }
        const gfrf::Result r = gfrf::reject(pairs.data(), st.data(), n, thr, seed, cand.data(), row_of.data());
        int diff = 0, first = -1;
        for (int i = 0; i < n; i++) if (st[i] != want[i]) { diff++; if (first < 0) first = i; }
        CHECK(diff == 0, "case %d (n = %d): %d status bytes differ, the first at row %d (%d, restatement %d)", k, n, diff, first, first < 0 ? 0 : st[first], first < 0 ? 0 : want[first]);
        CHECK(r.m == want_res[0] && r.rejected == want_res[1] && r.winner == want_res[2] && r.inliers == want_res[3],
              "case %d: result m %d rejected %d winner %d inliers %d, restatement %d %d %d %d", k, r.m, r.rejected, r.winner, r.inliers, want_res[0], want_res[1], want_res[2], want_res[3]);
        printf("case %d: n %d m %d rejected %d winner %d inliers %d\n", k, n, r.m, r.rejected, r.winner, r.inliers);
    }
    fclose(f);
    // the draw depends on (seed, h, d) alone and is a pure function
    CHECK(gfrf::draw_word(1, 2, 3) == gfrf::draw_word(1, 2, 3) && gfrf::draw_word(1, 2, 3) != gfrf::draw_word(1, 3, 2), "draw_word");
    char msg[160];
    CHECK(!gfrf::check_cfg(0.0, 0.0, msg, sizeof msg) && strstr(msg, "f_threshold"), "a zero threshold passed");
    CHECK(!gfrf::check_cfg(1.0, -1.0, msg, sizeof msg) && strstr(msg, "focal_length"), "a negative focal length passed");
    CHECK(gfrf::check_cfg(1.0, 0.0, msg, sizeof msg), "1.0 / 0 refused");
    printf(failures ? "%d checks failed\n" : "all: ok\n", failures);
    return failures ? 1 : 0;
}
