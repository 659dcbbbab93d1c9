// The depth registration of csrc/gf_depth_reg.hpp -- the header the scatter kernel, the tracker's setter and the building blocks compile -- on the CPU.
//   depth_reg_host run CASE DEPTH OUT   CASE: one line "width height fx fy cx cy scale R0..R8 T0..T2 | fx fy cx cy k1 k2 p1 p2 | wc hc" (doubles as hex floats);
//                                       DEPTH: width x height u16, tight.  gfdreg::register_frame into OUT (wc x hc u16, tight), with source, destination
//                                       and z-buffer on heap blocks of exactly their sizes, so that the address sanitizer sees any access outside them.  The
//                                       result is held byte for byte against a brute force that, for every COLOUR pixel, scans every depth pixel's footprint.
//                                       Prints "census <zero> <behind> <not finite> <out of range> <over bound> <empty> <writes>" and "brute: ok".
//   depth_reg_host check                for every line of stdin in the first 20 fields of CASE: "ok", or the refusal of gfdreg::check
// Plain C++: the header needs no HIP for this part.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_depth_reg.hpp"

static bool read_reg(FILE* f, gf_depth_reg& r) {
    if (std::fscanf(f, "%d %d", &r.width, &r.height) != 2) return false;
    double* v[5] = {&r.fx, &r.fy, &r.cx, &r.cy, &r.scale};
    for (double* p : v) if (std::fscanf(f, "%la", p) != 1) return false;
    for (double& p : r.R) if (std::fscanf(f, "%la", &p) != 1) return false;
    for (double& p : r.T) if (std::fscanf(f, "%la", &p) != 1) return false;
    return true;
}

static int run(const char* case_path, const char* depth_path, const char* out_path) {
    FILE* f = std::fopen(case_path, "r");
    if (!f) { std::printf("cannot open %s\n", case_path); return 2; }
    gf_depth_reg reg;
    double proj[4], dist[4];
    int wc = 0, hc = 0;
    bool ok = read_reg(f, reg);
    for (double& p : proj) ok = ok && std::fscanf(f, "%la", &p) == 1;
    for (double& p : dist) ok = ok && std::fscanf(f, "%la", &p) == 1;
    ok = ok && std::fscanf(f, "%d %d", &wc, &hc) == 2;
    std::fclose(f);
    if (!ok) { std::printf("bad case file\n"); return 2; }
    char msg[320];
    if (!gfdreg::check(reg, msg, sizeof msg)) { std::printf("refused: %s\n", msg); return 2; }
    const gfdreg::Params p = gfdreg::params_of(reg, proj, dist);
    const int wd = reg.width, hd = reg.height;
    const size_t n_src = (size_t)wd * hd, n_dst = (size_t)wc * hc, n_z = gfdreg::zwords_of(wc, hc);
    uint16_t* src = static_cast<uint16_t*>(std::malloc(n_src * 2));
    uint16_t* dst = static_cast<uint16_t*>(std::malloc(n_dst * 2));
    uint32_t* z = static_cast<uint32_t*>(std::malloc(n_z * 4));
    f = std::fopen(depth_path, "rb");
    if (!f || std::fread(src, 2, n_src, f) != n_src) { std::printf("cannot read %s\n", depth_path); return 2; }
    std::fclose(f);
    std::memset(dst, 0xA5, n_dst * 2);
    for (size_t i = 0; i < n_z; i++) z[i] = gfdreg::kUntouched;
    long long census[gfdreg::kWrites + 1] = {};
    gfdreg::register_frame(p, src, (size_t)wd * 2, wd, hd, dst, (size_t)wc * 2, wc, hc, z, census);
    std::printf("census");
    for (long long c : census) std::printf(" %lld", c);
    std::printf("\n");
    int bad = 0;
    for (size_t i = 0; i < n_z; i++) if (z[i] != gfdreg::kUntouched) bad++;
    if (bad) std::printf("z-buffer: %d words not primed again\n", bad);
    // the brute force: every colour pixel against every depth pixel's footprint
    std::vector<gfdreg::Foot> foot(n_src);
    std::vector<uint8_t> writes(n_src);
    for (int y = 0; y < hd; y++)
        for (int x = 0; x < wd; x++) writes[(size_t)y * wd + x] = gfdreg::footprint(p, wc, hc, x, y, src[(size_t)y * wd + x], foot[(size_t)y * wd + x]) == gfdreg::kWrites;
    int differ = 0;
    for (int v = 0; v < hc; v++)
        for (int u = 0; u < wc; u++) {
            uint32_t best = gfdreg::kUntouched;
            for (size_t i = 0; i < n_src; i++)
                if (writes[i] && foot[i].x0 <= u && u <= foot[i].x1 && foot[i].y0 <= v && v <= foot[i].y1 && foot[i].val < best) best = foot[i].val;
            const uint16_t want = best == gfdreg::kUntouched ? 0 : (uint16_t)best;
            if (dst[(size_t)v * wc + u] != want && differ++ < 8) std::printf("colour pixel (%d, %d): walk %u, brute force %u\n", u, v, dst[(size_t)v * wc + u], want);
        }
    std::printf(differ || bad ? "brute: %d differ\n" : "brute: ok\n", differ);
    f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(dst, 2, n_dst, f) != n_dst) { std::printf("cannot write %s\n", out_path); return 2; }
    std::fclose(f);
    std::free(src); std::free(dst); std::free(z);
    return differ || bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3], argv[4]);
    if (argc == 2 && !std::strcmp(argv[1], "check")) {
        gf_depth_reg r;
        while (read_reg(stdin, r)) {
            char msg[320];
            if (gfdreg::check(r, msg, sizeof msg)) std::printf("ok\n"); else std::printf("%s\n", msg);
        }
        return 0;
    }
    std::printf("usage: depth_reg_host run CASE DEPTH OUT | depth_reg_host check\n");
    return 2;
}
