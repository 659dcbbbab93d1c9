// gnss_models_host.hip -- csrc/gf_gnss_models.hpp as the estimator's host code compiles it (no contraction), in a stand-alone program: reads
// (receiver ECEF, satellite ECEF, time of week, Klobuchar table) tuples, one per line, and prints what the models give for each:
//   lla (3)  R_ecef_enu (9)  az  el  trop  ion
// Numbers go in and out as hexadecimal floats, so no digit is lost on the way.  tests/test_gnss_hard_cases_host.py compares the output with the same tuples evaluated
// at 60 digits (tests/golden/ref_gnss_models.json.gz) and runs the program once more under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../ground-fusion_amd/csrc/gf_gnss_models.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: gnss_models_host TUPLES\n"); return 2; }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<char> line(4096);
    int n = 0;
    while (std::fgets(line.data(), (int)line.size(), f)) {
        double v[15];
        char* p = line.data();
        int got = 0;
        for (; got < 15; got++) {
            char* e = nullptr;
            v[got] = std::strtod(p, &e);
            if (e == p) break;
            p = e;
        }
        if (got == 0) continue;
        if (got != 15) { std::fprintf(stderr, "line %d: %d of 15 numbers\n", n + 1, got); std::fclose(f); return 3; }
        const gfd::V3 rcv = gfd::v3(v[0], v[1], v[2]), sat = gfd::v3(v[3], v[4], v[5]);
        const gfd::V3 lla = gfd::gn_ecef2geo(rcv);
        const gfd::M3 R = gfd::gn_geo2rotation(lla);
        double az = 0, el = 0;
        gfd::gn_sat_azel(rcv, sat, az, el);
        const double trop = gfd::gn_trop_delay(lla, el), ion = gfd::gn_ion_delay(v[6], v + 7, lla, az, el);
        std::printf("%a %a %a", lla.x, lla.y, lla.z);
        for (int i = 0; i < 9; i++) std::printf(" %a", R.m[i]);
        std::printf(" %a %a %a %a\n", az, el, trop, ion);
        n++;
    }
    std::fclose(f);
    std::printf("tuples: %d\nall: ok\n", n);
    return 0;
}
