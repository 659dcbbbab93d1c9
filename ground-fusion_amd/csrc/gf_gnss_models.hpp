// gf_gnss_models.hpp — the geodesy and atmosphere models of gnss_comm (not vendored by the reference): ecef2geo / geo2rotation / sat_azel / Saastamoinen / Klobuchar,
// restated from the published algorithms (RTKLIB lineage), the same formulas as the CPU oracle -- both documented as "parity unpinned" against gnss_comm itself.
// One source for the GNSS factor kernels (gf_ba_gnss.hpp) and the estimator's host code (GNSS intake and initialisation).  It sets no floating-point contraction of
// its own: the kernels compile it under gf_ba.hip's contract(fast), the host code without contraction (the build's default), as each did with its own copy.
#pragma once
#include "gf_dmath.hpp"

namespace gfd {

constexpr double GN_C = 2.99792458e8, GN_OMG = 7.2921151467e-5, GN_A = 6378137.0, GN_E2 = 6.69437999014e-3, GN_PI = 3.14159265358979323846;

__host__ __device__ inline V3 gn_ecef2geo(V3 p) {   // latitude [deg], longitude [deg], height [m]
    if (p.x == 0 && p.y == 0) return v3(0, 0, 0);
    const double a = GN_A, a2 = a * a, b2 = a2 * (1 - GN_E2), b = sqrt(b2), ep2 = (a2 - b2) / b2, rho = sqrt(p.x * p.x + p.y * p.y);
    double s1 = p.z * a, s2 = rho * b, h = sqrt(s1 * s1 + s2 * s2);
    const double st = s1 / h, ct = s2 / h;
    s1 = p.z + ep2 * b * st * st * st;
    s2 = rho - a * GN_E2 * ct * ct * ct;
    h = sqrt(s1 * s1 + s2 * s2);
    const double sin_lat = s1 / h, cos_lat = s2 / h;
    const double N = a2 / sqrt(a2 * cos_lat * cos_lat + b2 * sin_lat * sin_lat);
    return v3(atan(s1 / s2) * 180.0 / GN_PI, atan2(p.y, p.x) * 180.0 / GN_PI, rho / cos_lat - N);
}
__host__ __device__ inline M3 gn_geo2rotation(V3 lla) {   // R_ecef_enu
    const double lat = lla.x * GN_PI / 180.0, lon = lla.y * GN_PI / 180.0, sl = sin(lat), cl = cos(lat), so = sin(lon), co = cos(lon);
    M3 R;
    R.m[0] = -so; R.m[1] = -sl * co; R.m[2] = cl * co;
    R.m[3] = co;  R.m[4] = -sl * so; R.m[5] = cl * so;
    R.m[6] = 0;   R.m[7] = cl;       R.m[8] = sl;
    return R;
}
__host__ __device__ inline void gn_sat_azel(V3 rcv, V3 sat, double& az, double& el) {
    V3 dl = sat - rcv; dl = dl / sqrt(sqn(dl));
    const V3 enu = transpose(gn_geo2rotation(gn_ecef2geo(rcv))) * dl;
    az = (sqrt(dl.x * dl.x + dl.y * dl.y) < 1e-12) ? 0.0 : atan2(enu.x, enu.y);
    if (az < 0) az += 2 * GN_PI;
    el = asin(enu.z);
}
__host__ __device__ inline double gn_trop_delay(V3 lla, double el) {   // Saastamoinen, standard atmosphere, humidity 0.7
    if (lla.z < -100.0 || 1e4 < lla.z || el <= 0) return 0.0;
    const double hgt = lla.z < 0.0 ? 0.0 : lla.z;
    const double pres = 1013.25 * pow(1.0 - 2.2557e-5 * hgt, 5.2568), temp = 15.0 - 6.5e-3 * hgt + 273.16;
    const double e = 6.108 * 0.7 * exp((17.15 * temp - 4684.0) / (temp - 38.45)), z = GN_PI / 2.0 - el;
    const double trph = 0.0022768 * pres / (1.0 - 0.00266 * cos(2.0 * lla.x * GN_PI / 180.0) - 0.00028 * hgt / 1e3) / cos(z);
    const double trpw = 0.002277 * (1255.0 / temp + 0.05) * e / cos(z);
    return trph + trpw;
}
__host__ __device__ inline double gn_ion_delay(double tow, const double* ion_in, V3 lla, double az, double el) {   // Klobuchar
    const double ion_default[8] = {0.1118e-07, -0.7451e-08, -0.5961e-07, 0.1192e-06, 0.1167e+06, -0.2294e+06, -0.1311e+06, 0.1049e+07};
    if (lla.z < -1e3 || el <= 0) return 0.0;
    double nrm = 0;
    for (int i = 0; i < 8; i++) nrm += ion_in[i] * ion_in[i];
    double ion[8];
    for (int i = 0; i < 8; i++) ion[i] = nrm <= 0.0 ? ion_default[i] : ion_in[i];
    const double psi = 0.0137 / (el / GN_PI + 0.11) - 0.022;
    double phi = lla.x / 180.0 + psi * cos(az);
    if (phi > 0.416) phi = 0.416; else if (phi < -0.416) phi = -0.416;
    const double lam = lla.y / 180.0 + psi * sin(az) / cos(phi * GN_PI);
    phi += 0.064 * cos((lam - 1.617) * GN_PI);
    double tt = 43200.0 * lam + tow;
    tt -= floor(tt / 86400.0) * 86400.0;
    const double f = 1.0 + 16.0 * pow(0.53 - el / GN_PI, 3.0);
    double amp = ion[0] + phi * (ion[1] + phi * (ion[2] + phi * ion[3])), per = ion[4] + phi * (ion[5] + phi * (ion[6] + phi * ion[7]));
    amp = amp < 0.0 ? 0.0 : amp; per = per < 72000.0 ? 72000.0 : per;
    const double x = 2.0 * GN_PI * (tt - 50400.0) / per;
    return GN_C * f * (fabs(x) < 1.57 ? 5e-9 + amp * (1.0 + x * x * (-0.5 + x * x / 24.0)) : 5e-9);
}

}  // namespace gfd
