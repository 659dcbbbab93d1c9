"""GNSS windows that take every branch of csrc/gf_gnss_models.hpp and every list shape of ba_linearize_gnss (plain numpy, no GPU).

Every GNSS window the suite had comes from synth_window.add_gnss with one site (31.03 N, 121.44 E, 20 m), one time of week (345600 + t), the YAML's Klobuchar table,
satellites at 32..80 degrees and three satellites of each constellation in every frame: every factor takes the day branch of the Klobuchar model with no clamp, the
middle height class of both delay models, and every (frame, lower) group holds every constellation.  The cases here vary the site, the time, the table, the elevation
bands and the visibility; `census_of` restates the BRANCH DECISIONS of the models in numpy (the values come from tests/golden/make_ref_golden.py at 60 digits) and
counts which classes a window's factors take, with each factor's distance from every switch: the cases are chosen so that double and 60-digit arithmetic decide alike.

  python tests/gnss_hard_cases.py      writes profiles/gnss_model_census.json (the new cases and the older inputs side by side)

tests/test_gnss_hard_cases_host.py holds the census to its bars and to the committed file; tests/test_gnss_hard_cases_gpu.py runs the cases on the device."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "ground-fusion_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SMALL = dict(max_features=6, n_landmarks=9)          # the size of tests/golden/ref_window_gnss
MARG = dict(max_features=10, n_landmarks=15)         # the size of tests/golden/ref_marg_old_gnss
ZERO_TABLE = [0.0] * 8
SHORT_PERIOD_TABLE = [0.1118e-07, 0.2235e-07, -0.4172e-06, 0.6557e-06, 0.60e+05, 0.20e+05, -0.30e+05, 0.10e+05]     # per stays below 72000 for every |phi| < 0.5
BANDS_LOW = [(-4.5, -0.5), (0.5, 4.5), (32.0, 80.0)]   # below the horizon, (0, 5] degrees, the suite's band: the satellites of a constellation in turn


# ---------------------------------------------------------------- visibility rules (frame, constellation, satellite) -> bool
def thinned(i, sys, q):
    """frame 4 without observations, constellation 3 absent, constellation 2 in frames 0 and 7 only, frame 9 one observation, frame 10 two"""
    if i == 4 or sys == 3:
        return False
    if sys == 2:
        return i in (0, 7) and q == 0
    if i == 9:
        return sys == 0 and q == 0
    if i == 10:
        return (sys, q) in ((0, 0), (1, 1))
    return True


def not_frame0(i, sys, q):
    return i != 0


def only_frame0(i, sys, q):
    return i == 0


def single(i0, sys0, q0):
    def rule(i, sys, q):
        return (i, sys, q) == (i0, sys0, q0)
    rule.__name__ = "single_%d_%d_%d" % (i0, sys0, q0)
    return rule


SOUTH_WEST = dict(lat=-33.9, lon=-70.6, alt=520.0, tow0=1800.0, el_range=BANDS_LOW)
POLAR_NORTH = dict(lat=78.2, lon=15.6, alt=-50.0, tow0=345600.0 + 36000.0)
POLAR_SOUTH = dict(lat=-78.0, lon=-120.0, alt=12000.0, tow0=345600.0 + 75000.0, iono=ZERO_TABLE)
RIFT = dict(lat=31.5, lon=35.5, alt=-430.0, tow0=345600.0 + 41880.0, iono=SHORT_PERIOD_TABLE)
DEEP = dict(lat=-26.4, lon=27.4, alt=-1500.0, tow0=345600.0 + 30000.0)
NIGHT = dict(tow0=345600.0 - 21900.0)

# The table of cases.  name -> (seed, make_window keywords, add_gnss keywords, fixture kind).  kinds: "window" (H, g, cost), "marg" (the MARGIN_OLD prior after four iterations)
CASES = {
    "night_thinned": (21, SMALL, dict(NIGHT, visible=thinned), "window"),
    "south_west_low": (22, SMALL, SOUTH_WEST, "window"),
    "polar_north_352": (23, SMALL, dict(POLAR_NORTH, sats_per_sys=8), "window"),
    "polar_south_high": (24, SMALL, POLAR_SOUTH, "window"),
    "rift_short_period": (25, SMALL, RIFT, "window"),
    "deep": (26, SMALL, DEEP, "window"),
    "marg_frame0_empty": (27, MARG, dict(visible=not_frame0), "marg"),
    "marg_frame0_only": (28, MARG, dict(SOUTH_WEST, visible=only_frame0), "marg"),
}
# Single-factor windows: one representative factor of each Klobuchar / Saastamoinen class, the sites, times and tables of the cases above, the list cut to that factor
# (kind "single": H, g, cost and the factor's own r, J).  They exist for ONE comparison: each entry of g in the factor's own columns against its 60-digit terms, relative to
# the sum of the absolute terms -- under max |g| of a full window a low-weight factor hides.  The anchor columns are fed by the pseudorange row alone, and the pseudorange
# residual is a difference of numbers of 2.5e7 m: ulp(2.5e7) = 3.7e-9 m, and the factor rounds about ten times on the way (three coordinate differences, the norm, six
# additions), so double precision places the residual to ~1.7e-8 m at the worst, whatever its size.  A tolerance of 1e-11 of the term is above that rounding only for a
# residual of more than 1.7 km.  CLOCK_OFFSET is added to every receiver clock bias of these windows (the clock factors see differences and do not change): 5 000 m, 17 us of
# receiver clock error -- less than a receiver has at its first fix --, so the bar asks for 5e-8 m in absolute terms: three times the rounding, a hundred-millionth of any delay.
CLOCK_OFFSET = 5000.0
SINGLES = {
    "one_day": (31, SMALL, dict(visible=single(5, 0, 1)), "single"),
    "one_night": (32, SMALL, dict(NIGHT, visible=single(3, 1, 0)), "single"),
    "one_polar_north": (33, SMALL, dict(POLAR_NORTH, visible=single(6, 2, 2)), "single"),
    "one_polar_south": (34, SMALL, dict(POLAR_SOUTH, visible=single(2, 3, 1)), "single"),
    "one_rift": (35, SMALL, dict(RIFT, visible=single(7, 0, 0)), "single"),
    "one_deep": (36, SMALL, dict(DEEP, visible=single(4, 1, 2)), "single"),
    "one_low_elevation": (37, SMALL, dict(SOUTH_WEST, visible=single(5, 2, 1)), "single"),
    "one_below_horizon": (38, SMALL, dict(SOUTH_WEST, visible=single(8, 3, 0)), "single"),
}
ALL = dict(CASES, **SINGLES)
SOLVE_CASE = "south_west_low"
WINDOW_CASES = [k for k, v in CASES.items() if v[3] == "window"]
MARG_CASES = [k for k, v in CASES.items() if v[3] == "marg"]
SINGLE_CASES = list(SINGLES)

# the GNSS windows the suite had before (tests/test_backend_gpu.py, tests/test_golden.py, tests/golden/make_ref_golden.py, scripts/stale_probe.py): seed, make_window keywords
OLD_INPUTS = {
    "seed_1": (1, {}), "seed_2": (2, {}), "seed_78": (78, dict(max_features=30, n_landmarks=45)), "ref_window_gnss": (11, SMALL), "ref_marg_old_gnss": (12, MARG),
    "config5_W20": (1, dict(W=20, n_landmarks=750, max_features=500)),
}

_made = {}


def window_of(name, pre=None):
    """the case's window (a fresh copy; built once per process).  pre: the pre-integration provider (default: the CPU oracle)"""
    if name not in _made:
        import synth_window as SW
        if pre is None:
            import oracle_py as pre
        seed, kw, gkw, kind = ALL[name]
        w = SW.make_window(seed, pre, gnss=True, gnss_kw=gkw, **kw).finalize()
        if kind == "single":
            w["para_rcv_dt"] = w["para_rcv_dt"] + CLOCK_OFFSET
        _made[name] = w
    return _made[name].copy()


def max_gnss_of(name):
    return max(1, int(window_of(name)["n_gnss"]))


# ---------------------------------------------------------------- the branch decisions of gf_gnss_models.hpp, restated
A, E2, PI = 6378137.0, 6.69437999014e-3, np.pi


def _ecef2geo(p):
    a2 = A * A; b2 = a2 * (1 - E2); b = np.sqrt(b2); ep2 = (a2 - b2) / b2; rho = np.hypot(p[0], p[1])
    s1, s2 = p[2] * A, rho * b
    h = np.hypot(s1, s2)
    st, ct = s1 / h, s2 / h
    s1, s2 = p[2] + ep2 * b * st ** 3, rho - A * E2 * ct ** 3
    h = np.hypot(s1, s2)
    sl, cl = s1 / h, s2 / h
    N = a2 / np.sqrt(a2 * cl * cl + b2 * sl * sl)
    return np.array([np.degrees(np.arctan(s1 / s2)), np.degrees(np.arctan2(p[1], p[0])), rho / cl - N])


def _rot(lla):
    lat, lon = np.radians(lla[0]), np.radians(lla[1])
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    return np.array([[-so, -sl * co, cl * co], [co, -sl * so, cl * so], [0, cl, sl]])


DEFAULT_TABLE = np.array([0.1118e-07, -0.7451e-08, -0.5961e-07, 0.1192e-06, 0.1167e+06, -0.2294e+06, -0.1311e+06, 0.1049e+07])
HEIGHT_SWITCHES = (-1000.0, -100.0, 0.0, 1e4)


def factor_census(w, k):
    """classes and distances from the switches of observation k of a finalized window"""
    lo, ratio = int(w["gnss_lower"][k]), float(w["gnss_ratio"][k])
    d = w["gnss_data"][16 * k:16 * k + 16]
    P = ratio * w["para_Pose"][7 * lo:7 * lo + 3] + (1 - ratio) * w["para_Pose"][7 * lo + 7:7 * lo + 10]
    anc, yaw = w["para_anc_ecef"], float(w["para_yaw_enu_local"][0])
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
    Pe = _rot(_ecef2geo(anc)) @ Rz @ P + anc
    lla = _ecef2geo(Pe)
    dl = d[0:3] - Pe
    dl = dl / np.linalg.norm(dl)
    enu = _rot(lla).T @ dl
    az0 = np.arctan2(enu[0], enu[1])
    az = az0 + 2 * PI if az0 < 0 else az0
    el = np.arcsin(enu[2])
    hgt, tow = lla[2], d[14]
    c = {"lat_sign": "north" if lla[0] > 0 else "south", "lon_sign": "east" if lla[1] > 0 else "west", "az_wrapped": bool(az0 < 0),
         "el_class": "<=0" if el <= 0 else "(0,5deg]" if el <= np.radians(5.0) else ">5deg",
         "trop_height": "<-100" if hgt < -100 else "[-100,0)" if hgt < 0 else "[0,1e4]" if hgt <= 1e4 else ">1e4",
         "ion_height": "<-1000" if hgt < -1000 else ">=-1000"}
    m = {"el": abs(el), "height": min(abs(hgt - s) for s in HEIGHT_SWITCHES)}
    c["trop"] = "zero" if (hgt < -100 or hgt > 1e4 or el <= 0) else "clamped_height" if hgt < 0 else "model"
    if hgt < -1000 or el <= 0:
        c["ion"] = "zero"
        return c, m
    tab = np.asarray(w["gnss_iono"], np.float64)
    c["table"] = "default" if float(tab @ tab) <= 0 else "given"
    ion = DEFAULT_TABLE if c["table"] == "default" else tab
    psi = 0.0137 / (el / PI + 0.11) - 0.022
    phi = lla[0] / 180 + psi * np.cos(az)
    c["phi_clamp"] = "upper" if phi > 0.416 else "lower" if phi < -0.416 else "none"
    m["phi"] = abs(abs(phi) - 0.416)
    phi = min(max(phi, -0.416), 0.416)
    lam = lla[1] / 180 + psi * np.sin(az) / np.cos(phi * PI)
    phi += 0.064 * np.cos((lam - 1.617) * PI)
    tt = 43200 * lam + tow
    c["tt_sign"] = "negative" if tt < 0 else "positive"
    q = tt / 86400
    m["tt_wrap"] = abs(q - np.round(q))
    tt -= np.floor(q) * 86400
    terms = [ion[0], phi * ion[1], phi * phi * ion[2], phi ** 3 * ion[3]]
    amp, per = sum(terms), ion[4] + phi * (ion[5] + phi * (ion[6] + phi * ion[7]))
    c["amp_clamp"], c["per_clamp"] = bool(amp < 0), bool(per < 72000)
    m["amp_rel"], m["per"] = abs(amp) / max(abs(t) for t in terms), abs(per - 72000)
    x = 2 * PI * (tt - 50400) / max(per, 72000.0)
    c["ion"] = "day" if abs(x) < 1.57 else "night"
    m["x"] = abs(abs(x) - 1.57)
    c["x"] = float(x)
    return c, m


# what every factor of every case must keep from the switches, so that double and 60-digit arithmetic take the same branch
MARGINS = {"x": 1e-3, "el": 1e-4, "phi": 1e-6, "per": 1.0, "amp_rel": 1e-3, "height": 1.0, "tt_wrap": 1e-9}
CLASS_KEYS = ("ion", "trop", "table", "phi_clamp", "amp_clamp", "per_clamp", "tt_sign", "trop_height", "ion_height", "el_class", "lat_sign", "lon_sign", "az_wrapped")


def census_of_window(w):
    """per factor: the classes, counted; the smallest distance from each switch; the Klobuchar phase x (its range).  Per window: ng, the (frame, lower) groups, their sizes,
    the constellations absent per group and from the window, the frames without observations, the rcv_dt columns no observation feeds"""
    ng, NP = int(w["n_gnss"]), int(w["W"]) + 1
    counts = {k: {} for k in CLASS_KEYS}
    margins, xs = {}, []
    for k in range(ng):
        c, m = factor_census(w, k)
        for key in CLASS_KEYS:
            if key in c:
                v = str(c[key]).lower() if isinstance(c[key], bool) else c[key]
                counts[key][v] = counts[key].get(v, 0) + 1
        for key, v in m.items():
            margins[key] = min(margins.get(key, np.inf), float(v))
        if "x" in c:
            xs.append(c["x"])
    groups = {}
    for k in range(ng):
        groups.setdefault((int(w["gnss_frame"][k]), int(w["gnss_lower"][k])), []).append(int(w["gnss_sys"][k]))
    sizes, absent = {}, {}
    for mem in groups.values():
        sizes[str(len(mem))] = sizes.get(str(len(mem)), 0) + 1
        n_abs = 4 - len(set(mem))
        absent[str(n_abs)] = absent.get(str(n_abs), 0) + 1
    fed = {(int(w["gnss_frame"][k]), int(w["gnss_sys"][k])) for k in range(ng)}
    frames = {int(f) for f in w["gnss_frame"]}
    return {"ng": ng, "passes_of_256": (ng + 255) // 256, "groups": len(groups), "group_sizes": dict(sorted(sizes.items(), key=lambda kv: int(kv[0]))),
            "groups_by_constellations_absent": dict(sorted(absent.items())), "constellations_absent_from_window": sorted(set(range(4)) - {int(s) for s in w["gnss_sys"]}),
            "frames_without_observations": sorted(set(range(NP)) - frames), "rcv_dt_columns_without_observation": 4 * NP - len(fed),
            "classes": {k: dict(sorted(v.items())) for k, v in counts.items()}, "min_distance_from_switch": {k: float("%.6g" % v) for k, v in sorted(margins.items())},
            "x_range": [float("%.4f" % min(xs)), float("%.4f" % max(xs))] if xs else None}


def census_of(case, pre=None):
    return census_of_window(window_of(case, pre))


# every class the new cases must take between them (the old inputs take the first of each line only)
REQUIRED = {"ion": ("day", "night", "zero"), "trop": ("model", "clamped_height", "zero"), "table": ("given", "default"), "phi_clamp": ("none", "upper", "lower"),
            "amp_clamp": ("false", "true"), "per_clamp": ("false", "true"), "tt_sign": ("positive", "negative"), "trop_height": ("[0,1e4]", "<-100", "[-100,0)", ">1e4"),
            "ion_height": (">=-1000", "<-1000"), "el_class": (">5deg", "<=0", "(0,5deg]"), "lat_sign": ("north", "south"), "lon_sign": ("east", "west"), "az_wrapped": ("false", "true")}


def census_document(pre=None, measured=None):
    """the file profiles/gnss_model_census.json: the census of every case here, of the windows the suite had, and the union of the classes of each.  measured: the oracle's distance from each new 60-digit
    fixture, which only the fixture generator computes (tests/golden/make_ref_golden.py gnss_hard writes it when it writes the fixture); recomputing the census carries
    that block over from the committed file unchanged"""
    import synth_window as SW
    if pre is None:
        import oracle_py as pre
    doc = {"about": "branch census of the GNSS factor models (tests/gnss_hard_cases.py census_of): classes taken and the smallest distance from each switch, per case",
           "margins_required": MARGINS, "cases": {k: census_of(k, pre) for k in CASES}, "single_factor_windows": {k: census_of(k, pre) for k in SINGLES}, "inputs_before": {}}
    for name, (seed, kw) in OLD_INPUTS.items():
        doc["inputs_before"][name] = census_of_window(SW.make_window(seed, pre, gnss=True, **kw).finalize())

    def union(group):
        out = {k: set() for k in CLASS_KEYS}
        for c in group.values():
            for k in CLASS_KEYS:
                out[k] |= set(c["classes"][k])
        return {k: sorted(v) for k, v in out.items()}
    doc["classes_taken"] = {"cases": union(doc["cases"]), "inputs_before": union(doc["inputs_before"])}
    doc["measured"] = measured if measured is not None else committed().get("measured", {})
    return doc


CENSUS_PATH = os.path.join(ROOT, "profiles", "gnss_model_census.json")


def committed():
    if not os.path.exists(CENSUS_PATH):
        return {}
    with open(CENSUS_PATH) as f:
        return json.load(f)


def write(doc):
    with open(CENSUS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    doc = census_document()
    write(doc)
    print(json.dumps(doc["classes_taken"], indent=1))
    for name, c in list(doc["cases"].items()) + list(doc["single_factor_windows"].items()):
        print(name, "ng", c["ng"], "groups", c["groups"], c["group_sizes"], "x", c["x_range"], c["min_distance_from_switch"])
