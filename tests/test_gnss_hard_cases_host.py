"""CPU tests of the GNSS hard cases (tests/gnss_hard_cases.py): the branch census as a condition on the INPUTS, the CPU oracle against the new 60-digit fixtures
(tests/golden/ref_window_gnss_<case>, ref_marg_old_gnss_<case>, ref_solve_gnss_south_west_low) at the bars tests/test_golden.py holds for the older GNSS fixtures, and
csrc/gf_gnss_models.hpp as the estimator's host code compiles it (tests/native/gnss_models_host.hip, a stand-alone program, also under the address and
undefined-behaviour sanitizers) against the models at 60 digits.  No GPU needed."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import gnss_hard_cases as GH
import synth_window as SW
from test_golden import load_ref_window, load_ref_marg, check_against_ref, check_prior_against_ref, check_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def census(oracle):
    return GH.census_document(oracle)


def test_census_is_the_committed_one_and_takes_every_class(census):
    """profiles/gnss_model_census.json is its own recomputation; the new cases take every class of every switch between them, each factor at the required distance from
    every switch (so double and 60-digit arithmetic decide alike); the inputs the suite had take the first class of each and nothing else (either azimuth sign excepted)"""
    with open(GH.CENSUS_PATH) as f:
        committed = json.load(f)
    assert committed == json.loads(json.dumps(census)), "profiles/gnss_model_census.json differs from its recomputation (python tests/gnss_hard_cases.py rewrites it)"
    taken, before = census["classes_taken"]["cases"], census["classes_taken"]["inputs_before"]
    for key, classes in GH.REQUIRED.items():
        assert set(classes) <= set(taken[key]), (key, taken[key])
        if key != "az_wrapped":
            assert before[key] == [classes[0]], (key, before[key])
    for name, c in list(census["cases"].items()) + list(census["single_factor_windows"].items()):
        for key, least in GH.MARGINS.items():
            if key in c["min_distance_from_switch"]:
                assert c["min_distance_from_switch"][key] >= least, (name, key, c["min_distance_from_switch"][key])
    # list shapes of ba_linearize_gnss
    cs = census["cases"]
    assert cs["polar_north_352"]["ng"] == 352 and cs["polar_north_352"]["passes_of_256"] == 2
    th = cs["night_thinned"]
    assert th["frames_without_observations"] == [4] and th["constellations_absent_from_window"] == [3] and th["group_sizes"].get("1", 0) >= 1
    assert th["rcv_dt_columns_without_observation"] >= 11 and th["groups_by_constellations_absent"].get("3", 0) >= 1     # a group with one constellation: item_local is -1 for three clock columns
    assert cs["marg_frame0_empty"]["frames_without_observations"] == [0] and cs["marg_frame0_only"]["frames_without_observations"] == list(range(1, 11))
    assert all(census["single_factor_windows"][k]["ng"] == 1 for k in GH.SINGLE_CASES)
    for key, classes in GH.REQUIRED.items():      # one factor of each Klobuchar / Saastamoinen class stands alone in a window
        if key in ("ion", "trop", "table", "phi_clamp", "amp_clamp", "per_clamp", "tt_sign", "trop_height", "ion_height", "el_class"):
            assert set(classes) <= {k for c in census["single_factor_windows"].values() for k in c["classes"][key]}, key
    for c in census["inputs_before"].values():
        assert c["passes_of_256"] == 1 and not c["frames_without_observations"] and not c["constellations_absent_from_window"] and "1" not in c["group_sizes"]
        assert c["rcv_dt_columns_without_observation"] == 0


def test_the_parameters_of_add_gnss_leave_every_older_window_as_it_was(oracle):
    """the window stored in tests/golden/ref_window_gnss (made before add_gnss had parameters) comes out of make_window bit for bit, with and without the defaults spelled out"""
    stored = load_ref_window("ref_window_gnss")[0]
    spelled = dict(sats_per_sys=3, lat=31.03, lon=121.44, alt=20.0, yaw=0.3, tow0=345600.0, iono=SW.IONO, el_range=(32.0, 80.0), visible=None)
    for kw in (None, spelled, dict(visible=lambda i, s, q: True)):
        w = SW.make_window(11, oracle, gnss=True, gnss_kw=kw, **GH.SMALL).finalize()
        for k in ("gnss_frame", "gnss_lower", "gnss_sys", "gnss_ratio", "gnss_data", "gnss_iono", "gnss_headers", "para_rcv_dt", "para_rcv_ddt", "para_yaw_enu_local", "para_anc_ecef",
                  "para_Pose", "para_SpeedBias"):
            assert np.array_equal(np.asarray(w[k]), np.asarray(stored[k])), k
    # an observation a visibility rule leaves out takes nothing from the ones that stay
    full = SW.make_window(21, oracle, gnss=True, gnss_kw=dict(GH.NIGHT), **GH.SMALL).finalize()
    thin = GH.window_of("night_thinned", oracle)
    keep = [k for k in range(full["n_gnss"]) if GH.thinned(int(full["gnss_frame"][k]), int(full["gnss_sys"][k]), k % 12 % 3)]
    assert np.array_equal(thin["gnss_data"].reshape(-1, 16), full["gnss_data"].reshape(-1, 16)[keep]) and np.array_equal(thin["gnss_ratio"], full["gnss_ratio"][keep])


def test_fixtures_hold_the_windows_of_the_table(oracle):
    """every new fixture stores the window tests/gnss_hard_cases.py makes today (the GPU tests take the windows from either)"""
    for name in GH.WINDOW_CASES + GH.SINGLE_CASES:
        stored, now = load_ref_window("ref_window_gnss_" + name)[0], GH.window_of(name, oracle)
        for k in ("gnss_frame", "gnss_lower", "gnss_sys", "gnss_ratio", "gnss_data", "gnss_iono", "para_rcv_dt", "para_anc_ecef", "para_Pose", "imu_delta_p", "vis_pts_j"):
            assert np.array_equal(np.asarray(stored[k]), np.asarray(now[k])), (name, k)


@pytest.mark.parametrize("name", GH.WINDOW_CASES + GH.SINGLE_CASES)
def test_oracle_meets_the_reference_formulas_at_60_digits(oracle, name):
    """the bar of test_golden.test_oracle_meets_the_reference_formulas_at_60_digits (1e-11, H scaled by its diagonal, g by its largest entry), on every new window"""
    w, fx, H, g = load_ref_window("ref_window_gnss_" + name)
    dev = check_against_ref(oracle.ba_linearize(w), fx, H, g)
    print(name, "oracle vs reference formulas at 60 digits: H scaled %.1e, g %.1e" % dev)


@pytest.mark.parametrize("name", GH.SINGLE_CASES)
def test_single_factor_fixtures_are_consistent(oracle, name):
    """the terms stored for the factor's own columns add up to the fixture's g there, and the factor's r and J give the factor's own terms; the pseudorange residual is
    large enough for a bar of 1e-11 of a term to lie above the rounding of a 2.5e7-m range (gnss_hard_cases.CLOCK_OFFSET); the oracle's distance in those columns,
    relative to the sum of the absolute terms, is printed (profiles/gnss_model_census.json keeps it: 4e-14 .. 1.5e-12)"""
    w, fx, H, g = load_ref_window("ref_window_gnss_" + name)
    fac = fx["factor"]
    lin = oracle.ba_linearize(w)
    assert len(fac["own_columns"]) >= 5
    pr_weight = fac["J"][0][12]
    assert abs(fac["r"][0] / pr_weight) > 1700.0        # metres of pseudorange residual: 1e-11 of it is more than the 1.7e-8 m double precision places it to
    for c in fac["own_columns"]:
        assert fx["ids"][c["column"] - c["offset"]] == c["block"]
        assert abs(g[c["column"]] - c["g"]) <= 1e-15 * c["abs_sum"] and abs(sum(c["terms"]) - c["g"]) <= 1e-14 * c["abs_sum"]
        kind = c["block"] // 4096
        lc = 12 if kind == 10 else 13 if kind == 11 else 14 if kind == 12 else 15 + c["offset"]
        own = [fac["J"][row][lc] * fac["r"][row] for row in range(2)]
        assert np.allclose(own, c["terms"][:2], rtol=1e-14, atol=0)
        print(name, "column", c["block"], c["offset"], "oracle %.1e of the sum of absolute terms" % (abs(lin["g"][c["column"]] - c["g"]) / c["abs_sum"]))


@pytest.mark.parametrize("name", GH.MARG_CASES)
def test_oracle_marginalisation_meets_the_reference_route_at_60_digits(oracle, name):
    """MARGIN_OLD with frame 0 without GNSS observations, and with observations in frame 0 only: the bars of check_prior_against_ref for a GNSS window"""
    w, fx, A, b, ids = load_ref_marg("ref_marg_old_gnss_" + name[5:])
    dev = check_prior_against_ref(oracle.ba_marginalize(w, fx["mode"]), fx, A, b, ids)
    print(name, "oracle vs reference route at 60 digits: J^T J scaled %.1e, J^T r %.1e" % dev)


def test_oracle_solve_meets_the_loop_at_60_digits(oracle):
    """the low-elevation south-west window through the whole trust-region loop (tests/golden/ref_solve_gnss_south_west_low), check_solve's bars"""
    print("oracle vs the loop at 60 digits:", check_solve(lambda a: oracle.ba_solve(a, 8), "ref_solve_gnss_" + GH.SOLVE_CASE))


# ---------------------------------------------------------------- gf_gnss_models.hpp on the host
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "native", "gnss_models_host.hip")


@pytest.fixture(scope="module")
def model_tuples(tmp_path_factory):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "ref_gnss_models.json.gz"), "rt") as f:
        tuples = json.load(f)["tuples"]
    path = tmp_path_factory.mktemp("gnss_models") / "tuples.txt"
    with open(path, "w") as f:
        for t in tuples:
            f.write(" ".join(float(x).hex() for x in t["rcv"] + t["sat"] + [t["tow"]] + t["iono"]) + "\n")
    return tuples, str(path)


def _run(exe, path, n):
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "all: ok" and lines[-2] == "tuples: %d" % n
    return np.array([[float.fromhex(x) for x in ln.split()] for ln in lines[:n]])


def test_host_models_meet_the_models_at_60_digits(tmp_path, model_tuples):
    """built as the library builds the estimator's host code (-O3, no contraction).  Bars: 1e-12 relative on the two delays (a delay that is exactly 0 must come out 0),
    1e-12 on the rotation entries (of unit columns), 1e-12 on the direction cosines azimuth and elevation stand for.  Latitude and longitude are held to 1e-12 relative;
    the height is a difference of two 6.4e6-m numbers and is held to 1e-8 m."""
    tuples, path = model_tuples
    exe = str(tmp_path / "gnss_models_host")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC])
    got = _run(exe, path, len(tuples))
    worst = {"lat_lon": 0.0, "height": 0.0, "R": 0.0, "cosines": 0.0, "trop": 0.0, "ion": 0.0}
    classes = set()
    for t, o in zip(tuples, got):
        lla, R, az, el, trop, ion = o[0:3], o[3:12], o[12], o[13], o[14], o[15]
        worst["lat_lon"] = max(worst["lat_lon"], abs(lla[0] - t["lla"][0]) / abs(t["lla"][0]), abs(lla[1] - t["lla"][1]) / abs(t["lla"][1]))
        worst["height"] = max(worst["height"], abs(lla[2] - t["lla"][2]))
        worst["R"] = max(worst["R"], float(np.abs(R - np.array(t["R"])).max()))
        cos = np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)])
        worst["cosines"] = max(worst["cosines"], float(np.abs(cos - np.array(t["cosines"])).max()))
        assert 0 <= az < 2 * np.pi
        for key, v in (("trop", trop), ("ion", ion)):
            if t[key] == 0:
                assert v == 0, (t["case"], t["factor"], key, v)
            else:
                worst[key] = max(worst[key], abs(v - t[key]) / abs(t[key]))
        classes.add((t["trop"] == 0, t["ion"] == 0, t["el"] <= 0))
    print("host models vs 60 digits:", {k: "%.1e" % v for k, v in worst.items()})
    assert len(classes) >= 4
    assert worst["lat_lon"] < 1e-12 and worst["height"] < 1e-8 and worst["R"] < 1e-12 and worst["cosines"] < 1e-12 and worst["trop"] < 1e-12 and worst["ion"] < 1e-12, worst


def test_host_models_under_the_sanitizers(tmp_path, model_tuples):
    """the same program with -fsanitize=address,undefined on the host side: a stand-alone program, nothing is loaded into Python"""
    tuples, path = model_tuples
    exe = str(tmp_path / "gnss_models_host_san")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    _run(exe, path, len(tuples))
