"""The GNSS residual blocks on the device (csrc/gf_ba_gnss.hpp: gn_psr_dopp, ba_linearize_gnss; models in csrc/gf_gnss_models.hpp) on the windows of tests/gnss_hard_cases.py:
every branch of the Klobuchar and Saastamoinen models, both hemispheres, and the list shapes the kernel's phases can go wrong on (more than 256 factors, one factor,
an empty list, a frame without observations, groups of one, a constellation absent, a shorter list behind a longer one, a reversed list).  Against the CPU oracle, and
against the reference's formulas at 60 digits (tests/golden/ref_window_gnss_<case>, ref_marg_old_gnss_<case>, ref_solve_gnss_south_west_low).  Run with -m gpu."""
import numpy as np
import pytest

import gfwindow as gw
import gnss_hard_cases as GH
import synth_window as SW
from test_golden import load_ref_window, load_ref_marg, check_against_ref, check_prior_against_ref, check_solve

pytestmark = pytest.mark.gpu
F, NV = 16, 256          # the handle of the 60-digit tests of tests/test_backend_gpu.py


def _est(gf, max_gnss, batch=1):
    return gf.Estimator(max_features=F, max_visual=NV, batch=batch, max_gnss=max(1, max_gnss))


def _pose_diff(a, b):
    pa, pb = a["para_Pose"].reshape(-1, 7), b["para_Pose"].reshape(-1, 7)
    return np.abs(pa[:, :3] - pb[:, :3]).max(), 2 * min(np.abs(pa[:, 3:] - pb[:, 3:]).max(), np.abs(pa[:, 3:] + pb[:, 3:]).max())


def _lin_close(lo, lg, tol=1e-12):
    assert list(lo["ids"]) == list(lg["ids"]) and lo["n_f"] == lg["n_f"]
    dev = (abs(lo["cost"] - lg["cost"]) / lo["cost"], np.abs(lo["H"] - lg["H"]).max() / np.abs(lo["H"]).max(), np.abs(lo["g"] - lg["g"]).max() / np.abs(lo["g"]).max())
    print("cost %.1e  H %.1e  g %.1e (relative to the largest entry)" % dev)
    assert max(dev) <= tol, dev


def _solve_close(wo, so, wg, sg):
    assert (so["iterations"], so["successful_steps"]) == (sg["iterations"], sg["successful_steps"]), (so, sg)
    dp, dr = _pose_diff(wo, wg)
    dev = (dp, dr, np.abs(wo["para_rcv_dt"] - wg["para_rcv_dt"]).max(), np.abs(wo["para_rcv_ddt"] - wg["para_rcv_ddt"]).max(), np.abs(wo["para_anc_ecef"] - wg["para_anc_ecef"]).max())
    print("after the solve: position %.1e m, rotation %.1e rad, rcv_dt %.1e m, rcv_ddt %.1e m/s, anchor %.1e m" % dev)
    assert max(dev) < 1e-6, dev


def _same_lin(a, b):
    return a["cost"] == b["cost"] and np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"]) and np.array_equal(a["ids"], b["ids"])


def _same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in gw.STATE_KEYS if k in a)


@pytest.fixture(scope="module")
def oracle_results(oracle):
    """the oracle's linearisation and solve of every case, once"""
    made = {}

    def get(name):
        if name not in made:
            w = GH.window_of(name, oracle)
            a = w.copy()
            made[name] = (oracle.ba_linearize(w.copy(), cap=1024), a, oracle.ba_solve(a, 8))
        return made[name]
    return get


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", list(GH.CASES))
def test_normal_equations_and_solve_match_oracle(gf, oracle, oracle_results, name):
    """every case of the table at the bars of test_backend_gpu.test_gnss_normal_equations_and_solve_match_oracle: H, g, cost within 1e-12 (relative to the largest entry),
    then the same iterations and accepted steps over 8 iterations, poses, clocks and anchor within 1e-6 (measured on an MI355X: cost 1e-13, H 2e-16, g 3e-15; positions
    1e-9 m, clocks and anchor 6e-9 m at the most)"""
    w = GH.window_of(name, oracle)
    lo, wo, so = oracle_results(name)
    est = _est(gf, w["n_gnss"])
    _lin_close(lo, est.linearize(w.copy(), cap=1024))
    wg = w.copy()
    _solve_close(wo, so, wg, est.solve([wg], 8)[0])
    est.close()


@pytest.mark.parametrize("name", GH.SINGLE_CASES)
def test_single_factor_windows_match_oracle(gf, oracle, oracle_results, name):
    """The single-factor windows are not cases of the table (they are one factor of a case each, made for the comparison of g's columns below), but they go the same way:
    H, g, cost within 1e-12 of the oracle's, the same iterations and accepted steps, poses and clocks within 1e-6.  The anchor is not compared: one pseudorange is all
    that sees it, J_anc = -unit * weight beside J_rcv_dt = weight, so H has rank 1 in the three anchor columns, nothing across the line of sight, and along it only the
    sum with a clock bias whose chain of clock factors has a free common offset; the dogleg's mu D^2 term (1e-8 x the 1e-6 floor of D^2) alone bounds the anchor's step
    and turns the last bits of g into metres.  Where the anchor ends is printed (measured: 4e-8 .. 1.1e-6 m along the line of sight, 3e-5 .. 7e-4 m across it); no
    number follows from the formulas for it.  The eight cases of the table, whose lists observe the anchor, hold all three components to 1e-6 above."""
    w = GH.window_of(name, oracle)
    lo, wo, so = oracle_results(name)
    est = _est(gf, 1)
    _lin_close(lo, est.linearize(w.copy(), cap=1024))
    wg = w.copy()
    sg = est.solve([wg], 8)[0]
    est.close()
    assert (so["iterations"], so["successful_steps"]) == (sg["iterations"], sg["successful_steps"]), (so, sg)
    unit = w["gnss_data"][0:3] - w["para_anc_ecef"]
    unit = unit / np.linalg.norm(unit)
    d_anc = wo["para_anc_ecef"] - wg["para_anc_ecef"]
    along = abs(float(unit @ d_anc))
    dp, dr = _pose_diff(wo, wg)
    dev = (dp, dr, np.abs(wo["para_rcv_dt"] - wg["para_rcv_dt"]).max(), np.abs(wo["para_rcv_ddt"] - wg["para_rcv_ddt"]).max())
    print("after the solve: position %.1e m, rotation %.1e rad, rcv_dt %.1e m, rcv_ddt %.1e m/s; anchor along the line of sight %.1e m, across it %.1e m"
          % (dev + (along, float(np.linalg.norm(d_anc - unit * (unit @ d_anc))))))
    assert max(dev) < 1e-6, dev


# ---------------------------------------------------------------- against the reference's formulas at 60 digits
@pytest.mark.parametrize("name", GH.WINDOW_CASES + GH.SINGLE_CASES)
def test_normal_equations_meet_the_reference_formulas_at_60_digits(gf, name):
    w, fx, H, g = load_ref_window("ref_window_gnss_" + name)
    est = _est(gf, w["n_gnss"])
    dev = check_against_ref(est.linearize(w, cap=1024), fx, H, g, tol=1e-11)
    print(name, "HIP vs reference formulas at 60 digits: H scaled %.1e, g %.1e" % dev)
    est.close()


@pytest.mark.parametrize("name", GH.MARG_CASES)
def test_marginalisation_meets_the_reference_route_at_60_digits(gf, name):
    """MARGIN_OLD (frame_filter 1) with frame 0 without GNSS observations -- the kernel's phases A and B skip every item, the clock factors of the pair (0, 1) stay -- and
    with observations in frame 0 only"""
    w, fx, A, b, ids = load_ref_marg("ref_marg_old_gnss_" + name[5:])
    est = _est(gf, w["n_gnss"])
    dev = check_prior_against_ref(est.marginalize([w], fx["mode"])[0], fx, A, b, ids)
    print(name, "HIP vs reference route at 60 digits: J^T J scaled %.1e, J^T r %.1e" % dev)
    est.close()


def test_solve_meets_the_loop_at_60_digits(gf):
    est = _est(gf, 132)
    print("HIP vs the loop at 60 digits:", check_solve(lambda a: est.solve([a], 8)[0], "ref_solve_gnss_" + GH.SOLVE_CASE))
    est.close()


@pytest.mark.parametrize("name", GH.SINGLE_CASES)
def test_single_factor_columns_of_g_meet_the_factor_at_60_digits(gf, name):
    """The window's list holds one GnssPsrDoppFactor.  Every entry of g in the columns only GNSS blocks feed -- the factor's rcv_dt and rcv_ddt, the three anchor columns,
    yaw_enu_local where it is a column -- against the sum of J_k,col r_k over the factor's two rows and the clock factors' rows, all from the fixture's 60-digit values.
    Tolerance: 1e-11 of the sum of the absolute terms of the entry (not of max |g|, under which a low-weight factor hides).

    The pseudorange residual of these windows is 5 km (gnss_hard_cases.CLOCK_OFFSET): double precision places a difference of 2.5e7-m numbers to ~1.7e-8 m, so 1e-11
    of the term is a bar the arithmetic can meet, and it still asks for 5e-8 m.  The CPU oracle sits at 4e-14 .. 1.5e-12."""
    w, fx, H, g = load_ref_window("ref_window_gnss_" + name)
    est = _est(gf, 1)
    lin = est.linearize(w, cap=1024)
    est.close()
    assert [int(x) for x in lin["ids"]] == fx["ids"]
    worst = {}
    for c in fx["factor"]["own_columns"]:
        dev = abs(lin["g"][c["column"]] - c["g"]) / c["abs_sum"]
        print(name, "block", c["block"], "offset", c["offset"], "%.1e of the sum of absolute terms (%d terms)" % (dev, len(c["terms"])))
        worst[(c["block"], c["offset"])] = dev
    assert max(worst.values()) <= 1e-11, worst


# ---------------------------------------------------------------- list shapes in one handle
def _empty_list_window(oracle):
    return SW.make_window(41, oracle, gnss=True, gnss_kw=dict(visible=lambda i, s, q: False), **GH.SMALL).finalize()


def _run_all(est, wins):
    """linearisation of each window, then solve and MARGIN_OLD of the batch: everything the GNSS kernel has a hand in"""
    lins = [est.linearize(w.copy(), cap=1024) for w in wins]
    ws = [w.copy() for w in wins]
    sums = est.solve(ws, 8)
    pri = est.marginalize(ws, 0)
    return lins, ws, sums, pri


def _same_run(a, b):
    return (all(_same_lin(x, y) for x, y in zip(a[0], b[0])) and all(_same_state(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]
            and all(np.array_equal(p["J"], q["J"]) and np.array_equal(p["r"], q["r"]) and np.array_equal(p["block_id"], q["block_id"]) for p, q in zip(a[3], b[3])))


def test_four_list_shapes_in_one_launch_give_the_bits_of_each_alone(gf, oracle):
    """352 factors (two passes of phase A), one factor, GNSS enabled with an empty list, GNSS disabled: one batch, every window as it comes out alone in a fresh handle"""
    wins = [GH.window_of("polar_north_352", oracle), GH.window_of("one_day", oracle), _empty_list_window(oracle), SW.make_window(42, oracle, **GH.SMALL).finalize()]
    assert [int(w["n_gnss"]) for w in wins] == [352, 1, 0, 0] and [int(w["gnss_enabled"]) for w in wins] == [1, 1, 1, 0]
    est = _est(gf, 352, batch=4)
    lins = [est.linearize(w.copy(), cap=1024) for w in wins]
    ws = [w.copy() for w in wins]
    sums = est.solve(ws, 8)
    pri = est.marginalize(ws, 0)
    est.close()
    for b, w in enumerate(wins):
        alone = _est(gf, 352, batch=4)
        ref = _run_all(alone, [w])
        alone.close()
        assert _same_run(([lins[b]], [ws[b]], [sums[b]], [pri[b]]), ref), b
    # the empty list is not the disabled window: its clock factors are there
    assert gw.bid(gw.RCV_DT, 5) in lins[2]["ids"] and gw.bid(gw.RCV_DT, 5) not in lins[3]["ids"]
    lo = oracle.ba_linearize(wins[2].copy(), cap=1024)
    _lin_close(lo, lins[2])


def test_a_shorter_list_behind_a_longer_one_and_a_second_run(gf, oracle):
    """the 352-factor window, then the thinned one in the same slot (gn_rows, gn_gptr, gn_gitem keep the longer list's tail): the bits of the thinned window in a fresh
    handle; and the same window twice in one handle: the same bits"""
    big, thin = GH.window_of("polar_north_352", oracle), GH.window_of("night_thinned", oracle)
    est = _est(gf, 352)
    first = _run_all(est, [big])
    behind = _run_all(est, [thin])
    again = _run_all(est, [thin])
    est.close()
    fresh = _est(gf, 352)
    ref = _run_all(fresh, [thin])
    ref_big = _run_all(fresh, [big])
    fresh.close()
    assert _same_run(behind, ref) and _same_run(again, ref) and _same_run(first, ref_big)


def test_reversed_list_keeps_the_normal_equations(gf, oracle, oracle_results):
    """the observations in reversed order: groups follow the (frame, lower) key, not the position in the list; H, g and cost stay within the oracle bar of the window as
    it was (the sums inside a group run in another order, so not the same bits)"""
    for name in ("night_thinned", "polar_north_352"):
        w = GH.window_of(name, oracle)
        r = w.copy()
        for k, width in (("gnss_frame", 1), ("gnss_lower", 1), ("gnss_sys", 1), ("gnss_ratio", 1), ("gnss_data", 16)):
            r[k] = np.ascontiguousarray(w[k].reshape(-1, width)[::-1]).reshape(-1)
        est = _est(gf, 352)
        _lin_close(oracle_results(name)[0], est.linearize(r, cap=1024))
        est.close()


# ---------------------------------------------------------------- the kept variants of the step
@pytest.mark.parametrize("variant", ["four_wavefronts", "global_W20"])
@pytest.mark.parametrize("name", ["polar_north_352", "south_west_low"])
def test_step_variants_solve_as_the_oracle(gf, oracle, oracle_results, monkeypatch, name, variant):
    """the variants of ba_step a GNSS handle can take: four wavefronts (GF_BA_STEP_WAVES=4, read when the handle is created) and the reduced system in global memory (a
    20-frame window has 440 reduced columns whatever its feature count: the shapes of test_config5_window_with_gnss cut to 64 features; 336 and 252 factors).  The
    oracle's iterations and accepted steps, within 1e-6 of it.  The chain form is not among them: a handle with max_gnss > 0 never takes it (gf_ba_create), see the test below."""
    monkeypatch.delenv("GF_BA_CHAIN", raising=False)
    if variant == "global_W20":
        seed, _, gkw, _ = GH.CASES[name]
        gkw = dict(gkw, sats_per_sys=4) if name == "polar_north_352" else gkw
        w = SW.make_window(seed, oracle, W=20, n_landmarks=96, max_features=64, gnss=True, gnss_kw=gkw).finalize()
        assert w["n_gnss"] == (336 if name == "polar_north_352" else 252)
        wo = w.copy()
        so = oracle.ba_solve(wo, 8)
        est = gf.Estimator(20, 64, 64 * 20, 1, max_gnss=int(w["n_gnss"]))
    else:
        monkeypatch.setenv("GF_BA_STEP_WAVES", "4")
        w = GH.window_of(name, oracle)
        _, wo, so = oracle_results(name)
        est = _est(gf, w["n_gnss"])
    wg = w.copy()
    _solve_close(wo, so, wg, est.solve([wg], 8)[0])
    est.close()


def test_chain_switch_is_inert_for_gnss_handles(gf, oracle, monkeypatch):
    """GF_BA_CHAIN=1 on a handle with max_gnss > 0 changes nothing (gf_ba_create: the chain form is taken only without GNSS columns): linearisation, solve and prior of the
    352-factor and the low-elevation window have the bits they have without the switch.  So a suite run under GF_BA_CHAIN=1 runs every GNSS test in the dense form."""
    wins = [GH.window_of("polar_north_352", oracle), GH.window_of("south_west_low", oracle)]
    runs = []
    for on in (False, True):
        if on:
            monkeypatch.setenv("GF_BA_CHAIN", "1")
        else:
            monkeypatch.delenv("GF_BA_CHAIN", raising=False)
        est = _est(gf, 352, batch=2)
        runs.append(_run_all(est, wins))
        est.close()
    assert _same_run(runs[0], runs[1])
