"""ba_step keeps the solver state (and what its vector phases hand each other) on chip for the life of a launch: the places where an operand now crosses a
phase through LDS or registers instead of global memory, each on a batch of tiny windows (W = 3, 12 features: the best-conditioned
size of the range the cases were asked for), held to the CPU oracle on what the solver
tests of test_backend_gpu.py compare, and to itself run twice (bits).  Every case asserts from the ORACLE's summary that the oracle takes the branch the case
is named after, so that a case cannot pass on another path.  Run with -m gpu.

The oracle's summary has no field for a mu retry (a failed Cholesky): that branch is established from the oracle's own normal equations
(_first_factorisation); a rejection is told from an invalid step by the oracle's radius (_oracle_rejections)."""
import numpy as np
import pytest
import gfwindow as gw
import synth_window as SW

pytestmark = pytest.mark.gpu

W, F, ITERS = 3, 12, 8


def _win(oracle, seed, **kw):
    return SW.make_window(seed, oracle, W=W, n_landmarks=3 * F, max_features=F, **kw)


def _pose_diff(a, b):
    pa, pb = a["para_Pose"].reshape(-1, 7), b["para_Pose"].reshape(-1, 7)
    dp = np.abs(pa[:, :3] - pb[:, :3]).max()
    dq = min(np.abs(pa[:, 3:] - pb[:, 3:]).max(), np.abs(pa[:, 3:] + pb[:, 3:]).max())
    return dp, 2 * dq


def _solve_both(gf, oracle, wins, iters=ITERS):
    """the batch on the oracle (window by window) and twice on the GPU (two handles): summaries and solved windows"""
    ref = [w.copy() for w in wins]
    so = [oracle.ba_solve(w, iters) for w in ref]
    runs = []
    for rep in range(2):
        est = gf.Estimator(W, F, F * W, batch=len(wins))
        mine = [w.copy() for w in wins]
        runs.append((mine, est.solve(mine, iters)))
        est.close()
    return ref, so, runs


def _hold_to_oracle(ref, so, runs):
    (g0, s0), (g1, s1) = runs
    for a, b, sa, sb in zip(g0, g1, s0, s1):   # the same bits from two handles
        for k in gw.STATE_KEYS:
            assert np.array_equal(a[k], b[k]), k
        assert sa == sb
    for wo, wg, o, g in zip(ref, g0, so, s0):
        dp, dr = _pose_diff(wo, wg)
        print("oracle", (o["iterations"], o["successful_steps"], o["termination"]), "gpu", (g["iterations"], g["successful_steps"], g["termination"]),
              "cost rel %.3g" % (abs(g["final_cost"] - o["final_cost"]) / max(o["final_cost"], 1e-300)), "dp %.3g dr %.3g" % (dp, dr))
        assert (g["iterations"], g["successful_steps"], g["termination"]) == (o["iterations"], o["successful_steps"], o["termination"])
        assert abs(g["final_cost"] - o["final_cost"]) <= 1e-8 * max(o["final_cost"], 1e-300)
        dp, dr = _pose_diff(wo, wg)
        assert dp < 1e-6 and dr < 1e-6, (dp, dr)
        for k in ("para_SpeedBias", "para_Feature", "para_Ex_Pose", "para_Ex_Pose_wheel"):
            assert (np.abs(wo[k] - wg[k]) / np.maximum(1.0, np.abs(wo[k]))).max() < 1e-6, k


def _oracle_rejections(oracle, w, iters):
    """iterations the oracle REJECTS (not: finds invalid), from its summaries after 1 .. iters iterations: a rejection leaves the count of successful steps
    and halves the radius (exactly); an invalid step leaves both; an accepted one raises the count"""
    prev, out = oracle.ba_solve(w.copy(), 0), []
    for k in range(1, iters + 1):
        s = oracle.ba_solve(w.copy(), k)
        if s["iterations"] == k and s["successful_steps"] == prev["successful_steps"] and s["radius"] == 0.5 * prev["radius"]:
            out.append(k)
        prev = s
    return out


def _first_factorisation(oracle, w, mu=1e-8):
    """The oracle's first Gauss-Newton solve, redone from its own normal equations (ba_linearize): Jacobi scaling s = 1 / (1 + sqrt(H_jj)), dogleg diagonal
    D^2 = clamp(s^2 H_jj, 1e-6, 1e32), Schur complement of s H s + mu D^2 on the reduced columns, Cholesky with the oracle's test (a pivot that is not > 0 fails).
    Returns (succeeds, smallest pivot / its diagonal entry)."""
    lin = oracle.ba_linearize(w.copy())
    H, nf, ne = lin["H"], lin["n_f"], lin["n_e"]
    with np.errstate(all="ignore"):
        sc = 1.0 / (1.0 + np.sqrt(np.diag(H)))
        A = H * np.outer(sc, sc)
        A = A + mu * np.diag(np.clip(np.diag(A), 1e-6, 1e32))
        S = A[:nf, :nf] - A[nf:, :nf].T @ (A[nf:, :nf] / np.diag(A)[nf:, None]) if ne else A[:nf, :nf].copy()
        rel = np.inf
        for j in range(nf):
            d = S[j, j] - S[j, :j] @ S[j, :j]
            if not d > 0.0:
                return False, d / A[j, j]
            rel = min(rel, d / A[j, j])
            S[j, j] = np.sqrt(d)
            S[j + 1:, j] = (S[j + 1:, j] - S[j + 1:, :j] @ S[j, :j]) / S[j, j]
    return True, rel


def test_rejected_step_reuses_the_vectors_of_the_launch_before(gf, oracle):
    """a rejected step: the next launch takes the `reuse` path and reads the gradient, Gauss-Newton step, diagonal and scaling the launch before it left"""
    wins = [_win(oracle, s) for s in (1, 2, 3)]
    rej = [_oracle_rejections(oracle, w, ITERS) for w in wins]
    print("iterations the oracle rejects", rej)
    assert all(len(r) >= 2 and any(k < ITERS for k in r) for r in rej)   # rejections (not invalid steps), and a launch behind one of them
    ref, so, runs = _solve_both(gf, oracle, wins)
    assert all(o["iterations"] == ITERS and o["termination"] == 0 for o in so)
    _hold_to_oracle(ref, so, runs)


def test_unobservable_direction(gf, oracle):
    """Camera extrinsic free without a prior: its translation is barely observable.  The first factorisation does NOT fail here, and the test says so: every
    reduced system is J^T J (positive semi-definite) plus mu D^2 with D^2 its own clamped diagonal, so the smallest pivot stays near mu = 1e-8 of its diagonal
    entry (6e-8 over 180 windows of W = 3, 4 .. 12 features, extrinsics / td / intrinsics free or not) against a rounding error of 1e-14: no finite window of
    this kind makes the oracle retry.  The retry loop is taken in test_factorisation_fails_for_every_mu."""
    wins = [_win(oracle, s, fix_ex_pose=0) for s in (1, 5)]
    piv = [_first_factorisation(oracle, w) for w in wins]
    print("first factorisation (succeeds, smallest relative pivot)", piv)
    assert all(ok and 1e-9 < rel < 1e-6 for ok, rel in piv)   # nearly singular: held up by the damping alone
    ref, so, runs = _solve_both(gf, oracle, wins)
    assert all(o["iterations"] == ITERS for o in so)
    _hold_to_oracle(ref, so, runs)


def test_factorisation_fails_for_every_mu(gf, oracle):
    """The mu retry: a feature at infinity (inverse depth 1e-300: its column of the Jacobian overflows, the cost stays finite) makes the first Cholesky fail,
    and every retry after it -- the loop runs mu = 1e-8 .. 0.1 through the state's LDS copy in each of five launches, each step is invalid, mu goes on growing
    from launch to launch, and the solve ends with termination 4 and the state it came with.  Asserted on the oracle: its own first factorisation fails (redone
    from its normal equations), and its summary is five iterations, no successful step, termination 4.  Next to a window that solves normally."""
    far = _win(oracle, 1)
    far["para_Feature"] = far["para_Feature"].copy()
    far["para_Feature"][0] = 1e-300
    wins = [far, _win(oracle, 2)]
    assert not _first_factorisation(oracle, far)[0] and _first_factorisation(oracle, wins[1])[0]
    ref, so, runs = _solve_both(gf, oracle, wins)
    assert (so[0]["iterations"], so[0]["successful_steps"], so[0]["termination"]) == (5, 0, 4) and np.isfinite(so[0]["final_cost"])
    assert so[1]["iterations"] == ITERS
    _hold_to_oracle(ref, so, runs)
    for k in gw.STATE_KEYS:
        assert np.array_equal(runs[0][0][0][k], far[k]), k


def test_window_without_a_prior_and_every_step_accepted(gf, oracle):
    wins = [_win(oracle, 4)]
    assert len(wins[0]["prior_r"]) == 0
    ref, so, runs = _solve_both(gf, oracle, wins)
    assert (so[0]["iterations"], so[0]["successful_steps"], so[0]["termination"]) == (ITERS, ITERS, 0)
    _hold_to_oracle(ref, so, runs)


def test_ragged_column_counts(gf, oracle):
    """NE no multiple of four, R < 64: ten eliminated columns next to 60 reduced ones (no wheel factors)"""
    wins = [_win(oracle, 1, use_wheel=False)]
    lin = oracle.ba_linearize(wins[0].copy())
    assert lin["n_e"] % 4 != 0 and lin["n_f"] < 64
    ref, so, runs = _solve_both(gf, oracle, wins)
    _hold_to_oracle(ref, so, runs)


def test_finished_window_is_left_alone_by_later_launches(gf, oracle):
    """a batch of one window that ends at its first iteration by the function-tolerance rule (it starts from a converged state) and two that run every iteration"""
    conv = _win(oracle, 2)
    oracle.ba_solve(conv, 150)
    wins = [_win(oracle, 1), conv, _win(oracle, 3)]
    ref, so, runs = _solve_both(gf, oracle, wins)
    assert (so[1]["iterations"], so[1]["termination"]) == (1, 1) and so[0]["iterations"] == ITERS and so[2]["iterations"] == ITERS
    _hold_to_oracle(ref, so, runs)
    for k in gw.STATE_KEYS:   # the rejected-by-tolerance candidate is not taken: the window keeps the state it came with
        assert np.array_equal(runs[0][0][1][k], conv[k]), k


def _last_bit(w, rng):
    """the window with every pose, speed-bias and feature entry moved by at most one unit in the last place"""
    p = w.copy()
    for k in ("para_Pose", "para_SpeedBias", "para_Feature"):
        p[k] = p[k] * (1 + 2.2e-16 * rng.integers(-1, 2, p[k].shape))
    return p


def _oracle_cost_noise(oracle, w, iters, reps=6):
    """the oracle against itself: largest relative change of its final cost when its start moves in the last bit (inf if its step counts change)"""
    rng = np.random.default_rng(7)
    ref = oracle.ba_solve(w.copy(), iters)
    out = 0.0
    for _ in range(reps):
        s = oracle.ba_solve(_last_bit(w, rng), iters)
        if (s["iterations"], s["successful_steps"], s["termination"]) != (ref["iterations"], ref["successful_steps"], ref["termination"]):
            return np.inf
        out = max(out, abs(s["final_cost"] - ref["final_cost"]) / ref["final_cost"])
    return out


def _oracle_prior_noise(oracle, w, mode, reps=4):
    """the oracle against itself: largest change of its prior's J^T J (relative to its largest entry; entry by entry relative to sqrt(A_ii A_jj)) and of J^T r
    when the solved state moves in the last bit"""
    rng = np.random.default_rng(7)
    po = oracle.ba_marginalize(w, mode)
    n = po["n"]
    Jo = po["J"].reshape(n, n)
    Ao, bo = Jo.T @ Jo, Jo.T @ po["r"]
    sc = np.sqrt(np.outer(np.diag(Ao), np.diag(Ao))) + 1e-6 * np.abs(Ao).max()
    dA = dS = db = 0.0
    for _ in range(reps):
        pp = oracle.ba_marginalize(_last_bit(w, rng), mode)
        Jp = pp["J"].reshape(n, n)
        dA = max(dA, np.abs(Jp.T @ Jp - Ao).max() / np.abs(Ao).max())
        dS = max(dS, (np.abs(Jp.T @ Jp - Ao) / sc).max())
        db = max(db, np.abs(Jp.T @ pp["r"] - bo).max() / np.abs(bo).max())
    return dA, dS, db


@pytest.mark.parametrize("iters", [0, 1])
def test_first_and_closing_launch_only(gf, oracle, iters):
    """max_iters = 0: the first launch is the closing one; 1: first launch, one candidate, closing launch.
    After ONE dogleg step a 4-frame window is far from a minimum (cost 2e6 -> 1e2) and its cost follows the state's rounding to first order: the oracle
    itself, started one unit in the last place away, lands 1.5e-9 .. 4e-8 (relative) from its own cost over seeds 1 .. 60 -- above the 1e-8 bar for most of
    them (seed 2: 1.2e-8, where the solver measured 1.33e-8 from the oracle).  The windows are therefore chosen by the reference's own error, which the test
    asserts: at most half the bar (seeds 28 and 31 measure 2.0e-9 and 1.5e-9)."""
    wins = [_win(oracle, 28), _win(oracle, 31)]
    noise = [_oracle_cost_noise(oracle, w, iters) for w in wins]
    print("oracle's own cost noise", noise)
    assert max(noise) <= 0.5e-8
    ref, so, runs = _solve_both(gf, oracle, wins, iters=iters)
    assert all(o["iterations"] == iters for o in so)
    _hold_to_oracle(ref, so, runs)


def test_marginalisation_after_a_solve_on_the_same_handle(gf, oracle):
    """ba_marg_finish borrows the step's yv / u vectors as scratch: solves and both kinds of prior on one handle, held to the oracle's as in
    test_backend_gpu.py::test_marginalisation_matches_oracle.
    Which prior carries the numeric bars is decided by the reference's own error, asserted below.  MARGIN_OLD of a 4-frame window drops pose 0, its
    speed-bias and every feature (27 of 71 columns) through the eigen pseudo-inverse of that block: the oracle's own J^T J moves by 2.6e-9 .. 9e-8 of its largest
    entry when its solved state moves in the last bit (240 windows of W = 3, 4 .. 12 features, with and without wheel factors: none below the 1e-9 bar; this
    window 2e-8, where the solver measured 1.24e-8 from the oracle), so that prior is held to what is exact -- blocks, sizes, x0, the same bits twice --, to four times the
    reference's own error measured in the test (J^T J, its scaled entries, J^T r), and through the next window's solve, which takes the solver's prior.  MARGIN_SECOND_NEW of that next window (which carries a prior) is reproduced by the oracle to 1e-12: it takes the bars."""
    w = _win(oracle, 4)
    wo, wg = w.copy(), w.copy()
    oracle.ba_solve(wo, 4)
    est = gf.Estimator(W, F, F * W)
    est.solve([wg], 4)
    dp, dr = _pose_diff(wo, wg)
    assert dp < 1e-6 and dr < 1e-6, (dp, dr)
    po, pg = oracle.ba_marginalize(wo, 0), est.marginalize([wo.copy()], 0)[0]
    pg2 = est.marginalize([wo.copy()], 0)[0]
    assert pg is not None and np.array_equal(po["block_id"], pg["block_id"]) and po["n"] == pg["n"] and po["m"] == pg["m"]
    assert np.array_equal(po["x0"], pg["x0"])
    assert np.array_equal(pg["J"], pg2["J"]) and np.array_equal(pg["r"], pg2["r"])
    # MARGIN_OLD: the existing bars where the reference reaches them itself, else four times the reference's own error (the largest of four last-bit draws
    # underestimates its maximum)
    nA0, nS0, nb0 = _oracle_prior_noise(oracle, wo, 0)
    n0 = po["n"]
    Jo0, Jg0 = po["J"].reshape(n0, n0), pg["J"].reshape(n0, n0)
    Ao0, Ag0, bo0, bg0 = Jo0.T @ Jo0, Jg0.T @ Jg0, Jo0.T @ po["r"], Jg0.T @ pg["r"]
    dA0, db0 = np.abs(Ao0 - Ag0).max() / np.abs(Ao0).max(), np.abs(bo0 - bg0).max() / np.abs(bo0).max()
    sc0 = np.sqrt(np.outer(np.diag(Ao0), np.diag(Ao0))) + 1e-6 * np.abs(Ao0).max()
    dS0 = (np.abs(Ao0 - Ag0) / sc0).max()
    print("MARGIN_OLD: the oracle's own noise (J^T J, scaled entries, J^T r)", (nA0, nS0, nb0), "solver against oracle", (dA0, dS0, db0))
    assert dA0 <= max(1e-9, 4 * nA0) and dS0 <= max(5e-7, 4 * nS0) and db0 <= max(1e-8, 4 * nb0)
    # the next window on the same handle: solved by the solver with ITS prior, by the oracle with the oracle's
    w2o = _win(oracle, 4, frame0=1, prior=po)
    w2g = _win(oracle, 4, frame0=1, prior=pg)
    s2o, s2g = oracle.ba_solve(w2o, ITERS), est.solve([w2g], ITERS)[0]
    assert len(w2g["prior_r"]) > 0
    assert (s2g["iterations"], s2g["successful_steps"], s2g["termination"]) == (s2o["iterations"], s2o["successful_steps"], s2o["termination"])
    dp, dr = _pose_diff(w2o, w2g)
    assert dp < 1e-6 and dr < 1e-6, (dp, dr)
    # ... and its MARGIN_SECOND_NEW prior
    nA, nS, nb = _oracle_prior_noise(oracle, w2o, 1)
    print("MARGIN_SECOND_NEW: the oracle's own noise (J^T J, scaled entries, J^T r)", (nA, nS, nb))
    assert nA <= 0.5e-9 and nS <= 2.5e-7 and nb <= 0.5e-8
    p1o, p1g = oracle.ba_marginalize(w2o, 1), est.marginalize([w2o.copy()], 1)[0]
    p1g2 = est.marginalize([w2o.copy()], 1)[0]
    est.close()
    assert p1g is not None and np.array_equal(p1o["block_id"], p1g["block_id"]) and p1o["n"] == p1g["n"] and p1o["m"] == p1g["m"]
    assert np.array_equal(p1g["J"], p1g2["J"]) and np.array_equal(p1g["r"], p1g2["r"])
    n = p1o["n"]
    Jo, Jg = p1o["J"].reshape(n, n), p1g["J"].reshape(n, n)
    Ao, Ag, bo, bg = Jo.T @ Jo, Jg.T @ Jg, Jo.T @ p1o["r"], Jg.T @ p1g["r"]
    print("prior: n", n, "m", p1o["m"], "J^T J rel %.3g, J^T r rel %.3g" % (np.abs(Ao - Ag).max() / np.abs(Ao).max(), np.abs(bo - bg).max() / np.abs(bo).max()))
    assert np.abs(Ao - Ag).max() <= 1e-9 * np.abs(Ao).max()
    sc = np.sqrt(np.outer(np.diag(Ao), np.diag(Ao))) + 1e-6 * np.abs(Ao).max()
    assert (np.abs(Ao - Ag) / sc).max() < 5e-7
    assert np.abs(bo - bg).max() <= 1e-8 * np.abs(bo).max()
