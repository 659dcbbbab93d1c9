"""Inputs that drive the pyramidal LK kernels through every exit of lk_level and to sums of 32 bits and more (plain numpy, no GPU).

Every LK input of the older tests is a synth.make_texture image: blurred, grey levels 20..235, moved by a few pixels.  On those a point ends a level pass with
|delta|^2 <= eps almost everywhere and the exact sums stay below 2^28.5.  The frames here are binary (0 / 255) patterns -- 2 x 2 block checkerboards, cell noise,
per-pixel noise, the 1 x 1 checkerboard whose Scharr derivative is zero -- and quilts of them, tracked against shifted copies, inverses and fresh noise, with points
on a rim grid around the image border.  tests/test_lk_hard_cases_host.py holds the oracle's exit census of these inputs to fixed bars, and
tests/test_lk_hard_cases_gpu.py holds the HIP kernels to the oracle on them.

A case is a dict: name, prev, next (u8 frames), pts [n, 2] float32, init (None or [n, 2] float32: the predicted start), max_level.  Everything is seeded; cases() builds
the list once per process."""
import numpy as np

W, H = 176, 192          # the smallest frame with four pyramid levels (level 3 is 22 x 24)
W3, H3 = 160, 120        # three levels
N_PTS = 336              # points per case (a multiple of 4; the GPU test also runs a list of 1 mod 4)
CASE_NAMES = ("block2_shift", "block2_inverse", "cells_small_shift", "cells_large_shift", "pixel_noise_shift", "pixel_noise_fresh", "mixed_checker_cells", "quilt",
              "quilt_predicted", "quilt_three_levels", "pixel_noise_shift_predicted", "block2_shift_predicted", "pixel_noise_shift_edge_start", "quilt_edge_start")

# x (and, with the height, y) coordinates of the rim grid: outside by more than the window, by less, on the edge, half a window inside, on the far edge and beyond.
# The template window of a point leaves level L when x * 2^-L - 10 < -21 or >= the level's width: -11.5 and n + 10.6 do that at level 0 only, the first and the last
# coordinate (-45.5, n + 40.3) at levels 0, 1 and 2.
def _rim_axis(n):
    return [-45.5, -11.5, -10.4, -0.3, 0.0, 9.9, 10.0, 10.5, n - 11.0, n - 10.5, n - 1.0, n - 0.2, n + 9.6, n + 10.6, n + 40.3]


def rim_points(w, h):
    """the points of the 15 x 15 grid that lie around the rim (at least one coordinate within half a window of an edge, or outside): 221 of the 225"""
    xs, ys = _rim_axis(w), _rim_axis(h)
    inner_x, inner_y = {10.5, w - 11.0}, {10.5, h - 11.0}
    return np.array([(x, y) for y in ys for x in xs if not (x in inner_x and y in inner_y)], np.float32)


# ---------------------------------------------------------------- patterns (all 0 / 255 unless `hi` says otherwise)
def block_checker(w, h, block=2, dx=0, dy=0):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x + dx) // block + (y + dy) // block) & 1) * 255).astype(np.uint8)


def cell_field(seed, w, h, cell, hi=255):
    """binary noise in cells of cell x cell pixels, as one large field that frames are cut out of"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell)).astype(np.uint8) * np.uint8(hi)
    return np.kron(c, np.ones((cell, cell), np.uint8))[:h, :w]


def window(field, x, y, w, h):
    return np.ascontiguousarray(field[y:y + h, x:x + w])


def quilt(parts, w, h):
    """parts: [(image, x0, x1)] -- vertical bands [x0, x1) of the frame taken from the images"""
    out = np.zeros((h, w), np.uint8)
    for img, x0, x1 in parts:
        out[:, x0:x1] = img[:, x0:x1]
    return out


# ---------------------------------------------------------------- point sets
def _interleave(families, n):
    """round-robin over the point families until n points are taken: neighbours in the list come from different families.  A family that runs out starts again
    from its first point moved by a fraction of a pixel."""
    out, k = [], 0
    while len(out) < n:
        f = families[k % len(families)]
        j = k // len(families)
        rep, idx = divmod(j, len(f))
        out.append(f[idx] + np.float32(0.171 * rep))
        k += 1
    return np.array(out, np.float32)


def _uniform(rng, n, x0, x1, y0, y1):
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1).astype(np.float32)


def _case(name, prev, nxt, pts, max_level=3, init=None):
    assert prev.shape == nxt.shape and prev.dtype == np.uint8 and nxt.dtype == np.uint8
    return dict(name=name, prev=prev, next=nxt, pts=np.ascontiguousarray(pts, np.float32), init=init, max_level=max_level)


def _predicted(rng, pts):
    return (pts + rng.normal(0, 3.0, pts.shape)).astype(np.float32)


# (point x, y, start x, y) on the quilt frames, level 0 alone: the last step of each carries the search window across the edge of the search range
_RECHECK_STARTS = (
    (114.11076, 45.87747, -10.515177, 45.87747),
    (57.476738, 150.37103, -10.511838, 150.37103),
    (60.161114, 96.05374, -10.730334, 96.05374),
    (70.03549, 132.49333, 185.89977, 132.49333),
    (92.481995, 26.357733, 185.45766, 26.357733),
    (128.15741, 35.439693, 185.50665, 35.439693),
    (104.76638, 98.25487, 104.76638, -10.87539),
    (70.10111, 46.28288, 70.10111, -10.400556),
    (123.67152, 102.16925, 123.67152, -10.69823),
    (125.421684, 147.04579, 125.421684, 201.72672),
    (72.83512, 136.11203, 72.83512, 201.48773),
    (77.452324, 52.584755, 77.452324, 201.73538))

_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(20250)
    rim = rim_points(W, H)
    rim = rim[rng.permutation(len(rim))]
    out = []

    # 1, 2: the 2 x 2 block checkerboard against itself one pixel on and against its inverse: flat at levels 3..1, the largest sums at level 0
    b0 = block_checker(W, H)
    inner = _uniform(rng, 200, 12, W - 12, 12, H - 12)
    grid = np.array([(x + 0.5 * (k & 1), y + 0.25 * (k & 3)) for k, (y, x) in enumerate((y, x) for y in range(14, H - 12, 9) for x in range(13, W - 12, 9))], np.float32)
    out.append(_case("block2_shift", b0, block_checker(W, H, dx=1), _interleave([inner, rim, grid], N_PTS)))
    out.append(_case("block2_inverse", b0, 255 - b0, _interleave([grid, inner, rim], N_PTS)))

    # 3, 4: cell noise, 8 x 8 cells on the left and 4 x 4 on the right, cut out of one field at a small and at a large offset
    f8, f4 = cell_field(31, W + 64, H + 64, 8), cell_field(32, W + 64, H + 64, 4)
    def cells(x, y):
        return quilt([(window(f8, x, y, W, H), 0, W // 2), (window(f4, x, y, W, H), W // 2, W)], W, H)
    left, right = _uniform(rng, 150, 0, W // 2, 0, H), _uniform(rng, 150, W // 2, W, 0, H)
    out.append(_case("cells_small_shift", cells(32, 32), cells(32 + 2, 32 - 3), _interleave([left, rim, right], N_PTS)))
    out.append(_case("cells_large_shift", cells(32, 32), cells(32 + 20, 32 + 25), _interleave([left, right, rim, _uniform(rng, 100, 0, 40, 0, 50)], N_PTS)))

    # 5, 6: per-pixel noise against a shifted copy (oscillation) and against fresh noise (the iteration cap)
    f1 = cell_field(33, W + 64, H + 64, 1)
    anyw = _uniform(rng, 250, 0, W, 0, H)
    out.append(_case("pixel_noise_shift", window(f1, 32, 32, W, H), window(f1, 33, 31, W, H), _interleave([anyw, rim], N_PTS)))
    out.append(_case("pixel_noise_fresh", window(f1, 32, 32, W, H), cell_field(34, W, H, 1), _interleave([anyw, rim, inner], N_PTS)))

    # 7: the 1 x 1 checkerboard (zero derivative) on the left, cell noise on the right: a window of a coarse level spans both, level 0 rejects the left half
    def mixed(x, y, width=W, height=H):
        return quilt([(block_checker(width, height, block=1), 0, width // 2), (window(f8, x, y, width, height), width // 2, width)], width, height)
    out.append(_case("mixed_checker_cells", mixed(32, 32), mixed(33, 34), _interleave([left, right, rim, _uniform(rng, 80, W // 2 - 30, W // 2 + 10, 0, H)], N_PTS)))

    # 8..10: quilts of four bands -- 1 x 1 checkerboard | per-pixel noise against fresh noise | cell noise moved a little | 2 x 2 blocks one pixel on -- with the
    # point list dealt band by band and the rim in between: neighbours in a wavefront leave level 0 by different exits.  Once with four levels, once as the tracker's
    # own passes (max_level 1 from a predicted start), once on the three-level frame.
    def quilt_pair(w, h, seed):
        q = [0, w // 4, w // 2, 3 * w // 4, w]
        fresh = cell_field(seed, w, h, 1)
        prev = quilt([(block_checker(w, h, block=1), q[0], q[1]), (window(f1, 10, 10, w, h), q[1], q[2]), (window(f8, 8, 8, w, h), q[2], q[3]), (block_checker(w, h), q[3], q[4])], w, h)
        nxt = quilt([(block_checker(w, h, block=1), q[0], q[1]), (fresh, q[1], q[2]), (window(f8, 9, 10, w, h), q[2], q[3]), (block_checker(w, h, dx=1), q[3], q[4])], w, h)
        bands = [_uniform(rng, 90, q[k] + 3, q[k + 1] - 3, 8, h - 8) for k in range(4)]
        return prev, nxt, bands
    qp, qn, qb = quilt_pair(W, H, 35)
    qpts = _interleave([qb[0], qb[1], qb[2], rim, qb[3], qb[1], rim, qb[2]], N_PTS)
    out.append(_case("quilt", qp, qn, qpts))
    out.append(_case("quilt_predicted", qp, qn, qpts, max_level=1, init=_predicted(rng, qpts)))
    rim3 = rim_points(W3, H3)
    rim3 = rim3[rng.permutation(len(rim3))]
    qp3, qn3, qb3 = quilt_pair(W3, H3, 36)
    out.append(_case("quilt_three_levels", qp3, qn3, _interleave([qb3[0], qb3[1], rim3, qb3[2], qb3[3], rim3, qb3[1], qb3[2]], N_PTS)))

    # 11, 12: the tracker's own passes on the families with oscillation and cap exits: max_level 1 from pts + N(0, 3 px)
    p5 = out[4]["pts"]
    out.append(_case("pixel_noise_shift_predicted", out[4]["prev"], out[4]["next"], p5, max_level=1, init=_predicted(rng, p5)))
    p1 = out[0]["pts"]
    out.append(_case("block2_shift_predicted", out[0]["prev"], out[0]["next"], p1, max_level=1, init=_predicted(rng, p1)))

    # 13, 14: the bounds re-check after the level-0 loop fires when the LAST step of a point (the 30th, or the half step back of the oscillation exit) carries its
    # window out of the search range, which the loop itself would only have seen one iteration later.  Level 0 alone, from starts on the edge of that range
    # (window corner at -21 .. -20.4 or at n - 1.6 .. n - 1): steps that do not converge wander across the edge.
    def edge_start(pts, w, h):
        side, t = rng.integers(0, 4, len(pts)), rng.uniform(0, 0.6, len(pts))
        init = pts.copy()
        init[:, 0] = np.where(side == 0, -10.99 + t, np.where(side == 1, w + 9.99 - t, pts[:, 0]))
        init[:, 1] = np.where(side == 2, -10.99 + t, np.where(side == 3, h + 9.99 - t, pts[:, 1]))
        return init.astype(np.float32)
    pe = _interleave([inner, anyw, grid], N_PTS)
    out.append(_case("pixel_noise_shift_edge_start", out[4]["prev"], out[4]["next"], pe, max_level=0, init=edge_start(pe, W, H)))
    # Such a last step is rare (about one start in a thousand): twelve that a seeded search over 48 000 starts on the quilt found (three per edge; eps and cap exits)
    # are kept as literals and dealt into the quilt's list, 28 points apart.
    qe_pts, qe_init = qpts.copy(), edge_start(qpts, W, H)
    for k, (px, py, sx, sy) in enumerate(_RECHECK_STARTS):
        qe_pts[13 + 28 * k] = (px, py)
        qe_init[13 + 28 * k] = (sx, sy)
    out.append(_case("quilt_edge_start", qp, qn, qe_pts, max_level=0, init=qe_init))
    assert tuple(c["name"] for c in out) == CASE_NAMES
    for c in out:
        assert 300 <= len(c["pts"]) <= 350
    _CASES = out
    return out


def old_inputs(oracle):
    """the two main cases of test_tracker_gpu.test_lk_bit_exact, rebuilt as that test builds them: (name, prev, next, pts, init, max_level)"""
    import synth
    tex = synth.make_texture(21)
    f0 = synth.warp_frame(tex, 0, 0)
    f1 = synth.warp_frame(tex, -3.7, 2.2, 0.004, 1.003)
    res = []
    for max_level, use_init in ((3, False), (1, True)):
        pts = oracle.good_features(f0, 300, min_dist=15.0)
        rng = np.random.default_rng(4)
        extra = np.array([[0.2, 0.3], [639.5, 479.2], [-30.0, 10.0], [700.0, 100.0], [320.25, 1.5], [5.5, 470.1]], np.float32)
        pts = np.concatenate([pts, extra, rng.uniform(0, 1, (40, 2)).astype(np.float32) * [640, 480]]).astype(np.float32)
        init = (pts + rng.normal(0, 1.5, pts.shape)).astype(np.float32) if use_init else None
        res.append(_case("make_texture_level%d%s" % (max_level, "_predicted" if use_init else ""), f0, f1, pts, max_level, init))
    return res


# ---------------------------------------------------------------- frames for the detector and the whole tracker
def detector_frames():
    """the 2 x 2 block checkerboard, cell noise and the checkerboard | cell-noise frame: periodic binary patterns with thousands of exactly equal eigenvalues"""
    c = {x["name"]: x for x in cases()}
    return [("block2", c["block2_shift"]["prev"]), ("cells", c["cells_small_shift"]["prev"]), ("mixed", c["mixed_checker_cells"]["prev"])]


TW, TH = 320, 240


def tracker_sequences(n_frames=6):
    """two 320 x 240 sequences of windows sliding by (2, 3) px over one larger field.  Sequence 0: 8 x 8 cell noise with grey levels 0 / 250 -- the brightness test
    (feature_tracker.cpp:160-163) drops tracks on pixels above 250, so with 255 a sequence mostly tests that drop; frames 3 and 4 are at 255 for exactly that.
    Sequence 1: the 1 x 1 checkerboard on the left and the same cell noise on the right."""
    field = cell_field(41, TW + 64, TH + 64, 8, hi=1)
    seq0, seq1 = [], []
    for k in range(n_frames):
        cut = window(field, 8 + 2 * k, 8 + 3 * k, TW, TH)
        hi = 255 if k in (3, 4) else 250
        seq0.append((cut * np.uint8(hi)).astype(np.uint8))
        seq1.append(quilt([(block_checker(TW, TH, block=1), 0, TW // 2), (cut * np.uint8(250), TW // 2, TW)], TW, TH))
    return seq0, seq1


# ---------------------------------------------------------------- the census of a list of cases
def census_of(oracle, case_list):
    """runs the cases through oracle.lk_census; returns (per-case results, the summary that profiles/lk_exit_census.json keeps)"""
    names = oracle.LK_EXITS
    results, per_case = [], {}
    for c in case_list:
        nxt, st, it, exits, recheck, max_a, max_b = oracle.lk_census(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
        results.append(dict(case=c, next=nxt, status=st, iters=it, exits=exits, recheck=recheck, max_A=max_a, max_b=max_b))
        table = {names[e]: [int((exits[:, lv] == e).sum()) for lv in (3, 2, 1, 0)] for e in range(1, len(names))}
        per_case[c["name"]] = dict(points=len(c["pts"]), max_level=c["max_level"], predicted_start=c["init"] is not None, status_1=int(st.sum()),
                                   iterations=int(it), recheck=int(recheck.sum()), max_abs_A=max_a, max_abs_b=max_b,
                                   log2_max_abs_A=round(float(np.log2(max(max_a, 1))), 2), log2_max_abs_b=round(float(np.log2(max(max_b, 1))), 2),
                                   exits_at_levels_3_2_1_0=table)
    total = {n: [sum(pc["exits_at_levels_3_2_1_0"][n][k] for pc in per_case.values()) for k in range(4)] for n in names[1:]}
    summary = dict(cases=per_case, total=dict(points=sum(pc["points"] for pc in per_case.values()), status_1=sum(pc["status_1"] for pc in per_case.values()),
                                              recheck=sum(pc["recheck"] for pc in per_case.values()), max_abs_A=max(pc["max_abs_A"] for pc in per_case.values()),
                                              max_abs_b=max(pc["max_abs_b"] for pc in per_case.values()), exits_at_levels_3_2_1_0=total))
    return results, summary


def figures(results):
    """the counts tests/test_lk_hard_cases_host.py holds to its bars, over the whole set (exit codes: oracle.LK_EXITS)"""
    T_OUT, MIN_EIG, START_OUT, LEFT, OSC, CAP = 1, 2, 3, 4, 6, 7
    ex = np.concatenate([r["exits"] for r in results])
    st = np.concatenate([r["status"] for r in results])
    pred = np.concatenate([np.full(len(r["status"]), r["case"]["init"] is not None and r["case"]["max_level"] == 1) for r in results])
    at0 = lambda e: int((ex[:, 0] == e).sum())
    above = lambda e: int((ex[:, 1:] == e).any(axis=1).sum())
    groups = {}
    for size, need in ((4, 3), (2, 2)):
        n = ok = 0
        for r in results:
            e0 = r["exits"][:, 0]
            for i in range(0, len(e0) - size + 1, size):
                n += 1
                ok += len(set(e0[i:i + size].tolist())) >= need
        groups[size] = (ok, n)
    return dict(
        min_eig_level0=at0(MIN_EIG), min_eig_above_then_status_1=int(((ex[:, 1:] == MIN_EIG).any(axis=1) & (st == 1)).sum()),
        template_out_level0=at0(T_OUT), template_out_above=above(T_OUT),
        start_outside_level0=at0(START_OUT), start_outside_above=above(START_OUT),
        left_image_level0=at0(LEFT), left_image_above=above(LEFT),
        oscillation_level0=at0(OSC), oscillation_level1=int((ex[:, 1] == OSC).sum()), oscillation_level0_predicted_pass=int(((ex[:, 0] == OSC) & pred).sum()),
        max_count_by_level_3_2_1_0=[int((ex[:, lv] == CAP).sum()) for lv in (3, 2, 1, 0)],
        recheck=int(sum(r["recheck"].sum() for r in results)),
        max_abs_A=max(r["max_A"] for r in results), max_abs_b=max(r["max_b"] for r in results),
        groups_of_4_with_3_level0_exits=list(groups[4]), groups_of_2_with_2_level0_exits=list(groups[2]),
        points=int(len(st)), status_1=int(st.sum()))


def census_document(oracle):
    """what profiles/lk_exit_census.json holds: the census of the inputs above, the figures of it the host test holds to bars, and the census of the inputs the
    suite had before (test_lk_bit_exact's two main cases)"""
    results, summary = census_of(oracle, cases())
    _, old = census_of(oracle, old_inputs(oracle))
    return dict(exit_codes=list(oracle.LK_EXITS), hard_cases=summary, figures=figures(results), test_lk_bit_exact_inputs=old)


if __name__ == "__main__":   # python tests/lk_hard_cases.py: rewrite profiles/lk_exit_census.json
    import json, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "ground-fusion_amd"), os.path.join(root, "oracle")]
    import oracle_py
    oracle_py.build()
    with open(os.path.join(root, "profiles", "lk_exit_census.json"), "w") as f:
        json.dump(census_document(oracle_py), f, indent=1)
        f.write("\n")
