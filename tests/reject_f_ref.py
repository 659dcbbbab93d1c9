"""rejectWithF as csrc/gf_reject_f.hpp defines it, restated for the tests: Python floats (IEEE doubles: + - * / and math.sqrt round as the header's do) in
explicit loops in the header's order of operations, no np.linalg, no reduction whose order numpy chooses.  The one vectorised part is the score, which is
element-wise over the candidates (each candidate sees the header's operations in the header's order); the count is a sum of integers.
Also the cases of the CPU and GPU tests, a census of the rules a case takes, and planted two-view scenes: a yardstick that is not the same hand."""
import math

import numpy as np

HYPOTHESES = 512
SAMPLE = 8
MAX_DRAWS = 64
MAX_PAIRS = 1024
PIVOT_MIN = 1e-12
SQRT2 = 1.4142135623730951
M32 = 0xFFFFFFFF


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def frame_seed(seed, frames):
    return mix32(seed ^ mix32((frames + 0x9E3779B9) & M32))


def draw_word(seed, h, d):
    return mix32(seed ^ mix32((h * MAX_DRAWS + d + 1) & M32))


def draw_sample(seed, h, m, census=None):
    idx = []
    for d in range(MAX_DRAWS):
        if len(idx) == SAMPLE:
            break
        i = draw_word(seed, h, d) % m
        if i in idx:
            if census is not None:
                census["redraws"] += 1
            continue
        idx.append(i)
    return idx if len(idx) == SAMPLE else None


def hartley(px, py):
    sx = sy = 0.0
    for k in range(SAMPLE):
        sx = sx + px[k]
        sy = sy + py[k]
    cx, cy = sx / 8.0, sy / 8.0
    sd = 0.0
    for k in range(SAMPLE):
        dx, dy = px[k] - cx, py[k] - cy
        sd = sd + math.sqrt(dx * dx + dy * dy)
    d = sd / 8.0
    if not d > 0.0:
        return None
    return cx, cy, SQRT2 / d


def model(cand, seed, h, census=None):
    """F (9 floats, row-major) of hypothesis h over the float32 candidates cand[m][4] = ax ay bx by, or None: void"""
    c = census if census is not None else {"redraws": 0, "void_draw": 0, "void_scale": 0, "void_pivot": 0}
    idx = draw_sample(seed, h, len(cand), c)
    if idx is None:
        c["void_draw"] += 1
        return None
    P = [[float(cand[i][k]) for i in idx] for k in range(4)]   # float32 -> double is exact
    na, nb = hartley(P[0], P[1]), hartley(P[2], P[3])
    if na is None or nb is None:
        c["void_scale"] += 1
        return None
    (cax, cay, sa), (cbx, cby, sb) = na, nb
    A = []
    for k in range(SAMPLE):
        ax, ay = (P[0][k] - cax) * sa, (P[1][k] - cay) * sa
        bx, by = (P[2][k] - cbx) * sb, (P[3][k] - cby) * sb
        A.append([bx * ax, bx * ay, bx, by * ax, by * ay, by, ax, ay, 1.0])
    row_used, col_used, pivots = [False] * SAMPLE, [False] * 9, []
    for _ in range(SAMPLE):
        best, pr, pc = -1.0, 0, 0
        for r in range(SAMPLE):
            if row_used[r]:
                continue
            v, col = -1.0, 0
            for cc in range(9):
                if not col_used[cc] and abs(A[r][cc]) > v:
                    v, col = abs(A[r][cc]), cc
            if v > best:
                best, pr, pc = v, r, col
        if not best >= PIVOT_MIN:
            c["void_pivot"] += 1
            return None
        row_used[pr] = col_used[pc] = True
        pivots.append((pr, pc))
        for r in range(SAMPLE):
            if row_used[r]:
                continue
            f = A[r][pc] / A[pr][pc]
            for cc in range(9):
                if not col_used[cc]:
                    A[r][cc] = A[r][cc] - f * A[pr][cc]
    solved = [not u for u in col_used]
    x = [1.0] * 9
    for pr, pc in reversed(pivots):
        acc = 0.0
        for cc in range(9):
            if solved[cc]:
                acc = acc + A[pr][cc] * x[cc]
        x[pc] = -acc / A[pr][pc]
        solved[pc] = True
    G = [0.0] * 9
    for r in range(3):
        G[3 * r] = x[3 * r] * sa
        G[3 * r + 1] = x[3 * r + 1] * sa
        G[3 * r + 2] = x[3 * r + 2] - (G[3 * r] * cax + G[3 * r + 1] * cay)
    F = [0.0] * 9
    for cc in range(3):
        F[cc] = sb * G[cc]
        F[3 + cc] = sb * G[3 + cc]
        F[6 + cc] = G[6 + cc] - (F[cc] * cbx + F[3 + cc] * cby)
    return F


def inliers(F, cand64, tt):
    """the mask of the header's `inlier` over cand64[m][4] (float64 copies of the float32 candidates): element-wise, the header's order"""
    ax, ay, bx, by = cand64[:, 0], cand64[:, 1], cand64[:, 2], cand64[:, 3]
    with np.errstate(all="ignore"):
        l2x = F[0] * ax + F[1] * ay + F[2]
        l2y = F[3] * ax + F[4] * ay + F[5]
        l2z = F[6] * ax + F[7] * ay + F[8]
        r = bx * l2x + by * l2y + l2z
        rr = r * r
        l1x = F[0] * bx + F[3] * by + F[6]
        l1y = F[1] * bx + F[4] * by + F[7]
        return (rr <= tt * (l2x * l2x + l2y * l2y)) & (rr <= tt * (l1x * l1x + l1y * l1y))


def reject(pairs, status, threshold, seed):
    """-> (status bytes after the stage, (m, rejected, winner, inliers), census)"""
    pairs = np.ascontiguousarray(pairs, np.float32).reshape(-1, 4)
    st = np.array(status, np.uint8).copy()
    census = {"redraws": 0, "void_draw": 0, "void_scale": 0, "void_pivot": 0, "void_fit": 0, "ties": 0, "valid": 0, "nonfinite": 0}
    rows = []
    rejected = 0
    for i in range(len(pairs)):
        if not st[i]:
            continue
        if not np.all(np.isfinite(pairs[i])):
            st[i] = 0
            rejected += 1
            census["nonfinite"] += 1
            continue
        rows.append(i)
    m = len(rows)
    if m < SAMPLE:
        return st, (m, rejected, -1, 0), census
    cand = pairs[rows]
    cand64 = cand.astype(np.float64)
    tt = float(threshold) * float(threshold)
    best, winner, best_mask = 0, -1, None
    for h in range(HYPOTHESES):
        F = model(cand, seed, h, census)
        if F is None:
            continue
        mask = inliers(np.array(F, np.float64), cand64, tt)
        count = int(mask.sum())
        if count < SAMPLE:
            census["void_fit"] += 1
            continue
        census["valid"] += 1
        if count > best:
            best, winner, best_mask = count, h, mask
        elif count == best:
            census["ties"] += 1
    if winner < 0:
        return st, (m, rejected, -1, 0), census
    for j in range(m):
        if not best_mask[j]:
            st[rows[j]] = 0
            rejected += 1
    return st, (m, rejected, winner, best), census


# ---- planted two-view scenes: random 3-D points at 2-8 m, a 3-degree rotation and a 0.3 m translation, a 460-pixel pinhole, uniform pixel noise, outliers moved
# 20-60 px off their epipolar line.  Not derived from the definition above: the truth is the plant.

def planted_scene(n, n_out, noise, rng_seed, width=640, height=480, focal=460.0):
    rng = np.random.RandomState(rng_seed)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 8.0, n)], 1)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = math.radians(3.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
    t = rng.normal(size=3)
    t *= 0.3 / np.linalg.norm(t)
    Y = X @ R.T + t
    cx, cy = width / 2.0, height / 2.0
    a = np.stack([focal * X[:, 0] / X[:, 2] + cx, focal * X[:, 1] / X[:, 2] + cy], 1)
    b = np.stack([focal * Y[:, 0] / Y[:, 2] + cx, focal * Y[:, 1] / Y[:, 2] + cy], 1)
    # the true F in pixels, for the direction across each outlier's epipolar line
    Kin = np.array([[1 / focal, 0, -cx / focal], [0, 1 / focal, -cy / focal], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ftrue = Kin.T @ tx @ R @ Kin
    a = a + rng.uniform(-noise, noise, a.shape)
    b = b + rng.uniform(-noise, noise, b.shape)
    planted = np.zeros(n, bool)
    planted[rng.permutation(n)[:n_out]] = True
    for i in np.nonzero(planted)[0]:
        l = Ftrue @ np.array([a[i, 0], a[i, 1], 1.0])
        nrm = l[:2] / np.linalg.norm(l[:2])
        b[i] += nrm * rng.uniform(20.0, 60.0) * rng.choice([-1.0, 1.0])
    return np.concatenate([a, b], 1).astype(np.float32), planted


# ---- the cases of the CPU and GPU tests: name -> (pairs float32 [n][4], threshold, seed)

def cases():
    out = {}
    for m in (7, 8, 9, 64, 65):
        p, _ = planted_scene(max(m, 30), max(m, 30) // 4, 0.05, 100 + m)
        out["m%d" % m] = (p[:m].copy(), 1.0, 7 * m)
    p, _ = planted_scene(MAX_PAIRS, 300, 0.05, 5)
    out["capacity"] = (p, 1.0, 11)
    p, _ = planted_scene(40, 0, 0.0, 6)
    p[:, 2:] = p[:, :2]
    p[:] = p[0]
    out["identical"] = (p.copy(), 1.0, 12)          # bit-identical points: every hypothesis void, nothing rejected
    q = np.zeros((40, 4), np.float32)
    q[:, 0] = np.arange(40) * 7.0 + 20
    q[:, 1] = np.arange(40) * 3.0 + 40
    q[:, 2] = q[:, 0] + 2.0
    q[:, 3] = q[:, 1] + 1.0
    out["collinear"] = (q, 1.0, 13)
    p, _ = planted_scene(50, 10, 0.05, 7)
    p[3, 0] = np.nan
    p[17, 3] = np.inf
    out["nonfinite"] = (p, 1.0, 14)
    p, _ = planted_scene(48, 0, 0.0, 8)              # noise-free, no outliers: many hypotheses keep all 48, the first wins
    out["tie"] = (p, 1.0, 15)
    p, _ = planted_scene(12, 2, 0.05, 9)
    p[5] = p[4]
    p[9] = p[4]
    out["duplicate"] = (p, 1.0, 16)                  # 12 candidates, three of them one point: redraws, and samples that hold it twice are void
    p, _ = planted_scene(150, 45, 0.05, 10)
    out["planted150"] = (p, 1.0, 17)
    return out


_REFERENCE = None


def reference():
    """the restatement's answer for every case, computed once per process and shared by the tests: name -> (status, result tuple, census)"""
    global _REFERENCE
    if _REFERENCE is None:
        _REFERENCE = {}
        for name, (pairs, thr, seed) in cases().items():
            _REFERENCE[name] = reject(pairs, np.ones(len(pairs), np.uint8), thr, seed)
    return _REFERENCE


# ---- a synthetic stream in which a patch of features moves against the scene: the scene drifts, turns and grows slowly as under a moving camera; inside a fixed
# window another texture turns about the window's centre, so the displacements of its features circulate and no epipolar geometry of the scene holds them

def stream(w, h, n, seed=3, turn=0.05):
    import synth
    tex, tex2 = synth.make_texture(seed, size=512), synth.make_texture(seed + 1, size=512)
    px, py, pw, ph = w // 2, h // 5, (2 * w) // 5, (3 * h) // 5
    ys, xs = np.mgrid[0:ph, 0:pw].astype(np.float64)
    frames = []
    for k in range(n):
        f = synth.warp_frame(tex, 1.3 * k, 0.7 * k, 0.004 * k, 1.0 + 0.002 * k, w, h, ox=100.0, oy=100.0)
        c, s = math.cos(turn * k), math.sin(turn * k)
        xc, yc = xs - pw / 2, ys - ph / 2
        patch = synth._bilinear(tex2, c * xc - s * yc + 250.0, s * xc + c * yc + 250.0)
        f[py:py + ph, px:px + pw] = np.clip(np.rint(patch), 0, 255).astype(np.uint8)
        frames.append(f)
    return frames


# ---- a planted scene seen through a camera of the library: the virtual pixels of planted_scene are rays of the 460-pixel pinhole; projected through `cam`
# (gfamd.camera_project, spaceToPlane on the host) they become the pixel rows a tracker would hold.  noise 0.04 px in the plant, the float32 rounding of the
# pixels and the round trip of the model's lift stay below 0.05 px together.
KB = ("KANNALA_BRANDT", [460.0, 461.5, 318.5, 242.25], [-0.012, 0.006, -0.003, 0.0006])
KB_SIZE = (640, 480)


def camera_scene(gfamd, cam, n, n_out, rng_seed, noise=0.04):
    pairs, planted = planted_scene(n, n_out, noise, rng_seed)
    p = pairs.astype(np.float64)
    rays = lambda xy: np.stack([(xy[:, 0] - 320.0) / 460.0, (xy[:, 1] - 240.0) / 460.0, np.ones(len(xy))], 1)
    prev, cur = gfamd.camera_project([cam, cam], [rays(p[:, :2]), rays(p[:, 2:])])
    return prev.astype(np.float32), cur.astype(np.float32), planted
