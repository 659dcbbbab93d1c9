"""The track image ("Track image") restated in plain Python from its definition, not from csrc/gf_track_draw.hpp: the expected pictures
of tests/test_track_draw_host.py and tests/test_track_draw_gpu.py.  Integers are Python's (exact at any size); the arrow tips go through math.atan2 / cos / sin,
the C library's functions the host code calls, not numpy's vectorised ones.

A frame's lists: cur [n, 2] float32, track_cnt [n] int, prev [n, 2] float32, has_prev [n] bool."""
import math

import numpy as np

C0 = (255, 242, 230, 217, 204, 191, 178, 166, 153, 140, 128, 115, 102, 89, 77, 64, 51, 38, 25, 13, 0)
C2 = (0, 13, 26, 38, 51, 64, 76, 89, 102, 115, 128, 140, 153, 166, 178, 191, 204, 217, 230, 242, 255)
GREEN = (0, 255, 0)


def rnd(v):
    """lrintf of a float32: round half to even"""
    return int(np.rint(np.float32(v)))


def _lrint(v):
    return int(round(v))   # Python's round of a float to an int is round half to even, like lrint in the default rounding mode


def tips(a, b):
    """the two ends of an arrow's head: a = rounded current point, b = rounded previous point (where the head sits).  Returns (p+, p-) and how far the nearest
    tip coordinate lies from a half-integer (the tests keep away from lrint's ties)"""
    tip = 0.2 * math.sqrt(float((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2))
    ang = math.atan2(a[1] - b[1], a[0] - b[0])
    out, margin = [], 1.0
    for s in (1.0, -1.0):
        x, y = b[0] + tip * math.cos(ang + s * math.pi / 4), b[1] + tip * math.sin(ang + s * math.pi / 4)
        for v in (x, y):
            margin = min(margin, abs(v - math.floor(v) - 0.5))
        out.append((_lrint(x), _lrint(y)))
    return out[0], out[1], margin


def strokes(cur, prev, has_prev):
    """every stroke of a frame as (ux, uy, vx, vy), and the smallest distance of a tip coordinate from a half-integer"""
    out, margin = [], 1.0
    for i in range(len(cur)):
        if not has_prev[i]:
            continue
        a, b = (rnd(cur[i][0]), rnd(cur[i][1])), (rnd(prev[i][0]), rnd(prev[i][1]))
        p, q, m = tips(a, b)
        margin = min(margin, m)
        out += [a + b, p + b, q + b]
    return out, margin


def stroke_mask(s, w, h):
    """the pixels of a w x h image that stroke s = (ux, uy, vx, vy) covers: squared distance to the segment <= 9/4, in exact integers"""
    ux, uy, vx, vy = s
    m = np.zeros((h, w), bool)
    dx, dy = vx - ux, vy - uy
    L = dx * dx + dy * dy
    for y in range(max(min(uy, vy) - 2, 0), min(max(uy, vy) + 3, h)):
        for x in range(max(min(ux, vx) - 2, 0), min(max(ux, vx) + 3, w)):
            px, py = x - ux, y - uy
            t = px * dx + py * dy
            if t <= 0:
                m[y, x] = 4 * (px * px + py * py) <= 9
            elif t >= L:
                m[y, x] = 4 * ((x - vx) ** 2 + (y - vy) ** 2) <= 9
            else:
                m[y, x] = 4 * (px * dy - py * dx) ** 2 <= 9 * L
    return m


def dot_mask(cx, cy, w, h):
    m = np.zeros((h, w), bool)
    for y in range(max(cy - 5, 0), min(cy + 6, h)):
        for x in range(max(cx - 5, 0), min(cx + 6, w)):
            m[y, x] = (x - cx) ** 2 + (y - cy) ** 2 <= 25
    return m


def render(gray, cur, track_cnt, prev=None, has_prev=None, with_rules=False):
    """the [h, w, 3] u8 picture of one frame.  with_rules: also the number of pixels that "the largest index wins" decided (covered by two or more dots of
    different colours, by no stroke) and that "green over dots" decided (covered by a stroke and by a dot), and the tips' margin"""
    gray = np.asarray(gray)
    h, w = gray.shape
    n = len(cur)
    img = np.repeat(gray[:, :, None], 3, 2).astype(np.uint8)
    ndots = np.zeros((h, w), np.int32)
    mixed = np.zeros((h, w), bool)
    for i in range(n):
        assert track_cnt[i] >= 0
        k = min(int(track_cnt[i]), 20)
        col = np.array((C0[k], 0, C2[k]), np.uint8)
        m = dot_mask(rnd(cur[i][0]), rnd(cur[i][1]), w, h)
        mixed |= m & (ndots > 0) & (img != col).any(2)
        ndots += m
        img[m] = col
    margin = 1.0
    green = np.zeros((h, w), bool)
    if prev is not None and has_prev is not None:
        ss, margin = strokes(cur, prev, has_prev)
        for s in ss:
            green |= stroke_mask(s, w, h)
    img[green] = GREEN
    if with_rules:
        return img, int((mixed & ~green).sum()), int((green & (ndots > 0)).sum()), margin
    return img


def random_lists(rng, n, w, h, p_prev=0.7, reach=12.0, spill=4.0):
    """seeded lists of n features around a w x h frame (some a little outside it), arrows up to `reach` long"""
    cur = np.stack([rng.uniform(-spill, w + spill, n), rng.uniform(-spill, h + spill, n)], 1).astype(np.float32)
    prev = (cur + rng.uniform(-reach, reach, (n, 2))).astype(np.float32)
    cnt = rng.integers(1, 30, n).astype(np.int32)
    has = rng.random(n) < p_prev
    return cur, cnt, prev, has
