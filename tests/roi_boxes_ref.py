"""TEST INFRASTRUCTURE: exclusion boxes restated in Python -- the rasterisation of a box list (R_eff = R_base AND NOT union(boxes)), the box lists the tests
share (the "hard lists"), the moving boxes of the tracker tests, and the track image with the boxes' frames, which extends tests/track_draw_ref.py's picture by
importing it.  Nothing here calls the library."""
import numpy as np

import roi_ref as RR
import track_draw_ref as TD

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
CAP = 256   # GF_MAX_BOXES_PER_SEQ

# gf_roi_boxes_batch is held to the raster at these; the host program at HOST_SIZES
GPU_SIZES = [(64, 61), (132, 97), (188, 122), (640, 480)]
HOST_SIZES = [(64, 61), (132, 97), (33, 1), (1, 31)]


def raster(boxes, w, h, base=None):
    """[h, w] u8 of 0 / 255: the base (None: all allowed; non-zero = allowed) minus the pixels xmin <= x <= xmax && ymin <= y <= ymax of every box, in Python's
    unbounded integers"""
    R = np.full((h, w), 255, np.uint8) if base is None else np.where(np.asarray(base) != 0, 255, 0).astype(np.uint8)
    for xmin, ymin, xmax, ymax in boxes:
        x0, y0, x1, y1 = max(int(xmin), 0), max(int(ymin), 0), min(int(xmax), w - 1), min(int(ymax), h - 1)
        if x0 <= x1 and y0 <= y1:
            R[y0:y1 + 1, x0:x1 + 1] = 0
    return R


def hard_lists(w, h):
    """name -> list of (xmin, ymin, xmax, ymax): every edge the composition has -- band borders (rows 29 | 30, 59 | 60), the last row and column, boxes partly and
    wholly outside, negative and extreme coordinates, degenerate boxes, one pixel, the whole frame, overlaps, no box, and a list of exactly the cap"""
    rng = np.random.default_rng(7 * w + h)
    cap = []
    for _ in range(CAP):   # small boxes all over the frame and a little beyond it
        x, y = int(rng.integers(-4, w + 4)), int(rng.integers(-4, h + 4))
        cap.append((x, y, x + int(rng.integers(-1, 6)), y + int(rng.integers(-1, 6))))
    return {
        "none": [],
        "band_edges": [(5, 10, 20, 29), (25, 30, 40, 41), (3, 29, 9, 30), (w // 2, 59, w // 2 + 5, 60), (0, 58, 3, 59), (w - 9, 60, w - 4, 61), (11, 28, 12, 61)],
        "last_row": [(2, h - 1, 7, h - 1), (w // 2, h - 3, w // 2 + 4, h + 5)],
        "side_columns": [(0, 3, 0, 8), (w - 1, 2, w - 1, 12), (w - 3, 0, w + 10, 4), (-7, h // 2, 1, h // 2 + 2)],
        "outside": [(-10, -10, 3, 3), (-50, -50, -1, -1), (w, 0, w + 5, 5), (0, h, 5, h + 5), (w // 3, -20, w // 3 + 2, 2)],
        "extremes": [(I32_MIN, I32_MIN, 2, 2), (w - 2, h - 2, I32_MAX, I32_MAX), (I32_MIN, 7, I32_MAX, 7), (I32_MAX, I32_MAX, I32_MAX, I32_MAX),
                     (I32_MIN, I32_MIN, I32_MIN, I32_MIN), (w // 2, I32_MIN, w // 2, I32_MAX), (I32_MAX - 1, 0, I32_MAX, 5), (0, I32_MIN, 3, I32_MIN + 1)],
        "degenerate": [(10, 2, 5, 8), (2, 9, 8, 3), (I32_MAX, 0, I32_MIN, h), (0, I32_MAX, w, I32_MIN), (6, 6, 5, 5)],
        "one_pixel": [(4, 4, 4, 4)],
        "whole_frame": [(0, 0, w - 1, h - 1)],
        "overlapping": [(w // 4, h // 4, w // 2, h // 2), (w // 3, h // 3, 2 * w // 3, 2 * h // 3), (w // 4, h // 4, w // 2, h // 2), (w // 3 + 1, 0, w // 3 + 1, h)],
        "cap": cap,
    }


def bases(w, h):
    """name -> base mask or None: none, and regions A and B of tests/roi_ref.py"""
    return {"no_base": None, "A": RR.region("A", w, h), "B": RR.region("B", w, h)}


def moving_boxes(w, h, k):
    """The boxes of frame k of the tracker tests: one to three rectangles that move every frame -- a wide one that sweeps down from the top, a tall one that
    sweeps right, and on every second frame a small one near the centre"""
    bw, bh = max(w // 3, 8), max(h // 4, 6)
    out = [(w // 8 + 5 * k, h // 10 + 4 * k, w // 8 + 5 * k + bw, h // 10 + 4 * k + bh)]
    if k % 3 != 2:
        out.append((w // 2 + 3 * k, h // 3 - 2 * k, w // 2 + 3 * k + bw // 2, h // 3 - 2 * k + bh * 2))
    if k % 2:
        out.append((w // 2 - 6, h // 2 - 4 + k, w // 2 + 6, h // 2 + 4 + k))
    return out


# ---- the track image with boxes (drawTrackbox, feature_tracker.cpp:960-975): cv::rectangle(Rect(xmin, ymin, xmax - xmin, ymax - ymin), (0, 128, 255), 5)
FRAME_COLOR = (0, 128, 255)


def frame_covers(box, w, h):
    """[h, w] bool: the pixels of the 5-wide frame of one box, the three inequalities in Python's integers; nothing unless xmax > xmin and ymax > ymin"""
    xmin, ymin, xmax, ymax = (int(v) for v in box)
    m = np.zeros((h, w), bool)
    if not (xmax > xmin and ymax > ymin):
        return m
    X0, X1, Y0, Y1 = xmin, xmax - 1, ymin, ymax - 1
    for y in range(max(Y0 - 2, 0), min(Y1 + 2, h - 1) + 1):
        for x in range(max(X0 - 2, 0), min(X1 + 2, w - 1) + 1):
            if not (X0 + 2 < x < X1 - 2 and Y0 + 2 < y < Y1 - 2):
                m[y, x] = True
    return m


def draw_boxes(picture, boxes):
    """the frames of `boxes` over a [h, w, 3] picture, in list order: they cover dots and strokes, a later box covers an earlier one"""
    out = np.array(picture, np.uint8, copy=True)
    h, w = out.shape[:2]
    for b in boxes:
        out[frame_covers(b, w, h)] = FRAME_COLOR
    return out


def render(gray, cur, track_cnt, prev=None, has_prev=None, boxes=()):
    """tests/track_draw_ref.py's picture of a frame with the frames of `boxes` drawn over it"""
    return draw_boxes(TD.render(gray, cur, track_cnt, prev, has_prev), boxes)
