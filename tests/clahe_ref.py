"""Restatement of cv::CLAHE::apply on CV_8UC1 (OpenCV 4.2, modules/imgproc/src/clahe.cpp: CLAHE_Impl::apply, CLAHE_CalcLut_Body, CLAHE_Interpolation_Body,
scalar path) in numpy: the parity target of gf_clahe_batch* and of the tracker's `equalize`.  No OpenCV build is available to the tests, so this file is the
yardstick; it is written to be read against clahe.cpp, one rule per function, not to be fast.

Every float below is a float32 and every product or sum is rounded to float32 on its own (numpy float32 arithmetic, no fused multiply-add), as the library's
scalar code is evaluated with contraction off.
"""
import numpy as np

F = np.float32


def tile_geometry(w, h, tiles_x, tiles_y):
    """(tile_w, tile_h, pad_right, pad_bottom).  A grid that divides the frame tiles the frame itself; otherwise the histograms are taken on the frame padded
    by copyMakeBorder(src, 0, ty - h % ty, 0, tx - w % tx, BORDER_REFLECT_101) -- both pads, even for the dimension that divides (it gets a whole tile more)."""
    if w <= tiles_x or h <= tiles_y:
        raise ValueError("needs width > tiles_x and height > tiles_y")
    if w % tiles_x == 0 and h % tiles_y == 0:
        return w // tiles_x, h // tiles_y, 0, 0
    pr, pb = tiles_x - w % tiles_x, tiles_y - h % tiles_y
    return (w + pr) // tiles_x, (h + pb) // tiles_y, pr, pb


def reflect101(p, n):
    """BORDER_REFLECT_101 index past the right / bottom edge: p -> 2 (n - 1) - p"""
    return p if p < n else 2 * (n - 1) - p


def padded(img, tiles_x, tiles_y):
    h, w = img.shape
    _, _, pr, pb = tile_geometry(w, h, tiles_x, tiles_y)
    rows = [reflect101(y, h) for y in range(h + pb)]
    cols = [reflect101(x, w) for x in range(w + pr)]
    return img[np.ix_(rows, cols)]


def clip_pixels(clip_limit, tile_area):
    """clipLimit = max((int)(clipLimit_ * tileSizeTotal / histSize), 1) in double, truncated; only meaningful when clip_limit > 0"""
    return max(int(float(clip_limit) * tile_area / 256), 1)


def clip_histogram(hist, clip):
    """cut every bin at `clip`, add excess // 256 to every bin, then +1 to bins 0, step, 2 step, ... (step = max(256 // residual, 1)) while the residual lasts"""
    hist = [int(v) for v in hist]
    clipped = 0
    for i in range(256):
        if hist[i] > clip:
            clipped += hist[i] - clip
            hist[i] = clip
    batch, residual = clipped // 256, clipped % 256
    for i in range(256):
        hist[i] += batch
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    return hist


def saturate_u8(v):
    """saturate_cast<uchar>(float): cvRound (half to even) then clamp"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def make_lut(hist, tile_area):
    """lut[i] = saturate_cast<uchar>(sum_{j <= i} hist[j] * lutScale), lutScale = 255.0f / tileSizeTotal; int * float is a float"""
    scale = F(255.0) / F(tile_area)
    return saturate_u8(np.cumsum(np.asarray(hist, np.int64)).astype(F) * scale)


def tile_luts(img, clip_limit, tiles_x, tiles_y):
    """[tiles_y][tiles_x][256] u8"""
    h, w = img.shape
    tw, th, _, _ = tile_geometry(w, h, tiles_x, tiles_y)
    src = padded(img, tiles_x, tiles_y)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    for j in range(tiles_y):
        for i in range(tiles_x):
            hist = np.bincount(src[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256)
            if clip_limit > 0:
                hist = clip_histogram(hist, clip_pixels(clip_limit, tw * th))
            luts[j, i] = make_lut(hist, tw * th)
    return luts


def interp_weights(n, tile, tiles):
    """per column (row): txf = x * inv_tw - 0.5f with inv_tw = 1.0f / tileSize.width; tx1 = floor(txf), xa = txf - tx1, xa1 = 1 - xa; then tx1 clamped to >= 0
    and tx2 = tx1 + 1 (before the clamp) to <= tiles - 1.  (clahe.cpp multiplies by the float reciprocal; it does not divide.)"""
    inv = F(1.0) / F(tile)
    f = np.arange(n).astype(F) * inv - F(0.5)
    i1 = np.floor(f).astype(np.int64)
    a = f - i1.astype(F)
    a1 = F(1.0) - a
    return np.maximum(i1, 0), np.minimum(i1 + 1, tiles - 1), a, a1


def clahe(img, clip_limit=40.0, tiles=(8, 8)):
    """cv::createCLAHE(clip_limit, Size(tiles[0], tiles[1]))->apply(img, dst) on one [h, w] u8 frame, or on [batch, h, w]"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 3:
        return np.stack([clahe(f, clip_limit, tiles) for f in img])
    tx, ty = tiles
    h, w = img.shape
    tw, th, _, _ = tile_geometry(w, h, tx, ty)
    luts = tile_luts(img, clip_limit, tx, ty).astype(F)     # u8 * float is a float
    x1, x2, xa, xa1 = interp_weights(w, tw, tx)
    y1, y2, ya, ya1 = interp_weights(h, th, ty)
    v = img.astype(np.int64)
    out = np.empty_like(img)
    for y in range(h):
        p1, p2, r = luts[y1[y]], luts[y2[y]], v[y]
        res = (p1[x1, r] * xa1 + p1[x2, r] * xa) * ya1[y] + (p2[x1, r] * xa1 + p2[x2, r] * xa) * ya[y]
        out[y] = saturate_u8(res)
    return out
