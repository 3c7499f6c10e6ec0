"""rtm_resize (include/rtm.h) restated in float64 NumPy, from the header's text: the integer taps, the tables rounded to
float32 and widened again, the two matrices, the normalised convolution with the counting rule, the threshold, and the work
buffer's size.  The ground truth of tests/test_resize_host.py and tests/test_resize_gpu.py."""
import functools
import math

import numpy as np

from _denoise_ref import tolerance_excess  # noqa: F401  (|got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)
from _tonemap_ref import counts as _counts3, quantise_u8  # noqa: F401

FILTERS = ("box", "triangle", "mitchell", "lanczos3")  # RTM_RESIZE_BOX .. RTM_RESIZE_LANCZOS3
TWICE_RADIUS = {"box": 1, "triangle": 2, "mitchell": 4, "lanczos3": 6}  # q = 2 r
DEFAULTS = {"filter": "mitchell"}
MIN_WEIGHT = 0.0625  # D below it: the pixel is NaN
SIZE_MAX = 2 ** 64 - 1


def counts(src):
    """Step 4: the pixels all of whose components are finite; (h, w) for a frame and for a plane."""
    src = np.asarray(src)
    return _counts3(src) if src.ndim == 3 else np.isfinite(src.astype(np.float64))


def kernel(filter, t):
    """Step 1: k(t) for a Python float t (BOX is decided in integers by taps())."""
    a = abs(t)
    if filter == "triangle":
        return max(0.0, 1.0 - a)
    if filter == "mitchell":
        if a < 1.0:
            return (7.0 * a * a * a - 12.0 * a * a + 16.0 / 3.0) / 6.0
        if a < 2.0:
            return (-7.0 / 3.0 * a * a * a + 12.0 * a * a - 20.0 * a + 32.0 / 3.0) / 6.0
        return 0.0
    assert filter == "lanczos3"
    if a == 0.0:
        return 1.0
    if a >= 3.0:
        return 0.0
    x = math.pi * t
    return (math.sin(x) / x) * (math.sin(x / 3.0) / (x / 3.0))


def tap_count(filter, n, N):
    q, M = TWICE_RADIUS[filter], max(n, N)
    return (q * M + N - 1) // N  # ceil(q M / N)


def taps(filter, n, N, X):
    """Step 2 for destination index X of an axis n -> N: (j0, the T raw weights k(t_i)), in Python integers and floats."""
    q, M = TWICE_RADIUS[filter], max(n, N)
    b = (2 * X + 1) * n - N
    j0 = (b - q * M) // (2 * N) + 1  # Python's // floors toward minus infinity
    raw = []
    for i in range(tap_count(filter, n, N)):
        a = 2 * N * (j0 + i) - b
        if filter == "box":
            raw.append(1.0 if -M < a <= M else 0.0)
        else:
            raw.append(kernel(filter, a / (2 * M)))
    return j0, raw


@functools.lru_cache(maxsize=None)
def table(filter, n, N):
    """Step 3: (j0[N] int64, w[N][T] float64 holding float32 values): the weights over the sum of all T raw weights, evaluated
    in double, rounded to float32, widened."""
    T = tap_count(filter, n, N)
    j0 = np.zeros(N, np.int64)
    w = np.zeros((N, T), np.float64)
    for X in range(N):
        j0[X], raw = taps(filter, n, N, X)
        total = sum(raw)  # ascending, as the device adds them
        assert total > 0.0
        w[X] = np.array([k / total for k in raw], np.float64).astype(np.float32)
    j0.setflags(write=False)
    w.setflags(write=False)
    return j0, w


@functools.lru_cache(maxsize=None)
def matrix(filter, n, N):
    """The (N, n) matrix of an axis: the table's weights at their source indices; taps outside the frame are skipped."""
    j0, w = table(filter, n, N)
    m = np.zeros((N, n), np.float64)
    for X in range(N):
        for i in range(w.shape[1]):
            j = int(j0[X]) + i
            if 0 <= j < n:
                m[X, j] += w[X, i]
    m.setflags(write=False)
    return m


def resize_ref(src, size, filter="mitchell"):
    """Steps 4-6 in float64: (out, D), out (H, W, C) or (H, W) with NaN where D < 1/16, D the (H, W) normalising weight."""
    src = np.asarray(src)
    plane = src.ndim == 2
    h, w = src.shape[:2]
    H, W = size
    ok = counts(src)
    c = np.where(ok[..., None], src.reshape(h, w, -1).astype(np.float64), 0.0)  # selected out
    rec = np.concatenate([c, ok[..., None].astype(np.float64)], axis=-1)         # the records (m c, m)
    mx, my = matrix(filter, w, W), matrix(filter, h, H)
    horizontal = np.einsum("Xx,yxk->yXk", mx, rec)
    vertical = np.einsum("Yy,yXk->YXk", my, horizontal)
    D = vertical[..., -1]
    hole = np.asarray(D, np.float64) < MIN_WEIGHT
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(hole[..., None], np.nan, vertical[..., :-1] / np.where(hole, 1.0, D)[..., None])
    return (out[..., 0] if plane else out), D


def resize_direct(src, size, filter="mitchell"):
    """The same value without the separation: every destination pixel as one 2-D sum over its Tx Ty taps."""
    src = np.asarray(src)
    plane = src.ndim == 2
    h, w = src.shape[:2]
    H, W = size
    ok = counts(src)
    c = src.reshape(h, w, -1).astype(np.float64)
    (j0x, wx), (j0y, wy) = table(filter, w, W), table(filter, h, H)
    out = np.full((H, W, c.shape[2]), np.nan)
    for Y in range(H):
        for X in range(W):
            num, den = np.zeros(c.shape[2]), 0.0
            for iy in range(wy.shape[1]):
                y = int(j0y[Y]) + iy
                if not 0 <= y < h:
                    continue
                for ix in range(wx.shape[1]):
                    x = int(j0x[X]) + ix
                    if 0 <= x < w and ok[y, x]:
                        num += wy[Y, iy] * wx[X, ix] * c[y, x]
                        den += wy[Y, iy] * wx[X, ix]
            if den >= MIN_WEIGHT:
                out[Y, X] = num / den
    return out[..., 0] if plane else out


def _round256(v):
    return (v + 255) // 256 * 256


def work_bytes(w, h, W, H, filter, channels):
    """rtm_resize_work_bytes: the records, the two tables, the two j0 arrays, each rounded up to 256 bytes; `filter` by index
    or by name."""
    name = filter if isinstance(filter, str) else (FILTERS[filter] if 0 <= filter < len(FILTERS) else None)
    if min(w, h, W, H) <= 0 or name not in FILTERS or channels not in (1, 3):
        return 0
    rec = 16 if channels == 3 else 8
    parts = (rec * W * h, 4 * W * tap_count(name, w, W), 4 * H * tap_count(name, h, H), 4 * (W + H))
    if any(p > SIZE_MAX - 255 for p in parts):
        return SIZE_MAX
    total = sum(_round256(p) for p in parts)
    return total if total <= SIZE_MAX else SIZE_MAX


def frame(w, h, channels=3, seed=0):
    """The tests' input: uniform in [0, 4) with three pixels at 12.0, the Cornell light's emission (fewer on a frame of
    fewer pixels)."""
    rng = np.random.default_rng(1000003 * w + 1009 * h + 7 * channels + seed)
    f = (rng.random((h, w, channels)) * 4.0).astype(np.float32)
    for k in range(min(3, w * h)):
        p = (k * 7919 + 13) % (w * h) if w * h > 3 else k
        f[p // w, p % w] = 12.0
    return f[..., 0].copy() if channels == 1 else f


def holes_frame(channels=3):
    """The 16 x 16 frame of the holes test: rows 3..8, columns 4..9 do not count — NaN, one +inf, and (for a frame) one pixel
    with a single NaN component."""
    f = frame(16, 16, channels, seed=5).reshape(16, 16, -1).copy()
    f[3:9, 4:10] = np.nan
    f[4, 5] = np.inf
    f[6, 7] = 1.5
    f[6, 7, -1] = np.nan
    return f[..., 0].copy() if channels == 1 else f
