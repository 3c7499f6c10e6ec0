"""NumPy restatement of rtm_firefly (include/rtm.h), written from the header text, and the frame recipe of
test_firefly_host.py / test_firefly_gpu.py.  The decisions (Y, n, S, T, the mask) are computed in float32 in the contract's
order, so that they are the library's bit for bit; the values of the changed pixels (a clamped pixel's c (T / Y), a repaired
pixel's mean) are computed in float64 from those float32 T and Y.  One pass of whole-frame array operations per tap."""
import numpy as np

from _denoise_ref import tolerance_excess  # noqa: F401  (max |got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)
from _tonemap_ref import quantise_u8  # noqa: F401  (rtm_quantise of (double)out_f32)

DEFAULTS = {"radius": 1, "rank": 3, "k": 4.0, "floor": 0.01, "repair": True}  # rtm.h's RTM_FIREFLY_DEFAULTS
F = np.float32


def counts(color):
    """Step 1: the pixels whose three components are finite."""
    return np.all(np.isfinite(np.asarray(color, np.float32)), axis=-1)


def luminance(color):
    """Step 1 in float32: Y = max(l, +0) of a pixel that counts, -1 of one that does not."""
    c = np.asarray(color, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        l = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
        y = np.where(l > 0, l, F(0.0)).astype(np.float32)
    return np.where(counts(c), y, F(-1.0)).astype(np.float32)


def taps(radius):
    """Step 2's offsets (dy, dx), dy outer and dx inner, the centre excluded."""
    r = int(radius)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]


def _shifted(plane, radius, dy, dx, fill):
    """plane[y + dy, x + dx], `fill` outside the frame."""
    h, w = plane.shape[:2]
    pad = np.pad(plane, [(radius, radius), (radius, radius)] + [(0, 0)] * (plane.ndim - 2), constant_values=fill)
    return pad[radius + dy:radius + dy + h, radius + dx:radius + dx + w]


def decide(color, radius=DEFAULTS["radius"], rank=DEFAULTS["rank"], k=DEFAULTS["k"], floor=DEFAULTS["floor"], select="sort",
           order=None):
    """Steps 1-5 in float32: (Y, n, T, firefly).  Y is -1 where a pixel does not count, T +inf where there is no statistic.
    select: "sort" sorts the taps' values and takes index rank - 1; "chain" keeps the rank largest by the insertion chain of
    max / min the kernel uses.  order: a permutation of the taps' visiting order (a selection cannot depend on it)."""
    y = luminance(color)
    offs = taps(radius)
    if order is not None:
        offs = [offs[i] for i in order]
    vals = np.stack([_shifted(y, radius, dy, dx, F(-1.0)) for dy, dx in offs])  # -1: outside the frame or not counting
    n = (vals >= 0).sum(axis=0)
    if select == "sort":
        s = -np.sort(-vals, axis=0)[rank - 1] if rank <= len(offs) else np.full(y.shape, F(-1.0))
    else:
        top = [np.full(y.shape, F(-1.0)) for _ in range(rank)]
        for v in vals:
            for j in range(rank):
                top[j], v = np.maximum(top[j], v), np.minimum(top[j], v)
        s = top[rank - 1]
    has = (y >= 0) & (n >= rank)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (F(k) * s.astype(np.float32)) + F(floor)  # two roundings, in float32
    t = np.where(has, t, F(np.inf)).astype(np.float32)
    return y, n, t, has & (y > t)


def firefly_ref(color, radius=DEFAULTS["radius"], rank=DEFAULTS["rank"], k=DEFAULTS["k"], floor=DEFAULTS["floor"],
                repair=DEFAULTS["repair"], **how):
    """{"out": float64 (H, W, 3), "mask": uint8, "threshold": float32, "Y": float32, "n": int}.  out is the input where the
    mask is 0 (compare those pixels by their words, taken from the input itself)."""
    c32 = np.asarray(color, np.float32)
    y, n, t, fire = decide(c32, radius, rank, k, floor, **how)
    out = c32.astype(np.float64)
    mask = np.zeros(y.shape, np.uint8)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        scale = t.astype(np.float64) / y.astype(np.float64)
    out[fire] = out[fire] * scale[fire][:, None]
    mask[fire] = 1
    if repair:
        bad = y < 0
        ok = (y >= 0)
        c0 = np.where(ok[..., None], c32.astype(np.float64), 0.0)
        total = np.zeros(out.shape, np.float64)
        for dy, dx in taps(radius):
            total = total + _shifted(c0, radius, dy, dx, 0.0)  # a tap that is skipped adds nothing
        mean = np.where(n[..., None] > 0, total / np.maximum(n, 1)[..., None], 0.0)
        out[bad] = mean[bad]
        mask[bad] = 2
    return {"out": out, "mask": mask, "threshold": t, "Y": y, "n": n}


# ---- the frame recipe ---------------------------------------------------------------------------------------------------
# One block of planted features, 32 x 16 pixels, every feature further than radius 1 from the next.  (x, y) in the block.
SPIKES = (((3, 3), 50.0), ((8, 3), 1000.0), ((13, 3), 200.0))  # isolated, times the pixel's own value
CLUSTER2 = ((18, 3), (19, 3))
CLUSTER3 = ((23, 3), (24, 3), (23, 4))
BLOCK = tuple((x, y) for y in (2, 3) for x in (28, 29))             # 2 x 2, one bright value
RECT = tuple((x, y) for y in (7, 8, 9) for x in (0, 1, 2, 3))       # 4 x 3, one bright value; the first block's touches x = 0
LINE = tuple((x, 12) for x in range(8, 16))                         # one pixel wide, one bright value
TIES = tuple((x, y) for y in range(7, 12) for x in range(18, 24))   # greys quantised to four values
ZEROS = tuple((x, y) for y in (7, 8, 9) for x in range(26, 30))
NEGATIVE = tuple((x, y) for y in (12, 13, 14) for x in range(26, 30))  # (two rows below ZEROS: one bright row between two
#                                                                       dark patches would be a one-pixel line)
NONFINITE = (((5, 14), (np.nan, 0.5, 0.5)), ((6, 14), (0.5, np.inf, 0.5)), ((16, 14), (0.5, 0.5, -np.inf)),
             ((20, 14), (np.nan, np.nan, np.nan)))  # the first two are adjacent
BLOCK_W, BLOCK_H = 32, 16


def block_origins(w, h):
    """Where frame(w, h) plants its blocks: (0, 0) when the frame holds one, and a second one across tile seams (32 x 16
    tiles) in a frame of 64 x 36 or more."""
    if w < BLOCK_W or h < BLOCK_H:
        return []
    return [(0, 0)] + ([(w - 40, h - 20)] if w >= 64 and h >= 36 else [])


def frame(w, h):
    """(color, marks): a seeded smooth gradient with mild noise, float32 (h, w, 3), and marks: name -> bool (h, w) of the
    planted pixels.  A frame that holds a block gets the features above (spikes, clusters, the 2 x 2 block, the rectangle at
    the frame's edge, the line, the patches of ties, zeros and negative components, four non-finite pixels); a smaller one a
    spike in its middle from 5 pixels on and two adjacent non-finite pixels from 5 x 3 on.  From 3 pixels on the last pixel,
    a frame corner, is NaN."""
    rng = np.random.default_rng(1000 * w + h)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    base = 0.2 + 0.6 * xx / w + 0.3 * yy / h
    color = (base[..., None] * np.array([1.0, 0.9, 0.8]) * (1.0 + 0.05 * (2.0 * rng.random((h, w, 3)) - 1.0))).astype(np.float32)
    names = ("spikes", "cluster2", "cluster3", "block", "rect", "line", "line_inner", "ties", "zeros", "negative", "nonfinite")
    marks = {k: np.zeros((h, w), bool) for k in names}

    def put(name, x, y, value):
        color[y, x] = value
        marks[name][y, x] = True

    for ox, oy in block_origins(w, h):
        for (x, y), gain in SPIKES:
            put("spikes", ox + x, oy + y, color[oy + y, ox + x] * F(gain))
        for x, y in CLUSTER2:
            put("cluster2", ox + x, oy + y, color[oy + y, ox + x] * F(100.0))
        for x, y in CLUSTER3:
            put("cluster3", ox + x, oy + y, color[oy + y, ox + x] * F(100.0))
        for x, y in BLOCK:
            put("block", ox + x, oy + y, F(30.0))
        for x, y in RECT:
            put("rect", ox + x, oy + y, F(20.0))
        for x, y in LINE:
            put("line", ox + x, oy + y, F(25.0))
            marks["line_inner"][oy + y, ox + x] = LINE[0][0] < x < LINE[-1][0]
        for x, y in TIES:
            put("ties", ox + x, oy + y, F(0.25) * F(1 + rng.integers(4)))
        for x, y in ZEROS:
            put("zeros", ox + x, oy + y, F(0.0))
        for i, (x, y) in enumerate(NEGATIVE):  # a negative luminance, or a positive one with a negative component
            put("negative", ox + x, oy + y, (F(-0.5), F(0.1), F(0.2)) if i % 2 else (F(0.6), F(-0.05), F(0.3)))
        for (x, y), value in NONFINITE:
            put("nonfinite", ox + x, oy + y, np.array(value, np.float32))
    if not block_origins(w, h):
        if w * h >= 5:
            i = (w * h) // 2
            put("spikes", i % w, i // w, color[i // w, i % w] * F(100.0))
        if w >= 5 and h >= 3:
            put("nonfinite", 0, 0, np.array([0.5, np.inf, 0.5], np.float32))
            put("nonfinite", 1, 0, np.array([np.nan, 0.5, 0.5], np.float32))
    if w * h >= 3:
        put("nonfinite", w - 1, h - 1, np.array([np.nan, 0.25, 0.25], np.float32))
    for k in names:
        if k != "nonfinite":
            marks[k] &= ~marks["nonfinite"]  # (a corner NaN planted over a feature)
    return color, marks
