"""NumPy restatement of rtm_defocus (include/rtm.h): the count rule, the circle of confusion, the choice of disc per tap, the
weight and the combine, in float64 (or in the `dtype` asked for), written from the header text.  One pass of whole-frame array
operations per offset of the (2R+1)^2 window, rows first, then columns.  The ground truth of test_defocus_host.py /
test_defocus_gpu.py, and the frame recipe both use."""
import numpy as np

from _denoise_ref import tolerance_excess  # noqa: F401  (max |got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)
from _tonemap_ref import quantise_u8  # noqa: F401  (rtm_quantise of (double)out_f32)

DEFAULTS = {"aperture": 4.0, "max_radius": 8}  # rtm.h's RTM_DEFOCUS_DEFAULTS; focus_distance has none
PI_F = np.float32(np.pi)
FLT_MAX = np.finfo(np.float32).max
DISCS = (((0.3, 0.4), 0.2, 1.0), ((0.7, 0.6), 0.25, 4.0), ((0.55, 0.3), 0.12, 9.0))  # (centre, radius, depth) of frame()


def counts(color, depth):
    """Step 1: the pixels whose three colour components are finite and whose depth is > 0 (+inf counts, NaN does not)."""
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(np.asarray(color, np.float64)), axis=-1) & (np.asarray(depth, np.float64) > 0)


def disc_mask(w, h, which):
    """The pixels of frame()'s disc `which` (0, 1, 2) as drawn, before a later disc covers some of them."""
    (fx, fy), fr, _ = DISCS[which]
    y, x = np.mgrid[:h, :w]
    return (x - fx * w) ** 2 + (y - fy * h) ** 2 <= (fr * min(w, h)) ** 2


def frame(w, h):
    """The test frames: colour 8 u^4 (a long dark tail and highlights above 1); depth +inf, the left half a ramp from 2 to 8
    down the rows, three discs at the depths 1, 4 and 9 drawn in that order; beyond two pixels one NaN-colour pixel, one
    +inf-colour pixel and one NaN-depth pixel."""
    rng = np.random.default_rng(1000 * w + h)
    color = (8 * rng.random((h, w, 3)) ** 4).astype(np.float32)
    depth = np.full((h, w), np.inf, np.float32)
    depth[:, : w // 2] = np.linspace(2.0, 8.0, h, dtype=np.float32)[:, None]
    for i, (_, _, z) in enumerate(DISCS):
        depth[disc_mask(w, h, i)] = z
    if w * h > 2:
        color.reshape(-1, 3)[(w * h) // 2] = [np.nan, 0.5, 0.5]
        color.reshape(-1, 3)[w * h - 1] = [0.5, np.inf, 0.5]
        depth.reshape(-1)[(w * h) // 3] = np.nan
    return color, depth


def coc(depth, ok, focus_distance, aperture, max_radius, dtype=np.float64):
    """Step 2: (s, ia), both 0 where the pixel does not count."""
    f = dtype
    z = np.asarray(depth, f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # z = +inf: the quotient is +0; one that overflows counts as the largest float (A = 0 gives -0, not NaN)
        s = f(aperture) * np.maximum(f(1) - f(focus_distance) / z, f(-FLT_MAX))
        s = np.minimum(np.maximum(s, f(-max_radius)), f(max_radius))
        m = np.maximum(np.abs(s), f(0.5))
        ia = f(1) / ((f(PI_F) * m) * m)
    return np.where(ok, s, f(0)).astype(f), np.where(ok, ia, f(0)).astype(f)


def defocus_ref(color, depth, focus_distance, aperture=DEFAULTS["aperture"], max_radius=DEFAULTS["max_radius"], dtype=np.float64):
    """(out, s): out per step 6 where the pixel counts and a tap other than the centre weighs more than +0, the input
    elsewhere; s the signed radius, +0 where the pixel does not count."""
    f = dtype
    R = int(max_radius)
    c = np.asarray(color, f)
    ok = counts(color, depth)
    h, w = ok.shape
    s, ia = coc(depth, ok, focus_distance, aperture, R, f)
    r = np.abs(s)
    c0 = np.where(ok[..., None], c, f(0))
    z0 = np.where(ok, np.asarray(depth, f), f(np.nan))

    def padded(a, fill):
        return np.pad(a, [(R, R), (R, R)] + [(0, 0)] * (a.ndim - 2), constant_values=fill)

    cq_all, zq_all, rq_all, iaq_all = padded(c0, f(0)), padded(z0, f(np.nan)), padded(r, f(0)), padded(ia, f(0))
    sw = np.zeros((h, w), f)
    sc = np.zeros((h, w, 3), f)
    others = np.zeros((h, w), bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d = np.sqrt(f(dx * dx + dy * dy)).astype(f)
            win = (slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
            zq, rq, iaq = zq_all[win], rq_all[win], iaq_all[win]  # a tap outside the frame or not counting has ia = 0
            with np.errstate(invalid="ignore"):
                own = (zq > z0) & (r < rq)
            re, iae = np.where(own, r, rq), np.where(own, ia, iaq)
            wgt = (np.minimum(np.maximum(re + f(0.5) - d, f(0)), f(1)) * iae).astype(f)
            if dx or dy:
                others |= wgt > 0
            sw = sw + wgt
            sc = sc + wgt[..., None] * cq_all[win]
    blurred = ok & others
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(blurred[..., None], sc / sw[..., None], c)
    return out, s
