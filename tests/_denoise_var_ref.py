"""NumPy float64 restatement of rtm_denoise_variance (include/rtm.h): the variance-guided à-trous filter, step by step.

Built from the pieces of _denoise_ref (the shifted frame, the demodulation, the geometry weight); arrays as there."""
import numpy as np

from _denoise_ref import H_TAPS, demodulation, geometry_weight, shifted, tolerance_excess  # noqa: F401

K_TAPS = (1.0 / 4, 1.0 / 2, 1.0 / 4)
LUM = np.array([0.2126, 0.7152, 0.0722])
DEFAULTS = {"iterations": 5, "sigma_lum": 4.0, "sigma_normal": 64.0, "sigma_depth": 0.05}  # kept equal to rtm.h's


def luminance(e):
    return e @ LUM


def variance_estimate(e, z, n, o, sigma_normal, sigma_depth):
    """v0: the g_1-weighted moments of d = l_q - l_p over the 7 x 7 window, max(0, m2 - m1^2)."""
    l = luminance(e)
    U, s1, s2 = np.zeros_like(l), np.zeros_like(l), np.zeros_like(l)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            lq, inside = shifted(l, dy, dx)
            u = np.where(inside, geometry_weight(l.shape, 1, dy, dx, z, n, o, sigma_normal, sigma_depth), 0.0)
            d = np.where(inside, lq - l, 0.0)
            U += u
            s1 += u * d
            s2 += u * d * d
    m1, m2 = s1 / U, s2 / U
    return np.maximum(0.0, m2 - m1 * m1)


def prefiltered(v):
    """v~: the 3 x 3 {1/4, 1/2, 1/4} blur of v over the in-frame taps, normalised."""
    num, den = np.zeros_like(v), np.zeros_like(v)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            vq, inside = shifted(v, dy, dx)
            k = np.where(inside, K_TAPS[dy + 1] * K_TAPS[dx + 1], 0.0)
            num += k * vq
            den += k
    return num / den


def denoise_variance_ref(color, depth=None, normal=None, albedo=None, obj=None, iterations=DEFAULTS["iterations"],
                         sigma_lum=DEFAULTS["sigma_lum"], sigma_normal=DEFAULTS["sigma_normal"],
                         sigma_depth=DEFAULTS["sigma_depth"]):
    """(out, v0) in float64: the filtered frame (H, W, 3) and the variance estimate (H, W).  Guide planes may be None."""
    color = np.asarray(color)
    a = demodulation(albedo, color.shape)
    e = color.astype(np.float64) / a
    z = None if depth is None else np.asarray(depth, np.float64)
    n = None if normal is None else np.asarray(normal, np.float64)
    o = None if obj is None else np.asarray(obj, np.int64)
    v0 = variance_estimate(e, z, n, o, sigma_normal, sigma_depth)
    if iterations == 0:
        return color.astype(np.float64), v0
    v = v0
    for i in range(iterations):
        s = 1 << i
        l = luminance(e)
        scale = sigma_lum * np.sqrt(prefiltered(v)) + np.float64(np.float32(1e-4))
        num, den, vnum = np.zeros_like(e), np.zeros(e.shape[:2]), np.zeros(e.shape[:2])
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                eq, inside = shifted(e, s * dy, s * dx)
                vq, _ = shifted(v, s * dy, s * dx)
                w = H_TAPS[dy + 2] * H_TAPS[dx + 2] * geometry_weight(e.shape[:2], s, dy, dx, z, n, o, sigma_normal, sigma_depth)
                if sigma_lum > 0:
                    lq, _ = shifted(l, s * dy, s * dx)
                    w = w * np.exp(-np.abs(l - lq) / scale)
                w = np.where(inside, w, 0.0)
                num += w[..., None] * eq
                den += w
                vnum += w * w * vq
        e = num / den[..., None]
        v = vnum / (den * den)
    return e * a, v0
