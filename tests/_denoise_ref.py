"""NumPy float64 restatement of rtm_denoise (include/rtm.h): the edge-avoiding à-trous filter, step by step.

Every array is (H, W) or (H, W, 3), row-major like the library's planes.  The whole frame is one vectorised operation per
tap: the tap's neighbours are the frame shifted by (s·dy, s·dx), with a mask for the taps that fall outside it."""
import numpy as np

H_TAPS = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
DEFAULTS = {"iterations": 4, "sigma_color": 16.0, "sigma_normal": 64.0, "sigma_depth": 0.05}  # kept equal to rtm.h's


def shifted(a, oy, ox, fill=0):
    """b[y, x] = a[y + oy, x + ox] where that is inside the frame, else `fill`; and the inside mask."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def demodulation(albedo, shape):
    """a_p,k: the albedo where it is above 1e-3f, else 1 (and 1 everywhere without an albedo plane)."""
    if albedo is None:
        return np.ones(shape, np.float64)
    alb = np.asarray(albedo, np.float32)
    return np.where(alb > np.float32(1e-3), alb, np.float32(1.0)).astype(np.float64)


def geometry_weight(shape, s, dy, dx, depth, normal, obj, sigma_normal, sigma_depth):
    """g(p, q) for every p, q = p + s·(dx, dy) (inside or not: the caller masks the outside taps)."""
    if dy == 0 and dx == 0:
        return np.ones(shape)
    g = np.ones(shape)
    if obj is not None:
        oq, _ = shifted(obj, s * dy, s * dx, fill=-2)
        g = np.where(obj == oq, g, 0.0)
    both_miss = np.zeros(shape, bool)
    if depth is not None:
        zq, _ = shifted(depth, s * dy, s * dx, fill=np.inf)
        ip, iq = np.isinf(depth), np.isinf(zq)
        both_miss = ip & iq
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if sigma_depth > 0:
                wz = np.exp(-np.abs(depth - zq) / (sigma_depth * s * np.maximum(depth, zq)))
            else:
                wz = np.ones(shape)
        wz = np.where(ip != iq, 0.0, wz)
        g = g * np.where(both_miss, 1.0, wz)
    if normal is not None and sigma_normal > 0:
        nq, _ = shifted(normal, s * dy, s * dx)
        wn = np.maximum(0.0, np.sum(normal * nq, axis=-1)) ** sigma_normal
        g = g * np.where(both_miss, 1.0, wn)
    return g


def denoise_ref(color, depth=None, normal=None, albedo=None, obj=None, iterations=DEFAULTS["iterations"],
                sigma_color=DEFAULTS["sigma_color"], sigma_normal=DEFAULTS["sigma_normal"],
                sigma_depth=DEFAULTS["sigma_depth"]):
    """The filtered frame in float64 (H, W, 3).  Guide planes may be None: that term is off."""
    color = np.asarray(color)
    if iterations == 0:
        return color.astype(np.float64)
    a = demodulation(albedo, color.shape)
    e = color.astype(np.float64) / a
    z = None if depth is None else np.asarray(depth, np.float64)
    n = None if normal is None else np.asarray(normal, np.float64)
    o = None if obj is None else np.asarray(obj, np.int64)
    for i in range(iterations):
        s = 1 << i
        num, den = np.zeros_like(e), np.zeros(e.shape[:2])
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                eq, inside = shifted(e, s * dy, s * dx)
                w = H_TAPS[dy + 2] * H_TAPS[dx + 2] * geometry_weight(e.shape[:2], s, dy, dx, z, n, o, sigma_normal, sigma_depth)
                if sigma_color > 0:
                    w = w * np.exp(-np.sum((e - eq) ** 2, axis=-1) * 4.0 ** i / (sigma_color * sigma_color))
                w = np.where(inside, w, 0.0)
                num += w[..., None] * eq
                den += w
        e = num / den[..., None]
    return e * a


def tolerance_excess(got, ref):
    """max over components of |got - ref| / max(1, |ref|): rtm.h's accuracy bar is 1e-4."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if got.size else 0.0
