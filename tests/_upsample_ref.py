"""NumPy float64 restatement of rtm_upsample (include/rtm.h): the AOV-guided joint bilateral upsample, step by step.

Every array is (rows, cols) or (rows, cols, 3), row-major like the library's planes.  The tap positions are integers (the
header's rule), the spatial weights are the host's table (double, rounded through float32), and the albedo thresholds are
compared on the float32 inputs; everything else is float64.  One vectorised gather per tap."""
import numpy as np

DEFAULTS = {"factor": 2, "sigma_spatial": 0.5, "sigma_normal": 64.0, "sigma_depth": 0.05}  # kept equal to rtm.h's
EPS = np.float64(np.float32(1e-6))


def tap_base(n_out, f):
    """For the output coordinates 0 .. n_out-1: X0 = floor((2x + 1 - f) / 2f) and r = (2x + 1 - f) - 2f X0, in integers."""
    num = 2 * np.arange(n_out, dtype=np.int64) + 1 - f
    x0 = num // (2 * f)  # floor division: a negative num rounds down
    return x0, num - 2 * f * x0


def spatial_weights(r, f, sigma_spatial):
    """h[i, k] = exp(-((k - 1) - r_i / 2f)^2 / (2 sigma^2)) for dx = k - 1 in -1..2: double, rounded through float32."""
    t = np.asarray(r, np.float64) / (2.0 * f)
    d = np.arange(-1, 3, dtype=np.float64)[None, :] - t[:, None]
    s = np.float64(np.float32(sigma_spatial))
    return np.exp(-d * d / (2.0 * s * s)).astype(np.float32).astype(np.float64)


def demodulation(albedo, shape):
    """a: the albedo where it is above 1e-3f, else 1 (and 1 everywhere without an albedo plane)."""
    if albedo is None:
        return np.ones(shape, np.float64)
    alb = np.asarray(albedo, np.float32)
    return np.where(alb > np.float32(1e-3), alb, np.float32(1.0)).astype(np.float64)


def upsample_ref(color_low, low=None, high=None, factor=DEFAULTS["factor"], sigma_spatial=DEFAULTS["sigma_spatial"],
                 sigma_normal=DEFAULTS["sigma_normal"], sigma_depth=DEFAULTS["sigma_depth"], return_weights=False):
    """The upsampled frame in float64 (f h, f w, 3).  `low` / `high`: dicts of the guide planes ("depth", "normal", "albedo",
    "object") at the two resolutions; a plane counts when both hold it.  return_weights: also (matched, sum_w), where
    matched[y, x] says that some in-frame tap carried the pixel's object id."""
    color_low = np.asarray(color_low)
    h, w = color_low.shape[:2]
    f = int(factor)
    H, W = f * h, f * w
    low, high = low or {}, high or {}
    for k in set(low) | set(high):
        assert (low.get(k) is None) == (high.get(k) is None), f"plane {k} is given at one resolution only"
    plane = lambda d, k, t: None if d.get(k) is None else np.asarray(d[k], t)
    zl, zh = plane(low, "depth", np.float64), plane(high, "depth", np.float64)
    nl, nh = plane(low, "normal", np.float64), plane(high, "normal", np.float64)
    ol, oh = plane(low, "object", np.int64), plane(high, "object", np.int64)
    e = color_low.astype(np.float64) / demodulation(low.get("albedo"), color_low.shape)
    A = demodulation(high.get("albedo"), (H, W, 3))
    X0, rx = tap_base(W, f)
    Y0, ry = tap_base(H, f)
    hx, hy = spatial_weights(rx, f, sigma_spatial), spatial_weights(ry, f, sigma_spatial)
    sd, sn = np.float64(np.float32(sigma_depth)), np.float64(np.float32(sigma_normal))
    num, den = np.zeros((H, W, 3)), np.zeros((H, W))
    matched = np.zeros((H, W), bool)
    for dy in range(-1, 3):
        qy = Y0 + dy
        for dx in range(-1, 3):
            qx = X0 + dx
            inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            iy, ix = np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]  # (only to index: outside taps get w = 0)
            g = np.ones((H, W))
            if oh is not None:
                same = oh == ol[iy, ix]
                g = np.where(same, g, 0.0)
                matched |= same & inside
            both_miss = np.zeros((H, W), bool)
            if zh is not None:
                zq = zl[iy, ix]
                ip, iq = np.isinf(zh), np.isinf(zq)
                both_miss = ip & iq
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    wz = np.exp(-np.abs(zh - zq) / (sd * f * np.maximum(zh, zq))) if sd > 0 else np.ones((H, W))
                wz = np.where(ip != iq, 0.0, wz)
                g = g * np.where(both_miss, 1.0, wz)
            if nh is not None and sn > 0:
                wn = np.maximum(0.0, np.sum(nh * nl[iy, ix], axis=-1)) ** sn
                g = g * np.where(both_miss, 1.0, wn)
            wgt = np.where(inside, hy[:, dy + 1][:, None] * hx[:, dx + 1][None, :] * (g + EPS), 0.0)
            num += wgt[..., None] * e[iy, ix]
            den += wgt
    out = num / den[..., None] * A
    return (out, matched, den) if return_weights else out


def sample_low(plane, f):
    """The low-resolution guide of a full-resolution plane: the value at each low pixel's centre ((f X + f // 2, f Y + f // 2),
    the full-resolution pixel that holds the centre; for an even f, the one just past it)."""
    return np.ascontiguousarray(np.asarray(plane)[f // 2::f, f // 2::f])


def tolerance_excess(got, ref):
    """max over components of |got - ref| / max(1, |ref|): rtm.h's accuracy bar is 1e-4."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if got.size else 0.0


THIN_ID = 9  # the object of synthetic_case that no low pixel samples


def synthetic_case(w, h, f, seed):
    """A low colour frame (4 u^2 noise) and guides built on the full grid, then sampled at the low pixels' centres: up to four
    object regions cut by slanted edges, a +inf depth patch (object -1), unit normals per region with small noise, depths per
    region with small noise, albedo in [0, 1] with some components below 1e-3, and one full-resolution column of object
    THIN_ID that lies between the low centres, so that no low tap carries its id.  Returns (color_low, low, high, thin),
    thin the (H, W) mask of that column."""
    rng = np.random.default_rng(seed)
    H, W = f * h, f * w
    yy, xx = np.mgrid[0:H, 0:W]
    region = np.minimum(3, (xx + yy // 2) * 4 // max(1, W + H // 2)).astype(np.int32)
    base = rng.standard_normal((4, 3))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    n = base[region] + 0.02 * rng.standard_normal((H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    depth = (1.0 + 0.5 * region + 0.01 * rng.random((H, W))).astype(np.float32)
    obj = region.copy()
    miss = (yy >= H // 3) & (yy < H // 3 + max(1, H // 4)) & (xx >= W // 4) & (xx < W // 4 + max(1, W // 5))
    depth[miss] = np.inf
    obj[miss] = -1
    xt = f * (w // 2) + (f // 2 + 1) % f  # never f X + f // 2: no low centre lies on it
    thin = xx == xt
    obj[thin] = THIN_ID
    depth[thin] = np.float32(1.25)
    albedo = rng.random((H, W, 3)).astype(np.float32)
    albedo[rng.random((H, W, 3)) < 0.05] = 0.0
    albedo[rng.random((H, W, 3)) < 0.03] = np.float32(5e-4)
    high = {"depth": depth, "normal": n.astype(np.float32), "albedo": albedo, "object": obj}
    low = {k: sample_low(v, f) for k, v in high.items()}
    assert not np.any(low["object"] == THIN_ID)
    u = rng.random((h, w, 3))
    return (4.0 * u * u).astype(np.float32), low, high, thin
