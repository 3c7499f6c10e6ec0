"""NumPy float64 restatement of the frame comparison (include/rtm.h: rtm_compare), written from the header's text.

compare_ref(a, b, ...) returns (result, maps): `result` a dict of rtm_compare_result's fields, `maps` {"abs", "ssim"} the two
per-pixel maps in float64 (the device rounds them to float).  ssim_map_direct is the same S_p summed tap by tap over the
2-D window instead of separably: a second summation order, for judging the bounds.
"""
import numpy as np

DEFAULTS = {"tolerance": 1e-4, "peak": 1.0, "rel_epsilon": 1e-2, "map": "abs"}
FIELDS = ("max_abs", "mse", "psnr", "rel_mse", "ssim", "pixels", "outside", "nonfinite", "nonfinite_mismatch", "argmax_x",
          "argmax_y")
EXACT = ("pixels", "outside", "nonfinite", "nonfinite_mismatch", "max_abs", "argmax_x", "argmax_y")
RADIUS = 5


def window():
    """g[k] = exp(-k^2 / 4.5), k = -5..5."""
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    return np.exp(-(k * k) / 4.5)


def border_weights(size):
    """(size, 11): row v holds the weights g[d] / G_v of pixel v's taps v + d, 0 for the taps outside [0, size)."""
    g = window()
    v = np.arange(size)[:, None] + np.arange(-RADIUS, RADIUS + 1)[None, :]
    w = np.where((v >= 0) & (v < size), g[None, :], 0.0)
    return w / w.sum(axis=1, keepdims=True)


def counts(a, b):
    """(H, W) bool: the pixels whose six components are finite."""
    return np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)


def luminance(frame, cnt):
    f = frame.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l = (0.2126 * f[..., 0] + 0.7152 * f[..., 1]) + 0.0722 * f[..., 2]
    return np.where(cnt, l, 0.0)


def _smooth(plane, wy, wx):
    """E[plane]: the renormalised window, horizontal then vertical."""
    H, W = plane.shape
    pad = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS))
    pad[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = plane
    hor = np.zeros((H + 2 * RADIUS, W))
    for d in range(2 * RADIUS + 1):
        hor += wx[None, :, d] * pad[:, d:d + W]
    out = np.zeros((H, W))
    for d in range(2 * RADIUS + 1):
        out += wy[:, None, d] * hor[d:d + H, :]
    return out


def _ssim_from_moments(mu_a, mu_b, e_aa, e_bb, e_ab, peak):
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    var_a, var_b, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    return ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))


def ssim_map(a, b, peak=1.0):
    cnt = counts(a, b)
    la, lb = luminance(a, cnt), luminance(b, cnt)
    wy, wx = border_weights(la.shape[0]), border_weights(la.shape[1])
    return _ssim_from_moments(_smooth(la, wy, wx), _smooth(lb, wy, wx), _smooth(la * la, wy, wx), _smooth(lb * lb, wy, wx),
                              _smooth(la * lb, wy, wx), peak)


def ssim_map_direct(a, b, peak=1.0):
    """The same S_p with every moment summed over the 2-D window tap by tap, dy outer, dx inner."""
    cnt = counts(a, b)
    la, lb = luminance(a, cnt), luminance(b, cnt)
    H, W = la.shape
    wy, wx = border_weights(H), border_weights(W)
    planes = [la, lb, la * la, lb * lb, la * lb]
    pads = []
    for p in planes:
        pad = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS))
        pad[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = p
        pads.append(pad)
    m = [np.zeros((H, W)) for _ in planes]
    for dy in range(2 * RADIUS + 1):
        for dx in range(2 * RADIUS + 1):
            w = wy[:, None, dy] * wx[None, :, dx]
            for i, pad in enumerate(pads):
                m[i] += w * pad[dy:dy + H, dx:dx + W]
    return _ssim_from_moments(*m, peak)


def compare_ref(a, b, tolerance=DEFAULTS["tolerance"], peak=DEFAULTS["peak"], rel_epsilon=DEFAULTS["rel_epsilon"]):
    assert a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3 and a.dtype == b.dtype
    H, W = a.shape[:2]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)  # exact for float32
    cnt = counts(a64, b64)
    n = int(cnt.sum())
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(a64 - b64)
        D = np.maximum(np.maximum(d[..., 0], d[..., 1]), d[..., 2])
        sq = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
        rel = d * d / (b64 * b64 + rel_epsilon)
        rel = (rel[..., 0] + rel[..., 1]) + rel[..., 2]
        same = (np.isnan(a64) & np.isnan(b64)) | (a64 == b64)
    mismatch = int((~cnt & ~same.all(axis=2)).sum())
    res = {"pixels": n, "nonfinite": W * H - n, "nonfinite_mismatch": mismatch}
    if n:
        Dc = np.where(cnt, D, -1.0)
        res["max_abs"] = float(Dc.max())
        idx = int(np.argmax(Dc.ravel()))  # the first occurrence: the lowest row-major index
        res["argmax_x"], res["argmax_y"] = idx % W, idx // W
        res["outside"] = int((cnt & (D > tolerance)).sum())
        res["mse"] = float(np.sum(sq[cnt]) / (3 * n))
        res["rel_mse"] = float(np.sum(rel[cnt]) / (3 * n))
    else:
        res.update(max_abs=0.0, argmax_x=-1, argmax_y=-1, outside=0, mse=0.0, rel_mse=0.0)
    res["psnr"] = float(10 * np.log10(peak * peak / res["mse"])) if res["mse"] > 0 else float("inf")
    S = ssim_map(a64, b64, peak)
    res["ssim"] = float(S.mean())
    return res, {"abs": np.where(cnt, D, np.nan), "ssim": S}
