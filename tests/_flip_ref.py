"""NumPy float64 restatement of the perceptual frame difference (include/rtm.h: rtm_flip), written from the header's text.

flip_ref(a, b, transfer, ppd) returns (result, map): `result` a dict of rtm_flip_result's fields (hist included), `map` the
per-pixel difference in float64 with NaN at the non-counting pixels (the device rounds it to float).  The evaluation exists
twice: order="separable" uses the 1-D tables the header states, horizontal pass then vertical pass, as the kernels do;
order="direct" forms every 2-D filter on its (2r+1)^2 grid, normalises it there as the published program does, and sums tap
by tap.  Their disagreement is what the tolerance of the tests is measured from.
"""
import numpy as np

DEFAULT_PPD = 0.7 * 3840 / 0.7 * np.pi / 180
DEFAULTS = {"transfer": "srgb", "pixels_per_degree": DEFAULT_PPD}
FIELDS = ("mean", "max", "min", "pixels", "nonfinite", "argmax_x", "argmax_y", "hist")
PPD_MIN, PPD_MAX = 8.0, 128.0

M_ROWS = ((10135552.0 / 24577794.0, 8788810.0 / 24577794.0, 4435075.0 / 24577794.0),
          (2613072.0 / 12288897.0, 8788810.0 / 12288897.0, 887015.0 / 12288897.0),
          (1425312.0 / 73733382.0, 8788810.0 / 73733382.0, 70074185.0 / 73733382.0))
M = np.array(M_ROWS)
WHITE = tuple((M[i, 0] + M[i, 1]) + M[i, 2] for i in range(3))  # M (1, 1, 1)
M_INV = np.linalg.inv(M)
CSF_B = {"y": 0.0047, "cx": 0.0053, "cz1": 0.04, "cz2": 0.025}
CZ_A1, CZ_A2 = 34.1 * np.sqrt(np.pi / 0.04), 13.5 * np.sqrt(np.pi / 0.025)


def csf_radius(ppd):
    return int(np.ceil(3.0 * np.sqrt(0.04 / (2.0 * np.pi ** 2)) * ppd))


def feature_sigma(ppd):
    return 0.5 * 0.082 * ppd


def feature_radius(ppd):
    return int(np.ceil(3.0 * feature_sigma(ppd)))


def _e(b, ppd, r):
    k = np.arange(-r, r + 1, dtype=np.float64)
    return np.exp(-np.pi ** 2 * (k / ppd) ** 2 / b)


def csf_tables(ppd):
    """The 1-D tables of step 4, each used in both axes: y and cx sum to 1; cz1 and cz2 are sqrt(A_i / S) e_i with S the
    sum of the 2-D Cz filter, so that the two separable parts share one normaliser."""
    r = csf_radius(ppd)
    ey, ex, e1, e2 = (_e(CSF_B[k], ppd, r) for k in ("y", "cx", "cz1", "cz2"))
    s = CZ_A1 * e1.sum() ** 2 + CZ_A2 * e2.sum() ** 2
    return {"y": ey / ey.sum(), "cx": ex / ex.sum(), "cz1": np.sqrt(CZ_A1 / s) * e1, "cz2": np.sqrt(CZ_A2 / s) * e2}


def csf_filters_2d(ppd):
    """The three 2-D filters as the published program forms them: each divided by its own sum over the grid."""
    r = csf_radius(ppd)
    out = {}
    for name in ("y", "cx"):
        e = _e(CSF_B[name], ppd, r)
        f = e[:, None] * e[None, :]
        out[name] = f / f.sum()
    e1, e2 = _e(0.04, ppd, r), _e(0.025, ppd, r)
    f = CZ_A1 * e1[:, None] * e1[None, :] + CZ_A2 * e2[:, None] * e2[None, :]
    out["cz"] = f / f.sum()
    return out


def feature_tables(ppd):
    """g, d, p of step 6 as 1-D tables: g / sum g; d over the sum of its positive values (its negative ones have the same
    magnitude); p's positive values over their sum and its negative values over the magnitude of theirs."""
    sigma, rf = feature_sigma(ppd), feature_radius(ppd)
    k = np.arange(-rf, rf + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    d = -k * g
    p = (k * k / (sigma * sigma) - 1.0) * g
    return {"g": g / g.sum(), "d": d / d[d > 0].sum(),
            "p": np.where(p > 0, p / p[p > 0].sum(), p / -p[p < 0].sum())}


def feature_filters_2d(ppd):
    """The x-direction edge and point filters on the (2 rf + 1)^2 grid, indexed [dy, dx], normalised as the published
    program does: positive weights over their sum, negative ones over the magnitude of theirs."""
    sigma, rf = feature_sigma(ppd), feature_radius(ppd)
    k = np.arange(-rf, rf + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    out = {}
    for name, f1 in (("edge", -k * g), ("point", (k * k / (sigma * sigma) - 1.0) * g)):
        f = g[:, None] * f1[None, :]
        out[name] = np.where(f > 0, f / f[f > 0].sum(), f / -f[f < 0].sum())
    return out


def counts(a, b):
    return np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)


def to_linear(frame, cnt, transfer):
    """Steps 1-2: black at a non-counting pixel, clamped, decoded."""
    c = np.where(cnt[..., None], frame, 0.0)
    c = np.minimum(np.maximum(c, 0.0), 1.0)
    if transfer == "srgb":
        c = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return c


def _xyz_over_white(rgb):
    return [((M_ROWS[i][0] * rgb[..., 0] + M_ROWS[i][1] * rgb[..., 1]) + M_ROWS[i][2] * rgb[..., 2]) / WHITE[i] for i in range(3)]


def to_ycxcz(rgb):
    x, y, z = _xyz_over_white(rgb)
    return 116.0 * y - 16.0, 500.0 * (x - y), 200.0 * (y - z)


def _lab_f(t):
    return np.where(t > (6.0 / 29.0) ** 3, np.cbrt(t), t / (3.0 * (6.0 / 29.0) ** 2) + 4.0 / 29.0)


def hunt_lab(rgb):
    x, y, z = (_lab_f(v) for v in _xyz_over_white(rgb))
    L = 116.0 * y - 16.0
    return L, 0.01 * L * (500.0 * (x - y)), 0.01 * L * (200.0 * (y - z))


def ycxcz_to_rgb(Y, Cx, Cz):
    y = (Y + 16.0) / 116.0
    xyz = [(Cx / 500.0 + y) * WHITE[0], y * WHITE[1], (y - Cz / 200.0) * WHITE[2]]
    rgb = np.stack([(M_INV[i, 0] * xyz[0] + M_INV[i, 1] * xyz[1]) + M_INV[i, 2] * xyz[2] for i in range(3)], axis=-1)
    return np.minimum(np.maximum(rgb, 0.0), 1.0)


def hyab(la, lb):
    return np.abs(la[0] - lb[0]) + np.sqrt((la[1] - lb[1]) ** 2 + (la[2] - lb[2]) ** 2)


def cmax():
    g = hunt_lab(np.array([0.0, 1.0, 0.0]))
    b = hunt_lab(np.array([0.0, 0.0, 1.0]))
    return float(hyab(g, b) ** 0.7)


def _filter_sep(plane, tx, ty):
    """sum_dy ty[dy] sum_dx tx[dx] plane[clamped], the horizontal pass first, taps in ascending offset."""
    H, W = plane.shape
    r = (len(tx) - 1) // 2
    pad = np.pad(plane, ((0, 0), (r, r)), mode="edge")
    hor = np.zeros((H, W))
    for d in range(2 * r + 1):
        hor += tx[d] * pad[:, d:d + W]
    pad = np.pad(hor, ((r, r), (0, 0)), mode="edge")
    out = np.zeros((H, W))
    for d in range(2 * r + 1):
        out += ty[d] * pad[d:d + H, :]
    return out


def _filter_2d(plane, f):
    H, W = plane.shape
    r = (f.shape[0] - 1) // 2
    pad = np.pad(plane, r, mode="edge")
    out = np.zeros((H, W))
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += f[dy, dx] * pad[dy:dy + H, dx:dx + W]
    return out


def _filtered(ycc, ppd, order):
    """The CSF-filtered (Y, Cx, Cz) and the four feature responses (ex, ey, px, py) of one frame."""
    Y, Cx, Cz = ycc
    y = (Y + 16.0) / 116.0
    if order == "separable":
        t, f = csf_tables(ppd), feature_tables(ppd)
        csf = (_filter_sep(Y, t["y"], t["y"]), _filter_sep(Cx, t["cx"], t["cx"]),
               _filter_sep(Cz, t["cz1"], t["cz1"]) + _filter_sep(Cz, t["cz2"], t["cz2"]))
        feat = (_filter_sep(y, f["d"], f["g"]), _filter_sep(y, f["g"], f["d"]),
                _filter_sep(y, f["p"], f["g"]), _filter_sep(y, f["g"], f["p"]))
    else:
        t, f = csf_filters_2d(ppd), feature_filters_2d(ppd)
        csf = (_filter_2d(Y, t["y"]), _filter_2d(Cx, t["cx"]), _filter_2d(Cz, t["cz"]))
        feat = (_filter_2d(y, f["edge"]), _filter_2d(y, f["edge"].T), _filter_2d(y, f["point"]), _filter_2d(y, f["point"].T))
    return csf, feat


def flip_map(a, b, transfer="srgb", ppd=DEFAULT_PPD, order="separable"):
    """Steps 1-7: the (H, W) float64 map, NaN at the non-counting pixels."""
    assert a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3
    assert transfer in ("srgb", "linear") and order in ("separable", "direct") and PPD_MIN <= ppd <= PPD_MAX
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    cnt = counts(a64, b64)
    res = []
    for frame in (a64, b64):
        csf, feat = _filtered(to_ycxcz(to_linear(frame, cnt, transfer)), float(ppd), order)
        res.append((hunt_lab(ycxcz_to_rgb(*csf)), np.sqrt(feat[0] ** 2 + feat[1] ** 2), np.sqrt(feat[2] ** 2 + feat[3] ** 2)))
    (lab_a, edge_a, point_a), (lab_b, edge_b, point_b) = res
    cm = cmax()
    c = hyab(lab_a, lab_b) ** 0.7
    lim = 0.4 * cm
    dec = np.where(c < lim, (0.95 / lim) * c, 0.95 + (c - lim) / (cm - lim) * 0.05)
    dEf = (np.maximum(np.abs(edge_b - edge_a), np.abs(point_b - point_a)) / np.sqrt(2.0)) ** 0.5
    with np.errstate(invalid="ignore"):
        dE = np.where(dec == 0.0, 0.0, dec ** (1.0 - dEf))
    return np.where(cnt, dE, np.nan)


def histogram(map32):
    """hist of step 8 from a FLOAT map: bin = min(255, (int)(m * 256.0f)) over the non-NaN pixels."""
    m = np.asarray(map32, np.float32)
    m = m[~np.isnan(m)]
    bins = np.minimum(255, (m * np.float32(256.0)).astype(np.int64))
    return np.bincount(bins, minlength=256).astype(np.uint32)


def pooled(dE):
    """Step 8 from a float64 map."""
    H, W = dE.shape
    cnt = ~np.isnan(dE)
    n = int(cnt.sum())
    res = {"pixels": n, "nonfinite": W * H - n, "hist": histogram(dE.astype(np.float32))}
    if n:
        v = np.where(cnt, dE, -1.0)
        idx = int(np.argmax(v.ravel()))  # the first occurrence: the lowest row-major index
        res.update(mean=float(dE[cnt].sum() / n), max=float(v.max()), min=float(dE[cnt].min()), argmax_x=idx % W, argmax_y=idx // W)
    else:
        res.update(mean=0.0, max=0.0, min=0.0, argmax_x=-1, argmax_y=-1)
    return res


def flip_ref(a, b, transfer="srgb", ppd=DEFAULT_PPD, order="separable"):
    dE = flip_map(a, b, transfer, ppd, order)
    return pooled(dE), dE


def weighted_quantile(hist, q):
    """The published tool's pooling: each bin weighted by count times its centre value (i + 0.5) / 256; the quantile is the
    centre of the first bin at which the running weight reaches q of the total.  0 for an empty histogram."""
    hist = np.asarray(hist, np.float64)
    centres = (np.arange(256) + 0.5) / 256.0
    run = np.cumsum(hist * centres)  # bin by bin, in ascending order
    if run[-1] <= 0:
        return 0.0
    return float(centres[int(np.searchsorted(run, q * run[-1], side="left"))])


# ---- the frames and cases the tests share -----------------------------------------------------------------------------
# (w, h): smaller than either radius in both axes, a strip, ragged in one tile, exactly one CSF window at the default ppd,
# ragged single and multiple tiles
FRAMES = [(1, 1), (1, 23), (7, 5), (21, 21), (37, 23), (64, 64), (131, 63)]
PPDS = [67.02, 8.0, 128.0]  # r = 10, rf = 9; r = 2, rf = 1 (the smallest tables); r = 18, rf = 16 (the largest)
LARGEST_ON = [(37, 23), (131, 63)]
CASES = [(w, h, ppd) for ppd in PPDS for (w, h) in FRAMES if ppd != 128.0 or (w, h) in LARGEST_ON]


def pair(w, h):
    """A synthetic display-referred pair, seeded by the size: a uniform in [0, 1] per component, 10 % of the pixels exactly
    black, a few components below 0 and above 1 (the clamp); b = a plus noise on 70 % of the pixels."""
    rng = np.random.default_rng(w * 1000 + h)
    a = rng.random((h, w, 3)).astype(np.float32)
    a[rng.random((h, w)) < 0.1] = 0.0
    flat = a.reshape(-1, 3)
    flat[0] = [0.75, -0.25, 1.5]
    if len(flat) > 4:
        flat[len(flat) // 2] = [1.25, 0.5, -0.125]
    rng = np.random.default_rng(w * 7 + h)
    b = (a + 0.05 * rng.standard_normal((h, w, 3)) * (rng.random((h, w, 1)) < 0.7)).astype(np.float32)
    return a, b
