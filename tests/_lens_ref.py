"""rtm_lens and rtm_lens_fit_zoom (include/rtm.h) restated in float64 NumPy, from the header's text: the positions in the
stated order (so every position, tap set and border decision is the device's bit for bit), the weights rounded to float32 and
widened again, the counting rule, the threshold, the border, the vignette, the fold-over check and the zoom fit.  The ground
truth of tests/test_lens_host.py and tests/test_lens_gpu.py."""
import numpy as np

from _denoise_ref import tolerance_excess  # noqa: F401  (|got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)
from _tonemap_ref import quantise_u8  # noqa: F401

FILTERS = ("nearest", "bilinear", "bicubic")  # RTM_LENS_NEAREST .. RTM_LENS_BICUBIC
MODES = ("direct", "inverse")  # RTM_LENS_DIRECT, RTM_LENS_INVERSE
DEFAULTS = {"k1": 0.0, "k2": 0.0, "zoom": 1.0, "chroma": 0.0, "vignette": 0.0, "falloff": 1.0, "border": 0.0,
            "mode": "direct", "filter": "bicubic"}
RANGES = {"k1": (-0.5, 0.5), "k2": (-0.25, 0.25), "zoom": (0.25, 4.0), "chroma": (-0.05, 0.05), "vignette": (0.0, 1.0),
          "falloff": (0.0, 4.0)}
MIN_WEIGHT = 0.0625  # D below it: the channel is NaN
NEWTON_STEPS = 12


def f32(v):
    """A parameter as the struct holds it: rounded to float32, widened to a float64."""
    return np.float64(np.float32(v))


def with_defaults(params):
    p = dict(DEFAULTS)
    p.update(params)
    return p


def folds_over(k1, k2, zoom, mode):
    """The fold-over check: True when the call refuses the radial map.  a = 3 k1, b = 5 k2, T = iz^2 (4 iz^2 for INVERSE);
    d(t) = 1 + t (a + t b) at T and at the vertex inside (0, T) must be 0.25 or more; INVERSE also needs g(T) >= 0.5."""
    k1, k2, iz = f32(k1), f32(k2), np.float64(1.0) / f32(zoom)
    a, b = 3.0 * k1, 5.0 * k2
    T = 4.0 * (iz * iz) if mode == "inverse" else iz * iz
    if not 1.0 + T * (a + T * b) >= 0.25:
        return True
    if b != 0.0:
        tv = -a / (2.0 * b)
        if 0.0 < tv < T and not 1.0 + tv * (a + tv * b) >= 0.25:
            return True
    return mode == "inverse" and not 1.0 + T * (k1 + T * k2) >= 0.5


def refused(channels=3, **params):
    """What rtm_lens refuses of the parameters (ranges, combinations, fold-over): the reason's keyword, or None."""
    p = with_defaults(params)
    for name, (lo, hi) in RANGES.items():
        if not np.float32(lo) <= np.float32(p[name]) <= np.float32(hi):
            return name
    if p["mode"] not in MODES:
        return "mode"
    if p["filter"] not in FILTERS:
        return "filter"
    if channels not in (1, 3):
        return "channels"
    if p["filter"] != "nearest" and not np.all(np.isfinite(np.broadcast_to(np.float32(p["border"]), (3,)))):
        return "border"
    if np.float32(p["chroma"]) != 0 and (channels == 1 or p["filter"] == "nearest"):
        return "chroma"
    if np.float32(p["vignette"]) != 0 and p["filter"] == "nearest":
        return "vignette"
    return "folds over" if folds_over(p["k1"], p["k2"], p["zoom"], p["mode"]) else None


def solve_inverse(r, k1, k2):
    """rho with rho g(rho^2) = r after exactly 12 Newton steps from rho = r; float64 arrays, k1 and k2 float64."""
    rho = r.copy()
    a, b = 3.0 * k1, 5.0 * k2
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_STEPS):
            t = rho * rho
            rho = rho - (rho * (1.0 + t * (k1 + t * k2)) - r) / (1.0 + t * (a + t * b))
    return rho


def factor(dx, dy, R2, k1, k2, zoom, mode):
    """Step 1's F for the offsets (dx, dy), float64 arrays, in the header's order of operations."""
    k1, k2, iz = f32(k1), f32(k2), np.float64(1.0) / f32(zoom)
    with np.errstate(all="ignore"):
        r2 = ((dx * dx + dy * dy) / R2) * (iz * iz)
        if mode == "direct":
            return (1.0 + r2 * (k1 + r2 * k2)) * iz
        r = np.sqrt(r2)
        rho = solve_inverse(r, k1, k2)
        return np.where(r > 0.0, rho / np.where(r > 0.0, r, 1.0), 1.0) * iz


def positions(w, h, channels=3, X=None, Y=None, **params):
    """(u, v, inside, rv): the source coordinates of every channel, shaped (..., C), whether each is inside the frame, and
    (dx dx + dy dy) / R2 for the vignette, for the pixels (X, Y) (default: the whole frame, shaped (h, w))."""
    p = with_defaults(params)
    if X is None:
        Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cx, cy = np.float64(w) / 2.0, np.float64(h) / 2.0
    dx, dy = (X.astype(np.float64) + 0.5) - cx, (Y.astype(np.float64) + 0.5) - cy
    R2 = cx * cx + cy * cy
    F = factor(dx, dy, R2, p["k1"], p["k2"], p["zoom"], p["mode"])
    chroma = f32(p["chroma"])
    u, v = [], []
    for c in range(channels):
        m = 1.0 + chroma * np.float64(1 - c) if channels == 3 else np.float64(1.0)
        Fc = F * m
        u.append(cx + dx * Fc - 0.5)
        v.append(cy + dy * Fc - 0.5)
    u, v = np.stack(u, axis=-1), np.stack(v, axis=-1)
    with np.errstate(invalid="ignore"):
        inside = (u >= -0.5) & (u < np.float64(w) - 0.5) & (v >= -0.5) & (v < np.float64(h) - 0.5)
    return u, v, inside, (dx * dx + dy * dy) / R2


def weights(filter, t):
    """Step 3: the axis weights at fraction t (float64 array), evaluated in double, rounded to float32 and widened: (first
    tap's offset from floor, [w_i])."""
    if filter == "bilinear":
        ws = [1.0 - t, t]
        first = 0
    else:
        ws = [(((2.0 - t) * t - 1.0) * t) / 2.0, (((3.0 * t - 5.0) * t) * t + 2.0) / 2.0,
              (((4.0 - 3.0 * t) * t + 1.0) * t) / 2.0, (((t - 1.0) * t) * t) / 2.0]
        first = -1
    return first, [w.astype(np.float32).astype(np.float64) for w in ws]


def counts(src):
    """The pixels all of whose components are finite, (h, w)."""
    s = np.asarray(src)
    return np.isfinite(s.reshape(s.shape[0], s.shape[1], -1).astype(np.float64)).all(axis=-1)


def gain(rv, vignette, falloff):
    """Step 5 in float64 from the float parameters and the float-rounded radius."""
    rvf = rv.astype(np.float32).astype(np.float64)
    q = 1.0 + (f32(falloff) * f32(falloff)) * rvf
    return 1.0 - f32(vignette) * (1.0 - 1.0 / (q * q))


def border_words(border):
    """The three float32 words of `border` (a number or three), bits kept."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(border, dtype=np.float32), (3,)))


def lens_ref(src, **params):
    """rtm_lens of `src`, (h, w, 3) or (h, w) float32: a dict of
    "out"     float64 shaped like src (float32 with NEAREST, whose words are the answer): the border's value where a channel is
              outside, NaN where D < 1/16;
    "inside"  bool, shaped (h, w, C);
    "D"       float64 (h, w, C), the normalising weight of the inside channels (NaN outside; absent with NEAREST);
    "u", "v"  the positions, (h, w, C)."""
    p = with_defaults(params)
    src = np.asarray(src, dtype=np.float32)
    plane = src.ndim == 2
    h, w = src.shape[:2]
    C = 1 if plane else 3
    assert refused(C, **params) is None, refused(C, **params)
    s3 = src.reshape(h, w, C)
    u, v, inside, rv = positions(w, h, C, **params)
    bw = border_words(p["border"])[:C]
    res = {"inside": inside, "u": u, "v": v}
    if p["filter"] == "nearest":
        out = np.empty((h, w, C), np.float32)
        out.view(np.uint32)[...] = bw.view(np.uint32)
        uu, vv = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
        xs = np.minimum(np.floor(uu + 0.5).astype(np.int64), w - 1)
        ys = np.minimum(np.floor(vv + 0.5).astype(np.int64), h - 1)
        for c in range(C):
            got = s3.view(np.uint32)[ys[..., c], xs[..., c], c]
            out.view(np.uint32)[..., c] = np.where(inside[..., c], got, out.view(np.uint32)[..., c])
        res["out"] = out[..., 0] if plane else out
        return res
    ok = counts(src)
    val = s3.astype(np.float64)
    T = 2 if p["filter"] == "bilinear" else 4
    out = np.empty((h, w, C), np.float64)
    Dall = np.full((h, w, C), np.nan)
    g = gain(rv, p["vignette"], p["falloff"])
    for c in range(C):
        uu, vv = np.where(inside[..., c], u[..., c], 0.0), np.where(inside[..., c], v[..., c], 0.0)
        fx, fy = np.floor(uu), np.floor(vv)
        x0, wx = weights(p["filter"], uu - fx)
        y0, wy = weights(p["filter"], vv - fy)
        x0, y0 = fx.astype(np.int64) + x0, fy.astype(np.int64) + y0
        N, D = np.zeros((h, w)), np.zeros((h, w))
        for j in range(T):
            y = y0 + j
            for i in range(T):
                x = x0 + i
                valid = (y >= 0) & (y < h) & (x >= 0) & (x < w)
                yc, xc = np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)
                valid &= ok[yc, xc]
                wgt = wx[i] * wy[j]
                N += np.where(valid, wgt * np.where(valid, val[yc, xc, c], 0.0), 0.0)
                D += np.where(valid, wgt, 0.0)
        hole = D < MIN_WEIGHT
        with np.errstate(all="ignore"):
            r = np.where(hole, np.nan, N / np.where(hole, 1.0, D)) * g
        out[..., c] = np.where(inside[..., c], r, np.float64(bw[c]))
        Dall[..., c] = np.where(inside[..., c], D, np.nan)
    res["out"] = out[..., 0] if plane else out
    res["D"] = Dall
    return res


def hides_border(w, h, z, channels=3, **params):
    """P(z): the parameters with zoom = z (a float32) pass the fold-over check, and every channel of every pixel of the
    frame's outermost rows and columns is inside."""
    p = with_defaults(params)
    p["zoom"] = z
    if folds_over(p["k1"], p["k2"], z, p["mode"]):
        return False
    X = np.concatenate([np.arange(w), np.arange(w), np.zeros(h, np.int64), np.full(h, w - 1)])
    Y = np.concatenate([np.zeros(w, np.int64), np.full(w, h - 1), np.arange(h), np.arange(h)])
    nc = channels if np.float32(p["chroma"]) != 0 else 1
    return bool(positions(w, h, nc if nc == 3 else 1, X=X, Y=Y, **{k: p[k] for k in ("k1", "k2", "zoom", "chroma", "mode")})[2].all())


def fit_zoom(w, h, channels=3, **params):
    """rtm_lens_fit_zoom: the float32 zoom of the 24-step bisection, or None where not even zoom 4 hides the border."""
    lo, hi = np.float32(0.25), np.float32(4.0)
    if hides_border(w, h, lo, channels, **params):
        return lo
    if not hides_border(w, h, hi, channels, **params):
        return None
    for _ in range(24):
        mid = np.float32((lo + hi) * np.float32(0.5))
        if hides_border(w, h, mid, channels, **params):
            hi = mid
        else:
            lo = mid
    return hi
