"""NumPy restatement of the frame scopes (include/rtm.h: rtm_scopes, rtm_scope_draw, rtm_scope_bin_range,
rtm_scope_percentile, rtm_scope_exposure).  Bins come from the float's 32-bit word (LOG2) or from one double product (CODE),
the luminance is float32 in the stated order, everything on the host side is float64.  Every count is an integer: the tests
compare word for word."""
from fractions import Fraction

import numpy as np

LOG2, CODE = 0, 1
MODES = {"log2": LOG2, "code": CODE}
LUMA, OVERLAY, PARADE = 0, 1, 2
LAYOUTS = {"luma": LUMA, "overlay": OVERLAY, "parade": PARADE}
DEFAULTS = {"mode": "log2", "columns": 256}
HIST_BYTES = 4144
HIST_OFFSETS = {"bins": 0, "below": 4096, "above": 4112, "pixels": 4128, "not_counting": 4132, "reserved": 4136}
BELOW, ABOVE = -1, 256  # what bin_of() gives outside the bins


def bin_of(v, mode):
    """The bin of each float32 in `v` (finite or +inf): 0..255, BELOW or ABOVE."""
    v = np.array(v, dtype=np.float32)  # (a copy: contiguous, and a scalar stays one)
    if mode == LOG2:
        u = v.view(np.uint32)
        top = (u >> np.uint32(20)).astype(np.int64)
        b = top - 888
        out = np.where(b > 255, ABOVE, b)
        return np.where((u >> np.uint32(31) != 0) | (top < 888), BELOW, out)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = np.where((v >= 0) & (v <= 1), v, np.float32(0)).astype(np.float64)
        b = (255.0 * inside).astype(np.int64)
    return np.where(v < 0, BELOW, np.where(v > 1, ABOVE, b))


def channels(frame):
    """(counts, values): the (H, W) mask of the pixels that count and the (4, H, W) float32 channel values Y, R, G, B."""
    f = np.ascontiguousarray(frame, dtype=np.float32)
    counts = np.isfinite(f).all(axis=2)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        l = (np.float32(0.2126) * r + np.float32(0.7152) * g) + np.float32(0.0722) * b
        y = np.where(l > 0, l, np.float32(0.0)).astype(np.float32)
    return counts, np.stack([y, r, g, b])


def histogram(frame, mode):
    """rtm_scope_histogram of an (H, W, 3) float32 frame as a dict of uint32 arrays and ints."""
    counts, vals = channels(frame)
    bins = np.zeros((4, 256), np.uint32)
    below, above = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    for c in range(4):
        b = bin_of(vals[c][counts], mode)
        below[c], above[c] = (b == BELOW).sum(), (b == ABOVE).sum()
        bins[c] = np.bincount(b[(b >= 0) & (b < 256)], minlength=256)
    return {"bins": bins, "below": below, "above": above, "pixels": int(counts.sum()), "not_counting": int((~counts).sum()),
            "reserved": np.zeros(2, np.uint32)}


def words(hist):
    """The 1036 words of the record."""
    return np.concatenate([hist["bins"].reshape(-1), hist["below"], hist["above"],
                           np.array([hist["pixels"], hist["not_counting"]], np.uint32), hist["reserved"]]).astype(np.uint32)


def from_words(w):
    w = np.asarray(w).reshape(-1).view(np.uint32)
    assert w.size == HIST_BYTES // 4
    return {"bins": w[:1024].reshape(4, 256).copy(), "below": w[1024:1028].copy(), "above": w[1028:1032].copy(),
            "pixels": int(w[1032]), "not_counting": int(w[1033]), "reserved": w[1034:1036].copy()}


def waveform(frame, mode, columns):
    """The (4, 256, columns) uint32 waveform: BELOW in row 0, ABOVE in row 255."""
    counts, vals = channels(frame)
    H, W = counts.shape
    oc = (np.arange(W, dtype=np.int64) * columns) // W
    oc = np.broadcast_to(oc, (H, W))[counts]
    out = np.zeros((4, 256, columns), np.uint32)
    for c in range(4):
        b = np.clip(bin_of(vals[c][counts], mode), 0, 255)
        np.add.at(out[c], (b, oc), 1)
    return out


def draw(wave, layout, gain):
    """rtm_scope_draw's bytes: (256, columns or 3 columns, 3) uint8, bin 255 on top."""
    wave = np.asarray(wave, dtype=np.uint64)
    v = np.minimum(wave * np.uint64(gain), 255).astype(np.uint8)[:, ::-1, :]  # (4, 256 rows from the top, columns)
    columns = wave.shape[2]
    if layout == LUMA:
        return np.stack([v[0], v[0], v[0]], axis=2)
    if layout == OVERLAY:
        return np.stack([v[1], v[2], v[3]], axis=2)
    out = np.zeros((256, 3 * columns, 3), np.uint8)
    for k in range(3):
        out[:, k * columns:(k + 1) * columns, k] = v[1 + k]
    return out


def _code_lower_edge(b):
    """The smallest float32 v with 255 v >= b: 255.0 * (double)v is exact (32 significant bits), so the bin is floor(255 v)."""
    v = np.float32(b / 255.0)
    if Fraction(float(v)) < Fraction(b, 255):
        v = np.nextafter(v, np.float32(2))
    assert Fraction(float(v)) >= Fraction(b, 255) > Fraction(float(np.nextafter(v, np.float32(0))))
    return v


def bin_range(mode, b):
    """(lo, hi) of bin b as float32."""
    if mode == LOG2:
        edge = lambda k: np.float32(np.ldexp(1.0 + (k & 7) / 8.0, (k >> 3) - 16))
        return edge(b), edge(b + 1)
    lo = np.float32(0) if b == 0 else _code_lower_edge(b)
    hi = np.float32(1) if b == 255 else _code_lower_edge(b + 1)
    return lo, hi


def percentile(hist, mode, channel, percent):
    """(value as float32, bin) by include/rtm.h's rule, in float64."""
    n_all = hist["pixels"]
    if n_all == 0:
        return np.float32(1), -2
    t = percent / 100.0 * float(n_all)
    cum = float(hist["below"][channel])
    if t <= cum:
        return np.float32(0), -1
    for b in range(256):
        n = float(hist["bins"][channel][b])
        if n > 0 and cum + n >= t:
            lo, hi = bin_range(mode, b)
            return np.float32(float(lo) + (t - cum) / n * (float(hi) - float(lo))), b
        cum += n
    return np.float32(65536 if mode == LOG2 else 1), 256


def exposure(hist, percent, target):
    value, _ = percentile(hist, LOG2, 0, percent)
    if not value > 0:
        return np.float32(0)
    return np.float32(min(32.0, max(-32.0, float(np.log2(target / float(value))))))


def invariants(hist, wave=None, size=None):
    """The three count rules of include/rtm.h; raises AssertionError."""
    bins = hist["bins"].astype(np.int64)
    below, above = hist["below"].astype(np.int64), hist["above"].astype(np.int64)
    assert np.array_equal(below + bins.sum(axis=1) + above, np.full(4, hist["pixels"]))
    assert not np.any(hist["reserved"])
    if size is not None:
        assert hist["pixels"] + hist["not_counting"] == size
    if wave is not None:
        rows = np.asarray(wave).astype(np.int64).sum(axis=2)
        expect = bins.copy()
        expect[:, 0] += below
        expect[:, 255] += above
        assert np.array_equal(rows, expect)


def specials():
    """Component values that sit on what the binning rules decide."""
    f32 = np.float32
    out = []
    for b in range(257):  # every LOG2 lower edge (and 2^16) with its neighbour towards 0
        lo = f32(np.ldexp(1.0 + (b & 7) / 8.0, (b >> 3) - 16))
        out += [lo, np.nextafter(lo, f32(0))]
    for k in range(256):  # k / 255 and its two neighbours
        v = f32(k / 255.0)
        out += [np.nextafter(v, f32(-1)), v, np.nextafter(v, f32(2))]
    out += [f32(0.0), f32(-0.0), f32(1e-40), f32(-1e-40), f32(1.4e-45), f32(-1.0), f32(-1e-3), f32(-3e38), f32(3e38), f32(0.18),
            f32(1.0), f32(65536.0), f32(np.inf), f32(-np.inf), f32(np.nan)]
    return np.array(out, dtype=np.float32)


def frame(w, h, seed, display=False):
    """A seeded (h, w, 3) float32 frame: values spread from 2^-20 to 2^18 (display=True: from -0.1 to 1.1), with specials()
    planted in components and grey pixels on bin edges planted whole (their luminance sums round across the edge)."""
    rng = np.random.default_rng(seed)
    if display:
        f = rng.uniform(-0.1, 1.1, (h, w, 3)).astype(np.float32)
    else:
        f = np.exp2(rng.uniform(-20.0, 18.0, (h, w, 3))).astype(np.float32)
    flat = f.reshape(-1)
    sp = specials()
    k = min(sp.size, flat.size // 2)
    flat[rng.choice(flat.size, k, replace=False)] = sp[rng.permutation(sp.size)[:k]]
    grey = sp[np.isfinite(sp) & (sp > 0)]
    pix = f.reshape(-1, 3)
    k = min(grey.size, pix.shape[0] // 4)
    pix[rng.choice(pix.shape[0], k, replace=False)] = grey[rng.permutation(grey.size)[:k], None]
    return f
