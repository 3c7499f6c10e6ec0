"""NumPy restatement of rtm_tonemap (include/rtm.h): the statistics, the map and the transfer function in float64, and the
8-bit stores in the float32 arithmetic the contract fixes.  The ground truth of test_tonemap_host.py / test_tonemap_gpu.py."""
import numpy as np

from _denoise_ref import tolerance_excess  # noqa: F401  (max |got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)

LUM = (0.2126, 0.7152, 0.0722)
OPS = ("clamp", "reinhard", "aces")
TRANSFERS = ("linear", "srgb")
DEFAULTS = {"op": "aces", "transfer": "srgb", "exposure": "auto", "key": 0.18, "white": 0.0, "dither": True}  # rtm.h's


def luminance(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def counts(color):
    """The pixels whose three components are finite."""
    return np.all(np.isfinite(np.asarray(color, np.float64)), axis=-1)


def bayer8():
    """B[y, x], the 8 x 8 Bayer index of rtm.h."""
    y, x = np.mgrid[:8, :8]
    b = np.zeros((8, 8), np.int64)
    for i in range(3):
        b |= ((((x >> i) ^ (y >> i)) & 1) << (2 * (2 - i) + 1)) | (((y >> i) & 1) << (2 * (2 - i)))
    return b


def tonemap_ref(color, op="aces", transfer="srgb", exposure="auto", key=0.18, white=0.0):
    """Steps 1-4 in float64.  Returns (out (H, W, 3) float64, {"log_average", "max_luminance", "exposure", "pixels"})."""
    c = np.asarray(color, np.float64)
    ok = counts(c)
    safe = np.where(ok[..., None], c, 0.0)
    y = np.maximum(luminance(safe), 0.0)[ok]
    n = int(ok.sum())
    if n:
        l_avg = float(np.exp(np.sum(np.log(1e-4 + y)) / n))
        l_max = float(np.max(y))
    else:
        l_avg = l_max = 1.0
    auto = isinstance(exposure, str)
    assert not auto or exposure == "auto"
    e = (key / l_avg) if auto else 2.0 ** float(exposure)
    x = np.maximum(safe * e, 0.0)
    if op == "clamp":
        t = x
    elif op == "reinhard":
        yx = luminance(x)
        w = white if white > 0 else e * l_max
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where((yx > 0) & (w > 0), (1 + yx / (w * w)) / (1 + yx), 1.0)
        t = x * s[..., None]
    elif op == "aces":
        t = x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    else:
        raise ValueError(op)
    t = np.minimum(np.maximum(t, 0.0), 1.0)
    if transfer == "srgb":
        t = np.where(t <= 0.0031308, 12.92 * t, 1.055 * t ** (1 / 2.4) - 0.055)
    elif transfer != "linear":
        raise ValueError(transfer)
    t = np.where(ok[..., None], t, 0.0)
    return t, {"log_average": l_avg, "max_luminance": l_max, "exposure": e, "pixels": n}


def quantise_u8(out_f32):
    """rtm_quantise of (double)out_f32: (unsigned char)(255 * min(v, 1.0)), out of range -> 0."""
    v = 255 * np.minimum(np.asarray(out_f32, np.float32).astype(np.float64), 1.0)
    return np.where((v >= 0) & (v < 256), np.floor(np.where(np.isfinite(v), v, 0.0)), 0).astype(np.uint8)


def dither_u8(out_f32):
    """Step 5 with dither, every operation rounded to float32: min(255, floor(255 t + (B(x & 7, y & 7) + 0.5) / 64))."""
    t = np.asarray(out_f32, np.float32)
    h, w = t.shape[:2]
    b = bayer8()[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7].astype(np.float32)
    bias = ((b + np.float32(0.5)) / np.float32(64.0)).astype(np.float32)
    v = (np.float32(255.0) * t).astype(np.float32)
    v = (v + bias[..., None]).astype(np.float32)
    return np.minimum(np.float32(255.0), np.floor(v)).astype(np.uint8)
