"""NumPy restatement of rtm_bloom (include/rtm.h): the count rule, the bright pass, the down pyramid, the up pass and the
combine, in float64 (or in the `dtype` asked for), written from the header text.  The 2-D filters are products of the
renormalised 1-D ones.  The ground truth of test_bloom_host.py / test_bloom_gpu.py."""
import numpy as np

from _denoise_ref import tolerance_excess  # noqa: F401  (max |got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)
from _tonemap_ref import counts, quantise_u8  # noqa: F401  (the same count rule; rtm_quantise of (double)out_f32)

LUM = (0.2126, 0.7152, 0.0722)
K4 = (0.125, 0.375, 0.375, 0.125)  # step 3's k over dx = -1, 0, 1, 2
DEFAULTS = {"threshold": 1.0, "knee": 0.5, "intensity": 0.2, "scatter": 0.7, "levels": 6}  # rtm.h's RTM_BLOOM_DEFAULTS
SIZE_MAX = 2 ** 64 - 1


def level_sizes(w, h, levels):
    """[(W_0, H_0), .., (W_L, H_L)]: each side halves rounding up; a side that has reached 1 stays 1."""
    sizes = [(w, h)]
    for _ in range(levels):
        w, h = -(-w // 2), -(-h // 2)
        sizes.append((w, h))
    return sizes


def work_bytes(w, h, levels):
    """rtm_bloom_work_bytes: one plane of 16-byte records per level 1..L, each rounded up to 256 bytes."""
    if w <= 0 or h <= 0 or not 1 <= levels <= 8:
        return 0
    if 12 * w * h > SIZE_MAX:
        return SIZE_MAX
    total = sum(-(-(16 * wl * hl) // 256) * 256 for wl, hl in level_sizes(w, h, levels)[1:])
    return SIZE_MAX if total > SIZE_MAX else total


def bright_pass(color, threshold, knee, dtype=np.float64):
    """Steps 1-2: b0, zero where the pixel does not count."""
    f = dtype
    c = np.asarray(color, f)
    ok = counts(color)
    x = np.maximum(np.where(ok[..., None], c, f(0)), f(0))
    y = (f(LUM[0]) * x[..., 0] + f(LUM[1]) * x[..., 1]) + f(LUM[2]) * x[..., 2]
    t = f(threshold)
    k = f(knee) * t
    soft = np.minimum(np.maximum(y - t + k, f(0)), f(2) * k)
    soft = soft * soft / (f(4) * k + f(1e-5))
    g = np.maximum(soft, y - t) / np.maximum(y, f(1e-5))
    return (x * g[..., None]).astype(f)


def down_matrix(n, dtype=np.float64):
    """The (ceil(n / 2), n) matrix of step 3 along one axis: row X holds k[dx] / K_x at column 2X + dx for the taps in the frame."""
    m = np.zeros((-(-n // 2), n), np.float64)
    for X in range(m.shape[0]):
        taps = [(2 * X + dx, K4[dx + 1]) for dx in (-1, 0, 1, 2) if 0 <= 2 * X + dx < n]
        norm = sum(k for _, k in taps)
        for x, k in taps:
            m[X, x] = k / norm
    return m.astype(dtype)


def up_matrix(n_fine, n_coarse, dtype=np.float64):
    """The (n_fine, n_coarse) matrix of step 4 along one axis: taps X0 = floor((x - 1) / 2) and X0 + 1, weights (1/4, 3/4) for
    even x and (3/4, 1/4) for odd x, the ones outside skipped and the rest renormalised."""
    m = np.zeros((n_fine, n_coarse), np.float64)
    for x in range(n_fine):
        x0 = (x - 1) // 2
        weights = (0.75, 0.25) if x & 1 else (0.25, 0.75)
        taps = [(X, wgt) for X, wgt in zip((x0, x0 + 1), weights) if 0 <= X < n_coarse]
        norm = sum(wgt for _, wgt in taps)
        for X, wgt in taps:
            m[x, X] = wgt / norm
    return m.astype(dtype)


def _apply(my, mx, plane):
    """Horizontal pass first: (my . (plane . mx^T)) per channel; plane is (H, W, 3)."""
    hor = np.einsum("hwc,xw->hxc", plane, mx)
    return np.einsum("yh,hxc->yxc", my, hor)


def pyramid(b0, scatter, levels, dtype=np.float64):
    """Steps 3-5 up to B = up_0(u_1), from b0."""
    f = dtype
    h, w = b0.shape[:2]
    sizes = level_sizes(w, h, levels)
    d = [np.asarray(b0, f)]
    for l in range(1, levels + 1):
        (wf, hf) = sizes[l - 1]
        d.append(_apply(down_matrix(hf, f), down_matrix(wf, f), d[l - 1]).astype(f))
    u = d[levels]
    for l in range(levels - 1, 0, -1):
        (wf, hf), (wc, hc) = sizes[l], sizes[l + 1]
        up = _apply(up_matrix(hf, hc, f), up_matrix(wf, wc, f), u)
        u = ((f(1) - f(scatter)) * d[l] + f(scatter) * up).astype(f)
    (wc, hc) = sizes[1]
    return _apply(up_matrix(h, hc, f), up_matrix(w, wc, f), u).astype(f)


def bloom_ref(color, threshold=DEFAULTS["threshold"], knee=DEFAULTS["knee"], intensity=DEFAULTS["intensity"],
              scatter=DEFAULTS["scatter"], levels=DEFAULTS["levels"], dtype=np.float64):
    """(out, B): out = c + intensity B where the pixel counts and the input where it does not; B at every pixel."""
    f = dtype
    c = np.asarray(color, f)
    ok = counts(color)
    B = pyramid(bright_pass(color, threshold, knee, f), scatter, levels, f)
    with np.errstate(invalid="ignore"):
        out = np.where(ok[..., None], c + f(intensity) * B, c)
    return out, B


def bloom_direct(color, threshold, knee, scatter, levels):
    """B again in float64, every coarse pixel from its 16 taps and every fine one from its 4, divided by K_x K_y: the same
    steps without the separable shortcut.  For small frames."""
    h, w = np.asarray(color).shape[:2]
    sizes = level_sizes(w, h, levels)
    d = [bright_pass(color, threshold, knee)]
    for l in range(1, levels + 1):
        (wf, hf), (wc, hc) = sizes[l - 1], sizes[l]
        out = np.zeros((hc, wc, 3))
        for Y in range(hc):
            for X in range(wc):
                acc, kx, ky = np.zeros(3), 0.0, 0.0
                for dy in (-1, 0, 1, 2):
                    if 0 <= 2 * Y + dy < hf:
                        ky += K4[dy + 1]
                for dx in (-1, 0, 1, 2):
                    if 0 <= 2 * X + dx < wf:
                        kx += K4[dx + 1]
                for dy in (-1, 0, 1, 2):
                    for dx in (-1, 0, 1, 2):
                        if 0 <= 2 * Y + dy < hf and 0 <= 2 * X + dx < wf:
                            acc += K4[dx + 1] * K4[dy + 1] * d[l - 1][2 * Y + dy, 2 * X + dx]
                out[Y, X] = acc / (kx * ky)
        d.append(out)

    def up(coarse, wf, hf):
        hc, wc = coarse.shape[:2]
        out = np.zeros((hf, wf, 3))
        for y in range(hf):
            for x in range(wf):
                acc, norm = np.zeros(3), 0.0
                for Y, wy in zip(((y - 1) // 2, (y - 1) // 2 + 1), (0.75, 0.25) if y & 1 else (0.25, 0.75)):
                    for X, wx in zip(((x - 1) // 2, (x - 1) // 2 + 1), (0.75, 0.25) if x & 1 else (0.25, 0.75)):
                        if 0 <= Y < hc and 0 <= X < wc:
                            acc += wx * wy * coarse[Y, X]
                            norm += wx * wy
                out[y, x] = acc / norm
        return out

    u = d[levels]
    for l in range(levels - 1, 0, -1):
        u = (1 - scatter) * d[l] + scatter * up(u, *sizes[l])
    return up(u, w, h)
