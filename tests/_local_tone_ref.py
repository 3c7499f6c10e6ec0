"""NumPy restatement of rtm_tonemap_local (include/rtm.h): the count rule, the exposed luminance, the three synthetic
exposures, the well-exposedness weights, the two pyramids, the blend and collapse and the apply step, in float64 (or in the
`dtype` asked for), written from the header text.  The filters are rtm_bloom's (_bloom_ref's matrices).  The ground truth of
test_local_tone_host.py / test_local_tone_gpu.py."""
import itertools

import numpy as np

from _bloom_ref import K4, down_matrix, level_sizes, up_matrix
from _denoise_ref import tolerance_excess  # noqa: F401  (max |got - ref| / max(1, |ref|): rtm.h's bar is 1e-4)
from _tonemap_ref import counts, quantise_u8  # noqa: F401  (the same count rule; rtm_quantise of (double)out_f32)

LUM = (0.2126, 0.7152, 0.0722)
DEFAULTS = {"anchor": 1.0, "shadows": 2.0, "highlights": 2.0, "sigma": 0.25, "levels": 5}  # RTM_TONEMAP_LOCAL_DEFAULTS
SIZE_MAX = 2 ** 64 - 1
# what the GPU test runs, and the host test checks the float32 evaluation on.  One pixel; single rows and columns; every
# ceil-halving case; 131 x 63 and 258 x 66: a level-1 plane of more than one 32 x 8 tile in both axes with ragged edges; at 8
# levels every frame ends in levels that have collapsed to 1 x 1
FRAMES = [(1, 1), (1, 17), (17, 1), (2, 2), (7, 5), (37, 23), (64, 64), (131, 63), (258, 66)]
# anchor, shadows, highlights, sigma, levels
CASES = list(itertools.product((0.25, 1.0, 16.0), (0.0, 2.0, 4.0), (0.0, 2.0, 4.0), (0.1, 0.25, 1.0), (0, 1, 3, 8)))
SUBSET = CASES[::13]  # 25 of the 324, fixed: every value of every parameter
SUBSET9 = CASES[::41] + CASES[-1:]  # nine, for 258 x 66: every value of every parameter as well


def work_bytes(w, h, levels):
    """rtm_tonemap_local_work_bytes: two planes of 16-byte records per level 1..L, each rounded up to 256 bytes."""
    if w <= 0 or h <= 0 or not 1 <= levels <= 8:
        return 0
    if 12 * w * h > SIZE_MAX:
        return SIZE_MAX
    total = sum(2 * (-(-(16 * wl * hl) // 256) * 256) for wl, hl in level_sizes(w, h, levels)[1:])
    return SIZE_MAX if total > SIZE_MAX else total


def exposed(color, A, dtype=np.float64):
    """Steps 1-2: (xc, x); a pixel that does not count is black."""
    f = dtype
    ok = counts(color)
    xc = np.maximum(np.where(ok[..., None], np.asarray(color, f), f(0)), f(0))
    y = (f(LUM[0]) * xc[..., 0] + f(LUM[1]) * xc[..., 1]) + f(LUM[2]) * xc[..., 2]
    with np.errstate(over="ignore"):
        x = np.minimum(f(A) * y, f(np.float32(1e6)))
    return xc, x.astype(f)


def exposures(x, shadows, highlights, dtype=np.float64):
    """Step 3: I, (H, W, 3)."""
    f = dtype
    e = (f(2.0) ** f(shadows), f(1), f(2.0) ** f(-highlights))
    return np.stack([(ek * x) / (f(1) + ek * x) for ek in e], axis=-1).astype(f)


def weights(I, sigma, dtype=np.float64):
    """Step 4: the normalised weights, (H, W, 3)."""
    f = dtype
    v = np.sqrt(I)
    w = np.exp(-(v - f(0.5)) ** 2 / (f(2) * f(sigma) * f(sigma)))
    return (w / w.sum(axis=-1, keepdims=True)).astype(f)


def _apply(my, mx, plane):
    """Horizontal pass first; plane is (H, W, C)."""
    hor = np.einsum("hwc,xw->hxc", plane, mx)
    return np.einsum("yh,hxc->yxc", my, hor)


def fuse(I, W, levels, dtype=np.float64):
    """Steps 5-6 before the clamp: R_0, (H, W)."""
    f = dtype
    h, w = I.shape[:2]
    sizes = level_sizes(w, h, levels)
    gi, gw = [np.asarray(I, f)], [np.asarray(W, f)]
    for l in range(1, levels + 1):
        wf, hf = sizes[l - 1]
        my, mx = down_matrix(hf, f), down_matrix(wf, f)
        gi.append(_apply(my, mx, gi[-1]).astype(f))
        gw.append(_apply(my, mx, gw[-1]).astype(f))
    R = (gw[levels] * gi[levels]).sum(axis=-1).astype(f)
    for l in range(levels - 1, -1, -1):
        (wf, hf), (wc, hc) = sizes[l], sizes[l + 1]
        my, mx = up_matrix(hf, hc, f), up_matrix(wf, wc, f)
        up_i = _apply(my, mx, gi[l + 1])
        up_r = _apply(my, mx, R[..., None])[..., 0]
        R = ((gw[l] * (gi[l] - up_i)).sum(axis=-1) + up_r).astype(f)
    return R


def local_ref(color, anchor=DEFAULTS["anchor"], shadows=DEFAULTS["shadows"], highlights=DEFAULTS["highlights"],
              sigma=DEFAULTS["sigma"], levels=DEFAULTS["levels"], exposure=None, dtype=np.float64, unclamped=False):
    """(out (H, W, 3), F (H, W)).  exposure: the statistics' E, None for a null stats_dev.  unclamped: F is R_0."""
    f = dtype
    A = f(anchor) * (f(1) if exposure is None else f(exposure))
    ok = counts(color)
    xc, x = exposed(color, A, f)
    I = exposures(x, shadows, highlights, f)
    R0 = fuse(I, weights(I, sigma, f), levels, f)
    F = R0 if unclamped else np.minimum(np.maximum(R0, f(0)), f(1))
    r = F / np.maximum(x, f(np.float32(1e-4)))
    with np.errstate(over="ignore"):
        out = xc * (A * r)[..., None]
    return np.where(ok[..., None], out, f(0)).astype(f), F.astype(f)


def fuse_direct(I, W, levels):
    """R_0 again in float64 without the separable shortcut: every coarse pixel from its 16 taps and every fine one from its 4,
    divided by the weight inside the frame.  For small frames."""
    h, w = I.shape[:2]
    sizes = level_sizes(w, h, levels)

    def down(fine, wc, hc):
        hf, wf = fine.shape[:2]
        out = np.zeros((hc, wc, fine.shape[2]))
        for Y in range(hc):
            for X in range(wc):
                acc, norm = np.zeros(fine.shape[2]), 0.0
                for dy in (-1, 0, 1, 2):
                    for dx in (-1, 0, 1, 2):
                        if 0 <= 2 * Y + dy < hf and 0 <= 2 * X + dx < wf:
                            acc += K4[dx + 1] * K4[dy + 1] * fine[2 * Y + dy, 2 * X + dx]
                            norm += K4[dx + 1] * K4[dy + 1]
                out[Y, X] = acc / norm
        return out

    def up(coarse, wf, hf):
        hc, wc = coarse.shape[:2]
        out = np.zeros((hf, wf, coarse.shape[2]))
        for y in range(hf):
            for x in range(wf):
                acc, norm = np.zeros(coarse.shape[2]), 0.0
                for Y, wy in zip(((y - 1) // 2, (y - 1) // 2 + 1), (0.75, 0.25) if y & 1 else (0.25, 0.75)):
                    for X, wx in zip(((x - 1) // 2, (x - 1) // 2 + 1), (0.75, 0.25) if x & 1 else (0.25, 0.75)):
                        if 0 <= Y < hc and 0 <= X < wc:
                            acc += wx * wy * coarse[Y, X]
                            norm += wx * wy
                out[y, x] = acc / norm
        return out

    gi, gw = [np.asarray(I, np.float64)], [np.asarray(W, np.float64)]
    for l in range(1, levels + 1):
        gi.append(down(gi[-1], *sizes[l]))
        gw.append(down(gw[-1], *sizes[l]))
    R = (gw[levels] * gi[levels]).sum(axis=-1)
    for l in range(levels - 1, -1, -1):
        R = (gw[l] * (gi[l] - up(gi[l + 1], *sizes[l]))).sum(axis=-1) + up(R[..., None], *sizes[l])[..., 0]
    return R
