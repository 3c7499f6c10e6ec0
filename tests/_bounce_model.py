"""The tolerance unit's bounce direction before its Normalize (csrc/rtm_path.h: bounce_nd_fused and bounce_nd_basis) restated in
numpy, with the float island behind y, and the long-double truth from the same y, sine and cosine; the input families that
tests/test_bounce_fused_host.py and tests/test_bounce_fused_gpu.py share.

What the model assumes of the hardware is what the project does (csrc/rtm_path.h, the head comment of the math policies):
v_rsq_f64 and v_rcp_f64 return the exact value times (1 + e) with |e| <= 2^-23.  `e` is an argument here: the tests run it at
both ends and at random values between.  A fused multiply-add is evaluated in long double and rounded once to double (64
mantissa bits do not always hold a 106-bit product: up to 2^-64 relative before the rounding, nothing against the 2^-45 of the
light roots)."""
import numpy as np

LD = np.longdouble
M24 = 1 << 24
TWO_PI_24 = 6.283185307179586 / M24


def fma(a, b, c):
    return (LD(a) * LD(b) + LD(c)).astype(np.float64)


def rsq(x, e):
    return ((LD(1) / np.sqrt(LD(x))) * (LD(1) + LD(e))).astype(np.float64)


def rcp(x, e):
    return ((LD(1) / LD(x)) * (LD(1) + LD(e))).astype(np.float64)


def light_root(x, e):  # MathSpecT::sqrt64_unit of the tolerance unit: seq_sqrt_batch<1, true>
    y0 = rsq(x, e)
    s0, h0 = x * y0, 0.5 * y0
    r0 = fma(-h0, s0, 0.5)
    return fma(s0, r0, s0)


def seq_rcp(y, e):  # r0 (1 + e + e^2)
    r = rcp(y, e)
    d = fma(-y, r, 1.0)
    return fma(r, fma(d, d, d), r)


def island(w):
    """L = w.z^2 + w.x^2 as the double sum and y = (double)sqrtf((float)L): src/Ray.h:67-69 on Cross((0,1,0), w)"""
    L = fma(w[:, 2], w[:, 2], w[:, 0] * w[:, 0])
    len2 = L.astype(np.float32)
    return L, np.sqrt(len2).astype(np.float64), len2


def draws(m1, m2):
    ang = TWO_PI_24 * m1.astype(np.float64)
    return np.sin(ang), np.cos(ang), m2.astype(np.float64) / M24


def nd_fused(w, m1, m2, e=0.0):
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    sn, cs, r2 = draws(m1, m2)
    L, y, _ = island(w)
    p = r2 * (y * y)
    y0 = rsq(p, e)
    s0, h0 = p * y0, 0.5 * y0
    r0 = fma(-h0, s0, 0.5)
    k0 = r2 * y0
    k = fma(k0, r0, k0)
    s1 = light_root(1.0 - r2, e)
    a, b = k * cs, k * sn
    t = fma(-b, wy, s1)
    return np.stack([fma(wz, a, wx * t), fma(b, L, wy * s1), fma(-wx, a, wz * t)], axis=1)


def nd_basis(w, m1, m2, e=0.0):
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    sn, cs, r2 = draws(m1, m2)
    _, y, _ = island(w)
    r2s = light_root(r2, e)
    r = seq_rcp(y, e)
    ux, uz = wz * r, -wx * r
    vx, vy, vz = wy * uz, fma(wz, ux, -wx * uz), -(wy * ux)
    s1 = light_root(1.0 - r2, e)
    x = fma(wx, s1, fma(ux * cs, r2s, (vx * sn) * r2s))
    yy = fma(vy * sn, r2s, wy * s1)
    z = fma(wz, s1, fma(uz * cs, r2s, (vz * sn) * r2s))
    return np.stack([x, yy, z], axis=1)


def nd_truth(w, m1, m2, trig=None):
    """long double throughout, from the SAME y, sine and cosine (doubles; `trig`: the device's own (sin, cos) where the caller
    has them, else numpy's as in the two forms above)"""
    wx, wy, wz = LD(w[:, 0]), LD(w[:, 1]), LD(w[:, 2])
    sn, cs, r2 = draws(m1, m2)
    if trig is not None:
        sn, cs = trig
    sn, cs, r2 = LD(sn), LD(cs), LD(r2)
    y = LD(island(w)[1])
    k = np.sqrt(r2) / y
    s1 = np.sqrt(LD(1) - r2)
    L = wz * wz + wx * wx
    return np.stack([k * (wz * cs - wx * wy * sn) + wx * s1, k * L * sn + wy * s1, k * (-wx * cs - wy * wz * sn) + wz * s1], axis=1)


def _odd(rng, lo, hi, n):
    return (2 * rng.integers(lo // 2, hi // 2, n) + 1).astype(np.uint32)


def families(n, seed):
    """(name, w, m1, m2) of n records each: unit normals with no zero component, odd draw integers below 2^24.  m1 runs through
    the four quadrants record by record; m2 is random, or one of 1, 3, 2^24 - 1 on every fourth record of the families' tails."""
    rng = np.random.default_rng(seed)
    q = np.arange(n) % 4
    m1 = (q * (M24 // 4) + _odd(rng, 0, M24 // 4, n)).astype(np.uint32)
    m1[:8] = [1, M24 // 4 - 1, M24 // 4 + 1, M24 // 2 - 1, M24 // 2 + 1, 3 * M24 // 4 - 1, 3 * M24 // 4 + 1, M24 - 1]  # the quadrants' edges
    m2 = _odd(rng, 0, M24, n)
    m2[np.arange(n) % 16 == 3] = 1
    m2[np.arange(n) % 16 == 7] = 3
    m2[np.arange(n) % 16 == 11] = M24 - 1
    signs = np.stack([np.where((np.arange(n) >> 2) % 2 == 0, 1.0, -1.0), np.where((np.arange(n) >> 3) % 2 == 0, 1.0, -1.0)], axis=1)
    out = []
    g = rng.normal(size=(n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    out.append(("random unit normals", g, m1, m2))
    # the box's floor and ceiling: |w.x|, |w.z| log-uniform in [1e-7, 1e-3], every sign pattern of (w.x, w.z), w.y up and down
    ex = 10.0 ** rng.uniform(-7, -3, n) * signs[:, 0]
    ez = 10.0 ** rng.uniform(-7, -3, n) * signs[:, 1]
    wy = np.sqrt(1.0 - ex * ex - ez * ez) * np.where((np.arange(n) >> 4) % 2 == 0, 1.0, -1.0)
    out.append(("floor and ceiling", np.stack([ex, wy, ez], axis=1), m1, m2))
    # side walls: w.y small, (w.x, w.z) anywhere on the circle, the four sign patterns by the angle's quadrant
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    ey = 10.0 ** rng.uniform(-7, -3, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    h = np.sqrt(1.0 - ey * ey)
    out.append(("side walls", np.stack([h * np.cos(ang), ey, h * np.sin(ang)], axis=1), m1, m2))
    # one of w.x, w.z tiny against the other
    big = rng.uniform(0.1, 0.9, n) * signs[:, 0]
    tiny = 10.0 ** rng.uniform(-7, -3, n) * signs[:, 1]
    swap = (np.arange(n) >> 5) % 2 == 0
    wx, wz = np.where(swap, big, tiny), np.where(swap, tiny, big)
    out.append(("lopsided", np.stack([wx, np.sqrt(1.0 - wx * wx - wz * wz), wz], axis=1), m1, m2))
    for _, w, _, _ in out:
        assert np.all(w != 0.0) and np.all(np.abs(w[:, 0]) > 1.2e-38)
    return out
