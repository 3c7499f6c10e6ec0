"""The colour grade restated in NumPy (include/rtm.h: rtm_grade, rtm_grade_white_balance), for the tests.

grade_ref evaluates steps 1-7 in float64 (the reference) or in float32 (the CPU-side margin check of test_grade_host: how
far plain float arithmetic lies from the float64 evaluation on the tests' own inputs), with what the library rounds to float
rounded to float first: the parameters, the exposure gain G and the LUT's scale inv_c.  white_balance_ref is the matrix in
float64.  write_cube writes a .cube file for a temporary directory; the tests commit no fixture."""
import numpy as np

INTERPS = ("trilinear", "tetrahedral")
IDENTITY = np.eye(3, dtype=np.float32)
EVERYTHING = dict(matrix=[[1.2, -0.1, -0.1], [-0.05, 1.0, 0.05], [0.02, -0.2, 1.18]], exposure=0.5, contrast=1.3, pivot=0.18,
                  slope=(1.1, 0.9, 1.05), offset=(0.01, -0.02, 0.0), power=(0.8, 1.2, 2.2), saturation=1.3)


def counts(frame):
    """(H, W): the pixels whose three components are finite."""
    return np.all(np.isfinite(frame), axis=-1)


def _three(v):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (3,)))


def lut_index(s, n):
    """Step 6's index arithmetic on an array of lattice coordinates (any float dtype): the cell i and the fraction f."""
    with np.errstate(invalid="ignore"):
        s = np.where(s > 0, np.minimum(s, s.dtype.type(n - 1)), s.dtype.type(0))
    i = np.minimum(s.astype(np.int64), n - 2)
    return i, s - i.astype(s.dtype)


def lut_apply(y, table, lut_domain=((0, 0, 0), (1, 1, 1)), interp="tetrahedral"):
    """Step 6 on y (..., 3) in y's dtype; table (N, N, N, 3) float32 indexed [b][g][r]."""
    dt = y.dtype.type
    n = table.shape[0]
    lo, hi = _three(lut_domain[0]), _three(lut_domain[1])
    inv = np.float32((n - 1) / (hi.astype(np.float64) - lo.astype(np.float64)))  # rounded to float, as on the host
    with np.errstate(invalid="ignore", over="ignore"):
        s = (y - lo.astype(dt)) * inv.astype(dt)
    i, f = lut_index(s, n)
    t = table.astype(dt)
    ir, ig, ib = i[..., 0], i[..., 1], i[..., 2]

    def at(dr, dg, db):
        return t[ib + db, ig + dg, ir + dr]

    if interp == "trilinear":
        fr, fg, fb = f[..., 0:1], f[..., 1:2], f[..., 2:3]
        c00 = at(0, 0, 0) + fr * (at(1, 0, 0) - at(0, 0, 0))
        c10 = at(0, 1, 0) + fr * (at(1, 1, 0) - at(0, 1, 0))
        c01 = at(0, 0, 1) + fr * (at(1, 0, 1) - at(0, 0, 1))
        c11 = at(0, 1, 1) + fr * (at(1, 1, 1) - at(0, 1, 1))
        c0 = c00 + fg * (c10 - c00)
        c1 = c01 + fg * (c11 - c01)
        return c0 + fb * (c1 - c0)
    assert interp == "tetrahedral"
    order = np.argsort(-f, axis=-1, kind="stable")  # descending, a tie taking the earlier channel first
    fs = np.take_along_axis(f, order, axis=-1)
    f1, f2, f3 = fs[..., 0:1], fs[..., 1:2], fs[..., 2:3]
    step1 = np.eye(3, dtype=np.int64)[order[..., 0]]  # (..., 3): one step along the first channel
    step2 = step1 + np.eye(3, dtype=np.int64)[order[..., 1]]
    c000 = at(0, 0, 0)
    c1 = t[ib + step1[..., 2], ig + step1[..., 1], ir + step1[..., 0]]
    c2 = t[ib + step2[..., 2], ig + step2[..., 1], ir + step2[..., 0]]
    c111 = at(1, 1, 1)
    one = dt(1)
    return (((one - f1) * c000 + (f1 - f2) * c1) + (f2 - f3) * c2) + f3 * c111


def grade_ref(frame, matrix=None, exposure=0.0, contrast=1.0, pivot=0.18, slope=1, offset=0, power=1, saturation=1.0, lut=None,
              lut_domain=((0, 0, 0), (1, 1, 1)), interp="tetrahedral", dtype=np.float64):
    """rtm_grade's out_f32 for `frame` (H, W, 3) float32, evaluated in `dtype` and returned in it; pixels that do not count
    carry the input's values (compare their words with the input's)."""
    dt = np.dtype(dtype).type
    m = IDENTITY if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(3, 3)
    ev, con, piv, sat = np.float32(exposure), np.float32(contrast), np.float32(pivot), np.float32(saturation)
    sl, of, pw = _three(slope), _three(offset), _three(power)
    frame = np.asarray(frame, dtype=np.float32)
    ok = counts(frame)
    y = frame[ok].astype(dt)  # (K, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if not np.array_equal(m, IDENTITY):
            r, g, b = y[:, 0].copy(), y[:, 1].copy(), y[:, 2].copy()
            y = np.stack([(dt(m[i, 0]) * r + dt(m[i, 1]) * g) + dt(m[i, 2]) * b for i in range(3)], axis=-1)
        if ev != 0:
            y = y * dt(np.float32(np.exp2(np.float64(ev))))
        if con != 1 or piv != np.float32(0.18):
            y = dt(piv) * np.power(np.maximum(y, dt(0)) / dt(piv), dt(con))
        if np.any(sl != 1) or np.any(of != 0) or np.any(pw != 1):
            v = np.maximum(y * sl.astype(dt) + of.astype(dt), dt(0))
            y = np.stack([v[:, c] if pw[c] == 1 else np.power(v[:, c], dt(pw[c])) for c in range(3)], axis=-1)
        if sat != 1:
            L = ((dt(np.float32(0.2126)) * y[:, 0] + dt(np.float32(0.7152)) * y[:, 1]) + dt(np.float32(0.0722)) * y[:, 2])[:, None]
            y = L + dt(sat) * (y - L)
        if lut is not None:
            y = lut_apply(y, np.asarray(lut, dtype=np.float32), lut_domain, interp)
    with np.errstate(invalid="ignore"):  # (widening a signalling NaN raises the flag)
        out = frame.astype(dt)
    out[ok] = y
    return out


def tolerance_excess(got, ref):
    """max |got - ref| / max(1, |ref|): the library's tolerance says it is 1e-4 or less."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if got.size else 0.0


def quantise_u8(f32):
    """rtm_quantise of (double)f32: (unsigned char)(255 * min(v, 1.0)), out of range (NaN included) -> 0."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(f32, dtype=np.float32).astype(np.float64)
        q = 255 * np.where(1.0 < v, 1.0, v)
        ok = (q >= 0.0) & (q < 256.0)
        return np.where(ok, np.where(ok, q, 0.0).astype(np.int64), 0).astype(np.uint8)


# ---- the white balance matrix, in float64 ----------------------------------------------------------
D65 = (0.3127, 0.3290)
BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])


def planckian_xy(kelvin):
    """Kang et al. (2002): the chromaticity of a black body at `kelvin`, 1667..25000."""
    T = float(kelvin)
    if T <= 4000.0:
        x = -0.2661239e9 / T ** 3 - 0.2343589e6 / T ** 2 + 0.8776956e3 / T + 0.179910
    else:
        x = -3.0258469e9 / T ** 3 + 2.1070379e6 / T ** 2 + 0.2226347e3 / T + 0.240390
    if T <= 2222.0:
        y = -1.1063814 * x ** 3 - 1.34811020 * x ** 2 + 2.18555832 * x - 0.20219683
    elif T <= 4000.0:
        y = -0.9549476 * x ** 3 - 1.37418593 * x ** 2 + 2.09137015 * x - 0.16748867
    else:
        y = 3.0817580 * x ** 3 - 5.87338670 * x ** 2 + 3.75112997 * x - 0.37001483
    return x, y


def source_white_xy(kelvin, tint=0.0):
    """The source white of rtm_grade_white_balance: the locus point moved by `tint` along v of CIE 1960 (u, v); kelvin and
    tint as the floats the call takes."""
    x, y = planckian_xy(np.float32(kelvin))
    d = -2.0 * x + 12.0 * y + 3.0
    u, v = 4.0 * x / d, 6.0 * y / d + float(np.float32(tint))
    e = 2.0 * u - 8.0 * v + 4.0
    return 3.0 * u / e, 2.0 * v / e


def _xyz(x, y):
    return np.array([x / y, 1.0, (1.0 - x - y) / y])


def rec709_to_xyz():
    p = np.stack([_xyz(0.64, 0.33), _xyz(0.30, 0.60), _xyz(0.15, 0.06)], axis=1)
    return p * np.linalg.solve(p, _xyz(*D65))[None, :]


def white_balance_ref(kelvin, tint=0.0):
    """(matrix, rgb): the 3 x 3 float64 matrix, and the source white's linear Rec.709 RGB, which it maps to equal components."""
    ws, wd = _xyz(*source_white_xy(kelvin, tint)), _xyz(*D65)
    adapt = np.linalg.inv(BRADFORD) @ np.diag((BRADFORD @ wd) / (BRADFORD @ ws)) @ BRADFORD
    to_xyz = rec709_to_xyz()
    return np.linalg.inv(to_xyz) @ adapt @ to_xyz, np.linalg.solve(to_xyz, ws)


# ---- .cube files and tables -----------------------------------------------------------------------
def write_cube(path, table, domain_min=None, domain_max=None, eol="\n", title=None, comments=False, input_range=None):
    """A .cube file of `table` (N, N, N, 3) float32 indexed [b][g][r], every number written so that it reads back to the
    same float.  domain_min / domain_max: DOMAIN_MIN / DOMAIN_MAX lines; input_range=(lo, hi): a LUT_3D_INPUT_RANGE line."""
    n = table.shape[0]
    lines = []
    if comments:
        lines += ["# written by the tests", ""]
    if title is not None:
        lines.append(f'TITLE "{title}"')
    lines.append(f"LUT_3D_SIZE {n}")
    if input_range is not None:
        lines.append("LUT_3D_INPUT_RANGE " + " ".join(repr(float(np.float32(v))) for v in input_range))
    if domain_min is not None:
        lines.append("DOMAIN_MIN " + " ".join(repr(float(np.float32(v))) for v in domain_min))
    if domain_max is not None:
        lines.append("DOMAIN_MAX " + " ".join(repr(float(np.float32(v))) for v in domain_max))
    if comments:
        lines += ["", "#the table", "   "]
    for row in np.asarray(table, dtype=np.float32).reshape(-1, 3):
        lines.append(" ".join("%.9g" % float(v) for v in row))
    with open(path, "wb") as f:
        f.write((eol.join(lines) + eol).encode("ascii"))


def lattice(n, lut_domain=((0, 0, 0), (1, 1, 1))):
    """(N, N, N, 3) float64: the input each lattice point stands for, indexed [b][g][r]."""
    lo, hi = _three(lut_domain[0]).astype(np.float64), _three(lut_domain[1]).astype(np.float64)
    k = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(k, k, k, indexing="ij")
    return np.stack([lo[0] + (hi[0] - lo[0]) * r, lo[1] + (hi[1] - lo[1]) * g, lo[2] + (hi[2] - lo[2]) * b], axis=-1)


def random_table(n, seed=0):
    return np.random.default_rng(7000 + 31 * n + seed).random((n, n, n, 3)).astype(np.float32)


def identity_table(n, lut_domain=((0, 0, 0), (1, 1, 1))):
    return lattice(n, lut_domain).astype(np.float32)


AFFINE_A = np.array([[0.5, 0.25, -0.125], [0.0625, 0.75, 0.125], [-0.25, 0.125, 0.5]])
AFFINE_B = np.array([0.125, 0.25, 0.375])


def affine_of(x):
    return np.asarray(x, dtype=np.float64) @ AFFINE_A.T + AFFINE_B


def affine_table(n, lut_domain=((0, 0, 0), (1, 1, 1))):
    return affine_of(lattice(n, lut_domain)).astype(np.float32)


def smooth_table(n):
    """A smooth look on [0, 1]^3: a gentle S-curve with a little cross-talk, values in [0, 1]."""
    x = lattice(n)
    s = x * x * (3.0 - 2.0 * x)
    mix = np.array([[0.9, 0.07, 0.03], [0.05, 0.9, 0.05], [0.02, 0.08, 0.9]])
    return np.clip(s @ mix.T, 0.0, 1.0).astype(np.float32)


# ---- the cases test_grade_gpu compares with grade_ref, and test_grade_host checks the float32 margin of --------------------
SIZES = [(1, 1), (7, 5), (67, 35), (130, 9), (300, 70)]  # (w, h): one pixel, under a block, odd sizes, several blocks
DOMAINS = (((0, 0, 0), (1, 1, 1)), ((-0.25, -0.25, -0.25), (4, 4, 4)))
CDL = dict(slope=EVERYTHING["slope"], offset=EVERYTHING["offset"], power=EVERYTHING["power"])


def gpu_cases():
    """[(name, grade_ref's keyword arguments)]: each parametric step alone, everything, a LUT alone (N in 2, 3, 17, 33, both
    interpolations, both domains; a random, an affine and the identity table), everything followed by a smooth 17^3 table."""
    out = [("matrix", dict(matrix=white_balance_ref(3200)[0].astype(np.float32))), ("exposure", dict(exposure=-1.5)),
           ("contrast", dict(contrast=1.3)), ("cdl", dict(CDL)), ("saturation-0", dict(saturation=0.0)),
           ("saturation-1.6", dict(saturation=1.6)), ("everything", dict(EVERYTHING))]
    for n in (2, 3, 17, 33):
        for k, dom in enumerate(DOMAINS):
            tables = (("random", random_table(n)), ("affine", affine_table(n, dom)), ("identity", identity_table(n, dom)))
            for interp in INTERPS:
                for kind, table in tables:
                    out.append((f"lut-{n}-{interp}-domain{k}-{kind}", dict(lut=table, lut_domain=dom, interp=interp)))
    for interp in INTERPS:
        out.append((f"everything-lut-17-{interp}", dict(EVERYTHING, lut=smooth_table(17), interp=interp)))
    return out
