"""The tolerance row's opposite-wall-pair search (csrc/rtm_path.h: sphere_chunk under kAxisPairsBit, pair_disc, accept_batch_lane;
round 10) in numpy, shared by tests/test_wall_pairs_host.py and tests/test_wall_pairs_gpu.py, with the seeded ray sets both use.

Float64 with every a * b + c of the device code fused: the product and the sum are formed in long double and rounded to double
(exact but for long double's own rounding of the product, 2^-64 — the same function of the same exact product on both sides of
every comparison made here, which is what "bit for bit" needs).  Square roots are numpy's: the kernel's light roots differ from
them by 2^-45, on both of ITS sides alike (rtm_debug_math_probe ops 55 / 56 compare those)."""
import numpy as np

import _axis_disc_rays as R

LD = np.longdouble
BETA, GAMMA = 2.0 ** -5, 2.0 ** -25  # csrc/rtm_path.h: kPairBeta, kPairGamma
TAU = GAMMA / (2.0 * BETA)            # kPairTau: what a dropped wall's far root can reach
T_NEAR, T_MIN = 0.001, float(np.float32(1e-5))
DBL_MAX = np.finfo(np.float64).max
PAIRS = ((1, 2), (3, 4), (5, 6))  # the Cornell box: +x, -x, +y, -y, +z, -z behind the light


def fma(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD) + np.asarray(c, dtype=LD)).astype(np.float64)


def shared(org, dir, rows, group):
    """o.d, o.o and o.o + K of the shared-K group, as AxisShared and sphere_chunk form them"""
    with np.errstate(all="ignore"):
        od = fma(org[:, 2], dir[:, 2], fma(org[:, 1], dir[:, 1], org[:, 0] * dir[:, 0]))
        oo = fma(org[:, 2], org[:, 2], fma(org[:, 1], org[:, 1], org[:, 0] * org[:, 0]))
        ook = oo + rows[int(np.argmax(group)), 2]
    return od, oo, ook


def sphere_disc(row, axis, in_group, org, dir, od, oo, ook):
    """sphere_disc's expanded form for an axis sphere: b = c d_a - o.d, q = (-2 c) o_a + (o.o + K) (or + o.o + K), D4 = b b - q"""
    a = axis - 1
    with np.errstate(all="ignore"):
        b = fma(row[0], dir[:, a], -od)
        q = fma(row[1], org[:, a], ook) if in_group else fma(row[1], org[:, a], oo) + row[2]
        return b, fma(b, b, -q), q


def accept(b, D4, dis, hit, index):
    """sphere_update's rule: t = t1 > 0.001 ? t1 : t2; accepted iff t < dis and not t < 1e-5f.  index: a scalar or per ray"""
    with np.errstate(all="ignore"):
        sq = np.sqrt(D4)
        t1, t2 = b - sq, b + sq
        t = np.where(t1 > T_NEAR, t1, t2)
        ok = (t < dis) & ~(t < T_MIN)
    dis[ok] = t[ok]
    hit[ok] = index[ok] if isinstance(index, np.ndarray) else index
    return ok


def seven_block(rows, axis, group, org, dir):
    """The seven-sphere block: every sphere through the general rule, in index order.  Returns dis, hit, and per sphere (b, D4)."""
    m = org.shape[0]
    od, oo, ook = shared(org, dir, rows, group)
    dis, hit, discs = np.full(m, DBL_MAX), np.full(m, -1), []
    for i in range(rows.shape[0]):
        b, D4, _ = sphere_disc(rows[i], int(axis[i]), bool(group[i]), org, dir, od, oo, ook)
        discs.append((b, D4))
        accept(b, D4, dis, hit, i)
    return dis, hit, discs


def pair_path(rows, axis, group, org, dir):
    """The pair path: singles as in the block, per pair the wall the ray heads for (the lower index where d_a's sign bit is
    clear) with |c|, |d_a| and o_a sgn(d_a), and the proof for the other one: b_u <= -beta and q_u >= 2 tau b_u.  Returns dis,
    hit (meaningful where proven), proven per ray, per pair (selected index, b, D4, b_u, q_u), and what the constant bound
    q_u >= -gamma in its place would have proven (reported by the tests, used by nothing)."""
    m = org.shape[0]
    od, oo, ook = shared(org, dir, rows, group)
    dis, hit = np.full(m, DBL_MAX), np.full(m, -1)
    proven, constant, per_pair = np.ones(m, dtype=bool), np.ones(m, dtype=bool), []
    lower = {lo: hi for lo, hi in PAIRS}
    for i in range(rows.shape[0]):
        if group[i] and i not in lower:
            continue  # a pair's upper member
        if not group[i]:
            b, D4, _ = sphere_disc(rows[i], int(axis[i]), False, org, dir, od, oo, ook)
            accept(b, D4, dis, hit, i)
            continue
        a = int(axis[i]) - 1
        cabs, m2c = rows[i, 0], rows[i, 1]
        assert cabs > 0.0 and rows[lower[i], 0] == -cabs
        da, oa = dir[:, a], org[:, a]
        sgn = np.signbit(da)
        with np.errstate(all="ignore"):
            osg, ada = np.where(sgn, -oa, oa), np.abs(da)
            b = fma(cabs, ada, -od)
            D4 = fma(b, b, -fma(m2c, osg, ook))
            bu, qu = fma(-cabs, ada, -od), fma(-m2c, osg, ook)
            proven &= (bu <= -BETA) & (fma(-2.0 * TAU, bu, qu) >= 0.0)  # NaN: not proven
            constant &= (bu <= -BETA) & (qu >= -GAMMA)
        idx = i + sgn.astype(np.int64)
        accept(b, D4, dis, hit, idx)
        per_pair.append((idx, b, D4, bu, qu))
    return dis, hit, proven, per_pair, constant


# ---- ray sets ---------------------------------------------------------------------------------------------------------------

def cornell():
    c, r2, cam, target, data = R.load_spheres("cornellBoxSetting.json")
    rows, axis = R.host_rows(data), R.axis_of(c)
    return c, r2, cam, target, data, rows, axis, R.shared_k_group(rows, axis)


def _wall_points(rng, c, r2, i, m, offset=0.0):
    """points on wall i's sphere (offset > 0: that far INSIDE the sphere, behind the wall), and the normal into the room"""
    r = np.sqrt(r2[i])
    a = int(np.argmax(np.abs(c[i])))
    p = rng.uniform(-10.0, 10.0, (m, 3))
    j, k = [q for q in range(3) if q != a]
    rr = r - np.asarray(offset, dtype=np.float64) * np.ones(m)
    p[:, a] = c[i, a] - np.sign(c[i, a]) * np.sqrt(rr * rr - p[:, j] ** 2 - p[:, k] ** 2)
    return p, (p - c[i]) / rr[:, None]


def _hit_points(rng, c, r2, i, m):
    """points on wall i as the KERNEL arrives at them, and the normal into the room: a ray from a point of the room towards the
    wall, its distance t = b - sqrt(D4) with the light root's relative error of 2^-45 (csrc/rtm_path.h: seq_sqrt_batch, LIGHT), the
    hit point org + dir t rounded to double.  The direction's length comes from a float root (|d.d - 1| <= 1.8e-7) while
    Intersect's t takes it for 1, so the point is off the sphere: a bounce ray's q = |c - o|^2 - r^2 for the wall it leaves is
    t^2 (d.d - 1), up to 2e-4 of either sign — four orders above what the light root or the rounding of the point add.
    (R.bounce_rays puts its points on the sphere to 1e-13: no such term.)"""
    w, _ = _wall_points(rng, c, r2, i, m)
    s = rng.uniform(-9.9, 9.9, (m, 3))
    e = R._normalize_like_the_reference(w - s)
    p = (c[i][None, :] - s).astype(LD)
    b = (p * e).sum(axis=1)
    t = (b - np.sqrt(b * b - (p * p).sum(axis=1) + LD(r2[i]))).astype(np.float64)
    t *= 1.0 + 2.0 ** -45 * rng.uniform(-1.0, 1.0, m)
    hit = s + e * t[:, None]
    return hit, (hit - c[i]) / np.sqrt(r2[i])


def _about(rng, nrm, cos_t):
    """unit directions at cosine cos_t to the unit normals, any azimuth"""
    m = nrm.shape[0]
    phi = 2.0 * np.pi * rng.random(m)
    helper = np.where(np.abs(nrm[:, :1]) > 0.1, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    u = np.cross(helper, nrm)
    u /= np.linalg.norm(u, axis=1)[:, None]
    v = np.cross(nrm, u)
    s = np.sqrt(1.0 - cos_t * cos_t)
    return R._normalize_like_the_reference(u * (np.cos(phi) * s)[:, None] + v * (np.sin(phi) * s)[:, None] + nrm * cos_t[:, None])


def ray_sets(m, seed, c, r2, cam, target):
    """name -> (org, dir), m rays each (a multiple of 6), seeded"""
    rng = np.random.default_rng(seed)
    walls, per = [1, 2, 3, 4, 5, 6], m // 6
    sets = {}
    # bounce rays from wall points, cosine-weighted; shuffled, as a wave holds rays from every wall
    orgs, dirs = [], []
    for i in walls:
        p, nrm = _hit_points(rng, c, r2, i, per)
        orgs.append(p)
        dirs.append(R._normalize_like_the_reference(R._cosine_about(rng, nrm)))
    o, d = np.concatenate(orgs), np.concatenate(dirs)
    order = rng.permutation(o.shape[0])
    sets["bounce"] = (o[order], d[order])
    # ... with the cosine down to 2^-17, log-uniform
    orgs, dirs = [], []
    for i in walls:
        p, nrm = _hit_points(rng, c, r2, i, per)
        orgs.append(p)
        dirs.append(_about(rng, nrm, 2.0 ** rng.uniform(-17.0, -3.0, per)))
    sets["grazing"] = (np.concatenate(orgs), np.concatenate(dirs))
    # origins within 5e-4 of a second wall on its far side (just inside that wall's sphere), heading back into the room:
    # the wall behind the ray returns its far root there
    orgs, dirs = [], []
    for i in walls:
        p, nrm = _wall_points(rng, c, r2, i, per, offset=10.0 ** rng.uniform(-9.0, np.log10(5e-4), per))
        orgs.append(p)
        dirs.append(R._normalize_like_the_reference(R._cosine_about(rng, nrm)))
    sets["behind_a_wall"] = (np.concatenate(orgs), np.concatenate(dirs))
    # origins on one wall within 5e-4 of a second one (the room's edges), heading INTO the second: its near root is under 0.001
    # for most of them and its far root is returned — by the wall the ray heads for, through the general updates
    orgs, dirs = [], []
    for i in walls:
        j = walls[(walls.index(i) + 2) % 6]  # a wall on another axis
        p, _ = _wall_points(rng, c, r2, i, per)
        a = int(np.argmax(np.abs(c[j])))
        k, l = [q for q in range(3) if q != a]
        rr = np.sqrt(r2[j]) + 10.0 ** rng.uniform(-9.0, np.log10(5e-4), per)
        p[:, a] = c[j, a] - np.sign(c[j, a]) * np.sqrt(rr * rr - p[:, k] ** 2 - p[:, l] ** 2)
        orgs.append(p)
        dirs.append(R._normalize_like_the_reference(R._cosine_about(rng, (c[j] - p) / rr[:, None])))
    sets["into_a_second_wall"] = (np.concatenate(orgs), np.concatenate(dirs))
    # |d_a| below 2e-3 on one axis, and +-0 there; origins anywhere in the room
    o = rng.uniform(-9.99, 9.99, (m, 3))
    d = R._normalize_like_the_reference(rng.normal(size=(m, 3)))
    a = rng.integers(0, 3, m)
    small = rng.uniform(-2e-3, 2e-3, m)
    small[::4] = 0.0
    small[1::4] = -0.0
    d[np.arange(m), a] = small
    sets["flat"] = (o, d)
    # origins inside a wall sphere, 1e-3 .. 100 units behind the wall, any direction
    orgs = []
    for i in walls:
        orgs.append(_wall_points(rng, c, r2, i, per, offset=10.0 ** rng.uniform(-3.0, 2.0, per))[0])
    sets["inside_a_wall"] = (np.concatenate(orgs), R._normalize_like_the_reference(rng.normal(size=(per * 6, 3))))
    # primary rays from the camera, which sits on the -z wall
    sets["camera"] = R.camera_rays(rng, cam, target, m)
    # non-finite rays: one component of the origin or the direction is NaN or +-inf
    o = rng.uniform(-9.99, 9.99, (m, 3))
    d = R._normalize_like_the_reference(rng.normal(size=(m, 3)))
    which, comp = rng.integers(0, 2, m), rng.integers(0, 3, m)
    bad = rng.choice(np.array([np.nan, np.inf, -np.inf]), m)
    o[np.arange(m)[which == 0], comp[which == 0]] = bad[which == 0]
    d[np.arange(m)[which == 1], comp[which == 1]] = bad[which == 1]
    sets["non_finite"] = (o, d)
    return sets
