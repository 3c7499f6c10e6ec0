"""The acceptance of the tolerance row's wall-pair search (csrc/rtm_path.h: accept_batch_lane; round 15) in numpy, shared by
tests/test_accept_walls_host.py and tests/test_accept_walls_gpu.py, with the seeded record families both use.

A record is what the search hands the acceptance for one ray: (b, sq, idx) of its four candidates — the lamp in slot 0, then per
opposite pair the wall the ray heads for.  Two forms answer "does some lane of the wave have a far root":
  with_t2   far  = OR (t2 >= 1e-5f) & ~(t1 > 0.001) over all four candidates (rounds 10 to 14; the lamp's slot still);
  walls     far' = the lamp's term | OR (t1 <= 0.001) over the three walls — no t2 —, and only where far' is set, far itself.
Either way a wave with far == 0 takes the packed minimum (v_min_f64 over t1 with the index in its last three bits, a NaN where
t1 is no near root) and any other wave the general chain (sphere_update's rule, candidate by candidate).  `literal_far_prime`
is the form that would take the general chain wherever far' is set: its distances differ in the last three bits, which is why
the kernels ask a second time instead.  `wave`: records per wave (the masks are a wave's)."""
import numpy as np

import _axis_disc_rays as R
import _wall_pairs_model as W

T_NEAR, T_MIN, DBL_MAX = W.T_NEAR, W.T_MIN, W.DBL_MAX
QNAN_HI = np.uint64(0x7FF80000) << np.uint64(32)
WALL_SLOTS = np.array([False, True, True, True])
PER_FAMILY = 65536


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _wave_any(mask, wave):
    return np.repeat(mask.reshape(-1, wave).any(axis=1), wave)


def _terms(b, sq):
    with np.errstate(all="ignore"):
        t1, t2 = b - sq, b + sq
        return t1, t2, t1 > T_NEAR, (t2 >= T_MIN) & ~(t1 > T_NEAR), t1 <= T_NEAR


def _packed(t1, keep, idx):
    """v_min_f64 over the candidates: t1 with the index in its last three bits where `keep`, else a quiet NaN; from DBL_MAX"""
    best = np.full(t1.shape[0], DBL_MAX)
    for k in range(t1.shape[1]):
        lo = (bits(t1[:, k]) & ~np.uint64(7)) | idx[:, k].astype(np.uint64)
        hi_lo = np.where(keep[:, k], lo, QNAN_HI | (lo & np.uint64(0xFFFFFFFF)))
        best = np.fmin(best, hi_lo.view(np.float64))  # (fmin: the other operand for a NaN, like the instruction for a quiet one)
    hit = ((bits(best).astype(np.int64) + 1) & 7) - 1
    return best, hit


def _general(b, sq, idx):
    m = b.shape[0]
    dis, hit = np.full(m, DBL_MAX), np.full(m, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(b.shape[1]):
            t1, t2 = b[:, k] - sq[:, k], b[:, k] + sq[:, k]
            t = np.where(t1 > T_NEAR, t1, t2)
            ok = (t < dis) & ~(t < T_MIN)
            dis[ok], hit[ok] = t[ok], idx[ok, k]
    return dis, hit


def _choose(general, b, sq, idx, keep):
    t1 = _terms(b, sq)[0]
    pd, ph = _packed(t1, keep, idx)
    gd, gh = _general(b, sq, idx)
    return np.where(general, gd, pd), np.where(general, gh, ph)


def with_t2(b, sq, idx, wave=1):
    """-> dis, hit, far per record, general per record (the wave's)"""
    _, _, near, far_k, _ = _terms(b, sq)
    far = far_k.any(axis=1)
    general = _wave_any(far, wave)
    dis, hit = _choose(general, b, sq, idx, near)
    return dis, hit, far, general


def walls(b, sq, idx, wave=1, literal_far_prime=False):
    """-> dis, hit, far' per record, general per record, asked-again per record (the wave's)"""
    t1, _, near, far_k, le = _terms(b, sq)
    far_prime = (far_k[:, ~WALL_SLOTS].any(axis=1)) | (le[:, WALL_SLOTS].any(axis=1))
    again = _wave_any(far_prime, wave)
    general = again if literal_far_prime else again & _wave_any(far_k.any(axis=1), wave)
    keep = np.where(WALL_SLOTS[None, :], ~le, near)  # a wall's t1v keeps t1's high word unless le: a NaN t1 stays its own NaN
    dis, hit = _choose(general, b, sq, idx, keep)
    return dis, hit, far_prime, general, again


# ---- records --------------------------------------------------------------------------------------------------------------------

def box():
    c, r2, cam, target, data, rows, axis, group = W.cornell()
    table = np.concatenate([np.concatenate([c, r2[:, None]], axis=1), rows]).reshape(-1)  # rtm_debug_math_probe ops 55, 61, 62
    return dict(c=c, r2=r2, cam=cam, target=target, rows=rows, axis=axis, group=group, table=table)


def candidates(bx, org, dir):
    """(b, sq, idx) [m, 4] of the pair path's four candidates and `proven` [m], from tests/_wall_pairs_model.py's arithmetic"""
    rows, axis, group = bx["rows"], bx["axis"], bx["group"]
    od, oo, ook = W.shared(org, dir, rows, group)
    lb, lD4, _ = W.sphere_disc(rows[0], int(axis[0]), False, org, dir, od, oo, ook)
    _, _, proven, per_pair, _ = W.pair_path(rows, axis, group, org, dir)
    b = np.stack([lb] + [p[1] for p in per_pair], axis=1)
    D4 = np.stack([lD4] + [p[2] for p in per_pair], axis=1)
    idx = np.stack([np.zeros(org.shape[0], dtype=np.int64)] + [p[0] for p in per_pair], axis=1)
    with np.errstate(all="ignore"):
        return b, np.sqrt(D4), idx, proven


def _towards(rng, bx, i, m, gap):
    """rays from `gap` in front of wall i (in the room), cosine-weighted about the direction INTO the wall"""
    p, nrm = W._wall_points(rng, bx["c"], bx["r2"], i, m, offset=-np.asarray(gap, dtype=np.float64) * np.ones(m))
    return p, R._normalize_like_the_reference(R._cosine_about(rng, -nrm))


def ray_families(seed=1500, per=PER_FAMILY):
    """name -> (org, dir): the families that are RAYS (the probe ops take these; candidates() makes records of them).
    bounce: rays leaving each of the six walls from hit points as the kernel arrives at them — a third cosine-weighted from
    anywhere on the wall, a third at cosines from 2e-3 to 1 (log-uniform) from anywhere, a third at cosines from 1e-4 from within
    0.5 of the wall's middle on both lateral axes.  (Narrowed so: a ray at cosine g from lateral offset s still has a component
    TOWARDS the wall it leaves where g < s / 10000, and then that wall is the pair's candidate with both roots at or behind
    the origin — the one case with far' and not far.  0.5 sqrt(2) / 10000 = 0.7e-4, 10 sqrt(2) / 10000 = 1.4e-3.)
    primary: camera rays.  gap_*: rays that start 1e-3, 1e-6 and 0 in front of the wall they head for."""
    bx = box()
    rng = np.random.default_rng(seed)
    c, r2 = bx["c"], bx["r2"]
    fam = {}
    n6 = per // 6 + 1
    orgs, dirs = [], []
    for i in range(1, 7):
        third = n6 // 3 + 1
        p, nrm = W._hit_points(rng, c, r2, i, third)
        orgs.append(p)
        dirs.append(R._normalize_like_the_reference(R._cosine_about(rng, nrm)))
        p, nrm = W._hit_points(rng, c, r2, i, third)
        orgs.append(p)
        dirs.append(W._about(rng, nrm, 10.0 ** rng.uniform(np.log10(2e-3), 0.0, third)))
        # (the middle of the wall: points up to 1e-8 off the sphere on either side, which is what a hit point's q of 2e-4 means)
        a, r = int(np.argmax(np.abs(c[i]))), np.sqrt(r2[i])
        j, k = [q for q in range(3) if q != a]
        p = rng.uniform(-0.5, 0.5, (third, 3))
        rr = r + rng.uniform(-1e-8, 1e-8, third)
        p[:, a] = c[i, a] - np.sign(c[i, a]) * np.sqrt(rr * rr - p[:, j] ** 2 - p[:, k] ** 2)
        orgs.append(p)
        dirs.append(W._about(rng, (p - c[i]) / rr[:, None], 10.0 ** rng.uniform(-4.0, 0.0, third)))
    o, d = np.concatenate(orgs), np.concatenate(dirs)
    order = rng.permutation(o.shape[0])[:per]
    fam["bounce"] = (o[order], d[order])
    fam["primary"] = R.camera_rays(rng, bx["cam"], bx["target"], per)
    for name, gap in (("gap_1e-3", 1e-3), ("gap_1e-6", 1e-6), ("gap_0", 0.0)):
        orgs, dirs = [], []
        for i in range(1, 7):
            p, dd = _towards(rng, bx, i, n6, gap)
            orgs.append(p)
            dirs.append(dd)
        o, d = np.concatenate(orgs), np.concatenate(dirs)
        order = rng.permutation(o.shape[0])[:per]
        fam[name] = (o[order], d[order])
    assert all(v[0].shape == (per, 3) and v[1].shape == (per, 3) for v in fam.values())
    return bx, fam


def record_families(seed=1500, per=PER_FAMILY):
    """name -> (b, sq, idx): the ray families' records (proven rays: the others never reach this acceptance) and the
    families that exist as records alone, each a bounce record with one wall slot (or the lamp's, a quarter of them) rewritten:
    sq_nan; d4_zero (sq = +0); t1_at_0.001 (t1 exactly 0.001, its lower and its upper neighbour, from sq = 0 and from sq = 16
    with b on 0.001 + 16's grid); small_b (b of either sign from 1e-12 to 10, sq from |b| (1 - 1e-3) to |b| (1 + 1e-3): t2 on both
    sides of 1e-5f)."""
    bx, rays = ray_families(seed, per)
    fam = {}
    for name, (o, d) in rays.items():
        b, sq, idx, proven = candidates(bx, o, d)
        fam[name] = (b[proven], sq[proven], idx[proven])
    rng = np.random.default_rng(seed + 1)
    b0, sq0, idx0 = fam["bounce"]

    def rewritten(new_b, new_sq):
        pick = rng.integers(0, b0.shape[0], per)
        b, sq, idx = b0[pick].copy(), sq0[pick].copy(), idx0[pick].copy()
        slot = rng.integers(0, 4, per)
        rows = np.arange(per)
        if new_b is not None:
            b[rows, slot] = new_b
        sq[rows, slot] = new_sq
        return b, sq, idx

    fam["sq_nan"] = rewritten(None, np.where(rng.random(per) < 0.5, np.nan, -np.nan))
    fam["d4_zero"] = rewritten(np.where(rng.random(per) < 0.5, 1.0, -1.0) * 10.0 ** rng.uniform(-12.0, 1.5, per), 0.0)
    which = rng.integers(0, 3, per)
    target = np.array([np.nextafter(T_NEAR, 0.0), T_NEAR, np.nextafter(T_NEAR, 1.0)])[which]
    with_root = rng.random(per) < 0.5
    # (behind a root of 16 a t1 lives on 16's grid of 2^-48: the two grid points under 0.001 and the one above, b - 16 exact)
    on_grid = (np.floor(T_NEAR * 2.0 ** 48) + np.array([-1.0, 0.0, 1.0])[which]) * 2.0 ** -48
    fam["t1_at_0.001"] = rewritten(np.where(with_root, 16.0 + on_grid, target), np.where(with_root, 16.0, 0.0))
    sb = np.where(rng.random(per) < 0.5, 1.0, -1.0) * 10.0 ** rng.uniform(-12.0, 1.0, per)
    fam["small_b"] = rewritten(sb, np.abs(sb) * (1.0 + rng.uniform(-1e-3, 1e-3, per)))
    return fam
