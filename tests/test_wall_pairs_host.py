"""The tolerance row's opposite-wall-pair search (csrc/rtm_path.h: sphere_chunk under kAxisPairsBit; round 10) in numpy on the
CPU — no device.  Per pair of walls at +c and -c on one axis the search tests the wall the ray heads for, with sphere_disc's
own operands, and proves from b_u <= -2^-5 and q_u >= 2^-20 b_u that the other one misses; a ray that cannot prove it takes the
seven-sphere block.  tests/_wall_pairs_model.py has both in float64 with fused multiply-adds.

Asserted on eight seeded ray sets of at least a million rays each: where the proof passes, the pair path's hit id and distance
bits are the general rule's over all seven spheres (csrc/rtm_path.h: sphere_update); the selected wall's b and D4 are
sphere_disc's for that wall bit for bit; in long double, a wall the proof drops has its near root under 0.001 and its far root
under half of 1e-5f; the host grants the extension to the Cornell box and refuses three near misses of it; and on the
cosine-weighted bounce rays at most 0.20 of 64-ray groups hold a ray that fails the proof (0.122 seen; above 0.20 the fast path
cannot pay for its fallback)."""
import ctypes as C

import numpy as np
import pytest

import _axis_disc_rays as R
import _wall_pairs_model as W

LD = np.longdouble
M = 1_000_002  # rays per set: a multiple of 6
SETS = ["bounce", "grazing", "behind_a_wall", "into_a_second_wall", "flat", "inside_a_wall", "camera", "non_finite"]


@pytest.fixture(scope="module")
def box():
    assert np.finfo(LD).nmant >= 63, "this test needs numpy's long double to be wider than float64 (x87: 64 bits)"
    c, r2, cam, target, data, rows, axis, group = W.cornell()
    assert group.tolist() == [False] + [True] * 6
    return dict(c=c, r2=r2, rows=rows, axis=axis, group=group, sets=W.ray_sets(M, 2010, c, r2, cam, target))


def _same_bits(x, y):
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


@pytest.mark.parametrize("name", SETS)
def test_pair_path_is_the_general_rule_where_the_proof_passes(box, name):
    org, dir = box["sets"][name]
    rows, axis, group, c, r2 = box["rows"], box["axis"], box["group"], box["c"], box["r2"]
    assert org.shape[0] >= 1_000_000
    dis7, hit7, discs = W.seven_block(rows, axis, group, org, dir)
    dis4, hit4, proven, per_pair, constant = W.pair_path(rows, axis, group, org, dir)
    share = 1.0 - float(proven.mean())
    groups = 1.0 - float(proven[:proven.size // 64 * 64].reshape(-1, 64).all(axis=1).mean())
    far = int(((hit7 >= 0) & proven).sum())
    print(f"{name}: {org.shape[0]} rays, {share:.4%} fail the proof, {groups:.4f} of 64-ray groups hold one ({1.0 - float(constant.mean()):.4%} "
          f"of rays with q_u >= -gamma in place of q_u >= 2 tau b_u); {far} proven rays hit something, ids seen {np.unique(hit7).tolist()}")
    # (id, bits of t) where the proof passes
    assert np.array_equal(hit4[proven], hit7[proven]), name
    assert bool(_same_bits(dis4[proven], dis7[proven]).all()), name
    # the selected wall's b and D4 are sphere_disc's for that wall, on every ray (proven or not)
    B7, D7 = np.stack([b for b, _ in discs]), np.stack([d for _, d in discs])
    rays, dropped_hits = np.arange(org.shape[0]), 0
    for idx, b, D4, bu, qu in per_pair:
        assert bool(_same_bits(b, B7[idx, rays]).all()) and bool(_same_bits(D4, D7[idx, rays]).all()), name
        other = idx + np.where(idx % 2 == 1, 1, -1)  # (1, 2), (3, 4), (5, 6)
        assert bool(_same_bits(bu, B7[other, rays]).all()), name
        dropped_hits += int((hit7 == other).sum())  # the block's hit is the wall the pair path would drop: never proven
        assert not proven[hit7 == other].any(), name
        # the dropped wall in long double, from (c, r*r) themselves: near root under 0.001, far root under half of 1e-5f
        with np.errstate(all="ignore"):
            a = int(axis[idx[0]]) - 1
            cu = np.where(other % 2 == 1, 1.0, -1.0).astype(LD) * LD(abs(c[idx[0], a]))
            p = -org.astype(LD)
            p[:, a] += cu
            bt = (p * dir.astype(LD)).sum(axis=1)
            Dt = bt * bt - (p * p).sum(axis=1) + LD(r2[idx[0]])
            real = proven & (Dt >= 0) & np.isfinite(org).all(axis=1) & np.isfinite(dir).all(axis=1)
            st = np.sqrt(np.where(real, Dt, 0))
        assert bool(((bt - st)[real] < W.T_NEAR).all()) and bool(((bt + st)[real] < 0.5 * W.T_MIN).all()), name
    if name == "bounce":
        assert share < 0.01 and groups <= 0.20, (share, groups)
    if name in ("behind_a_wall", "inside_a_wall"):  # the wall behind such a ray returns its far root (past 1e-5f: most of them)
        assert dropped_hits > org.shape[0] // 4, (name, dropped_hits)
    if name == "non_finite":  # a NaN anywhere reaches o.d or o.o: never proven (an infinity may be: the block misses too)
        assert not proven[np.isnan(org).any(axis=1) | np.isnan(dir).any(axis=1)].any()
    if name in ("into_a_second_wall", "flat", "camera", "grazing"):
        assert proven.mean() > 0.5, name  # the set does exercise the pair path


def _facts(spheres):
    from raytracingmin_amd import Camera, SettingData, _lib, vec3
    d = SettingData(width=8, height=8, samples=1, superSamples=1, camera=Camera(vec3(0, 0, -10), vec3(0, 0, 0), vec3(0, 1, 0), 2.0),
                    object=spheres)
    _, arr, n = d.to_c()
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().rtm_debug_wall_pairs(arr, n, out), "wall pairs")
    return int(out[0]), int(out[1])


def box_spheres(cx=(10010.0, -10010.0), radii=(10000.0,) * 6, c=10010.0):
    """the Cornell box's seven spheres with the x walls at cx, the walls' radii `radii` and the y and z walls at +-c"""
    from raytracingmin_amd import Material, SphereObject, vec3
    grey = Material(vec3(.7, .7, .7), vec3(0, 0, 0))
    pos = [vec3(cx[0], 0, 0), vec3(cx[1], 0, 0), vec3(0, c, 0), vec3(0, -c, 0), vec3(0, 0, c), vec3(0, 0, -c)]
    return [SphereObject(vec3(0, 10, 0), 5.0, Material(vec3(0, 0, 0), vec3(5, 5, 5)))] + [SphereObject(p, r, grey) for p, r in zip(pos, radii)]


def test_the_host_grants_the_extension_to_the_cornell_box_alone():
    data = R.load_spheres("cornellBoxSetting.json")[4]
    assert _facts(list(data.object)) == (1, 0b0101010)
    assert _facts(box_spheres()) == (1, 0b0101010)
    assert _facts(box_spheres(cx=(10010.0, -10011.0)))[0] == 0            # walls that are not symmetric
    assert _facts(box_spheres(radii=(10000.0, 9999.0) + (10000.0,) * 4))[0] == 0  # a pair of two radii
    # r 2^-17 < 2 beta = 2^-4: radius 8000 (every wall, so that they still share one K; c = 8010 keeps the room)
    granted, lower = _facts(box_spheres(cx=(8010.0, -8010.0), radii=(8000.0,) * 6, c=8010.0))
    assert (granted, lower) == (0, 0)
    assert _facts(box_spheres(cx=(8202.0, -8202.0), radii=(8192.0,) * 6, c=8202.0)) == (1, 0b0101010)  # ... and just above it
    assert _facts(box_spheres(cx=(-10010.0, 10010.0)))[0] == 0            # the lower index must hold +c
    for name in ("simpleSetting1.json", "settingData.json"):
        assert _facts(list(R.load_spheres(name)[4].object))[0] == 0, name
