"""Round 15 (profiles/r15/accept_walls.md): the acceptance of the tolerance row's wall-pair search forms no far-root sum t2 for a
pair's wall on its hot path (csrc/rtm_path.h: accept_batch_lane's WALLS).  Both forms restated in numpy (tests/_accept_walls_model.py)
over (b, sq, idx) records, 65 536 per family: bounce rays leaving each of the six walls of scenes/cornellBoxSetting.json down to
cosines of 1e-4, primary rays, rays that start 1e-3, 1e-6 and 0 in front of the wall they head for, sq NaN, D4 = 0, t1 exactly
0.001 and its two neighbours, b of either sign down to 1e-12.  Per record (a wave of one) and in waves of 8, as the probe ops hold
them:
  * far is a subset of far';
  * (dis, hit_object) are the same bits in both forms;
  * no record of the bounce and the primary family has far' without far — the second question is never asked for nothing
    there (the bounce family is narrowed for this as ray_families says: a grazing ray from far off a wall's middle does ask);
  * and what the second question is for: the form that takes the general chain wherever far' is set returns OTHER distances
    (the packed minimum's carry the index in their last three bits) on the families that have far' without far."""
import numpy as np
import pytest

import _accept_walls_model as A


@pytest.fixture(scope="module")
def records():
    return A.record_families()


FAMILIES = ["bounce", "primary", "gap_1e-3", "gap_1e-6", "gap_0", "sq_nan", "d4_zero", "t1_at_0.001", "small_b"]


def _both(records, name, wave):
    b, sq, idx = records[name]
    m = b.shape[0] // wave * wave
    assert m > 0.9 * A.PER_FAMILY, name  # (the ray families keep the rays that prove their pairs: the others never get here)
    b, sq, idx = b[:m], sq[:m], idx[:m]
    return (b, sq, idx), A.with_t2(b, sq, idx, wave), A.walls(b, sq, idx, wave)


@pytest.mark.parametrize("wave", [1, 8])
@pytest.mark.parametrize("name", FAMILIES)
def test_both_forms_return_the_same_bits(records, name, wave):
    _, (d0, h0, far, g0), (d1, h1, far_prime, g1, again) = _both(records, name, wave)
    print(f"{name}, waves of {wave}: far {far.mean():.4f}, far' {far_prime.mean():.4f}, far' without far {int((far_prime & ~far).sum())}, "
          f"general {g0.mean():.4f}, asked again {again.mean():.4f}, ids {np.unique(h0).tolist()}")
    assert bool((~far | far_prime).all()), name
    assert np.array_equal(A.bits(d0), A.bits(d1)) and np.array_equal(h0, h1), name
    assert np.array_equal(g0, g1), name          # the same chain in every wave
    assert bool((again | ~g1).all()), name       # ... the general one only behind the second question


@pytest.mark.parametrize("name", ["bounce", "primary"])
def test_no_second_question_for_nothing_on_bounce_and_primary_rays(records, name):
    _, (_, _, far, _), (_, _, far_prime, _, _) = _both(records, name, 1)
    assert int((far_prime & ~far).sum()) == 0
    assert 0.0 < far.mean() < 0.2  # (the families do hold far roots: bounce rays from a room's edge, primary rays from the wall)


def test_the_families_reach_what_they_are_for(records):
    for name in FAMILIES:
        (b, sq, idx), (_, h0, far, _), (_, _, far_prime, _, _) = _both(records, name, 1)
        with np.errstate(all="ignore"):
            t1 = b - sq
        assert np.all(idx[:, 0] == 0) and np.all((idx[:, 1:] - np.array([1, 3, 5])) >> 1 == 0), name
        if name == "sq_nan":
            assert np.isnan(sq).any(axis=1).all() and np.signbit(sq[np.isnan(sq)]).any() and not np.signbit(sq[np.isnan(sq)]).all()
        if name == "d4_zero":
            assert (sq == 0.0).any(axis=1).all()
        if name == "t1_at_0.001":
            for v in (np.nextafter(A.T_NEAR, 0.0), A.T_NEAR, np.nextafter(A.T_NEAR, 1.0)):
                assert ((t1 == v) & (sq == 0.0)).any(), v  # (from sq = 16, t1 lands on 16's grid around 0.001: the line below)
            near16 = t1[sq == 16.0]
            assert (near16 <= A.T_NEAR).any() and (near16 > A.T_NEAR).any()
        if name == "small_b":
            with np.errstate(all="ignore"):
                t2 = b + sq
            assert (np.abs(b) < 1e-11).any() and (b < 0).any() and (b > 0).any()
            assert ((t2 < A.T_MIN) & (t2 > 0)).any() and (t2 >= A.T_MIN).any()
        if name in ("gap_1e-6", "gap_0"):
            assert far.all()
        if name in ("d4_zero", "small_b"):
            assert (far_prime & ~far).mean() > 0.25, name


@pytest.mark.parametrize("name", ["d4_zero", "small_b"])
def test_changing_chains_where_far_prime_is_set_would_move_the_distance(records, name):
    (b, sq, idx), (d0, h0, far, _), _ = _both(records, name, 1)
    d2, h2, far_prime, general, _ = A.walls(b, sq, idx, 1, literal_far_prime=True)
    moved = A.bits(d0) != A.bits(d2)
    assert np.array_equal(h0, h2)                       # the same sphere ...
    assert moved.any() and not moved[~(far_prime & ~far)].any()  # ... at another distance, exactly where the chains differ
    assert np.all((A.bits(d0[moved]) ^ A.bits(d2[moved])) < 8)   # in the last three bits: the packed index


def _more_ray_sets():
    import _wall_pairs_model as W
    bx = A.box()
    return bx, W.ray_sets(A.PER_FAMILY // 6 * 6 + 6, 2015, bx["c"], bx["r2"], bx["cam"], bx["target"])


def test_an_infinite_b_never_reaches_the_acceptance():
    """Point 1 of the proof (far is a subset of far') has one way out: b = sq = +inf, a far root whose t1 is NaN.  As records the
    two forms then part — and no ray gets there: a wall candidate's b = |c| |d_a| - o.d is +inf only with -o.d = +inf or |d_a|
    infinite, which leaves the other wall's b_u at +inf or NaN, the lane unproven and its wave in the seven-sphere block.
    tests/_wall_pairs_model.py's non-finite rays (one component of the origin or the direction NaN or +-inf)."""
    b = np.array([[-1.0, np.inf, 30.0, 40.0]])
    sq = np.array([[np.nan, np.inf, 1.0, 2.0]])
    idx = np.array([[0, 1, 3, 5]])
    _, _, far, _ = A.with_t2(b, sq, idx)
    _, _, far_prime, _, _ = A.walls(b, sq, idx)
    assert far[0] and not far_prime[0]  # what the kernels would get wrong, if it could happen
    bx, sets = _more_ray_sets()
    org, dir = sets["non_finite"]
    b, sq, idx, proven = A.candidates(bx, org, dir)
    with np.errstate(all="ignore"):
        od = (org * dir).sum(axis=1)
    assert np.isposinf(b[:, 1:]).any() and (np.isinf(od) | np.isnan(od)).mean() > 0.9  # the set does hold such candidates
    assert not proven[np.isposinf(b[:, 1:]).any(axis=1)].any()
    # (b = -inf or NaN does get there — b_u = -inf proves — and is harmless: t2 is then no number at or above 1e-5f)
    odd = proven & ~np.isfinite(b[:, 1:]).all(axis=1)
    assert odd.any()
    d0, h0, far, g0 = A.with_t2(b[odd], sq[odd], idx[odd])
    d1, h1, far_prime, g1, _ = A.walls(b[odd], sq[odd], idx[odd])
    assert bool((~far | far_prime).all()) and np.array_equal(A.bits(d0), A.bits(d1)) and np.array_equal(h0, h1) and np.array_equal(g0, g1)


def test_grazing_rays_from_anywhere_on_a_wall():
    """What the bounce family is narrowed away from: cosines down to 2^-17 from hit points anywhere on a wall
    (tests/_wall_pairs_model.py's grazing set).  The rays that prove their pairs do ask the second question for nothing — and get
    the same bits; their share is bounded by the geometry: the ray must still point at the wall it leaves, cosine under
    s / 10000 <= 1.5e-3 for a lateral offset s <= 10 sqrt(2), a fifth of a log-uniform cosine between 2^-17 and 2^-3."""
    bx, sets = _more_ray_sets()
    org, dir = sets["grazing"]
    b, sq, idx, proven = A.candidates(bx, org, dir)
    b, sq, idx = b[proven], sq[proven], idx[proven]
    assert b.shape[0] > 1000
    d0, h0, far, g0 = A.with_t2(b, sq, idx)
    d1, h1, far_prime, g1, _ = A.walls(b, sq, idx)
    share = float((far_prime & ~far).mean())
    print(f"grazing: {b.shape[0]} proven rays, far {far.mean():.4f}, far' without far {share:.4f}")
    assert bool((~far | far_prime).all())
    assert np.array_equal(A.bits(d0), A.bits(d1)) and np.array_equal(h0, h1) and np.array_equal(g0, g1)
    assert 0.0 < share  # the case exists ...
    assert (far_prime & ~far).sum() <= 0.5 * org.shape[0]  # ... and stays a part of the set (of ALL its rays: under a half)
