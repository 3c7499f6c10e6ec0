"""Round 14 (profiles/r14/bounce_fused.md): the tolerance unit's shading block takes the bounce direction from ONE reciprocal root,
k = sqrt(r2) / y = r2 rsqrt(r2 y y), without building the reference's orthonormal basis (csrc/rtm_path.h: bounce_nd_fused,
MathSpecT::bounce_scale_xz).  No GPU here: both forms restated in numpy with the float island (tests/_bounce_model.py), the
truth in long double from the same y, sine and cosine.

The bound: per component |nd - truth| <= 2^-44 — two light roots (k and s1 = sqrt(1 - r2)) at the project's 2^-45 each, on
components of magnitude at most 1.  v_rsq_f64 / v_rcp_f64 are modelled as exact times (1 + e), |e| <= 2^-23, at both ends and at
random e per record.  The device's own figures: tests/test_bounce_fused_gpu.py."""
import numpy as np
import pytest

import _bounce_model as bm

BOUND = 2.0 ** -44
N = 1 << 16
FAMILIES = bm.families(N, 1401)
E23 = 2.0 ** -23


def _errors(e):
    rows = []
    for name, w, m1, m2 in FAMILIES:
        truth = bm.nd_truth(w, m1, m2)
        ef = np.abs(bm.LD(bm.nd_fused(w, m1, m2, e)) - truth).max(axis=0).astype(np.float64)
        eb = np.abs(bm.LD(bm.nd_basis(w, m1, m2, e)) - truth).max(axis=0).astype(np.float64)
        rows.append((name, ef, eb))
    return rows


@pytest.mark.parametrize("e", ["+2^-23", "-2^-23", "random", "0"])
def test_fused_form_is_within_two_light_roots_of_the_truth(e):
    ev = {"+2^-23": E23, "-2^-23": -E23, "0": 0.0}.get(e)
    if ev is None:
        ev = np.random.default_rng(1402).uniform(-E23, E23, N)
    for name, ef, eb in _errors(ev):
        print(f"e = {e}, {name}: max |fused - truth| per component {ef / 2.0 ** -45} x 2^-45, basis form {eb / 2.0 ** -45} x 2^-45")
        assert np.all(ef <= BOUND), (name, ef)


def test_families_hold_what_the_issue_names():
    """every sign pattern of (w.x, w.z), floor-like normals from 1e-7 to 1e-3, m2 = 1, 3, 2^24 - 1, m1 in all four quadrants"""
    for name, w, m1, m2 in FAMILIES:
        assert {(a > 0, b > 0) for a, b in zip(w[:256, 0], w[:256, 2])} == {(True, True), (True, False), (False, True), (False, False)}, name
        assert set(np.unique(m1 // (bm.M24 // 4))) == {0, 1, 2, 3} and np.all(m1 % 2 == 1) and np.all(m2 % 2 == 1)
        assert {1, 3, bm.M24 - 1} <= set(m2[:16].tolist()) and m1.max() < bm.M24 and m2.max() < bm.M24
        assert np.allclose(np.linalg.norm(w, axis=1), 1.0, atol=1e-12)
    floor = FAMILIES[1][1]
    assert np.abs(floor[:, [0, 2]]).min() >= 1e-7 and np.abs(floor[:, [0, 2]]).max() <= 1e-3
    assert np.abs(floor[:, [0, 2]]).min() < 2e-7 and np.abs(floor[:, [0, 2]]).max() > 5e-4


def test_p_stays_inside_the_unscaled_sequences_range():
    """p = r2 y y for r2 in [2^-24, 1) and y in [2^-48, 2^64) (sqrtf_fast_ok): [2^-120, 2^128), far inside [2^-767, 2^1023) — at the
    corners, in doubles, with y a float"""
    for r2 in (2.0 ** -24, 1.0 - 2.0 ** -24):
        for y in (np.float32(2.0 ** -48), np.nextafter(np.float32(2.0 ** 64), np.float32(0))):
            p = r2 * (float(y) * float(y))
            assert 2.0 ** -120 <= p < 2.0 ** 128
            y0 = 1.0 / np.sqrt(p)
            assert 2.0 ** -64 < y0 <= 2.0 ** 60  # a normal number: half_of_rsq's condition
