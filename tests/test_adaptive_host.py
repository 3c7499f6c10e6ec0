"""Tile lists and tile-adaptive sampling without a GPU: the three entry points are exported and bound, their argument
checks run before the scene or the device is touched, rtm_adaptive_work_bytes follows its formula, and the NumPy
restatement of the schedule and the estimator (_adaptive_ref) behaves as include/rtm.h states."""
import ctypes as C

import numpy as np
import pytest

import _adaptive_ref as ref
import raytracingmin_amd as rtm
from raytracingmin_amd import _lib

INVALID_ARGUMENT = -1  # RTM_ERR_INVALID_ARGUMENT (include/rtm.h)
FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below fails before it would be


def _settings(w=20, h=12, s=4, ss=2):
    st = _lib.rtm_settings()
    st.width, st.height, st.samples, st.super_samples = w, h, s, ss
    return st


def _options(rows):
    opt = _lib.rtm_options()
    opt.row_end = rows
    return opt


def test_symbols_are_exported_and_bound():
    L = rtm.lib()
    for name, nargs in (("rtm_render_scene_tiles", 12), ("rtm_adaptive_work_bytes", 2), ("rtm_render_adaptive", 11)):
        assert name in _lib.SIGNATURES
        assert len(getattr(L, name).argtypes) == nargs
    assert C.sizeof(_lib.rtm_adaptive_params) == 8
    assert L.rtm_abi_version() == 5


def test_tile_list_arguments_are_checked_before_the_scene():
    L = rtm.lib()
    st, opt = _settings(), _options(12)  # N = 16

    def call(a, b, tiles, n, accum):
        return L.rtm_render_scene_tiles(C.byref(st), None, C.byref(opt), a, b, tiles, n, accum, None, None, None, None)

    assert call(5, 4, FAKE, 3, FAKE) == INVALID_ARGUMENT and b"sample range" in L.rtm_last_error_detail()
    assert call(0, 17, FAKE, 3, FAKE) == INVALID_ARGUMENT and b"sample range" in L.rtm_last_error_detail()
    assert call(0, 16, FAKE, 3, None) == INVALID_ARGUMENT and b"accum" in L.rtm_last_error_detail()
    assert call(0, 16, None, 3, FAKE) == INVALID_ARGUMENT and b"tile list" in L.rtm_last_error_detail()
    # an empty list (or range) enqueues nothing and never looks at the scene
    s = _lib.rtm_stats()
    s.samples = 7
    assert L.rtm_render_scene_tiles(C.byref(st), None, C.byref(opt), 0, 16, None, 0, FAKE, None, None, None,
                                    C.byref(s)) == 0
    assert s.samples == 0
    # valid arguments reach the scene check
    assert call(0, 16, FAKE, 3, FAKE) == INVALID_ARGUMENT and b"scene" in L.rtm_last_error_detail()


def test_adaptive_arguments_are_checked_before_the_scene_and_the_device():
    L = rtm.lib()
    st, opt = _settings(), _options(12)

    def call(prm, accum=FAKE, work=C.c_void_p(0x10000)):
        return L.rtm_render_adaptive(C.byref(st), None, C.byref(opt), prm, accum, None, None, None, work, None, None)

    good = _lib.rtm_adaptive_params(4, 0.05)
    assert call(None) == INVALID_ARGUMENT and b"params" in L.rtm_last_error_detail()
    assert call(C.byref(good), accum=None) == INVALID_ARGUMENT and b"accum" in L.rtm_last_error_detail()
    assert call(C.byref(good), work=None) == INVALID_ARGUMENT and b"work" in L.rtm_last_error_detail()
    assert call(C.byref(_lib.rtm_adaptive_params(0, 0.05))) == INVALID_ARGUMENT
    assert b"min_samples" in L.rtm_last_error_detail()
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(C.byref(_lib.rtm_adaptive_params(4, bad))) == INVALID_ARGUMENT
        assert b"threshold" in L.rtm_last_error_detail()
    assert call(C.byref(good), work=C.c_void_p(0x10008)) == INVALID_ARGUMENT and b"aligned" in L.rtm_last_error_detail()
    # a negative threshold is legal: the call reaches the scene check
    assert call(C.byref(_lib.rtm_adaptive_params(4, -1.0))) == INVALID_ARGUMENT and b"scene" in L.rtm_last_error_detail()


@pytest.mark.parametrize("w,h,band", [(20, 12, None), (1920, 1080, None), (45, 27, None), (7, 1, None), (45, 40, (3, 1))])
def test_work_bytes_match_the_formula(w, h, band):
    L = rtm.lib()
    st, opt = _settings(w, h), _options(h)
    if band:
        opt.band_count, opt.band_index = band
    rows = L.rtm_output_rows(C.byref(opt))
    assert L.rtm_adaptive_work_bytes(C.byref(st), C.byref(opt)) == ref.work_bytes(w, rows)
    opt.row_begin = opt.row_end = 0
    assert L.rtm_adaptive_work_bytes(C.byref(st), C.byref(opt)) == 0


def test_schedule():
    assert ref.schedule(64, 4) == [4, 8, 16, 32, 64]
    assert ref.schedule(72, 5) == [5, 10, 20, 40, 72]  # m not a power of two: the last pass is short
    assert ref.schedule(1024, 16) == [16, 32, 64, 128, 256, 512, 1024]
    assert ref.schedule(72, 72) == [72] and ref.schedule(72, 500) == [72]  # m >= N: one pass
    assert ref.schedule(1, 1) == [1]


def _states(n, rows, w, rng, scale=0.3):
    """Synthetic progressive accumulators: per-sample terms in [0, scale), their running sums at every sample count."""
    terms = rng.random((n, rows, w, 3)) * scale
    acc = np.zeros((rows, w, 3))
    out = {0: acc.copy()}
    for k in range(n):
        acc = acc + terms[k]
        out[k + 1] = acc.copy()
    return out


def test_all_zero_tile_stops_at_b1_and_negative_threshold_never_stops():
    rng = np.random.default_rng(1)
    rows, w, n, m = 20, 27, 64, 4
    states = _states(n, rows, w, rng)
    for k in states:  # tile 1 (columns 8..15 of row block 0) sees only black
        states[k][0:8, 8:16] = 0.0
    tx, ty = 4, 3
    ts, trace = ref.run(states, n, m, 0.0, tx, ty)
    assert ts[0, 1] == 8  # E = 0 <= 0
    assert ref.tile_error(states[8], states[4], n, 4, 8, tx, 1) == 0.0
    ts, _ = ref.run(states, n, m, -1e-30, tx, ty)
    assert (ts == n).all()


def test_nan_keeps_a_tile_active_and_equal_error_stops():
    rng = np.random.default_rng(2)
    rows, w, n, m = 16, 16, 32, 4
    states = _states(n, rows, w, rng)
    for k in states:
        if k >= 4:
            states[k][3, 2, 1] = np.nan  # one pixel of tile 0
    ts, _ = ref.run(states, n, m, 1e30, 2, 2)
    assert ts[0, 0] == n and (ts.flat[1:] == 8).all()
    # the threshold equal to E (as a float32 holds it) stops the tile
    clean = _states(n, rows, w, np.random.default_rng(3))
    E = ref.tile_error(clean[8], clean[4], n, 4, 8, 2, 3)
    thr = float(np.float32(E))
    assert ref.stays_active(E, 8, n, thr) == (not (E <= np.float64(np.float32(thr))))
    E_exact = np.float64(np.float32(E))  # an E that a float threshold holds exactly
    assert not ref.stays_active(E_exact, 8, n, float(np.float32(E)))
    assert ref.stays_active(np.nextafter(E_exact, np.inf), 8, n, float(np.float32(E)))
    assert ref.stays_active(np.float64("nan"), 8, n, 1e30)
    assert not ref.stays_active(0.0, n, n, -1.0)  # b = N: never active


def test_reference_estimator_on_a_hand_computed_pixel():
    acc = np.zeros((8, 8, 3))
    snap = np.zeros((8, 8, 3))
    acc[0, 0] = (0.5, 0.25, 0.125)  # after b = 8 of N = 16: I = acc * 2
    snap[0, 0] = (0.25, 0.25, 0.0)  # after a = 4: J = snap * 4
    I, J = acc[0, 0] * 2.0, snap[0, 0] * 4.0
    d = (abs(I[0] - J[0]) + abs(I[1] - J[1])) + abs(I[2] - J[2])
    e = d / (1e-3 + np.sqrt((I[0] + I[1]) + I[2]))
    assert ref.tile_error(acc, snap, 16, 4, 8, 1, 0) == e


@pytest.mark.parametrize("n,m", [(64, 4), (72, 5), (48, 48)])
def test_mid_threshold_decisions_shrink_the_list(n, m):
    rng = np.random.default_rng(n)
    rows, w = 24, 40
    states = _states(n, rows, w, rng)
    for k in states:
        states[k][:, :16] *= 0.01  # quiet tiles on the left
    ts, trace = ref.run(states, n, m, 0.02, 5, 3)
    ends = ref.schedule(n, m)
    assert set(np.unique(ts)) <= set(ends)
    if len(ends) == 1:
        assert (ts == n).all() and trace == []
        return
    sizes = [len(t) for _, t in trace]
    assert sizes == sorted(sizes, reverse=True)
    for _, active in trace:
        assert active == sorted(active)
