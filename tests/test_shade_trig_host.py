"""The tolerance row's sin / cos table as the HOST builds it (csrc/rtm_kernels_tol.hip: trig_table_host, through the debug
hook rtm_debug_trig_table): entry i = (sin, cos) of i 2 pi / entries, evaluated in long double and rounded to double once.
No device is touched.

The bound: a value computed in x87 long double (64-bit significand) and rounded to double is within half an ulp of the long
double value; the long double argument i * (2 pi_L / entries) carries 2^-64 of up to 2 pi — 3.4e-19, 0.003 ulp of a result
near 1 — and numpy's own long double sine is the same libm's.  0.51 ulp covers both."""
import numpy as np
import pytest

TWO_PI_L = np.longdouble(2) * np.arctan2(np.longdouble(0), np.longdouble(-1))  # 2 pi, rounded to long double


def _table(rtm, entries):
    out = np.empty((entries, 2), dtype=np.float64)
    rtm._lib.check(rtm.lib().rtm_debug_trig_table(entries, out.ctypes.data), "trig table")
    return out


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _ulp_distance(table, want_l):
    """|table - want| in ulps of the double that `want` rounds to (want: long double)"""
    ulp = np.spacing(np.abs(want_l.astype(np.float64)))
    return np.abs(table.astype(np.longdouble) - want_l) / ulp.astype(np.longdouble)


@pytest.mark.parametrize("entries", [16384, 4096])
def test_table_entries_are_the_rounded_long_double_values(rtm, entries):
    assert np.finfo(np.longdouble).nmant >= 63, "the reference of this test is x87 long double"
    t = _table(rtm, entries)
    angle = np.arange(entries, dtype=np.longdouble) * (TWO_PI_L / np.longdouble(entries))
    for col, want in ((0, np.sin(angle)), (1, np.cos(angle))):
        d = _ulp_distance(t[:, col], want)
        print(f"{entries} entries, {'sin' if col == 0 else 'cos'}: worst distance from the long double value {float(d.max()):.4f} ulp")
        assert float(d.max()) <= 0.51
    assert t[0, 0] == 0.0 and not np.signbit(t[0, 0]) and t[0, 1] == 1.0
    # the quarter points: the component of magnitude one is exactly +-1, the other is what the long double sine of the
    # ROUNDED quarter turn is (|.| < 2^-63: k pi_L / 2 is not k pi / 2), to the same bound
    q = entries // 4
    for k, (s, c) in enumerate(((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0))):
        row = t[k * q]
        if s != 0.0:
            assert row[0] == s and abs(row[1]) < 2.0 ** -62
        else:
            assert row[1] == c and abs(row[0]) < 2.0 ** -62
        a = np.array([np.longdouble(k * q) * (TWO_PI_L / np.longdouble(entries))])
        assert float(_ulp_distance(row[:1], np.sin(a)).max()) <= 0.51 and float(_ulp_distance(row[1:], np.cos(a)).max()) <= 0.51


def test_table_hook_refuses_what_it_cannot_fill(rtm):
    out = np.empty(2, dtype=np.float64)
    assert rtm.lib().rtm_debug_trig_table(0, out.ctypes.data) != 0
    assert rtm.lib().rtm_debug_trig_table(16, None) != 0
