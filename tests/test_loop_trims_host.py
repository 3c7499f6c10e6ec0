"""The two bit tricks of the tolerance row's round-8 trip (csrc/rtm_device.h sincos_turn24_tab_load, csrc/rtm_path.h
half_of_rsq), restated in numpy and compared with the arithmetic they replace.  No GPU: the device's own instructions are
compared in tests/test_loop_trims_gpu.py.

The angle split.  A draw is the odd integer m < 2^24; the shading block needs k = rint(m 2^-10) (the table point, taken
modulo 16 384) and fl = m 2^-10 - k (the remainder in table steps), and the remainder's angle r = fl (2 pi / 16384).  In
integers: t = m + 512, byte offset of the point (t >> 6) & 0x3FFF0, fi = (t & 1023) - 512 = fl 2^10, and
r = fi ((2 pi / 16384) 2^-10).  Every odd m.

The half.  0.5 * y as y with its exponent field lowered by one, for normal y (what v_rsq_f64 returns for every positive
finite operand: 2^-512 .. 2^537)."""
import numpy as np

ENTRIES = 16384
STEP = 6.283185307179586 / ENTRIES


def test_integer_angle_split_is_the_rint_split_for_every_draw():
    worst_fi = 0
    chunk = 1 << 21
    for a in range(0, 1 << 23, chunk):
        mi = 2 * np.arange(a, a + chunk, dtype=np.int64) + 1
        # the split in doubles (round 7)
        x = mi.astype(np.float64) * 2.0 ** -10
        k = np.rint(x)
        fl = x - k
        off_old = (k.astype(np.int64) & (ENTRIES - 1)) * 16
        r_old = fl * STEP
        # ... in integers, in 32-bit unsigned arithmetic as the device does it
        t = (mi + 512).astype(np.uint32)
        off_new = (t >> np.uint32(6)) & np.uint32(0x3FFF0)
        fi = (t & np.uint32(1023)).astype(np.int32) - 512
        r_new = fi.astype(np.float64) * (STEP * 2.0 ** -10)
        assert np.array_equal(t >> np.uint32(10), k.astype(np.uint32))  # the point itself, before the wrap of 16 384 to 0
        assert np.array_equal(off_new.astype(np.int64), off_old)
        assert np.array_equal(fi.astype(np.float64) * 2.0 ** -10, fl)
        assert np.array_equal(r_new.view(np.uint64), r_old.view(np.uint64))
        assert not np.any(fi == 0)  # m is odd: never on a table point, never a tie
        worst_fi = max(worst_fi, int(np.abs(fi).max()))
    assert worst_fi == 511
    assert (STEP * 2.0 ** -10) * 2.0 ** 10 == STEP  # the scale: a power of two away from the old one, exactly


def _halve_by_exponent(y):
    hi_lo = np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
    hi = (hi_lo >> np.uint64(32)).astype(np.uint32) - np.uint32(0x00100000)  # (wraps like the device's 32-bit add)
    return ((hi.astype(np.uint64) << np.uint64(32)) | (hi_lo & np.uint64(0xFFFFFFFF))).view(np.float64)


def test_exponent_halving_is_half_on_normal_doubles():
    rng = np.random.default_rng(8)
    # random mantissas and signs under every exponent field from 2 (the smallest whose half is still normal) to 2046
    bits = rng.integers(0, 1 << 52, size=1 << 20, dtype=np.uint64)
    bits |= rng.integers(2, 2047, size=bits.size, dtype=np.uint64) << np.uint64(52)
    bits |= rng.integers(0, 2, size=bits.size, dtype=np.uint64) << np.uint64(63)
    y = bits.view(np.float64)
    assert np.all(np.isfinite(y))
    assert np.array_equal(_halve_by_exponent(y).view(np.uint64), (0.5 * y).view(np.uint64))
    # the powers of two 2^k, k = -1000 .. 999, and the range a reciprocal root can have: 2^-512 .. 2^537
    p = 2.0 ** np.arange(-1000, 1000, dtype=np.float64)
    assert np.array_equal(_halve_by_exponent(p).view(np.uint64), (0.5 * p).view(np.uint64))
    with np.errstate(divide="ignore"):
        roots = 1.0 / np.sqrt(np.array([5e-324, 2.2250738585072014e-308, 1.0, 1.7976931348623157e308]))
    assert np.array_equal(_halve_by_exponent(roots).view(np.uint64), (0.5 * roots).view(np.uint64))
    # exponent field 1 (the smallest normals) is where the two part: 0.5 * y is subnormal, the trick gives field 0 with the same
    # mantissa bits.  No reciprocal root is down there.
    tiny = np.array([2.2250738585072014e-308 * 1.5])
    assert _halve_by_exponent(tiny)[0] != 0.5 * tiny[0]
