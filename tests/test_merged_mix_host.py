"""Round 13 runs ONE pair of mix32 bodies per trip for both kinds of lane (csrc/rtm_device.h: rng_merged_mix): a lane whose path
goes on takes the pair's results as the bits of the bounce's two draws, a lane whose path ended as (ctr, k1) of the stream of the
sample it restarts with.  Nothing of the RNG's definition changes.  Here, without a GPU: the definition restated in
numpy is first tied to the host's own rng_open / rng_next through rtm_rng_u01, then a merged evaluation — inputs selected per lane,
the two bodies run once over all lanes — must give a continuing lane exactly the second and third draw of its stream and an ended
lane exactly rng_open(pkey, n'), for streams of (seed, pixel, sample) the host hook answers for and for raw seeded words."""
import numpy as np
import pytest

from raytracingmin_amd import _lib

PHI, C2 = np.uint32(0x9E3779B9), np.uint32(0x85EBCA6B)
U32 = np.uint32


def mix32(x):
    x = x.astype(U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x21F0AAAD)
    x ^= x >> U32(15)
    x *= U32(0x735A2D97)
    x ^= x >> U32(15)
    return x


def smfin64(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pixel_key(seed, pixel):
    mult = smfin64(np.array([seed], np.uint64) + np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    z = smfin64((pixel.astype(np.uint64) + np.uint64(1)) * mult)
    return (z & np.uint64(0xFFFFFFFF)).astype(U32), (z >> np.uint64(32)).astype(U32)


def rng_open(p0, p1, n):
    n = n.astype(U32)
    return mix32(p0 + n * PHI), mix32(p1 ^ (n * C2))


def draw_m(ctr, k1, j):
    """the odd integer m of draw j of the stream: u = m * 2^-24"""
    return U32(2) * (mix32((ctr + U32(j) * PHI) ^ k1) >> U32(9)) + U32(1)


def merged(ended, p0, p1, n_next, ctr, k1):
    """rng_merged_mix: `ctr` is the stream's counter as the roulette's draw left it (one draw on from the trip's incoming one)"""
    a = np.where(ended, p0 + n_next.astype(U32) * PHI, ctr ^ k1)
    b = np.where(ended, p1 ^ (n_next.astype(U32) * C2), (ctr + PHI) ^ k1)
    return mix32(a), mix32(b)


def host_u01(seed, pixel, sample, index):
    return _lib.lib().rtm_rng_u01(int(seed), int(pixel), int(sample), int(index))


S, SS = 16, 2                       # a frame of S * SS * SS = 64 samples per pixel, rendered in passes
N_END = 37                          # the end of a pass cut inside a sub-pixel
EDGE_SAMPLES = [0, 1, S - 1, S, 65535, N_END]


@pytest.fixture(scope="module")
def with_numpy_wrap():
    with np.errstate(over="ignore"):
        yield


def test_numpy_restatement_is_the_hosts_rng(with_numpy_wrap):
    seed = 0x5EED
    pixels = np.array([0, 1, 63, 64, 1919, 2073599], np.uint32)
    p0, p1 = pixel_key(seed, pixels)
    for n in EDGE_SAMPLES:
        ctr, k1 = rng_open(p0, p1, np.full(pixels.shape, n, np.uint32))
        for j in range(4):
            m = draw_m(ctr, k1, j)
            for k, px in enumerate(pixels):
                assert m[k] * 2.0 ** -24 == host_u01(seed, px, n, j), (px, n, j)


@pytest.mark.parametrize("pattern", ["all continue", "all end", "one of each kind", "alternating", "random"])
def test_merged_evaluation_on_host_streams(with_numpy_wrap, pattern):
    """streams the host hook answers for: pixel p, sample n, restarting with n' — every edge value of n' on every pattern"""
    seed = 77
    rng = np.random.default_rng(1300)
    lanes = 64 * len(EDGE_SAMPLES)
    pixels = rng.integers(0, 1920 * 1080, lanes).astype(np.uint32)
    samples = rng.integers(0, 65535, lanes).astype(np.uint32)
    n_next = np.repeat(np.array(EDGE_SAMPLES, np.uint32), 64)
    lane = np.arange(lanes) % 64
    ended = {"all continue": lane < 0, "all end": lane >= 0, "one of each kind": (lane == 5) ^ ((np.arange(lanes) // 64) % 2 == 1),
             "alternating": lane % 2 == 1, "random": rng.random(lanes) < 0.22}[pattern]
    p0, p1 = pixel_key(seed, pixels)
    ctr0, k1 = rng_open(p0, p1, samples)
    w0, w1 = merged(ended, p0, p1, n_next, ctr0 + PHI, k1)
    for k in range(lanes):
        if ended[k]:
            # the merged words are the stream (ctr, k1) of sample n': rng_open's own words, and the host's draws from them
            assert (w0[k], w1[k]) == tuple(x[0] for x in rng_open(p0[k:k + 1], p1[k:k + 1], n_next[k:k + 1]))
            for j in range(3):
                assert draw_m(w0[k:k + 1], w1[k:k + 1], j)[0] * 2.0 ** -24 == host_u01(seed, pixels[k], n_next[k], j)
        else:
            # ... the bits of the stream's second and third draw (the first was the roulette's)
            assert (2 * (int(w0[k]) >> 9) + 1) * 2.0 ** -24 == host_u01(seed, pixels[k], samples[k], 1)
            assert (2 * (int(w1[k]) >> 9) + 1) * 2.0 ** -24 == host_u01(seed, pixels[k], samples[k], 2)


def test_merged_evaluation_on_raw_words(with_numpy_wrap):
    """65 536 seeded (p0, p1, ctr, k1, n') sets, no key schedule behind them: the plain definition lane by lane"""
    rng = np.random.default_rng(1301)
    lanes = 65536
    p0, p1, ctr, k1 = (rng.integers(0, 2 ** 32, lanes, dtype=np.uint64).astype(U32) for _ in range(4))
    n_next = rng.integers(0, 65536, lanes).astype(np.uint32)
    n_next[:len(EDGE_SAMPLES) * 2] = np.repeat(np.array(EDGE_SAMPLES, np.uint32), 2)
    ended = rng.random(lanes) < 0.5
    ended[:len(EDGE_SAMPLES) * 2] = np.tile([False, True], len(EDGE_SAMPLES))
    w0, w1 = merged(ended, p0, p1, n_next, ctr + PHI, k1)
    o0, o1 = rng_open(p0, p1, n_next)
    d1, d2 = mix32((ctr + PHI) ^ k1), mix32((ctr + U32(2) * PHI) ^ k1)
    assert np.array_equal(w0[ended], o0[ended]) and np.array_equal(w1[ended], o1[ended])
    assert np.array_equal(w0[~ended], d1[~ended]) and np.array_equal(w1[~ended], d2[~ended])
    assert ended[:12].sum() == 6  # both kinds met every edge value
