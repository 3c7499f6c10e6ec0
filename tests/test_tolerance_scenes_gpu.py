"""The tolerance row (rtm_options.variant 18, csrc/rtm_kernels_tol.hip) beyond the Cornell box: the scenes built to break a nearest-hit
search or a shading block (tests/_edge_scenes.py and the other edge frames of tests/test_parity_gpu.py), a seeded population of 384
small frames that reaches every kernel the row dispatches to (tests/_tol_population.py; tests/test_tolerance_scenes_host.py proves the
reach on the CPU), and the one recorded frame of round 4's fuzz that left 1e-4 (tests/golden/tolerance_case_7376.json).

The radiance of this integrator is piecewise constant in path space: a frame of the row differs from the oracle's only where a
decision flips — which sphere is nearest, a threshold —, so a wrong root, tie or guard shows as whole samples, far above 1e-4, on
frames this small.  Per frame: the row ran (stats["variant"]), non-finite values sit where the oracle's do, every pixel is within
NORTH_STAR_TOL = 1e-4 of the oracle's, `casts` within the slack the row's other tests use (tests/test_tolerance_gpu.py: max(2, casts //
100000) under a cap of at most 8, 1e-4 casts + 8 at any other depth), and variant 0 of the same frame is the oracle's bit for bit, so
that a failure points at the row and not at the scene.  Every test prints how many pixels differ at all.

Measured on the MI355X: profiles/r16/tolerance_scenes.md."""
import time

import numpy as np
import pytest

import _tol_frames as F
import _tol_population as P

pytestmark = pytest.mark.gpu

TOL_VARIANT = F.TOL_VARIANT
NORTH_STAR_TOL = F.NORTH_STAR_TOL

# Cases of the population that go by the recorded frame's rule instead (at most 1 % of the pixels outside 1e-4): a path among small
# spheres that left the reference's after many bounces, found by replaying the frame through variants 0, 1 and 2 — {case: reason with
# the measured delta}.  At most 2 may ever stand here, and no frame of part one.
CHAOTIC = {}
assert len(CHAOTIC) <= 2


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _render(rtm, data, mode, mb, seed, variant):
    if mode == "repaired":
        return F.render(rtm, data, mb, seed, variant)
    out, st = rtm.Renderer(data, mode=mode, max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    return out["f64"].cpu().numpy(), st


def _oracle_frame(oracle, data, mode, mb, seed):
    if mode == "repaired":
        return F.oracle_frame(oracle, data, mb, seed)
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    return oracle.render(ost, oarr, n, oracle.make_options(mode=oracle.MODE_LITERAL, max_bounces=mb, seed=seed, row_begin=0,
                                                           row_end=data.height))


def _same_bits(a, b):
    """bit for bit; a NaN equals a NaN (its payload is not an IEEE result)"""
    return (F.bits(a) == F.bits(b)) | (np.isnan(a) & np.isnan(b))


def _measure(rtm, oracle, data, mode, mb, seed):
    """the frame through the oracle, variant 0 and variant 18: what the assertions below read"""
    ref, cnt = _oracle_frame(oracle, data, mode, mb, seed)
    img0, st0 = _render(rtm, data, mode, mb, seed, 0)
    img18, st18 = _render(rtm, data, mode, mb, seed, TOL_VARIANT)
    finite = np.isfinite(ref) & np.isfinite(img18)
    with np.errstate(invalid="ignore"):
        delta = np.where(finite, np.abs(img18 - ref), 0.0).max(axis=-1)
    return dict(ref=ref, cnt=cnt, img0=img0, st0=st0, img18=img18, st18=st18, pixels=ref.shape[0] * ref.shape[1],
                worst=float(delta.max()), outside=int((delta > NORTH_STAR_TOL).sum()),
                differing=int((~_same_bits(img18, ref)).any(axis=-1).sum()),
                same_holes=bool(np.array_equal(np.isfinite(img18), np.isfinite(ref))),
                exact0=bool(_same_bits(img0, ref).all()), exact0_counters={k: st0[k] for k in F.COUNTERS} == {k: cnt[k] for k in F.COUNTERS},
                slack=1e-4 * cnt["casts"] + 8 if P.any_depth(mb) else max(2, cnt["casts"] // 100000))


def _line(what, m):
    return (f"{what}: {m['differing']} of {m['pixels']} pixels differ at all, {m['outside']} outside 1e-4, max |delta| {m['worst']:.3e}; "
            f"casts {m['st18']['casts']} / variant 0 {m['st0']['casts']} / oracle {m['cnt']['casts']}")


def _faults(m, chaotic=False):
    """the assertions of a frame, as a list of what failed"""
    out = []
    if m["st18"]["variant"] != TOL_VARIANT:
        out.append(f"ran variant {m['st18']['variant']}")
    if not m["exact0"]:
        out.append("variant 0 is not the oracle's frame")
    if not m["same_holes"]:
        out.append("non-finite values in other places than the oracle's")
    if chaotic:
        if not m["exact0_counters"]:
            out.append("variant 0's counters are not the oracle's")
        if m["outside"] > m["pixels"] // 100:
            out.append(f"{m['outside']} pixels outside 1e-4, more than 1 % of {m['pixels']}")
        return out
    if not m["worst"] <= NORTH_STAR_TOL:
        out.append(f"max |delta| {m['worst']:.3e} > 1e-4")
    if not abs(m["st18"]["casts"] - m["cnt"]["casts"]) <= m["slack"]:
        out.append(f"casts {m['st18']['casts']} against {m['cnt']['casts']}, slack {m['slack']}")
    return out


# ---- part one: the edge scenes ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_frames(rtm):
    return P.edge_frames(rtm)


@pytest.mark.parametrize("group", P.EDGE_GROUPS)
def test_edge_scenes_through_the_tolerance_row(rtm, oracle, edge_frames, group):
    """EDGE_SCENES (45x27, S 3, SS 2, seed 17; repaired at caps 8, 3, 1, 0, literal at -1 and 2 — no repaired frame at unlimited depth:
    `albedo-above-one` never ends a path by roulette, the others hold small spheres in a large one), AXIS_ROOMS (56x40, S 4, SS 2, seed 23;
    repaired at 8, -1, 3, 12, literal at -1), the three near misses of the Cornell signature at 8 and -1 (none may take an axis kernel),
    the degenerate camera (all zeros, `casts` the oracle's exactly), twelve spheres of which eleven coincide (the row packs the sphere
    index into a root's low bits: the lowest index must still win — every one has another colour) and the 1x1x1 frame"""
    failed = []
    for what, data, mode, mb, seed, expect in edge_frames[group]:
        assert P.eligible(data), what
        if group == "near misses":
            assert not F.axis_signature_launch(rtm, data, P.SIG_CORNELL7), what
        m = _measure(rtm, oracle, data, mode, mb, seed)
        print(_line(what, m))
        faults = _faults(m)
        if expect == "zeros":
            if m["img18"].any() or m["ref"].any():
                faults.append("the frame is not all zeros")
            if m["st18"]["casts"] != m["cnt"]["casts"]:
                faults.append(f"casts {m['st18']['casts']} are not the oracle's {m['cnt']['casts']}")
        failed += [f"{what}: {f}" for f in faults]
    assert not failed, "\n" + "\n".join(failed)


# ---- part two: the seeded population ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def population(rtm):
    return P.population(rtm), P.families()


@pytest.mark.parametrize("k", range(P.CHUNKS))
def test_population_through_the_tolerance_row(rtm, oracle, population, k):
    """48 of the 384 seeded frames (tests/_tol_population.py: every family in every chunk), repaired mode, each with part one's
    assertions; printed: the frames outside 1e-4, the frames that differ at all, the chunk's wall time"""
    cases, families = population
    failed, outside, differing, split, t0 = [], [], [], 0, time.perf_counter()
    for i in P.chunk(k):
        data, mb, seed = cases[i]
        what = (f"case {i} ({families[i]}, class {P.cell(rtm, data, mb)[0]}, n {len(data.object)}, {data.width}x{data.height}, S {data.samples}, "
                f"SS {data.superSamples}, max_bounces {mb}, seed {seed})")
        m = _measure(rtm, oracle, data, "repaired", mb, seed)
        if m["differing"]:
            differing.append(i)
            print(_line(what, m))
        if m["outside"]:
            outside.append(i)
        split += m["st18"]["split"] > 1  # (rtm_stats.split: the launch's waves per split tile — the kSplit instantiations)
        failed += [f"{what}: {f}" for f in _faults(m, chaotic=i in CHAOTIC)]
    print(f"chunk {k}: {len(P.chunk(k))} frames in {time.perf_counter() - t0:.2f} s ({split} with the sample split), outside 1e-4: {outside}, "
          f"differing at all: {differing}")
    assert not failed, "\n" + "\n".join(failed)


# ---- part three: the recorded frame that leaves 1e-4 -----------------------------------------------------------------------------------
def test_recorded_fuzz_frame_7376(rtm, oracle):
    """profiles/r4/fuzz_parity.txt, seed 5201, case 7376: the shipped box with nine spheres of radius 0.3 to 1 inside, 25x41, S 4, SS 3,
    unlimited depth — the chaotic regime DESIGN.md §4 documents; round 4 saw 1.43e-4 on one pixel of 1 025.  Variant 0 is the oracle's
    frame and counters bit for bit; of the row's frame at most 1 % of the pixels lie outside 1e-4 (a condition: a broken kernel leaves
    most of them).  The delta itself is printed and not asserted: every change to the row's arithmetic moves it."""
    G = P.tolerance_case_generator()
    data = rtm.LoadData(G.FIXTURE).data
    r = G.RECORDED
    assert (len(data.object), data.width, data.height, data.samples, data.superSamples) == (r["n"], r["width"], r["height"], r["samples"],
                                                                                            r["superSamples"])
    m = _measure(rtm, oracle, data, r["mode"], r["max_bounces"], r["seed"])
    print(_line("fuzz seed 5201 case 7376", m))
    assert not _faults(m, chaotic=True), "; ".join(_faults(m, chaotic=True))
