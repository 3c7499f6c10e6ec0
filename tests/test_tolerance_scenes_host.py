"""The reference side of tests/test_tolerance_scenes_gpu.py, without a device: the seeded population (tests/_tol_population.py) is the same
in every process, every case is one the tolerance row serves, and it reaches every kernel the row dispatches to (csrc/rtm_kernels_tol.hip:
launch_n) — read from the host-only hooks rtm_debug_scene_facts, rtm_debug_wall_pairs and rtm_debug_axis_rows, the way the row's other
tests name the kernel a frame ran.  The oracle renders every frame of the three parts finite (the degenerate camera: black), and
the committed scene of fuzz case 7376 is what tests/golden/make_tolerance_case.py regenerates."""
import ctypes as C

import numpy as np
import pytest

import _tol_frames as F
import _tol_population as P


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


@pytest.fixture(scope="module")
def population(rtm):
    return P.population(rtm)


def _key(data, mb, seed):
    st, arr, n = data.to_c()
    return bytes(st), bytes(arr)[:n * C.sizeof(arr[0])], n, mb, seed


def test_population_is_deterministic_and_eligible(rtm, population):
    again = P.population(rtm)
    assert len(population) == len(again) == P.CASES == 384 and len(P.families()) == P.CASES
    assert [_key(*c) for c in population] == [_key(*c) for c in again]
    assert len({_key(*c) for c in population}) == P.CASES  # no frame twice
    for i, (data, mb, seed) in enumerate(population):
        assert P.eligible(data), i
        assert 1 <= data.width <= 70 and 1 <= data.height <= 50, i
        assert data.samples in (1, 2, 3, 4, 5, 8, 16, 32) and 1 <= data.superSamples <= 3, i
        assert all(c <= 0.9 for o in data.object for c in o.m_material.color), i
    # frame shapes: sides under 8 and sides that are no multiple of 8, samples per pixel on both sides of 16 (the stealing threshold)
    sides = [s for data, _, _ in population for s in (data.width, data.height)]
    spp = [data.samples * data.superSamples ** 2 for data, _, _ in population]
    assert sum(s < 8 for s in sides) >= 48 and sum(s % 8 != 0 for s in sides) >= 384 and sum(s % 8 == 0 for s in sides) >= 24
    assert sum(v < 16 for v in spp) >= 96 and sum(v >= 16 for v in spp) >= 96 and 16 in spp
    # every family in every chunk
    fam = P.families()
    for k in range(P.CHUNKS):
        assert {fam[i] for i in P.chunk(k)} == set(P.SLOTS), k


def test_population_reaches_every_kernel_of_the_row(rtm, population):
    """CELL_MINIMA: at least 8 cases per class and depth — conditions, not measurements (the classes: _tol_population.cell)"""
    counts = P.cell_counts(rtm, population)
    print("cells:", {f"{c} {d}": v for (c, d), v in sorted(counts.items())})
    for key, least in P.CELL_MINIMA.items():
        assert counts.get(key, 0) >= least, (key, counts.get(key, 0))
    by_n = {}
    for data, mb, _ in population:
        by_n.setdefault((len(data.object), "any" if P.any_depth(mb) else "capped"), []).append((data, mb))
    for depth in ("capped", "any"):
        for n in (8, 9, 15, 16, 17, 23, 24):  # the chunked kernel: a full chunk, one more, two less one, two, two more, three less one, three
            assert (n, depth) in by_n, (n, depth)
        for n in (3, 5, 7):                   # the exact-n kernels (capped) and the generic one: no signature
            assert sum(P.cell(rtm, d, mb)[0] == "f" for d, mb in by_n[(n, depth)]) >= 2, (n, depth)
        for n in (1, 2, 4, 6):
            assert len(by_n[(n, depth)]) >= 2, (n, depth)
        # class b is two kernels: the six walls with one K and no pairs (kAxisSigCornell7Walls), and the plain signature
        one_k = [P.walls_share_one_k(rtm, d) for d, mb in by_n[(7, depth)] if P.cell(rtm, d, mb)[0] == "b"]
        assert sum(one_k) >= 4 and len(one_k) - sum(one_k) >= 4, (depth, one_k)
    # class a is the hosts's grant AND the launch conditions; the shipped box is in it, as the row's own tests tie their frames to it
    shipped = [(d, mb) for d, mb in by_n[(7, "capped")] + by_n[(7, "any")] if F.through_the_pairs_kernels(rtm, d)]
    assert len(shipped) >= 2 and all(P.cell(rtm, d, mb)[0] == "a" for d, mb in shipped)
    # the axis kernels need the near-unit Normalize table in the launch (launch_n: unit_tab), in every shape of the row
    for n in (3, 5, 7):
        for deep in (0, 1):
            for split in (0, 1):
                out = (C.c_uint64 * 2)()
                rtm._lib.check(rtm.lib().rtm_debug_tol_lds_bytes(n, deep, split, 1, out), "tol lds bytes")
                assert int(out[1]) == 1, (n, deep, split)


def test_edge_scenes_are_what_the_row_serves(rtm):
    groups = P.edge_frames(rtm)
    assert sorted(groups) == sorted(P.EDGE_GROUPS)
    for frames in groups.values():
        for what, data, mode, mb, seed, expect in frames:
            assert P.eligible(data) and mode in ("repaired", "literal"), what
    # the rooms are axis-kernel scenes from where their cameras stand, the near misses are not
    for name in ("small-room", "negative-zeros"):
        assert P.cell(rtm, groups[name][0][1], 8)[0] == "b", name
    for what, data, *_ in groups["near misses"]:
        assert not F.axis_signature_launch(rtm, data, P.SIG_CORNELL7), what
    assert len(groups["coincident spheres"][0][1].object) == 12


def _oracle(oracle, data, mode, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    m = oracle.MODE_REPAIRED if mode == "repaired" else oracle.MODE_LITERAL
    return oracle.render(ost, oarr, n, oracle.make_options(mode=m, max_bounces=mb, seed=seed, row_begin=0, row_end=data.height))


def test_oracle_renders_every_frame_finite(rtm, oracle, population):
    lit, closed, hit, fam = 0, 0, 0, P.families()
    for frames in P.edge_frames(rtm).values():
        for what, data, mode, mb, seed, expect in frames:
            ref, cnt = _oracle(oracle, data, mode, mb, seed)
            assert np.isfinite(ref).all() and cnt["samples"] == data.width * data.height * data.samples * data.superSamples ** 2, what
            assert expect == "frame" or not ref.any(), what
    for i, (data, mb, seed) in enumerate(population):
        ref, cnt = F.oracle_frame(oracle, data, mb, seed)
        assert np.isfinite(ref).all(), i
        if fam[i] == "stress":  # (nearly empty by construction: tests/_tol_population.py's docstring)
            hit += cnt["casts"] > cnt["samples"]
        else:
            closed += 1
            lit += bool(ref.any())
    assert lit >= 0.9 * closed  # light arrives in nearly every frame of the closed families: a frame of zeros would test little
    assert hit >= 24            # ... and a third of the open ones at least bounce
    G = P.tolerance_case_generator()
    data = rtm.LoadData(G.FIXTURE).data
    ref, cnt = F.oracle_frame(oracle, data, G.RECORDED["max_bounces"], G.RECORDED["seed"])
    assert np.isfinite(ref).all() and cnt["casts"] == 186061  # profiles/r4/fuzz_parity.txt: the reference's casts of this frame


def test_committed_fuzz_case_is_what_the_generator_replays(rtm):
    G = P.tolerance_case_generator()
    text, params = G.generate()
    assert params == G.RECORDED
    with open(G.FIXTURE) as f:
        assert f.read() == text
    # ... and the loader reads it back as the scene the fuzz script built: the shipped box, then the nine spheres, value for value
    _, _, extra, _ = G.replay()
    data = rtm.LoadData(G.FIXTURE).data
    box = F.cornell(rtm, params["width"], params["height"], params["samples"], params["superSamples"])
    assert len(data.object) == 16 and len(extra) == 9
    assert (data.width, data.height, data.samples, data.superSamples) == (25, 41, 4, 3)
    want = rtm.SettingData(width=25, height=41, samples=4, superSamples=3, camera=box.camera,
                           object=list(box.object) + [rtm.SphereObject(rtm.vec3(*pos), r, rtm.Material(rtm.vec3(*col), rtm.vec3(0, 0, 0)))
                                                      for pos, r, col in extra])
    assert _key(data, -1, 0) == _key(want, -1, 0)
    assert all(0.3 <= r <= 1.0 for _, r, _ in extra)
