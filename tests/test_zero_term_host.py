"""Host side of the zero-term skip (csrc/rtm_kernels.hip: zero_term_flags_of; no device): kFoldZeroTermSkippable and the
per-object "emits" mask the deferred-fold kernels get, through rtm_debug_zero_term_facts, for the shipped scenes and for
near misses.  A path end on an object without a bit is neither queued nor folded nor stored, so the flag must only be proven
where that end's term is (+0, +0, +0) for certain."""
import ctypes as C
import os

from raytracingmin_amd import _lib

SCENES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes")
ALL = (1 << 64) - 1


def _facts(objs):
    from raytracingmin_amd import Camera, SettingData, vec3
    data = SettingData(width=8, height=8, samples=1, superSamples=1, camera=Camera(vec3(0, 0, -10), vec3(0, 0, 0), vec3(0, 1, 0), 2.0),
                       object=objs)
    _, arr, n = data.to_c()
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().rtm_debug_zero_term_facts(arr, n, out), "zero-term facts")
    return int(out[0]), int(out[1])


def _s(pos, col=(.5, .5, .5), em=(0, 0, 0)):
    from raytracingmin_amd import Material, SphereObject, vec3
    return SphereObject(vec3(*pos), 1.0, Material(vec3(*col), vec3(*em)))


def test_shipped_scenes():
    """Where rtm_debug_scene_facts proves bit 0 for a shipped scene, the skip is proven too and the mask has exactly the bits of
    the objects whose emission is not all zeros — none for the identity row (index n); elsewhere every bit is set.  The Cornell
    box: proven, one emitter (the light)."""
    import raytracingmin_amd as rtm
    for name in ("cornellBoxSetting.json", "simpleSetting1.json", "simpleSetting2.json", "settingData.json"):
        objs = list(rtm.LoadData(os.path.join(SCENES, name)).data.object)
        skippable, mask = _facts(objs)
        emits = [any(float(v) != 0.0 for v in o.m_material.emission) for o in objs]
        # the same rule restated: flag bit 0 of rtm_debug_scene_facts, finite colours, at most 63 objects
        out = (C.c_uint64 * 2)()
        from raytracingmin_amd import Camera, SettingData, vec3
        d = SettingData(width=8, height=8, samples=1, superSamples=1, camera=Camera(vec3(0, 0, -10), vec3(0, 0, 0), vec3(0, 1, 0), 2.0), object=objs)
        _, arr, n = d.to_c()
        _lib.check(_lib.lib().rtm_debug_scene_facts(arr, n, out), "scene facts")
        if int(out[1]) & 1:
            assert skippable == 1, name
            assert mask == sum(1 << i for i, e in enumerate(emits) if e), name
            assert (mask >> len(objs)) == 0, name
        else:
            assert (skippable, mask) == (0, ALL), name
    box = list(rtm.LoadData(os.path.join(SCENES, "cornellBoxSetting.json")).data.object)
    skippable, mask = _facts(box)
    assert skippable == 1 and bin(mask).count("1") == 1  # only the light emits


def test_near_misses_keep_every_path_end():
    light = _s((0, 9, 0), col=(0, 0, 0), em=(5, 5, 5))
    inf, nan = float("inf"), float("nan")
    assert _facts([light, _s((1, 0, 0))]) == (1, 1)
    assert _facts([_s((1, 0, 0)), light, _s((3, 0, 0))]) == (1, 2)
    assert _facts([light, _s((1, 0, 0), em=(0, 0.1, 0))]) == (0, ALL)      # a diffuse emitter
    assert _facts([light, _s((1, 0, 0), col=(.5, -0.0, .5))]) == (0, ALL)  # a -0 colour
    assert _facts([light, _s((1, 0, 0), col=(.5, -.2, .5))]) == (0, ALL)   # a negative colour
    assert _facts([light, _s((1, 0, 0), col=(.5, inf, .5))]) == (0, ALL)   # an inf colour: 0 x inf
    assert _facts([light, _s((1, 0, 0), col=(.5, nan, .5))]) == (0, ALL)
    assert _facts([light, _s((1, 0, 0), em=(0, -0.0, 0))]) == (0, ALL)     # a -0 emission
    assert _facts([_s((0, 9, 0), col=(.2, 0, 0), em=(5, 5, 5)), _s((1, 0, 0))]) == (0, ALL)  # a light with kd > 0: it is bounced off
    # an emitter nothing bounces off may have any finite or infinite colour: it is never a level of a fold
    assert _facts([light, _s((0, -9, 0), col=(0, 0, 0), em=(0, 0, 1e-300)), _s((1, 0, 0))]) == (1, 3)
    # a lightless scene: provable, nothing emits; the empty scene too
    assert _facts([_s((1, 0, 0)), _s((3, 0, 0))]) == (1, 0)
    assert _facts([]) == (1, 0)
    # the mask has 64 bits and the identity row needs none of them: 63 objects at most
    assert _facts([light] + [_s((float(i), 0, 0)) for i in range(62)]) == (1, 1)
    assert _facts([light] + [_s((float(i), 0, 0)) for i in range(63)]) == (0, ALL)
