"""tolerance_case_7376.json: the one frame of round 4's seeded fuzz that left 1e-4 in the tolerance row
(profiles/r4/fuzz_parity.txt, twelfth pass: seed 5201, case 7376), as a scene file in the loader's own schema.

    python tests/golden/make_tolerance_case.py          (rewrites the fixture; deterministic)

This replays the random stream of profiles/fuzz_parity.py — every draw of every case before 7376, in that script's order and
with its argument shapes, none of its renders — so it needs numpy and scenes/cornellBoxSetting.json and no device.  The case is
the shipped box with nine more spheres of radius 0.3 to 1.0 inside (16 in all), 25x41, S 4, SS 3, unlimited depth, render seed
433410301624; `generate()` returns the file's text and those parameters, tests/test_tolerance_scenes_host.py compares both with
what is committed."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tolerance_case_7376.json")
FUZZ_SEED, FUZZ_CASE = 5201, 7376
RECORDED = dict(n=16, width=25, height=41, samples=4, superSamples=3, max_bounces=-1, mode="repaired", seed=433410301624)

_N = [1, 2, 5, 7, 7, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 33, 64, 100, 254, 255, 256, 257, 400, 511, 512, 513, 1000, 2500]
_N_PLANES = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 24, 25, 40, 100, 254, 255, 256, 400, 1000]


def replay(seed0=FUZZ_SEED, stop=FUZZ_CASE):
    """The fuzz script's draws for cases 0 .. stop; returns case `stop`: its parameters and, for a closed box, the spheres it adds
    to the shipped one as (position, radius, colour)."""
    rng = np.random.default_rng(seed0)
    for case in range(stop + 1):
        n = int(rng.choice(_N))
        kind = case % 4
        planes, extra, family = False, [], "stress"
        if kind == 3:  # planes and spheres mixed, in a room
            family = "planes"
            n = int(rng.choice(_N_PLANES))
            for _ in range(n):
                rng.uniform(0.2, 0.9, 3)
                rng.uniform(-6, 6, 3)
                t = int(rng.integers(3))
                if t == 0:
                    rng.uniform(0.3, 2.0)
                elif t == 1:
                    rng.integers(3)
                    rng.uniform(1, 9)
                    planes = True
                else:
                    rng.uniform(-2, 2, 3)
                    rng.uniform(1, 9)
                    planes = True
            n += 1
        elif kind == 0 and n == 7 and case % 8 != 0:  # a seven-sphere room with the Cornell box's axis signature
            family = "axis room"
            rng.uniform(3, 12)
            rng.uniform(0.3, 1.0)
            rng.uniform(0.1, 0.5)
            for _ in range(6):
                rng.uniform(1, 4.5)
                rng.uniform(0.8, 1.2)
                rng.uniform(0.2, 0.9, 3)
            rng.uniform(-0.7, 0.7, 3)
            rng.uniform(-0.2, 0.2, 3)
            rng.uniform(0.8, 2.0)
        elif kind == 0:  # the shipped box's first spheres and small ones inside
            family = "closed box"
            for _ in range(max(1, min(n, 7)), n):
                pos = rng.uniform(-7, 7, 3)
                r = float(rng.uniform(0.3, 1.0))
                col = rng.uniform(0.2, 0.9, 3)
                extra.append(([float(v) for v in pos], r, [float(v) for v in col]))
        else:
            rng.integers(1 << 30)
        width, height = int(rng.integers(1, 90)), int(rng.integers(1, 60))
        samples, ss = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32])), int(rng.choice([1, 2, 3, 4]))
        mb = int(rng.choice([-1, -1, 0, 1, 2, 7, 8, 9, 15, 16, 17, 40, 200]))
        mode = "literal" if case % 5 == 4 else "repaired"
        seed = int(rng.integers(1 << 40))
        if n >= 1000:
            width, height = int(rng.integers(1, 40)), int(rng.integers(1, 24))
            samples, ss = int(rng.choice([1, 2, 3, 4])), int(rng.choice([1, 2]))
        rng.choice([0, 0, 0, 2, 9, 14, 3, 12])
        if planes:
            rng.choice([0, 0, 1, 2, 9]) if n < 256 else rng.choice([0, 0, 1, 17])
    tol = (not planes) and 1 <= n <= 24 and samples * ss ** 2 < 65536 and stop % 3 == 2 and not (stop % 11 == 5 and n >= 1)
    return dict(n=n, width=width, height=height, samples=samples, superSamples=ss, max_bounces=mb, mode=mode, seed=seed), \
        family, extra, tol


def _num(v):
    return format(float(v), ".17g")


def _vec(v):
    return "[" + ", ".join(_num(x) for x in v) + "]"


def generate():
    """(the fixture's text, the case's parameters)"""
    params, family, extra, tol = replay()
    assert family == "closed box" and tol, (family, tol)
    with open(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")) as f:
        box = json.load(f)
    cam = box["01 camera"]
    spheres = [(o["00 position"], o["01 size"], o["02 material"]["color"], o["02 material"]["emission"])
               for o in box["02 scene"]["00 object"] if "00 position" in o]
    assert len(spheres) == 7 and params["n"] == 7 + len(extra)
    spheres += [(pos, r, col, [0.0, 0.0, 0.0]) for pos, r, col in extra]
    lines = ["{", f'    "00 height": {params["height"]},', f'    "00 samples": {params["samples"]},',
             f'    "00 superSamples": {params["superSamples"]},', f'    "00 width": {params["width"]},',
             '    "01 camera": {', f'        "fov": {_num(cam["fov"])},', f'        "origin": {_vec(cam["origin"])},',
             f'        "target": {_vec(cam["target"])},', f'        "upVec": {_vec(cam["upVec"])}', "    },",
             '    "02 scene": {', '        "00 object": [']
    for k, (pos, r, col, em) in enumerate(spheres):
        lines += ["            {", f'                "00 position": {_vec(pos)},', f'                "01 size": {_num(r)},',
                  '                "02 material": {', f'                    "color": {_vec(col)},',
                  f'                    "emission": {_vec(em)}', "                }",
                  "            }" + ("," if k + 1 < len(spheres) else "")]
    lines += ["        ]", "    }", "}", ""]
    return "\n".join(lines), params


if __name__ == "__main__":
    text, params = generate()
    assert params == RECORDED, params
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("wrote", FIXTURE, params)
