"""The scenes built to break a nearest-hit search or a shading block: tests/test_parity_gpu.py renders them with the bit-exact
variants, tests/test_tolerance_scenes_gpu.py with the tolerance row (variant 18).  Every entry takes the package and returns the
objects and the camera's numbers; nothing here touches a device."""


def _mk(rtm, pos, r, col, em):
    return rtm.SphereObject(rtm.vec3(*pos), r, rtm.Material(rtm.vec3(*col), rtm.vec3(*em)))


EDGE_SCENES = {
    # camera inside one sphere, a second one touching the camera ray tangentially
    "inside-and-tangent": lambda rtm: ([_mk(rtm, (0, 0, 0), 30, (.6, .7, .8), (.1, 0, 0)),
                                        _mk(rtm, (1, 0, 5), 1, (.9, .9, .1), (0, 2, 0))], (0, 0, -3), 1.0),
    # radius 0 and a sphere behind the camera
    "degenerate-radius": lambda rtm: ([_mk(rtm, (0, 0, 4), 0.0, (.5, .5, .5), (1, 1, 1)),
                                       _mk(rtm, (0, 0, -20), 5, (.5, .5, .5), (3, 3, 3)),
                                       _mk(rtm, (0, -102, 0), 100, (.8, .8, .8), (0, 0, 0))], (0, 0, -3), 1.5),
    # albedo above 1 (RR always passes: only the cap or a miss ends a path) and a negative colour
    "albedo-above-one": lambda rtm: ([_mk(rtm, (0, 0, 0), 12, (1.5, 1.2, 1.0), (0, 0, 0)),
                                      _mk(rtm, (0, 9, 0), 3, (-0.5, -0.2, -0.1), (4, 4, 4)),
                                      _mk(rtm, (3, -2, 1), 1.5, (0.2, 0.3, 0.4), (0, 0, .5))], (0, 0, -5), 1.2),
    # every sphere black (kd = 0, colorKD = 0/0 never used) and emissive
    "all-black": lambda rtm: ([_mk(rtm, (0, 0, 6), 2, (0, 0, 0), (.5, .25, .125)),
                               _mk(rtm, (-3, 1, 7), 2, (0, 0, 0), (0, 1, 0))], (0, 0, -3), 1.0),
    # thresholds of Intersect: origin a hair above a huge sphere (t1 inside [1e-5, 0.001])
    "grazing-thresholds": lambda rtm: ([_mk(rtm, (0, -1000.0005, 0), 1000, (.7, .7, .7), (0, 0, 0)),
                                        _mk(rtm, (0, 50, 0), 30, (0, 0, 0), (2, 2, 2))], (0, 0.0, -3), 1.0),
}


def _axis_room(rtm, light, walls, zero=0.0):
    """Seven spheres with the shipped Cornell box's AXIS SIGNATURE (light on y; walls on +x -x +y -y +z -z), other numbers."""
    ly, lr = light
    objs = [_mk(rtm, (zero, ly, zero), lr, (0, 0, 0), (4, 3.5, 3))]
    cols = [(.8, .3, .3), (.3, .8, .3), (.3, .3, .8), (.7, .7, .7), (.8, .3, .8), (.3, .8, .8)]
    for k, (c, r) in enumerate(walls):
        pos = [zero, zero, zero]
        pos[k // 2] = c
        objs.append(_mk(rtm, tuple(pos), r, cols[k], (0, 0, 0)))
    return objs


AXIS_ROOMS = {
    # a smaller room, walls of different radii, an off-axis camera: every shared product is a generic number
    "small-room": lambda rtm: (_axis_room(rtm, (6.0, 2.5), [(1005.5, 1000), (-806.25, 800), (507, 500), (-1204, 1200), (2008, 2000), (-307, 300)]),
                               (0.75, -1.25, -4.0)),
    # centres written with NEGATIVE zeros, the camera on the z axis (ox = oy = 0: the shared products are signed zeros)
    "negative-zeros": lambda rtm: (_axis_room(rtm, (9.0, 4.0), [(108, 100), (-108, 100), (108, 100), (-108, 100), (108, 100), (-108, 100)], zero=-0.0),
                                   (0.0, 0.0, -7.0)),
    # small spheres on the axes in open space (rays miss; some start inside the light)
    "open-space": lambda rtm: (_axis_room(rtm, (0.5, 3.0), [(4, 1.5), (-4, 1.0), (5, 2.0), (-3.5, 1.0), (6, 2.5), (-9, 0.5)]),
                               (0.0, 0.5, -2.0)),
}
