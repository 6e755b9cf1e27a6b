"""Shared by test_lambert_static.py (CPU) and test_lambert_static_gpu.py: what a scene's generated kernel unit (Scene.kernel_source:
the library's own text) says about its light list and about where its Lambertian materials sit (Topo::n_lights, light_kind,
lambert_general, lambert_xy / _xz / _yz; rt_core.h: RtLightShape, RtLambertWalls), and small hand-built scenes, each named for
the branch of the Lambertian shading it pins."""
import re

XY, XZ, YZ, SPHERE, DEFAULT = 4, 5, 6, 2, 11
LEAF_FLIPPED = 0x100
NEW_MEMBERS = ("n_lights", "light_kind", "lambert_general")


def shape(sc):
    """(kind words of the light list, lambert_general, (lambert_xy, lambert_xz, lambert_yz)) as the generated unit declares them"""
    src = sc.kernel_source()
    n = int(re.search(r"n_lights = (\d+)u;", src).group(1))
    m = re.search(r"light_kind\[(\d+)\] = \{([^}]*)\};", src)
    kinds = [int(x) for x in re.findall(r"\d+", m.group(2))]
    assert int(m.group(1)) == len(kinds) == max(n, 1)
    w = re.search(r"lambert_general = (\w+), lambert_xy = (\w+), lambert_xz = (\w+), lambert_yz = (\w+);", src)
    flags = [x == "true" for x in w.groups()]
    return kinds[:n], flags[0], tuple(flags[1:])


def strip_new_members(topo):
    """a Topo as the library generated it before it knew lights and walls: the lines of the new members taken out"""
    lines = [ln for ln in topo.splitlines(keepends=True) if not any(("constexpr uint32_t " + m) in ln or ("constexpr bool " + m) in ln for m in NEW_MEMBERS)]
    out = "".join(lines)
    assert all(m not in out for m in NEW_MEMBERS) and "reuse[" in out
    return out


def _finish(s, objects, light_makers, look_from=(2.0, 2.0, 7.5), look_at=(2.0, 1.5, 0.0), vfov=50.0, background=(0.5, 0.7, 1.0)):
    """`light_makers`: one callable per light; each is built twice, once for the world and once for the light list, as main.rs does"""
    s.set_world(s.bvh_node(objects + [make() for make in light_makers]))
    s.set_lights([make() for make in light_makers])
    s.set_background(background)
    s.set_camera(look_from, look_at, (0, 1, 0), vfov, 1.0, 0.0, 6.0, 0.0, 1.0)
    s.commit()
    return s


def _lam(s, rgb):
    return s.lambertian(s.solid_color(rgb))


def _emit(s, v=7.0):
    return s.diffuse_light(s.solid_color((v, v, v)))


def _corner(s):
    """a floor (XZ), a back wall (XY) and a side wall (YZ), all Lambertian and outside any wrapper, open to the sky"""
    return [s.xz_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.7, 0.7, 0.7))), s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.2, 0.6, 0.3))),
            s.yz_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.7, 0.2, 0.2)))]


def _xz_light(s, y=3.5):
    return s.xz_rect(1.2, 2.6, 1.1, 2.4, y, _emit(s))


def _sphere_light(s, c=(3.2, 2.8, 2.6)):
    return s.sphere(c, 0.35, _emit(s, 9.0))


def six_frames(rt):
    """a closed room of six Lambertian rects around the camera, lit by an XZ rect light below the ceiling: every wall is seen from
    inside, so the two YZ walls give the normals +x and -x, the XZ pair +y and -y, the XY pair +z and -z -- all six frames"""
    s = rt.Scene(build_seed=1)
    g, r, b = _lam(s, (0.7, 0.7, 0.7)), _lam(s, (0.7, 0.2, 0.2)), _lam(s, (0.2, 0.3, 0.7))
    walls = [s.yz_rect(0.0, 4.0, 0.0, 4.0, 0.0, r), s.yz_rect(0.0, 4.0, 0.0, 4.0, 4.0, b), s.xz_rect(0.0, 4.0, 0.0, 4.0, 0.0, g),
             s.xz_rect(0.0, 4.0, 0.0, 4.0, 4.0, g), s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, g), s.xy_rect(0.0, 4.0, 0.0, 4.0, 4.0, g)]
    return _finish(s, walls, [lambda: _xz_light(s, 3.9)], look_from=(2.0, 2.0, 3.8), look_at=(2.0, 1.8, 0.0), vfov=80.0, background=(0.0, 0.0, 0.0))


def sphere_beside_rects(rt, lights=("xz",)):
    """a Lambertian sphere in a corner of Lambertian rects: lanes of one wave take the constant frames and the computed one.
    `lights`: the light list, in order, of "xz" (XZ rect), "sphere" and "xy" (an XY rect: the trait-default pdf and lobe)"""
    s = rt.Scene(build_seed=1)
    objs = _corner(s) + [s.sphere((2.0, 0.8, 2.0), 0.8, _lam(s, (0.3, 0.4, 0.8))), s.sphere((0.9, 0.5, 3.0), 0.5, s.metal((0.8, 0.8, 0.8), 0.05))]
    makers = {"xz": lambda k: s.xz_rect(1.2 - 0.3 * k, 2.6 - 0.3 * k, 1.1, 2.4, 3.5 + 0.25 * k, _emit(s)), "sphere": lambda k: _sphere_light(s),
              "xy": lambda k: s.xy_rect(2.8, 3.8, 2.6, 3.6, 0.05, _emit(s))}
    return _finish(s, objs, [lambda k=k, what=what: makers[what](k) for k, what in enumerate(lights)])


def walls_without_lights(rt):
    return sphere_beside_rects(rt, lights=())


def lights_one_sphere(rt):
    return sphere_beside_rects(rt, lights=("sphere",))


def lights_rect_and_sphere(rt):
    return sphere_beside_rects(rt, lights=("xz", "sphere"))


def lights_three(rt):
    """two XZ rect lights and a sphere: the record of a chosen XZ light is read by its drawn index, the sphere's by a constant"""
    return sphere_beside_rects(rt, lights=("xz", "sphere", "xz"))


def lights_default_xy(rt):
    """an XY rect in the light list: pdf_value 0 and the lobe (1, 0, 0) of the trait defaults"""
    return sphere_beside_rects(rt, lights=("xy",))


def rect_under_translate(rt):
    """a Lambertian XY rect below a Translate next to plain ones: its hit has a scope and takes the computed frame"""
    s = rt.Scene(build_seed=1)
    moved = s.translate(s.xy_rect(0.0, 1.5, 0.0, 1.5, 0.0, _lam(s, (0.8, 0.7, 0.2))), (1.5, 0.0, 1.5))
    return _finish(s, _corner(s) + [moved], [lambda: _xz_light(s)])


def rect_under_rotate_y(rt):
    """a Lambertian YZ rect below a RotateY: its world normal is no axis vector"""
    s = rt.Scene(build_seed=1)
    turned = s.translate(s.rotate_y(s.yz_rect(0.0, 1.8, -0.9, 0.9, 0.0, _lam(s, (0.8, 0.7, 0.2))), 33.0), (2.2, 0.0, 2.0))
    return _finish(s, _corner(s) + [turned], [lambda: _xz_light(s)])


def rect_under_flip(rt):
    """a Lambertian XZ floor wrapped directly by a FlipFace: the flattener folds the wrapper into the leaf, which stays a plain rect"""
    s = rt.Scene(build_seed=1)
    floor = s.flip_face(s.xz_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.7, 0.7, 0.7))))
    objs = [floor, s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.2, 0.6, 0.3))), s.sphere((2.0, 0.8, 2.0), 0.8, s.metal((0.8, 0.8, 0.8), 0.0))]
    return _finish(s, objs, [lambda: _xz_light(s)])


def checker_rect(rt):
    """a Lambertian floor with a checker texture (a textured albedo is a Lambertian material all the same)"""
    s = rt.Scene(build_seed=1)
    floor = s.xz_rect(0.0, 4.0, 0.0, 4.0, 0.0, s.lambertian(s.checker_texture(s.solid_color((0.2, 0.3, 0.1)), s.solid_color((0.9, 0.9, 0.9)))))
    objs = [floor, s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.2, 0.6, 0.3))), s.sphere((2.0, 0.8, 2.0), 0.8, s.dielectric(1.5))]
    return _finish(s, objs, [lambda: _xz_light(s)])


HAND_BUILT = (six_frames, sphere_beside_rects, walls_without_lights, rect_under_translate, rect_under_rotate_y, rect_under_flip, checker_rect,
              lights_one_sphere, lights_rect_and_sphere, lights_three, lights_default_xy)

# what each hand-built scene's unit must declare: (light kinds, lambert_general, (xy, xz, yz))
EXPECTED_SHAPE = {
    "six_frames": ([XZ], False, (True, True, True)),
    "sphere_beside_rects": ([XZ], True, (True, True, True)),
    "walls_without_lights": ([], True, (True, True, True)),
    "rect_under_translate": ([XZ], True, (True, True, True)),
    "rect_under_rotate_y": ([XZ], True, (True, True, True)),
    "rect_under_flip": ([XZ], False, (True, True, False)),
    "checker_rect": ([XZ], False, (True, True, False)),
    "lights_one_sphere": ([SPHERE], True, (True, True, True)),
    "lights_rect_and_sphere": ([XZ, SPHERE], True, (True, True, True)),
    "lights_three": ([XZ, SPHERE, XZ], True, (True, True, True)),
    "lights_default_xy": ([DEFAULT], True, (True, True, True)),
}
