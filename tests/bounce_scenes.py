"""Shared by test_light_cone.py (CPU) and test_bounce_terms_gpu.py: the scenes that pin the sphere light's cone in the Lambertian
bounce (rt_core.h: RtSphereCone, rt_sphere_cone, RtLightShape::cone).  The part is built where a unit's light list holds exactly one
sphere; every scene is named for what it holds."""
import lambert_scenes as L


def _lam(s, rgb):
    return s.lambertian(s.solid_color(rgb))


def _emit(s, v):
    return s.diffuse_light(s.solid_color((v, v, v)))


def _corner(s):
    """lambert_scenes' room: a floor (XZ), a back wall (XY) and a side wall (YZ), Lambertian, outside any wrapper, open to the sky"""
    return [s.xz_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.7, 0.7, 0.7))), s.xy_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.2, 0.6, 0.3))),
            s.yz_rect(0.0, 4.0, 0.0, 4.0, 0.0, _lam(s, (0.7, 0.2, 0.2)))]


def _finish(s, objects, light_makers):
    """every light is built twice, once for the world and once for the light list, as main.rs does"""
    s.set_world(s.bvh_node(objects + [make() for make in light_makers]))
    s.set_lights([make() for make in light_makers])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera((2.0, 2.0, 7.5), (2.0, 1.5, 0.0), (0, 1, 0), 50.0, 1.0, 0.0, 6.0, 0.0, 1.0)
    s.commit()
    return s


def cornell(rt):
    """arm 5: the XZ rect and the glass sphere are the light list -- the unit the part was written for"""
    return rt.Scene.reference(5, build_seed=1)


def cornel_smoke(rt):
    """arm 6: the XZ rect alone, and media"""
    return rt.Scene.reference(6, build_seed=1)


def sphere_only(rt):
    """a corner of Lambertian rects, a Lambertian and a metal sphere, one sphere light and nothing else in the list"""
    return L.lights_one_sphere(rt)


def rect_only(rt):
    """the same room under an XZ rect light: no sphere in the list, the part is not built"""
    return L.sphere_beside_rects(rt, lights=("xz",))


def two_spheres(rt):
    """two sphere lights at different places: more than one cone per point, the part is not built"""
    s = rt.Scene(build_seed=1)
    objs = _corner(s) + [s.sphere((2.0, 0.8, 2.0), 0.8, _lam(s, (0.3, 0.4, 0.8)))]
    return _finish(s, objs, [lambda: s.sphere((3.2, 2.8, 2.6), 0.35, _emit(s, 9.0)), lambda: s.sphere((1.0, 3.0, 1.2), 0.35, _emit(s, 9.0))])


# inside_light: the light (centre, radius), the one ball of the world, the camera (from, at, vfov) -- test_light_cone.py checks from
# these that a floor point in plain view lies inside the light
INSIDE_LIGHT = ((1.2, 0.3, 1.2), 1.4)
INSIDE_BALL = ((3.0, 0.6, 2.5), 0.6)
INSIDE_CAMERA = ((2.0, 2.0, 7.5), (2.0, 1.5, 0.0), 50.0)


def inside_light(rt):
    """a sphere light that is in the light list only, not in the world, and reaches through the floor and the walls: the Lambertian
    points inside it have R * R / d2 > 1, the cone's cosine is the square root of a negative number, and the lobe, the pdf and the
    path's weight carry that NaN (the pixel sum drops such a sample, as the reference does: those pixels come out darker or 0)"""
    s = rt.Scene(build_seed=1)
    s.set_world(s.bvh_node(_corner(s) + [s.sphere(INSIDE_BALL[0], INSIDE_BALL[1], _lam(s, (0.3, 0.4, 0.8)))]))
    s.set_lights([s.sphere(INSIDE_LIGHT[0], INSIDE_LIGHT[1], _emit(s, 9.0))])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera(INSIDE_CAMERA[0], INSIDE_CAMERA[1], (0, 1, 0), INSIDE_CAMERA[2], 1.0, 0.0, 6.0, 0.0, 1.0)
    s.commit()
    return s


def radius_zero(rt):
    """a sphere light of radius 0: the cone's cosine is exactly 1, its solid angle 0"""
    s = rt.Scene(build_seed=1)
    objs = _corner(s) + [s.sphere((2.0, 0.8, 2.0), 0.8, _lam(s, (0.3, 0.4, 0.8)))]
    return _finish(s, objs, [lambda: s.sphere((3.2, 2.8, 2.6), 0.0, _emit(s, 9.0)), lambda: s.xz_rect(1.2, 2.6, 1.1, 2.4, 3.5, _emit(s, 7.0))])


SCENES = (cornell, cornel_smoke, sphere_only, rect_only, two_spheres, inside_light, radius_zero)
# does the unit hold exactly one sphere light (RtLightShape::cone with RT_LIGHT_CONE on)?
ELIGIBLE = {"cornell": True, "cornel_smoke": False, "sphere_only": True, "rect_only": False, "two_spheres": False, "inside_light": True, "radius_zero": True}
# width, height, chunk (0: the library's), max_depth; 8 spp each.  8x4 is 32 work items: half of the only wave has retired from the start
FRAMES = ((32, 32, 0, 50), (32, 32, 0, 3), (8, 4, 8, 50), (8, 4, 8, 3))


def eligible(sc):
    """what the generated unit itself declares: exactly one sphere in its light list"""
    return L.shape(sc)[0].count(L.SPHERE) == 1
