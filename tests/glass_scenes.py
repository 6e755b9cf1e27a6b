"""Shared by test_glass_terms.py (CPU) and test_glass_terms_gpu.py: the scenes that pin the three parts of the glass and light bounces
(rt_core.h: RT_MAT_DERIVED, RT_NORMAL_SHARED, RT_LOBE_SHARED).  Every scene is named for what it holds."""
import lambert_scenes as L

# the switches, each alone at its other setting, and all three
OFF = {"A": "-DRT_MAT_DERIVED=0", "B": "-DRT_NORMAL_SHARED=0", "C": "-DRT_LOBE_SHARED=0"}
ALL_OFF = " ".join(OFF.values())


def only(part):
    """the options of a build with `part` alone"""
    return " ".join(v for k, v in OFF.items() if k != part)


def cornell(rt):
    """arm 5: one glass sphere (a scalar record in the static hit record), an XZ rect and that sphere as the light list"""
    return rt.Scene.reference(5, build_seed=1)


def random_scene(rt):
    """arm 0: glass, metal and Lambertian spheres on the stack-walk / pair-walk kernels; rendered as a crop (ARM0_TILE)"""
    return rt.Scene.reference(0, build_seed=1, aspect_ratio=1.5)


ARM0_FRAME = (48, 32)
ARM0_TILE = (8, 4, 32, 24)

# nested_and_aligned: the camera sits at z = 0 and looks down -z at a Lambertian XY wall in the plane z = WALL_K; the glass sphere
# ALIGNED has its centre in that plane and at the camera's height.  An XY rect in the light list has the trait-default lobe, the
# direction (1, 0, 0): a wall point that draws it sends a ray along +x whose z never changes, and where it meets ALIGNED the z
# component of p - c is an exact zero whenever the wall point's own z, (k / d.z) * d.z, rounded to k -- test_glass_terms.py checks
# that this is the common case.  NESTED: a sphere of ir 1 inside a sphere of ir 1.5 about one centre, for back faces and ratio 1.
WALL_K = -4.0
CAMERA = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 80.0)
ALIGNED = ((3.0, 0.0, WALL_K), 1.0)
NESTED = ((-1.0, -0.8, -2.5), 1.0, 0.6)


def nested_and_aligned(rt):
    s = rt.Scene(build_seed=1)
    lam = lambda rgb: s.lambertian(s.solid_color(rgb))
    emit = lambda v: s.diffuse_light(s.solid_color((v, v, v)))
    objs = [s.xy_rect(-3.0, 1.5, -2.0, 2.0, WALL_K, lam((0.7, 0.7, 0.7))), s.xz_rect(-3.0, 5.0, -5.0, 1.0, -2.0, lam((0.2, 0.6, 0.3))),
            s.sphere(NESTED[0], NESTED[1], s.dielectric(1.5)), s.sphere(NESTED[0], NESTED[2], s.dielectric(1.0)),
            s.sphere(ALIGNED[0], ALIGNED[1], s.dielectric(1.5))]
    lights = [lambda: s.xz_rect(-1.0, 1.0, -3.0, -1.0, 2.5, emit(7.0)), lambda: s.sphere((0.5, 1.5, -1.5), 0.3, emit(9.0)),
              lambda: s.xy_rect(-0.5, 0.5, 1.2, 1.8, -3.9, emit(5.0))]
    s.set_world(s.bvh_node(objs + [make() for make in lights]))
    s.set_lights([make() for make in lights])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera(CAMERA[0], CAMERA[1], (0, 1, 0), CAMERA[2], 1.0, 0.0, 1.0, 0.0, 1.0)
    s.commit()
    assert L.shape(s)[0] == [L.XZ, L.SPHERE, L.DEFAULT]
    return s


# the scenes that get a scene-specialised unit
SPECIALISED = (cornell, nested_and_aligned)
# width, height, chunk (0: the library's); 8 spp each.  8x4 with chunk 8 is 32 work items: half of the only wave has retired from the start
FRAMES = ((32, 32, 0), (8, 4, 8))
