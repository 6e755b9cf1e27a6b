"""Edge scenes for the feature buffers (tests/test_aov_literal.py), built call for call through the product's C ABI and in the literal
oracle (dual.Dual), each with a camera that looks at the case it is about; plus the eight reference arms and six random graphs.  Every
hand-built scene stays at or below 64 nodes.  Test infrastructure."""
import numpy as np

import orc
from dual import Dual, random_scene_pair

ASPECT = 1.5  # the 48 x 32 frame of the tests
UP = (0.0, 1.0, 0.0)


def back_of_a_light():
    """Seen from below: an xz_rect DiffuseLight as it is (its back: emitted() is 0, the normal looks down at the camera), beside it the
    same under a FlipFace (its front: the checker emit texture), below them a `()` rect, against a bright background and half a Lambertian wall."""
    d = Dual(11)
    emit = d.diffuse_light(d.checker(d.solid((4.0, 4.0, 4.0)), d.solid((1.0, 2.0, 0.5))))
    hs = [d.rect(1, -3.0, -0.3, -2.0, 2.0, 2.0, emit),
          d.flip_face(d.rect(1, 0.3, 3.0, -2.0, 2.0, 2.0, emit)),
          d.rect(0, -2.5, 2.5, -0.5, 1.6, -2.5, d.null_material()),
          d.rect(0, -9.0, 0.0, -9.0, 9.0, -6.0, d.lambertian(d.solid((0.4, 0.5, 0.6))))]
    return d.finish(d.bvh(hs), [], (0.5, 0.7, 1.0), ((0.0, -3.0, 6.0), (0.0, 2.5, -0.5), UP, 50.0, ASPECT, 0.0, 8.0, 0.0, 1.0))


HOLLOW = (-1.5, 0.0, -5.0)


def inside_glass():
    """The camera sits inside a Dielectric sphere of radius 2, 1.7 from its centre, and looks half along the chord: the camera rays
    that meet the surface beyond the critical angle (sin > 1 / 1.5; from this origin up to 0.85) are reflected totally and, in a
    sphere, for ever.  The others leave towards a hollow glass sphere (inner radius negative) and a noise-textured Lambertian wall."""
    d = Dual(12)
    glass = d.dielectric(1.5)
    hs = [d.sphere((0.0, 0.0, 0.0), 2.0, glass),
          d.sphere(HOLLOW, 1.5, glass),
          d.sphere(HOLLOW, -1.3, glass),
          d.rect(0, -30.0, 30.0, -30.0, 30.0, -9.0, d.lambertian(d.noise(2.0)))]
    return d.finish(d.bvh(hs), [], (0.6, 0.7, 0.9), ((0.0, 0.0, 1.7), (-3.0, 0.0, -1.3), UP, 80.0, ASPECT, 0.0, 5.0, 0.0, 1.0))


MEDIA_CAMERA, MEDIA_CAMERA_RADIUS = (0.0, 1.0, 8.0), 3.0


def media():
    """A ConstantMedium with a noise-textured Isotropic inside Translate(RotateY(box)), thin enough that a fifth of the samples
    that reach it pass through, half of it against the background, and a second, thinner medium in a sphere of radius 3 around the
    camera (the box is more than 5 away); a checker floor below."""
    d = Dual(13)
    boundary = d.translate(d.rotate_y(d.aabox((0.0, 0.0, 0.0), (2.0, 2.0, 2.0), d.dielectric(1.5)), 30.0), (-1.2, 0.0, -1.0))
    hs = [d.constant_medium(boundary, 0.8, d.noise(3.0)),
          d.constant_medium(d.sphere(MEDIA_CAMERA, MEDIA_CAMERA_RADIUS, d.dielectric(1.5)), 0.15, d.solid((0.9, 0.8, 0.7))),
          d.rect(1, -10.0, 10.0, -10.0, 10.0, 0.0, d.lambertian(d.checker(d.solid((0.9, 0.9, 0.9)), d.solid((0.2, 0.3, 0.1)))))]
    return d.finish(d.bvh(hs), [], (0.3, 0.5, 0.8), (MEDIA_CAMERA, (0.0, 1.0, 0.0), UP, 30.0, ASPECT, 0.0, 8.0, 0.0, 1.0))


def synthetic_image():
    """8 x 4 RGB, every texel different, made here (not the earth map)"""
    j, i = np.mgrid[0:4, 0:8]
    return np.stack([(37 * i + 11 * j + 20) % 256, (91 * j + 5 * i + 60) % 256, (23 * i * (j + 1) + 130) % 256], axis=-1).astype(np.uint8)


def moving_textured():
    """A moving sphere with an image texture over the horizon of a radius-1000 checker ground sphere; shutter 0 .. 1, aperture 0.3."""
    d = Dual(14)
    hs = [d.moving_sphere((0.0, 1.0, 0.0), (0.8, 1.3, 0.0), 0.0, 1.0, 1.0, d.lambertian(d.image(synthetic_image()))),
          d.sphere((0.0, -1000.0, 0.0), 1000.0, d.lambertian(d.checker(d.solid((0.9, 0.9, 0.9)), d.solid((0.2, 0.3, 0.1)))))]
    return d.finish(d.bvh(hs), [], (0.7, 0.8, 1.0), ((6.0, 0.6, 5.0), (0.3, 1.1, 0.0), UP, 30.0, ASPECT, 0.3, 8.0, 0.0, 1.0))


FUZZES = (0.0, 0.5, 1.0)


def three_wrappers():
    """Three Metal boxes of fuzz 0, exactly 0.5 and 1 over a Lambertian floor: max_fuzz = 0.5 follows the first two and stops on the
    third.  The product takes at most three wrappers above a primitive (RT_MAX_SCOPE_DEPTH), so the first and the third are
    Translate(RotateY(Translate(box))) and the second is Translate(RotateY(box)) in a BVH node under a FlipFace: three each."""
    d = Dual(15)
    boxes = []
    for k, fuzz in enumerate(FUZZES):
        m = d.metal((0.9 - 0.1 * k, 0.8, 0.6 + 0.1 * k), fuzz)
        if k == 1:
            box = d.translate(d.rotate_y(d.aabox((-0.7, 0.0, -0.7), (0.7, 1.8, 0.7), m), 45.0), (0.0, 0.0, 0.3))
            boxes.append(d.flip_face(d.bvh([box])))
        else:
            box = d.translate(d.aabox((0.0, 0.0, 0.0), (1.4, 1.8, 1.4), m), (-0.7, 0.0, -0.7))
            boxes.append(d.translate(d.rotate_y(box, 25.0 + 20.0 * k), (-2.2 + 2.2 * k, 0.0, 0.0)))
    hs = boxes + [d.rect(1, -8.0, 8.0, -8.0, 8.0, 0.0, d.lambertian(d.solid((0.5, 0.6, 0.4))))]
    return d.finish(d.bvh(hs), [], (0.6, 0.75, 0.95), ((0.0, 2.2, 7.0), (0.0, 0.8, 0.0), UP, 40.0, ASPECT, 0.0, 7.0, 0.0, 1.0))


def mirror_hall():
    """Two facing mirrors of fuzz 0 at x = -3 and x = 3 with a glass sphere between them, a Lambertian floor and back wall, open
    above and in front.  The camera stands inside and looks almost squarely at one mirror: at max_specular = 4 some chains are cut
    between the mirrors, some leave to the background and some end on the floor or the wall."""
    d = Dual(16)
    mirror = d.metal((0.9, 0.9, 0.9), 0.0)
    hs = [d.rect(2, 0.0, 4.0, -4.0, 4.0, -3.0, mirror),
          d.rect(2, 0.0, 4.0, -4.0, 4.0, 3.0, mirror),
          d.sphere((0.0, 1.5, 0.0), 1.0, d.dielectric(1.5)),
          d.rect(1, -3.0, 3.0, -4.0, 4.0, 0.0, d.lambertian(d.solid((0.7, 0.3, 0.2)))),
          d.rect(0, -3.0, 3.0, 0.0, 4.0, -4.0, d.lambertian(d.solid((0.2, 0.4, 0.7))))]
    return d.finish(d.bvh(hs), [], (0.5, 0.6, 0.8), ((2.5, 2.0, 3.5), (-3.0, 2.0, 2.5), UP, 60.0, ASPECT, 0.0, 5.0, 0.0, 1.0))


HAND_BUILT = {"back_of_a_light": back_of_a_light, "inside_glass": inside_glass, "media": media, "moving_textured": moving_textured,
              "three_wrappers": three_wrappers, "mirror_hall": mirror_hall}


def reference_arm(arm):
    rt = orc.rt()
    return rt.Scene.reference(arm, build_seed=1, aspect_ratio=ASPECT), orc.OracleScene(arm, build_seed=1, aspect_ratio=ASPECT)


def random_graph_seeds(n=6, first=2000, max_nodes=64):
    """the first n seeds from `first` on whose graph has at most max_nodes nodes"""
    seeds, seed = [], first
    while len(seeds) < n:
        if random_scene_pair(seed)[0].info()["n_nodes"] <= max_nodes:
            seeds.append(seed)
        seed += 1
    return seeds


_RANDOM = None


def names():
    return list(HAND_BUILT) + [f"arm{a}" for a in range(8)] + [f"random{k}" for k in range(6)]


_CACHE = {}


def scene_pair(name):
    """(product scene, oracle scene) of a name of names(); built once per process"""
    global _RANDOM
    if name not in _CACHE:
        if name in HAND_BUILT:
            _CACHE[name] = HAND_BUILT[name]()
        elif name.startswith("arm"):
            _CACHE[name] = reference_arm(int(name[3:]))
        else:
            _RANDOM = _RANDOM or random_graph_seeds()
            _CACHE[name] = random_scene_pair(_RANDOM[int(name[6:])])
    return _CACHE[name]
