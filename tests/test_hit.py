"""Ray queries (rt1w_hit, rt1w_hit_device, include/rt1w.h; csrc/rt_hit.h, csrc/hit.hip): Hittable::hit for a list of the caller's rays.

CPU tier: the CPU twin (librt1w_lab.so: rt1w_lab_hit_host, the same rt_hit.h built for the host) against the literal oracle's feature
buffers on the oracle's own camera rays, against the reference's formulas restated in numpy (tests/hit_reference.py), the media draw
computed from the Philox stream, the split rule, the refusals of tests/golden/hit_refusals.json, and a stand-alone sanitizer build
(tests/hit_driver.cpp) on the adversarial ray set.  GPU tier: the kernels bit for bit against the twin, the device entry between guard
bands, the literal oracle directly, and the diagnostics library's trace.

Bounds.  Against the oracle and the closed forms: t, t * |d| and p 1e-12 relative, normal, u, v 1e-12 absolute -- the project's bound
for product against literal (test_aov_literal.py); hit, front_face and the material id equal.  Kernel against twin, split calls against
one call, driver against twin: bit for bit (a NaN, which only rays of huge magnitude produce, equals a NaN: the host's and the GPU's
default NaN differ in the sign bit).

p against origin + t * direction: the record's p is ray.at(t) (ray.rs:12-14) in the leaf's own ray space, moved back by the wrappers
above the leaf (hittable.rs:215-225, :255-278).  For a leaf under no Translate / RotateY (its record's `b` chain holds none) that is
origin + t * direction in the world, and the test asks for those bits; under such a wrapper the reference itself returns
(origin - offset + t * direction) + offset, which is not the same bits, and the test asks for 1e-12 of the scene's extent."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_scenes
import hit_reference as HR
import orc

ROOT = orc.ROOT
REFUSALS = json.load(open(os.path.join(ROOT, "tests", "golden", "hit_refusals.json")))
INF = float("inf")
RTOL = 1e-12
W, H = 24, 16
SEEDS = [(0, 0), (7, 2)]  # (sample_offset, global_seed)
ORACLE_SCENES = [f"arm{a}" for a in range(6)] + ["back_of_a_light", "inside_glass", "moving_textured", "three_wrappers", "mirror_hall"]
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)  # a lone lane, a partial wave, a partial workgroup, a staging tail


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert np.all(err <= RTOL * np.maximum(1.0, np.abs(want))), (what, float(err.max()))


# ------------------------------------------------------------------------------------------------ 1, 8: the literal oracle --

_ORACLE = {}


def _oracle(name, so, gs):
    if (name, so, gs) not in _ORACLE:
        _ORACLE[(name, so, gs)] = aov_scenes.scene_pair(name)[1].aov(W, H, 1, sample_offset=so, global_seed=gs)[0]
    return _ORACLE[(name, so, gs)]


def _wrapped(nodes, node):
    """per ray: a Translate or RotateY is above the hit leaf (the chain of `b` from the leaf's record up)"""
    kind, up = nodes["kind"] & 0xFF, nodes["b"]
    out = np.zeros(len(node), dtype=bool)
    for i, n in enumerate(node):
        s = up[n] if n != HR.NO_NODE else HR.NO_NODE
        while s != HR.NO_NODE:
            out[i] |= kind[s] in (HR.TRANSLATE, HR.ROTATE_Y)
            s = up[s]
    return out


def _against_oracle(name, rays, rec, node, so, gs, what):
    """records of the frame's camera rays against the oracle's first-hit buffers of the same frame at 1 spp, every ray"""
    prod = aov_scenes.scene_pair(name)[0]
    want = _oracle(name, so, gs).reshape(-1, 8)
    hit = rec[:, 0] == 1.0
    assert np.array_equal(rec[:, 0], want[:, 7]), (what, "hit against coverage")
    assert np.array_equal(node == HR.NO_NODE, ~hit) and np.all(rec[~hit] == 0.0), (what, "a miss is zeros and no node")
    o, d, t = rays[:, 0:3], rays[:, 3:6], rec[:, 1]
    dist = t * np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    rel = np.abs(dist[hit] - want[hit, 6]) / want[hit, 6]
    assert rel.size == 0 or rel.max() <= RTOL, (what, "t * |d| against depth", float(rel.max()))
    dn = np.abs(rec[hit, 5:8] - want[hit, 3:6])
    assert dn.size == 0 or dn.max() <= RTOL, (what, "normal", float(dn.max()))
    at = o + t[:, None] * d  # rt_at's order: the product, then the sum
    nodes = HR.nodes_of(prod)
    wrapped = _wrapped(nodes, node)
    plain = hit & ~wrapped
    assert HR.same_bits(rec[plain, 2:5], at[plain]), (what, "p is origin + t * direction, bit for bit")
    extent = max(1.0, float(np.abs(at[hit]).max())) if hit.any() else 1.0
    assert np.all(np.abs(rec[hit & wrapped, 2:5] - at[hit & wrapped]) <= RTOL * extent), (what, "p under a wrapper")
    leaf = nodes["kind"][node[hit]] & 0xFF
    assert np.all((leaf >= HR.SPHERE) & (leaf <= HR.YZ)), (what, "the node is a leaf's record")
    assert np.array_equal(rec[hit, 11], (nodes["mat"][node[hit]] & 0xFFFF).astype(np.float64)), (what, "material id")
    return int(hit.sum()), int((hit & wrapped).sum())


@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_twin_against_the_literal_oracle(rt, name):
    """The twin's records of the camera rays of a 24 x 16 frame at 1 spp against the oracle's coverage, depth and normal of that frame,
    which the oracle makes from camera rays of its own: a wrong ray from rt1w_lab_camera_rays_host fails here.  Two (sample_offset,
    global_seed) pairs, every variant that covers the scene."""
    prod = aov_scenes.scene_pair(name)[0]
    for so, gs in SEEDS:
        rays = HR.camera_rays(rt, prod, W, H, 1, so, gs)
        for v in HR.valid_variants(prod.info()):
            rec, node = rt.hit_host(prod, rays, variant=v)
            hits, wrapped = _against_oracle(name, rays, rec, node, so, gs, (name, so, gs, v))
        print(name, (so, gs), "hits", hits, "of", len(rays), "under a Translate / RotateY", wrapped)
        assert hits > 0


# ------------------------------------------------------------------------------------------------ 2: closed forms --

CAM = ((0.0, 0.0, -10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0, 0.0, 1.0)


def _scene(rt, build):
    """a committed scene of the hittables build(scene) returns, under one BVH node"""
    s = rt.Scene(build_seed=1)
    s.set_world(s.bvh_node(build(s)))
    s.set_lights([])
    s.set_background((0.1, 0.2, 0.3))
    s.set_camera(*CAM)
    s.commit()
    return s


def _ray(o, d, t_min=0.001, t_max=INF, time=0.0):
    return [*o, *d, time, t_min, t_max]


def _check(rt, scene, rays, want, what, mats=None, uv=True):
    """the twin's records, in every variant that covers the scene, against the closed forms `want` (None = a miss)"""
    rays = np.array(rays, dtype=np.float64)
    for v in HR.valid_variants(scene.info()):
        rec, node = rt.hit_host(scene, rays, variant=v)
        for k, w in enumerate(want):
            tag = (what, "variant", v, "ray", k)
            if w is None:
                assert np.all(rec[k] == 0.0) and node[k] == HR.NO_NODE, tag
                continue
            assert rec[k, 0] == 1.0 and node[k] != HR.NO_NODE, tag
            _close(rec[k, 1], w["t"], tag + ("t",))
            _close(rec[k, 2:5], w["p"], tag + ("p",))
            _close(rec[k, 5:8], w["n"], tag + ("normal",))
            assert rec[k, 10] == (1.0 if w["front"] else 0.0), tag + ("front_face",)
            if uv:
                _close(rec[k, 8:10], [w["u"], w["v"]], tag + ("u, v",))
            else:
                assert rec[k, 8] == 0.0 and rec[k, 9] == 0.0, tag + ("u, v of a material whose texture reads neither",)
            if mats is not None:
                assert rec[k, 11] == float(mats[k]), tag + ("material id",)
    return rec, node


def _image_lambertian(s):
    """a material whose texture reads u, v: the kernels compute them for it (include/rt1w.h: slots 8, 9)"""
    return s.lambertian(s.image_texture(aov_scenes.synthetic_image()))


def test_sphere_from_outside_inside_and_the_window(rt):
    """sphere.rs:31-62 on a unit sphere at the origin: both roots exact (2 and 4 from z = -3), an unnormalised direction (t halves), the
    second root from inside with front_face 0, and the window -- a root equal to a bound is inside it (`root < t_min || t_max < root`),
    one ulp beyond it is not."""
    ids = {}

    def build(s):
        ids["m"] = _image_lambertian(s)
        return [s.sphere((0.0, 0.0, 0.0), 1.0, ids["m"])]
    sc = _scene(rt, build)
    o, d = (0.0, 0.0, -3.0), (0.0, 0.0, 1.0)
    cases = [(o, d, 0.001, INF), (o, (0.0, 0.0, 2.0), 0.001, INF), ((0.0, 0.0, 0.0), d, 0.001, INF), ((0.3, -0.2, -3.0), (0.01, 0.02, 1.1), 0.001, INF),
             (o, d, 5.0, 1.0), ((0.0, 2.0, -3.0), d, 0.001, INF)]
    # the window, off the axis: the roots r1 < r2 lie inside the sphere's box (entered at t = 2, left at t = 4), so the box test of the
    # BVH node above the sphere (aabb.rs:13-32: `t_max <= t_min` fails) decides nothing and sphere.rs's comparisons show
    o2 = (0.5, 0.0, -3.0)
    r1 = HR.sphere_hit((0.0, 0.0, 0.0), 1.0, o2, d, 0.001, INF)["t"]
    r2 = HR.sphere_hit((0.0, 0.0, 0.0), 1.0, o2, d, 3.0, INF)["t"]
    assert 2.0 < r1 < 3.0 < r2 < 4.0
    cases += [(o2, d, r1, INF), (o2, d, np.nextafter(r1, 3.0), INF), (o2, d, 0.001, r1), (o2, d, 0.001, np.nextafter(r1, 0.0)),
              (o2, d, 2.5, r2), (o2, d, 2.5, np.nextafter(r2, 0.0))]
    want = [HR.sphere_hit((0.0, 0.0, 0.0), 1.0, *c) for c in cases]
    assert [w and w["t"] for w in want] == [2.0, 1.0, 1.0, want[3]["t"], None, None, r1, r2, r1, None, r2, None]
    assert want[2]["front"] is False and want[2]["n"] == [0.0, 0.0, -1.0] and want[7]["front"] is False
    # on the axis the first root is where the ray enters the box: with t_max = 2 the sphere alone would answer 2 (`t_max < root` is false),
    # the world does not -- its BVH node's box test ends with t_max <= t_min (aabb.rs:27-29), and world.hit is what the entry states
    cases.append((o, d, 0.001, 2.0))
    want.append(None)
    _check(rt, sc, [_ray(c[0], c[1], c[2], c[3]) for c in cases], want, "sphere", mats=[ids["m"]] * len(cases))


def test_rects_with_u_v_flip_face_and_the_window(rt):
    """aarect.rs:46-72, :96-109, :164-177: each rect kind with its u, v (an image-textured material), the same rects with a solid colour
    (u = v = 0: no texture reads them), the window (`t < t_min || t > t_max`), an edge of the rect (inside: `<`, `>`), and FlipFace
    (hittable.rs:287-292): the flag flips, the normal does not."""
    ids = {}

    def build(s):
        ids["img"], ids["solid"] = _image_lambertian(s), s.lambertian(s.solid_color((0.5, 0.5, 0.5)))
        return [s.xy_rect(-1.0, 3.0, 0.0, 2.0, -2.0, ids["img"]), s.xz_rect(10.0, 12.0, -1.0, 1.0, 5.0, ids["img"]),
                s.yz_rect(-1.0, 1.0, 20.0, 24.0, -7.0, ids["img"]), s.flip_face(s.xz_rect(30.0, 32.0, -1.0, 1.0, 5.0, ids["img"])),
                s.xy_rect(40.0, 44.0, 0.0, 2.0, -2.0, ids["solid"])]
    sc = _scene(rt, build)
    xy, xz, yz = (0, -1.0, 3.0, 0.0, 2.0, -2.0), (1, 10.0, 12.0, -1.0, 1.0, 5.0), (2, -1.0, 1.0, 20.0, 24.0, -7.0)
    flipped = (1, 30.0, 32.0, -1.0, 1.0, 5.0)
    cases = [(xy, (0.5, 0.5, 1.0), (0.0, 0.0, -1.5), 0.001, INF), (xy, (0.5, 0.5, -4.0), (0.1, 0.05, 0.5), 0.001, INF),
             (xz, (11.25, 9.0, 0.5), (0.0, -2.0, 0.0), 0.001, INF), (yz, (-9.0, 0.25, 21.0), (4.0, 0.0, 0.5), 0.001, INF),
             (xy, (0.5, 0.5, 1.0), (0.0, 0.0, -1.5), 2.0, INF), (xy, (0.5, 0.5, 1.0), (0.0, 0.0, -1.5), np.nextafter(2.0, 3.0), INF),
             (xy, (0.5, 0.5, 1.0), (0.0, 0.0, -1.5), 0.001, 2.0), (xy, (0.5, 0.5, 1.0), (0.0, 0.0, -1.5), 0.001, np.nextafter(2.0, 1.0)),
             (xy, (3.0, 2.0, 1.0), (0.0, 0.0, -1.0), 0.001, INF), (xy, (np.nextafter(3.0, 4.0), 2.0, 1.0), (0.0, 0.0, -1.0), 0.001, INF)]
    want = [HR.rect_hit(*c[0], c[1], c[2], c[3], c[4]) for c in cases]
    assert [w and w["t"] for w in want][4:] == [2.0, None, 2.0, None, 3.0, None] and want[0]["u"] == 0.375 and want[0]["v"] == 0.25
    assert want[1]["front"] is False and want[1]["n"] == [0.0, 0.0, -1.0]
    rays = [_ray(c[1], c[2], c[3], c[4]) for c in cases]
    _check(rt, sc, rays, want, "rects", mats=[ids["img"]] * len(cases))
    for o, d in (((31.0, 9.0, 0.0), (0.0, -1.0, 0.0)), ((31.0, 1.0, 0.0), (0.0, 1.0, 0.0))):  # from above, from below
        plain = HR.rect_hit(*flipped, o, d, 0.001, INF)
        want = HR.flip_hit(lambda *a: HR.rect_hit(*flipped, *a), o, d, 0.001, INF)
        assert want["front"] is not plain["front"] and want["n"] == plain["n"]
        _check(rt, sc, [_ray(o, d)], [want], "FlipFace")
    o, d = (41.0, 0.5, 1.0), (0.0, 0.0, -1.5)
    _check(rt, sc, [_ray(o, d)], [HR.rect_hit(0, 40.0, 44.0, 0.0, 2.0, -2.0, o, d, 0.001, INF)], "solid rect", mats=[ids["solid"]], uv=False)


def test_box_under_translate_rotate_y(rt):
    """A box under Translate(RotateY(.)) (the Cornell boxes' shape): the ray goes in by hittable.rs:207-211 and :238-251, the record comes
    back by :215-225 and :255-278, HitRecord::new run again at each level with the wrapper's own ray."""
    p0, p1, deg, off = (0.0, 0.0, 0.0), (165.0, 330.0, 165.0), 15.0, (265.0, 0.0, 295.0)
    ids = {}

    def build(s):
        ids["m"] = s.lambertian(s.solid_color((0.73, 0.73, 0.73)))
        return [s.translate(s.rotate_y(s.aabox(p0, p1, ids["m"]), deg), off), s.sphere((-500.0, 0.0, 0.0), 1.0, ids["m"])]
    sc = _scene(rt, build)

    def world(o, d, t_min, t_max):
        return HR.translate_hit(off, lambda *a: HR.rotate_y_hit(deg, lambda *b: HR.box_hit(p0, p1, *b), *a), o, d, t_min, t_max)
    rays = [((278.0, 278.0, -800.0), (0.1, -0.1, 1.0)), ((278.0, 900.0, 350.0), (0.02, -1.0, 0.01)), ((330.0, 100.0, 370.0), (1.0, 0.3, 0.2)),
            ((330.0, 100.0, 370.0), (-0.5, 0.1, -1.0)), ((900.0, 50.0, 300.0), (-2.0, 0.0, 0.1)), ((0.0, 500.0, 0.0), (0.0, 1.0, 0.0))]
    want = [world(o, d, 0.001, INF) for o, d in rays]
    assert sum(w is not None for w in want) == 5 and want[5] is None
    # two rays start inside the box: the box's own record says front_face 0, and the wrappers' HitRecord::new, which take the child's
    # already turned normal as the outward one, make it 1 again (hittable.rs:216-224): the reference's answer, and the entry's
    local = [HR.box_hit(p0, p1, *HR.rotate_y_ray(deg, [o[k] - off[k] for k in range(3)], d), 0.001, INF) for o, d in rays[:5]]
    assert [h["front"] for h in local].count(False) == 2 and all(w["front"] for w in want[:5])
    _check(rt, sc, [_ray(o, d) for o, d in rays], want, "box under Translate(RotateY)", mats=[ids["m"]] * len(rays), uv=False)


def test_moving_sphere_at_two_times(rt):
    """moving_sphere.rs:23-26, :39-69: the centre at the ray's time; a ray that hits at time 0 misses at time 1 and the other way round."""
    c0, c1, r = (0.0, 0.0, 0.0), (4.0, 1.0, 0.0), 1.0
    ids = {}

    def build(s):
        ids["m"] = s.metal((0.8, 0.8, 0.8), 0.0)
        return [s.moving_sphere(c0, c1, 0.0, 1.0, r, ids["m"])]
    sc = _scene(rt, build)
    cases = [((0.2, 0.1, -5.0), (0.0, 0.0, 1.0), 0.0), ((0.2, 0.1, -5.0), (0.0, 0.0, 1.0), 1.0), ((4.1, 1.2, -5.0), (0.0, 0.0, 1.0), 1.0),
             ((4.1, 1.2, -5.0), (0.0, 0.0, 1.0), 0.0), ((2.0, 0.5, -5.0), (0.0, 0.0, 1.0), 0.5), ((2.0, 0.5, 0.2), (0.3, 0.0, 1.0), 0.5)]
    want = [HR.sphere_hit(HR.moving_center(c0, c1, 0.0, 1.0, tm), r, o, d, 0.001, INF) for o, d, tm in cases]
    assert [w is not None for w in want] == [True, False, True, False, True, True] and want[5]["front"] is False
    _check(rt, sc, [_ray(o, d, time=tm) for o, d, tm in cases], want, "moving sphere", mats=[ids["m"]] * len(cases), uv=False)


# ------------------------------------------------------------------------------------------------ 3: media --

def test_medium_free_flight_from_the_first_draw(rt):
    """constant_medium.rs:58-113 around a sphere of radius 2: t = rec1 + (-1 / density) * ln(u) / |d| with u the FIRST f64 of ray r's
    stream (first_stream + r, sample, global_seed), computed here from Philox4x32-10; a flight longer than the chord is a miss.  64 rays of
    one geometry, so only the draw differs; a window that cuts the chord; and a direction that is not a unit vector."""
    density, first, sample, seed = 0.2, 1000, 3, 5
    ids = {}

    def build(s):
        glass = s.dielectric(1.5)
        tex = s.solid_color((0.9, 0.9, 0.9))
        before = s.lambertian(tex)
        medium = s.constant_medium(s.sphere((0.0, 0.0, 0.0), 2.0, glass), density, tex)
        ids["after"], ids["isotropic"] = s.lambertian(tex), before + 1
        return [medium, s.sphere((50.0, 0.0, 0.0), 1.0, ids["after"])]
    sc = _scene(rt, build)
    assert ids["after"] == ids["isotropic"] + 1, "the medium's Isotropic took the next free id"
    n = 64
    for d, t_min, t_max in (((0.0, 0.0, 1.0), 0.001, INF), ((0.0, 0.0, 2.5), 0.001, INF), ((0.0, 0.0, 1.0), 3.5, 6.0)):
        o = (0.0, 0.0, -5.0)
        length = d[2]
        t1, t2 = 3.0 / length, 7.0 / length
        rays = np.array([_ray(o, d, t_min, t_max)] * n)
        rec, node = rt.hit_host(sc, rays, first_stream=first, sample=sample, global_seed=seed)
        hits = 0
        for r in range(n):
            u = HR.first_f64(first + r, sample, seed)
            rec1, rec2 = max(max(t1, t_min), 0.0), min(t2, t_max)
            flight = (-1.0 / density) * np.log(u)
            if flight > (rec2 - rec1) * length:
                assert np.all(rec[r] == 0.0) and node[r] == HR.NO_NODE, (d, r, "the flight leaves the boundary")
                continue
            hits += 1
            t = rec1 + flight / length
            assert rec[r, 0] == 1.0 and abs(rec[r, 1] - t) <= RTOL * t, (d, r, rec[r, 1], t)
            _close(rec[r, 2:5], [0.0, 0.0, o[2] + t * d[2]], (d, r, "p"))
            assert list(rec[r, 5:11]) == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0], (d, r, "normal (1, 0, 0), u = v = 0, front_face")
            assert rec[r, 11] == float(ids["isotropic"]) and (HR.nodes_of(sc)["kind"][node[r]] & 0xFF) == HR.MEDIUM
        print("direction", d, "window", (t_min, t_max), "hits", hits, "of", n)
        assert 8 <= hits <= n - 8, "both outcomes are populated"


def _split_rule(query, rays, what):
    """one call against two calls with first_stream advanced, and against a call whose list starts later"""
    one = query(rays, 11)
    for cut in (1, 100, len(rays) - 1):
        a, b = query(rays[:cut], 11), query(rays[cut:], 11 + cut)
        assert HR.same_bits(np.concatenate([a[0], b[0]]), one[0]) and np.array_equal(np.concatenate([a[1], b[1]]), one[1]), (what, cut)
    moved = query(rays, 12)
    return one, moved


@pytest.mark.parametrize("arm", [6, 7])
def test_split_rule(rt, arm):
    """The records of rays r.. of one call equal those of a second call with first_stream + r, bit for bit; and the draws do come from the
    stream: with another first_stream some medium hit moves."""
    sc = rt.Scene.reference(arm, build_seed=1)
    rays = HR.camera_rays(rt, sc, W, H, 1, 0, 3)
    one, moved = _split_rule(lambda r, fs: rt.hit_host(sc, r, first_stream=fs, sample=2, global_seed=9), rays, arm)
    in_medium = (HR.nodes_of(sc)["kind"][one[1][one[1] != HR.NO_NODE]] & 0xFF) == HR.MEDIUM
    print("arm", arm, "hits in a medium", int(in_medium.sum()), "of", len(rays))
    assert in_medium.sum() >= 4 and not HR.same_bits(one[0], moved[0])


# ------------------------------------------------------------------------------------------------ 4: refusals --

class _Arena:
    """the three buffers of a call laid out as a case of the golden table asks: each on its own, or one at a byte offset into another"""

    def __init__(self, case, rays, alloc, upload):
        n = len(rays)
        size = {"rays": n * 72, "out": n * 96, "out_node": n * 4}
        self.mem = {k: alloc(4096) for k in size}  # each its own, with room for a buffer laid into it
        self.ptr = {k: self.mem[k][0] for k in size}
        if case.get("overlap"):
            laid, base, offset = case["overlap"]
            self.ptr[laid] = self.mem[base][0] + offset
        upload(self.ptr["rays"], rays)
        for k in case.get("null", []):
            if k in self.ptr:
                self.ptr[k] = None


def _host_alloc(nbytes):
    a = np.zeros(nbytes + 16, dtype=np.uint8)
    p = (a.ctypes.data + 15) & ~15
    return p, a


def _host_upload(ptr, rays):
    C.memmove(ptr, rays.ctypes.data, rays.nbytes)


def _table_params(rt, case, n):
    return rt.HitParams(case.get("n", n), 0, case.get("global_seed", 0), 0, case.get("flags", 0))


def _table_rays(count=4):
    return np.array([[float(x) for x in REFUSALS["ok"]]] * count, dtype=np.float64)


def _run_table(rt, call, alloc, upload, download, with_text):
    """every case of the golden table through call(params or None, rays, out, out_node) -> code"""
    rays = _table_rays()
    for case in REFUSALS["refusals"]:
        ar = _Arena(case, rays, alloc, upload)
        p = None if "params" in case.get("null", []) else _table_params(rt, case, len(rays))
        rc = call(p, ar.ptr["rays"], ar.ptr["out"], ar.ptr["out_node"])
        assert rc == case["code"] == rt.ERR_INVALID, (case["name"], rc)
        if with_text:
            assert rt.last_error() == case["text"], (case["name"], rt.last_error())
    for case in REFUSALS["accepted"]:
        ar = _Arena(case, rays, alloc, upload)
        rc = call(_table_params(rt, case, len(rays)), ar.ptr["rays"], ar.ptr["out"], ar.ptr["out_node"])
        assert rc == rt.OK, (case["name"], rc, rt.last_error())
        rec = download(ar.ptr["out"], (len(rays), 12), np.float64)
        assert np.all(rec[:, 0] == 1.0) and HR.same_bits(rec, np.repeat(rec[:1], len(rays), axis=0)), case["name"]
        if ar.ptr["out_node"] is not None:
            assert np.all(download(ar.ptr["out_node"], (len(rays),), np.uint32) != HR.NO_NODE), case["name"]


def _host_download(ptr, shape, dtype):
    out = np.empty(shape, dtype=dtype)
    C.memmove(out.ctypes.data, ptr, out.nbytes)
    return out


def _nonfinite(rt, query):
    """the table's rays answered as misses before any walk, among rays that hit; and the infinite bounds that are literal"""
    ok = [float(x) for x in REFUSALS["ok"]]
    rows, expect = [ok], [1]
    for m in REFUSALS["misses"]:
        r = list(ok)
        r[m["slot"]] = float(m["value"])
        rows += [r, ok]
        expect += [0, 1]
    for m in REFUSALS["literal"]:
        r = list(ok)
        r[m["slot"]] = float(m["value"])
        rows.append(r)
        expect.append(m["hit"])
    rays = np.array(rows, dtype=np.float64)
    assert list(HR.refused(rays)) == [k % 2 == 1 for k in range(1 + 2 * len(REFUSALS["misses"]))] + [False] * len(REFUSALS["literal"])
    rec, node = query(rays)
    assert list(rec[:, 0]) == [float(e) for e in expect]
    miss = rec[:, 0] == 0.0
    assert np.all(rec[miss].view(np.uint64) == 0) and np.all(node[miss] == HR.NO_NODE) and np.all(node[~miss] != HR.NO_NODE)
    assert HR.same_bits(rec[~miss], np.repeat(rec[:1], int((~miss).sum()), axis=0)), "a refused neighbour changes nothing"


def test_refusals_and_rays_answered_as_misses(rt):
    """Every refusal of include/rt1w.h through the twin, which refuses what the entries refuse (tests/golden/hit_refusals.json; the GPU
    tier runs the same table through the two entries, with their texts); both entries without a context; the non-finite rays."""
    sc = rt.Scene.reference(6, build_seed=1)
    lab = rt.load_lab()

    def call(p, rays, out, node):
        return lab.rt1w_lab_hit_host(sc._h, None if p is None else C.byref(p), rays, out, node)
    _run_table(rt, call, _host_alloc, _host_upload, _host_download, with_text=False)
    rays = _table_rays()
    out, node, p = np.zeros((4, 12)), np.zeros(4, dtype=np.uint32), rt.HitParams(4, 0, 0, 0, 0)
    assert lab.rt1w_lab_hit_host(None, C.byref(p), rays.ctypes.data, out.ctypes.data, node.ctypes.data) == rt.ERR_INVALID
    for fn in (rt._lib.rt1w_hit, rt._lib.rt1w_hit_device):
        assert fn(None, C.byref(p), rays.ctypes.data, out.ctypes.data, node.ctypes.data, None) == rt.ERR_INVALID
        assert rt.last_error() == "null argument"
    with pytest.raises(ValueError):
        rt.hit_host(sc, np.zeros((4, 8)))
    _nonfinite(rt, lambda r: rt.hit_host(sc, r))
    seven = rt.hit_host(sc, rays[:, :7], t_min=0.001, t_max=INF)  # [n, 7] with the bounds filled in
    assert HR.same_bits(seven[0], rt.hit_host(sc, rays)[0])


# ------------------------------------------------------------------------------------------------ 5: the sanitizer build --

DRIVER_SCENES = {"arm5": lambda rt: (rt.Scene.reference(5, build_seed=1), None), "arm6": lambda rt: (rt.Scene.reference(6, build_seed=1), None),
                 "media, stack walk": lambda rt: (aov_scenes.scene_pair("media")[0], 3)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/hit_driver.cpp with -fsanitize=address,undefined: a stand-alone program, nothing of it is loaded into this process"""
    out = tmp_path_factory.mktemp("hit_driver") / "hit_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "raytracing-1w_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hit_driver.cpp"), "-o", str(out)])
    return out


@pytest.mark.parametrize("name", list(DRIVER_SCENES))
def test_sanitizer_build_on_the_adversarial_rays(rt, driver, tmp_path, name):
    """The fixed adversarial set (hit_reference.adversarial_rays: zero and denormal directions, huge magnitudes, t_min > t_max, t_max =
    +inf, origins on surfaces and box faces, rays along box edges, the non-finite rays) through the sanitizer build of rt_hit.h: exit 0, no
    report, and the records, node indices and checksum of the twin."""
    sc, variant = DRIVER_SCENES[name](rt)
    rays = HR.adversarial_rays(sc)
    rec, node = rt.hit_host(sc, rays, first_stream=5, sample=1, global_seed=2, variant=variant)
    (tmp_path / "nodes.bin").write_bytes(sc.flat(0).tobytes())
    (tmp_path / "rays.bin").write_bytes(rays.tobytes())
    root = int(sc.flat(6)[-8:].view(np.uint32)[0])
    v = sc.info()["variant"] if variant is None else variant
    p = subprocess.run([str(driver), str(tmp_path / "nodes.bin"), str(root), str(v), str(tmp_path / "rays.bin"), "5", "1", "2", str(tmp_path / "out.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    raw = (tmp_path / "out.bin").read_bytes()
    got_rec = np.frombuffer(raw[:rec.nbytes], dtype=np.float64).reshape(rec.shape)
    got_node = np.frombuffer(raw[rec.nbytes:], dtype=np.uint32)
    assert np.array_equal(got_rec.view(np.uint64), rec.view(np.uint64)) and np.array_equal(got_node, node)
    assert p.stdout.strip() == f"checksum {HR.checksum(rec, node):016x}"
    ref = HR.refused(rays)
    print(name, len(rays), "rays,", int(rec[:, 0].sum()), "hits,", int(ref.sum()), "answered as misses,", int(np.isnan(rec).any(axis=1).sum()), "records with a NaN")
    assert np.all(rec[ref] == 0.0) and rec[:, 0].sum() >= len(rays) // 8


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

def _lab_rays(rt, ctx, bounces=4):
    """the valid rays of bounces 1 .. bounces - 1 of the 24 x 16 x 2 tile's paths (rt1w_lab_dump_rays): incoherent"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import walk_lab as wl
    lab = wl.Lab(ctx)
    d = lab.dump_rays(W, H, 2, bounces)[1:].reshape(-1, 8)
    return lab, wl, d[d[:, 7] != 0.0]


GPU_SCENES = {5: "every", 6: "every", 0: "own", 7: "own"}  # arm -> the variants run


@pytest.mark.gpu
@pytest.mark.parametrize("arm", list(GPU_SCENES))
def test_gpu_kernel_equals_twin(rt, gpu_ctx_factory, arm):
    """Records and node indices of the kernels against the twin, bit for bit: camera rays 24 x 16 x 2, the incoherent rays of bounces 1-3 of
    the same paths, the adversarial set; and the first n rays of camera + bounce rays for every n of COUNTS.  Arm 5 sweep, 6 sweep with
    media, 0 stack walk with moving spheres, 7 stack walk with media; every variant that covers the small scenes."""
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=1.5)
    ctx = gpu_ctx_factory(sc)
    lab, _, bounce = _lab_rays(rt, ctx)
    lab.close()
    camera = HR.camera_rays(rt, sc, W, H, 2, 1, 4)
    bounce = HR.with_bounds(bounce[:, :7])
    both = np.concatenate([camera, bounce])
    assert len(bounce) >= 64 and len(both) >= max(COUNTS), (len(camera), len(bounce))
    sets = {"camera": camera, "bounces 1-3": bounce, "adversarial": HR.adversarial_rays(sc)}
    sets.update({f"first {n}": both[:n] for n in COUNTS})
    variants = HR.valid_variants(sc.info()) if GPU_SCENES[arm] == "every" else [None]
    for v in variants:
        for what, rays in sets.items():
            kw = dict(first_stream=77, sample=3, global_seed=6, variant=v)
            want_rec, want_node = rt.hit_host(sc, rays, **kw)
            rec, node, st = ctx.hit(rays, with_stats=True, **kw)
            assert HR.same_bits(rec, want_rec) and np.array_equal(node, want_node), (arm, v, what, int((node != want_node).sum()))
            assert st["paths"] == st["segments"] == len(rays) and st["block"] == 256 and st["grid"] == (len(rays) + 255) // 256
            assert st["variant"] == (sc.info()["variant"] if v is None else v) and st["kernel_ms"] > 0.0
        print("arm", arm, "variant", v, {k: int(rt.hit_host(sc, r, variant=v)[0][:, 0].sum()) for k, r in sets.items() if not k.startswith("first")})
    if arm == 6:  # the scene of the golden table
        _nonfinite(rt, lambda r: ctx.hit(r))
    ctx.close()


class _Device:
    """device memory from the HIP runtime librt1w.so itself uses (what a torch tensor's data_ptr() would hand over)"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.all = []

    def alloc(self, nbytes, fill=0):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        assert self.hip.hipMemset(p, fill, nbytes) == 0
        self.all.append(p.value)
        return p.value, None

    def upload(self, ptr, a):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0  # HostToDevice

    def download(self, ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # DeviceToHost
        return out

    def free(self):
        for p in self.all:
            self.hip.hipFree(p)
        self.all = []


GUARD = 4096  # bytes of 0xA5 before and after each buffer


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [6, 7])
def test_gpu_device_entry_guard_bands_and_split_rule(rt, gpu_ctx_factory, arm):
    """rt1w_hit_device on plain device buffers: it writes n * 96 and n * 4 bytes and nothing around them, with and without out_node, at an
    n that fills no workgroup and at ray buffers that are and are not 16-byte aligned; the records are the host entry's.  The split rule on
    the device.  Arm 6: the refusals of the golden table through both entries, with their texts."""
    sc = rt.Scene.reference(arm, build_seed=1)
    ctx = gpu_ctx_factory(sc)
    dev = _Device()
    rays = HR.camera_rays(rt, sc, W, H, 1, 0, 3)[:333]
    n = len(rays)
    want = ctx.hit(rays, first_stream=11, sample=2, global_seed=9)
    assert HR.same_bits(want[0], rt.hit_host(sc, rays, first_stream=11, sample=2, global_seed=9)[0])
    for shift in (0, 8):  # the buffers 16-byte aligned, and 8 bytes off
        for with_node in (True, False):
            d_rays, d_out, d_node = (dev.alloc(2 * GUARD + size + 8, 0xA5)[0] for size in (n * 72, n * 96, n * 4))
            dev.upload(d_rays + GUARD + shift, rays)
            st = ctx.hit_device(d_rays + GUARD + shift, d_out + GUARD + shift, d_node + GUARD if with_node else None, n, first_stream=11, sample=2, global_seed=9)
            assert st["paths"] == n and st["grid"] == 2
            out = dev.download(d_out, (2 * GUARD + n * 96 + 8,), np.uint8)
            assert np.all(out[:GUARD + shift] == 0xA5) and np.all(out[GUARD + shift + n * 96:] == 0xA5), (shift, with_node, "records written outside")
            assert HR.same_bits(out[GUARD + shift:GUARD + shift + n * 96].view(np.float64).reshape(n, 12), want[0])
            nodes = dev.download(d_node, (2 * GUARD + n * 4 + 8,), np.uint8)
            inner = nodes[GUARD:GUARD + n * 4]
            assert np.all(nodes[:GUARD] == 0xA5) and np.all(nodes[GUARD + n * 4:] == 0xA5), (shift, with_node, "node indices written outside")
            assert np.array_equal(inner.view(np.uint32), want[1]) if with_node else np.all(inner == 0xA5)
            assert np.all(dev.download(d_rays, (2 * GUARD + n * 72 + 8,), np.uint8)[:GUARD] == 0xA5)
            dev.free()

    def query(r, first_stream):
        d_rays, d_out, d_node = (dev.alloc(size)[0] for size in (len(r) * 72, len(r) * 96, len(r) * 4))
        dev.upload(d_rays, r)
        ctx.hit_device(d_rays, d_out, d_node, len(r), first_stream=first_stream, sample=2, global_seed=9)
        got = dev.download(d_out, (len(r), 12), np.float64), dev.download(d_node, (len(r),), np.uint32)
        dev.free()
        return got
    one, moved = _split_rule(query, rays, arm)
    assert HR.same_bits(one[0], want[0]) and not HR.same_bits(one[0], moved[0])
    if arm == 6:
        _run_table(rt, lambda p, r, o, nd: rt._lib.rt1w_hit(ctx._h, None if p is None else C.byref(p), r, o, nd, None),
                   _host_alloc, _host_upload, _host_download, with_text=True)
        _run_table(rt, lambda p, r, o, nd: rt._lib.rt1w_hit_device(ctx._h, None if p is None else C.byref(p), r, o, nd, None),
                   lambda nbytes: dev.alloc(nbytes), dev.upload, dev.download, with_text=True)
        dev.free()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_SCENES[:6])
def test_gpu_against_the_literal_oracle(rt, gpu_ctx_factory, name):
    """The comparison of test_twin_against_the_literal_oracle with the GPU's records, arms 0-5, in the scene's own variant."""
    prod = aov_scenes.scene_pair(name)[0]
    ctx = gpu_ctx_factory(prod)
    for so, gs in SEEDS:
        rays = HR.camera_rays(rt, prod, W, H, 1, so, gs)
        rec, node = ctx.hit(rays)
        assert _against_oracle(name, rays, rec, node, so, gs, (name, so, gs, "gpu"))[0] > 0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arm", [0, 7])
def test_gpu_against_the_lab_trace(rt, gpu_ctx_factory, arm):
    """With the bounds the diagnostics library's trace uses (0.001, inf): t bits and leaf of every dumped ray equal what rt1w_lab_trace
    returns for the product's walk (mode 0, the stack walk) -- on the scenes whose own variant is a stack walk, the walk the trace offers.
    The trace gives ray i the stream of pixel seed i, sample 0, global_seed 0: first_stream = 0 here, so a medium draws the same."""
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=1.5)
    ctx = gpu_ctx_factory(sc)
    lab, wl, rays = _lab_rays(rt, ctx)
    assert lab.variant >= 2 and lab.variant == sc.info()["variant"], "the product's walk of this scene is the stack walk"
    lab.set_rays(rays)
    base = lab.trace(0, repeats=1)
    lab.close()
    rec, node = ctx.hit(HR.with_bounds(rays[:, :7]), first_stream=0, sample=0, global_seed=0)
    assert np.array_equal(node, base["prim"])
    hit = node != HR.NO_NODE
    assert hit.sum() >= len(rays) // 4 and np.array_equal(rec[hit, 1].view(np.uint64), base["t"][hit].view(np.uint64))
    ctx.close()
