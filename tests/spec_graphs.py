"""Shared by test_spec_fuzz.py (CPU) and test_spec_fuzz_gpu.py: the corpus of scene graphs the scene-specialised kernels are fuzzed
with, and what a graph's generated unit declares (census).  Two sources of (product scene, literal-oracle scene) pairs, both built call
for call through dual.Dual:

  ("random", seed, None)      dual.random_scene_pair(seed): every coordinate from a continuous range
  ("lattice", seed, n_nodes)  lattice_scene_pair(seed, n_nodes): the same well-formed grammar on the lattice of multiples of 0.5 in
                              [-3, 3] -- bounds coincide, rects are coplanar, boxes share faces, -0.0 stands next to +0.0 -- with the
                              knobs of the specialised text drawn per seed; n_nodes pads the graph to that many flat nodes exactly

The seed lists are fixed here; what they cover is recorded in golden/spec_fuzz_census.json and held by test_spec_fuzz.py."""
import re

import numpy as np

import box_free_scenes as BF
import hit_scenes as H
import lambert_scenes as L
import slab_scenes as S
from dual import Dual, random_scene_pair

JIT_MAX_NODES = 256   # rt_flat.h: RT_JIT_MAX_NODES


def _lat(g, lo, hi):
    """a multiple of 0.5 in [lo, hi]"""
    return 0.5 * float(g.integers(int(round(lo * 2)), int(round(hi * 2)) + 1))


def _lat3(g, lo, hi):
    return [_lat(g, lo, hi) for _ in range(3)]


ANGLES = (0.0, 30.0, -30.0, 90.0, -90.0, 180.0)
CHAIN_COUNTS = (0, 1, 2, 7, 8, 9, 11)
MEDIA = (None, None, None, "sphere", "box", "wrapped_box")


def lattice_knobs(seed):
    """the knobs of a lattice graph, as lattice_scene_pair draws them (the first draws of the seed's stream)"""
    g = np.random.default_rng(seed)
    build_seed = int(g.integers(1, 1 << 30))
    k = {"build_seed": build_seed,
         # where Lambertian materials may sit, and must: bit 0 anything but an unwrapped rect, bits 1-3 unwrapped XY / XZ / YZ rects.
         # Stratified over the seed, so that 16 consecutive seeds hold every combination of the four lambert_* flags
         "lambert": int(seed) % 16,
         "chains": int(CHAIN_COUNTS[int(g.integers(0, len(CHAIN_COUNTS)))]),
         "media": MEDIA[int(g.integers(0, len(MEDIA)))],
         "n_lights": int(g.integers(0, 5)),
         "aperture": float(g.choice([0.0, 0.2])),
         "axis_camera": bool(g.integers(0, 2)),
         "n_nested": int(g.integers(1, 4)),
         "coplanar": int(g.integers(0, 3)),       # 0 none, 1 a pair of coplanar rects, 2 three of them
         "shared_face_boxes": bool(g.integers(0, 3) == 0),
         "signed_zero": bool(g.integers(0, 2)),
         "black_sky": bool(g.integers(0, 10) < 3)}   # a background of zeros, and then an emitter the camera sees
    return g, k


def _bvh_nodes(n):
    """BVH nodes over n objects (bvh.rs:84-117: one object is a node of its own, two share one, more are split in the middle)"""
    return 1 if n <= 2 else 1 + _bvh_nodes(n // 2) + _bvh_nodes(n - n // 2)


def lattice_scene_pair(seed, n_nodes=None, best_axis=True):
    """A well-formed scene graph on the lattice (module docstring).  n_nodes: pad with lattice spheres (some below a Translate: two
    nodes) to exactly that many flat nodes; the graph is built once to count and once more, from the same stream, with the pad."""
    if n_nodes is None:
        return _lattice(seed, None, best_axis)[:2]
    prod, _, n_obj = _lattice(seed, (0, 0), best_axis)
    own = prod.info()["n_nodes"] - _bvh_nodes(n_obj)
    fits = [(a, b) for b in range(3) for a in range(n_nodes) if own + a + 2 * b + _bvh_nodes(n_obj + a + b) == n_nodes]
    assert fits, (seed, n_nodes, prod.info()["n_nodes"])
    prod, oracle, _ = _lattice(seed, fits[0], best_axis)
    assert prod.info()["n_nodes"] == n_nodes, (seed, n_nodes, prod.info()["n_nodes"])
    return prod, oracle


def _lattice(seed, pad, best_axis):
    g, K = lattice_knobs(seed)
    d = Dual(K["build_seed"], best_axis)
    img = g.integers(0, 256, (8, 16, 3), dtype=np.uint8)
    lam_general, lam_rect = bool(K["lambert"] & 1), [bool(K["lambert"] & (2 << a)) for a in range(3)]
    small = pad is not None or K["chains"] >= 7   # graphs that get many objects of one kind keep the others few
    pad = pad or (0, 0)
    colour = lambda lo=0.25, hi=1.0: [0.25 * float(g.integers(int(lo * 4), int(hi * 4) + 1)) for _ in range(3)]

    def tex(depth=0):
        k = g.integers(0, 4 if depth < 2 else 1)
        if k == 0: return d.solid(colour())
        if k == 1: return d.checker(tex(depth + 1), tex(depth + 1))
        if k == 2: return d.noise(_lat(g, 0.5, 5.0))
        return d.image(img)   # reads (u, v)

    def other_material(mirror):
        """anything but a Lambertian; mirror: a Metal with fuzz 0 (on an axis rect a reflected ray keeps its exact zero components)"""
        if mirror: return d.metal(colour(0.5, 1.0), 0.0)
        k = g.integers(0, 6)
        if k < 2: return d.metal(colour(0.5, 1.0), float(g.choice([0.0, 0.5])))
        if k < 4: return d.dielectric(float(g.choice([1.5, 1.25, 2.5])))
        if k < 5: return d.diffuse_light(d.solid([float(x) for x in g.integers(1, 7, 3)]))
        return d.metal(colour(0.5, 1.0), 1.0)

    def material(lam_ok, mirror=False):
        if lam_ok and g.integers(0, 2): return d.lambertian(tex())
        return other_material(mirror)

    def rect(axis, lam_ok, k=None, force_lam=False):
        a0, b0 = _lat(g, -3, 1), _lat(g, -3, 1)
        a1, b1 = min(3.0, a0 + _lat(g, 0.5, 3)), min(3.0, b0 + _lat(g, 0.5, 3))
        m = d.lambertian(tex()) if force_lam else material(lam_ok, mirror=bool(g.integers(0, 2)))
        return d.rect(axis, a0, a1, b0, b1, _lat(g, -3, 3) if k is None else k, m)

    def sphere(lam_ok, force_lam=False):
        c, r = _lat3(g, -2, 2), _lat(g, 0.5, 1.0)
        m = d.lambertian(tex()) if force_lam else material(lam_ok)
        if g.integers(0, 4) == 0:
            return d.moving_sphere(c, [c[0], min(3.0, c[1] + 0.5), c[2]], 0.0, 1.0, r, m)
        return d.sphere(c, r, m)

    def box(lam_ok, p0=None, size=None):
        p0 = _lat3(g, -3, 1) if p0 is None else p0
        size = [_lat(g, 0.5, 2.0) for _ in range(3)] if size is None else size
        return d.aabox(p0, [min(3.0, p0[a] + size[a]) for a in range(3)], material(lam_ok))

    def primitive(wrapped_, allow_box=True):
        """a leaf (or a box) that will stand below a Translate / RotateY (wrapped_) or outside every wrapper"""
        k = int(g.integers(0, 6 if allow_box and not small else 5))
        if k < 2: return sphere(lam_general)
        if k < 5: return rect(k - 2, lam_general if wrapped_ else lam_rect[k - 2])
        return box(lam_general if wrapped_ else all(lam_rect))

    def wrap(h, depth, moving=None):
        """`depth` wrappers in a drawn order of Translate / RotateY / FlipFace; moving: at least one of the first two"""
        kinds = [int(x) for x in g.integers(0, 3, depth)]
        if moving and depth and all(k == 2 for k in kinds):
            kinds[int(g.integers(0, depth))] = int(g.integers(0, 2))
        for k in kinds:
            if k == 0: h = d.translate(h, _lat3(g, -1.5, 1.5))
            elif k == 1: h = d.rotate_y(h, float(g.choice(ANGLES)))
            else: h = d.flip_face(h)
        return h

    objects = []
    # -- Lambertian placement: one object for every flag the knob sets (the other objects may add more of the same, never another)
    for a in range(3):
        if lam_rect[a]: objects.append(rect(a, True, force_lam=True))
    if lam_general:
        objects.append(sphere(True, force_lam=True) if g.integers(0, 2) else d.translate(rect(int(g.integers(0, 3)), True, force_lam=True), _lat3(g, -1, 1)))
    # -- wrapper chains: every chain is a wrapped object of its own (a Translate / RotateY in it, so that the leaves below are wrapped)
    for c in range(K["chains"]):
        depth = int(g.integers(1, 4))
        what = int(g.integers(0, 8))
        if what == 0 and not small:   # a wrapped group: the chain stands above a BVH
            objects.append(wrap(d.bvh([primitive(True, allow_box=False) for _ in range(int(g.integers(1, 4)))]), min(depth, 2), moving=True))
        else:
            objects.append(wrap(primitive(True, allow_box=(c < 2)), depth, moving=True))
    # -- FlipFace on a leaf (folded into it), above a BVH, and between two BVH levels
    axis = int(g.integers(0, 3))
    objects.append(d.flip_face(rect(axis, lam_rect[axis])))
    if K["chains"] > 0:   # (a FlipFace that stays a node is a chain: the graphs with none have none)
        inner = d.bvh([sphere(lam_general), rect(1, lam_general)])
        objects.append(d.bvh([d.flip_face(inner)]) if g.integers(0, 2) else d.flip_face(inner))
    # -- nested BVHs of 1 to 4 elements whose boxes share faces with the parent's: a BVH of one element has its element's box, and the
    #    elements stand on common planes
    for _ in range(K["n_nested"]):
        n = int(g.integers(1, 5))
        x0, y0 = _lat(g, -3, 0), _lat(g, -3, 1)
        el = []
        for j in range(n):   # spheres of radius 0.5 in a row along x, on one floor and against one wall
            m = material(lam_general)
            el.append(d.sphere([x0 + 0.5 + j, y0 + 0.5, 0.5], 0.5, m))
        group = d.bvh(el)
        objects.append(d.bvh([group]) if g.integers(0, 2) else group)
    if K["signed_zero"]:
        # a bound written as -0.0 next to a +0.0 one: the rect's x range starts at -0.0 (the constructor keeps the sign), the sphere's box
        # at 0.5 - 0.5 = +0.0; each stands in a one-element BVH below the group's, whose own bound is one of the two
        a = d.bvh([d.rect(1, -0.0, 1.0, -0.0, 1.0, _lat(g, -2, 2), material(lam_rect[1], mirror=True))])
        b = d.bvh([d.sphere([0.5, _lat(g, -2, 2), 0.5], 0.5, material(lam_general))])
        objects.append(d.bvh([a, b]))
    # -- coplanar rects that overlap at equal t, in different subtrees; boxes that share a face
    if K["coplanar"]:
        axis, k = int(g.integers(0, 3)), _lat(g, -2, 2)
        a0 = _lat(g, -3, 0)
        for j in range(K["coplanar"] + 1):
            m = material(lam_rect[axis], mirror=(j == 0))
            objects.append(d.rect(axis, a0 + 0.5 * j, a0 + 0.5 * j + 2.0, -1.0, 1.5, k, m))
    if K["shared_face_boxes"] and not small:
        p0 = _lat3(g, -2, 0)
        objects.append(box(all(lam_rect), p0, [1.0, 1.0, 1.0]))
        objects.append(box(all(lam_rect), [p0[0] + 1.0, p0[1], p0[2]], [1.0, 1.5, 1.0]))
    if K["black_sky"]:
        objects.append(d.sphere([_lat(g, -1, 1), _lat(g, 1, 2), 2.0], 1.0, d.diffuse_light(d.solid([4.0, 4.0, 4.0]))))
    # -- media: closed boundaries (sphere, box, wrapped box), nothing inside
    if K["media"]:
        c = _lat3(g, -2, 1)
        if K["media"] == "sphere": b = d.sphere(c, _lat(g, 1.0, 1.5), d.dielectric(1.5))
        else:
            b = d.aabox(c, [c[a] + _lat(g, 1.0, 2.0) for a in range(3)], d.dielectric(1.5))
            if K["media"] == "wrapped_box": b = d.translate(d.rotate_y(b, float(g.choice(ANGLES))), _lat3(g, -1, 1))
        objects.append(d.constant_medium(b, _lat(g, 0.5, 2.0), tex()))
    # -- and a few more objects of any kind outside the wrappers
    for _ in range(int(g.integers(0, 2 if small else 4))):
        objects.append(primitive(False))
    # -- the pad (n_nodes): lattice spheres, the last below a Translate
    for j in range(pad[0]):
        objects.append(d.sphere([-2.5 + 0.5 * (j % 11), -2.5 + 0.5 * ((j // 11) % 11), -2.0], 0.5, other_material(j % 3 == 0)))
    for j in range(pad[1]):
        objects.append(d.translate(d.sphere([0.0, 0.0, 0.0], 0.5, other_material(False)), [2.5, 2.5, -1.0]))
    order = g.permutation(len(objects))
    world = d.bvh([objects[i] for i in order])
    # -- lights: 0 to 4 of the kinds random_scene_pair has, with repeats
    lights, null = [], None
    for _ in range(K["n_lights"]):
        null = null or d.null_material()
        k = g.integers(0, 4)
        if k == 0: lights.append(d.rect(1, -1.0, 1.0, -1.0, 1.0, 3.0, null))
        elif k == 1: lights.append(d.sphere(_lat3(g, -2, 2), _lat(g, 0.5, 1.0), null))
        elif k == 2: lights.append(d.rect(0, -1.0, 1.0, -1.0, 1.0, 3.0, null))          # XYRect: trait defaults
        else: lights.append(d.flip_face(d.rect(1, -1.0, 1.0, -1.0, 1.0, 2.5, null)))    # FlipFace forwards neither pdf nor random
    bg = [0.0, 0.0, 0.0] if K["black_sky"] else colour(0.25, 1.0)
    if K["axis_camera"]:   # along -z from a lattice point
        at = [_lat(g, -1, 1), _lat(g, -1, 1)]
        cam = (at + [_lat(g, 5, 8)], at + [0.0], (0.0, 1.0, 0.0), float(g.choice([40.0, 60.0])), float(g.choice([1.0, 1.5])), K["aperture"], 6.0, 0.0, 1.0)
    else:
        cam = ([_lat(g, -1, 1), _lat(g, -0.5, 1.5), _lat(g, 6, 9)], _lat3(g, -0.5, 0.5), (0.0, 1.0, 0.0), float(g.choice([40.0, 60.0])),
               float(g.choice([1.0, 1.5])), K["aperture"], _lat(g, 5, 9), 0.0, 1.0)
    return d.finish(world, lights, bg, cam) + (len(objects),)


# ------------------------------------------------------------------------------------------------------------------ the corpus --
def name_of(entry):
    return f"{entry[0]}{entry[1]}" + (f"_n{entry[2]}" if entry[2] else "")


# 48 random graphs: dual.random_scene_pair over the seeds from 3000 on, the first 45 graphs of at most 64 nodes and the first three of
# 65 to 100 whose frame is not empty (a third of that generator's graphs have a black sky and no emitter in sight)
RANDOM = tuple(("random", s, None) for s in (3000, 3001, 3002, 3004, 3007, 3008, 3009, 3010, 3011, 3012, 3013, 3014, 3015, 3016, 3017, 3018, 3019, 3020, 3025,
                                             3026, 3027, 3028, 3029, 3031, 3034, 3035, 3038, 3039, 3040, 3041, 3043, 3044, 3046, 3047, 3048, 3049, 3051, 3054,
                                             3056, 3057, 3058, 3059, 3060, 3061, 3063, 3064, 3066, 3067))
# 48 lattice graphs: for every value of the Lambertian knob (seed % 16) the first three seeds whose graph has at most 60 nodes and a frame
# that is not empty; five of them padded to the node counts on either side of RT_BOX_FREE_MAX_NODES and at RT_JIT_MAX_NODES
_SIZED = {2: 63, 8: 64, 19: 65, 36: 255, 90: 256}
LATTICE = tuple(("lattice", s, _SIZED.get(s)) for s in (0, 2, 8, 11, 12, 18, 19, 20, 21, 24, 29, 32, 33, 34, 36, 38, 39, 44, 54, 58, 60, 62, 65, 67, 70, 71, 72, 75,
                                                       81, 89, 90, 91, 103, 109, 112, 122, 127, 148, 149, 175, 185, 195, 207, 213, 221, 222, 238, 345))
REFUSED = ("lattice", 90, JIT_MAX_NODES + 1)   # one node too many: kernel_source() and specialise() refuse
# the GPU tier's 24: 12 of each source, none above 64 nodes, chosen so that the coverage conditions hold for them alone (test_spec_fuzz_gpu.py)
_BY_NAME = lambda names: tuple(next(e for e in RANDOM + LATTICE if name_of(e) == n) for n in names)
GPU_NAMES = ("random3047", "random3029", "random3007", "random3043", "random3013", "random3056", "random3035", "random3044", "random3009", "random3061",
             "random3031", "random3064", "lattice8_n64", "lattice2_n63", "lattice38", "lattice122", "lattice175", "lattice12", "lattice221", "lattice39",
             "lattice72", "lattice75", "lattice148", "lattice195")
GPU_F32_AND_TILES = ("random3047", "random3029", "random3013", "random3061", "lattice12", "lattice72", "lattice175", "lattice221")
GPU = _BY_NAME(GPU_NAMES)
GPU_BOX_FREE_BUILDS = ("lattice2_n63", "lattice8_n64", "lattice38", "lattice122")   # of the 24, the four that sweep without boxes with the most reused bounds


def build(entry):
    """(product scene, literal-oracle scene) of a corpus entry"""
    source, seed, n_nodes = entry
    return random_scene_pair(seed) if source == "random" else lattice_scene_pair(seed, n_nodes)


# ------------------------------------------------------------------------------------------------------------------- the census --
def _mixed_vbox(kind, skip, rows, root):
    """does a group of leaves that rt_box_free_verify takes together -- the world's, or those below one Translate / RotateY -- differ in
    its column of Topo::vbox?  (rt_core.h: rt_vbox_common gives RT_VBOX_MIXED then)"""
    found = False

    def walk(lo, hi, depth):
        nonlocal found
        col = {rows[i][depth] for i in range(lo, hi) if H.SPHERE <= (kind[i] & 0xFF) <= H.YZ} if depth < BF.SPACES else set()
        found |= len(col) > 1
        i = lo
        while i < hi:
            k = kind[i] & 0xFF
            if k in (S.TRANSLATE, S.ROTATE_Y):
                walk(i + 1, skip[i], depth + 1)
                i = skip[i]
            else:
                i += 1

    walk(root, skip[root], 0)
    return found


def census(sc):
    """what the scene's generated unit declares, from Scene.kernel_source() and Scene.info() alone"""
    src, info = sc.kernel_source(), sc.info()
    kind, skip = H._table(src, "kind"), H._table(src, "skip")
    root = int(re.search(r"root = (\d+)u;", src).group(1))
    rows, box_free = BF.declared(sc)
    other, pairs = S.counts(S.reuse_table(sc))
    wrap, _ = H.tables(sc)
    n_chains = len(H.chains({"kind": kind}, wrap))
    light_kinds, lam_general, lam_rects = L.shape(sc)
    return {"box_free": box_free, "reuse_entries": other, "reuse_whole_axes": pairs, "chains": n_chains,
            "chains_walked": max(0, n_chains - H.MAX_CHAINS), "vbox_mixed": bool(box_free and _mixed_vbox(kind, skip, rows, root)),
            "lambert": [lam_general] + list(lam_rects), "n_lights": len(light_kinds), "light_kinds": sorted(set(light_kinds)),
            "has_media": bool(info["has_media"]), "has_textures": bool(info["has_textures"]), "has_moving": bool(info["has_moving"]),
            "n_nodes": int(info["n_nodes"]), "scope_depth": int(info["scope_depth"])}


def coverage(cs, few=4):
    """the conditions a corpus must meet so that a test over it cannot pass by covering nothing: a dict of name -> bool.  `few`: the
    "at least four" of the whole corpus (two for the GPU's 24 graphs)"""
    n = len(cs)
    lam = {tuple(c["lambert"]) for c in cs}
    return {"a quarter sweep without boxes": 4 * sum(c["box_free"] for c in cs) >= n,
            "a quarter reuse a slab product": 4 * sum(c["reuse_entries"] > 0 for c in cs) >= n,
            "media with a whole-axis pair": sum(c["has_media"] and c["reuse_whole_axes"] > 0 for c in cs) >= few,
            "more chains than blocks": sum(c["chains_walked"] > 0 for c in cs) >= few,
            "a mixed vbox column": any(c["vbox_mixed"] for c in cs),
            "every combination of the lambert flags": len(lam) == 16,
            "no light, and three or more": any(c["n_lights"] == 0 for c in cs) and any(c["n_lights"] >= 3 for c in cs),
            "every light kind": {k for c in cs for k in c["light_kinds"]} >= {L.XZ, L.SPHERE, L.DEFAULT}}
