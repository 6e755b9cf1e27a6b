"""Ray sets of tests/test_query_oracle.py and tests/test_query_oracle_gpu.py: the rays rt1w_hit and rt1w_ray_color exist for -- rays
from anywhere into anywhere with windows of every kind, rays that leave a surface or run inside an object, axis-parallel rays on slab
planes, roots on the window's ends, degenerate rays -- on the reference arms, the hand-built scenes and eight random graphs.  Seeded;
nothing of csrc/ is in the formulas.  Every count a set is judged by comes from the literal oracle's output (orc.OracleScene.hit,
.ray_color, .census, .planes); the product's node table (hit_reference.nodes_of) is read only to point some rays at things: the slab
planes and rect planes of the axis-parallel set, and the leaves half of the generic rays are aimed at.  Test infrastructure.

Why half of the generic rays are aimed.  Origins are uniform in the world's root box scaled by 1.5 and directions uniform on the
sphere.  In random_scene and final_scene that box is set by a sphere of radius 1000 or 5000 while the glass spheres have radius 0.2 to
70: no uniform ray ever meets one, and the continuation rays, which start from the generic set's hits, could not start inside glass.
And in the sparse random graphs fewer than 20 % of uniform rays hit anything once the windows cut, which the set's own condition
asks for.  So the second half keeps its uniform origin and points at a leaf drawn uniformly by material and then by leaf (a point
within half its radius of its centre, in the leaf's own space).  What the rays then hit is still only what the oracle says."""
import json
import os

import numpy as np

import aov_scenes
import hit_reference as HR
import orc
from dual import Dual, random_scene_pair

INF = float("inf")
N_GENERIC, N_CONTINUATION, N_AXIS, N_DEGENERATE = 768, 768, 512, 120   # each at most 1024
PER_CLASS = 128          # continuation rays drawn from the hits on glass spheres, in media and on wrapped boxes, each, where there are any
ARMS = (0, 5, 6, 7)
N_GRAPHS = 8
FIRST_STREAM = 4000      # ray r draws from the stream of pixel seed FIRST_STREAM + r
CENSUS_PATH = os.path.join(orc.ROOT, "tests", "golden", "query_oracle_census.json")
HIT_SETS = ("generic", "continuation", "axis_parallel", "degenerate")
RADIANCE_SETS = ("generic", "continuation", "axis_parallel")
# The numpy seed of each scene's sets.  1 unless the sets of seed 1 missed a condition of check_conditions(); then the next seed that
# meets them all, found with the oracle alone (find_seed) before any product code saw the rays.  A seed that meets a tie between twin and
# oracle is replaced here too, and the tie recorded in the census file.
SEEDS = {"arm7": 3, "graph7": 7}
RTOL = 1e-12               # the project's bound for product against literal (test_hit.py, test_ray_color.py)
PAIRS = [(0, 0), (7, 2)]   # (sample, global_seed) of the hit comparisons
SAMPLES = (0, 7)           # of the radiance comparisons
DEPTHS = (1, 2, 50)


# ---------------------------------------------------------------------------------------------------------------- scenes --

def exact_scene():
    """Dyadic coordinates, no RotateY: nested BVHs (one of a single sphere), a Translate, a FlipFace, a box and a medium boundary, strung along x so that every
    case of exact_window() meets one object.  Every root below is a small integer and every intermediate of it is exact, whether a
    formulation divides or multiplies by a reciprocal, takes -half_b - sqrtd first or last."""
    d = Dual(21)
    img = d.lambertian(d.image(aov_scenes.synthetic_image()))
    grey = d.lambertian(d.solid((0.5, 0.5, 0.5)))
    spheres = d.bvh([d.sphere((0.0, 0.0, 0.0), 5.0, img), d.moving_sphere((20.0, 0.0, 0.0), (24.0, 0.0, 0.0), 0.0, 1.0, 5.0, grey)])
    rects = d.bvh([d.rect(0, 38.0, 42.0, -2.0, 2.0, -2.0, img), d.rect(1, 48.0, 52.0, -2.0, 2.0, 1.0, img), d.rect(2, -2.0, 2.0, -2.0, 2.0, 60.0, grey)])
    hs = [spheres, rects,
          d.translate(d.sphere((0.0, 0.0, 0.0), 5.0, d.metal((0.8, 0.8, 0.8), 0.0)), (80.0, 0.0, 0.0)),
          d.flip_face(d.rect(1, 98.0, 102.0, -2.0, 2.0, 1.0, d.diffuse_light(d.solid((4.0, 4.0, 4.0))))),
          d.aabox((110.0, 0.0, 0.0), (114.0, 4.0, 4.0), grey),
          d.constant_medium(d.sphere((130.0, 0.0, 0.0), 5.0, d.dielectric(1.5)), 0.5, d.solid((0.9, 0.9, 0.9))),
          d.bvh([d.sphere((150.0, 0.0, 0.0), 5.0, grey)])]   # alone in a BVH node: the node's box is the sphere's
    return d.finish(d.bvh(hs), [], (0.25, 0.5, 0.75), ((65.0, 0.0, -200.0), (65.0, 0.0, 0.0), aov_scenes.UP, 40.0, 1.5, 0.0, 10.0, 0.0, 1.0))


# (what, origin, direction, time, the roots along the ray in order)
EXACT_CASES = [
    ("sphere", (3.0, 0.0, -8.0), (0.0, 0.0, 1.0), 0.0, (4.0, 12.0)),           # 3-4-5: disc = 64 - 48 = 16
    ("sphere, |d| = 2", (3.0, 0.0, -8.0), (0.0, 0.0, 2.0), 0.0, (2.0, 6.0)),   # a = 4, half_b = -16, disc = 64
    ("moving sphere", (25.0, 0.0, -8.0), (0.0, 0.0, 1.0), 0.5, (4.0, 12.0)),   # centre (22, 0, 0) at time 0.5
    ("moving sphere, time 0.25", (24.0, 0.0, -8.0), (0.0, 0.0, 1.0), 0.25, (4.0, 12.0)),
    ("xy rect", (40.0, 0.0, 1.0), (0.0, 0.0, -1.5), 0.0, (2.0,)),
    ("xy rect, oblique", (39.5, 0.0, 2.0), (0.25, 0.0, -1.0), 0.0, (4.0,)),
    ("xz rect", (50.0, 9.0, 0.0), (0.0, -2.0, 0.0), 0.0, (4.0,)),
    ("yz rect", (56.0, 0.0, -4.0), (0.5, 0.0, 0.5), 0.0, (8.0,)),                # oblique: it passes the objects further along x
    ("sphere under Translate", (83.0, 0.0, -8.0), (0.0, 0.0, 1.0), 0.0, (4.0, 12.0)),
    ("xz rect under FlipFace", (100.0, 9.0, 0.0), (0.0, -2.0, 0.0), 0.0, (4.0,)),
    ("box", (112.0, 2.0, -3.0), (0.0, 0.0, 1.0), 0.0, (3.0, 7.0)),              # the faces z = 0 and z = 4
    ("box, oblique", (111.0, 1.0, -2.0), (0.25, 0.5, 1.0), 0.0, (2.0, 6.0)),
    ("medium boundary", (133.0, 0.0, -8.0), (0.0, 0.0, 1.0), 0.0, (4.0, 12.0)),
    ("sphere alone in a BVH node, through its centre", (150.0, 0.0, -8.0), (0.0, 0.0, 1.0), 0.0, (3.0, 13.0)),  # the roots are the box's slabs
]


def exact_window():
    """[n, 9] and a label per ray: for every root R of every case the windows [R, inf), (R + ulp, inf), (R - ulp, inf), (0.001, R],
    (0.001, R + ulp), (0.001, R - ulp); for a second root the same with t_min halfway between the roots."""
    rows, labels = [], []
    for what, o, d, time, roots in EXACT_CASES:
        for k, r in enumerate(roots):
            up, down = float(np.nextafter(r, INF)), float(np.nextafter(r, 0.0))
            lows = [0.001] + ([0.5 * (roots[k - 1] + r)] if k else [])
            windows = [(r, INF), (up, INF), (down, INF)] + [(lo, hi) for lo in lows for hi in (r, up, down)]
            for t_min, t_max in windows:
                rows.append([*o, *d, time, t_min, t_max])
                labels.append((what, r, t_min, t_max))
    return np.array(rows, dtype=np.float64), labels


_GRAPHS = None
FEATURES = ("media", "translates", "rotates", "flips", "moving_spheres")


def graph_seeds():
    """aov_scenes.random_graph_seeds's six, extended by the next seeds (at most 64 nodes) to N_GRAPHS so that media, each of the three
    wrapper kinds and moving spheres occur in at least two graphs each: a further seed is taken if it holds a feature still short,
    or if none is short."""
    global _GRAPHS
    if _GRAPHS is None:
        seeds, count = [], dict.fromkeys(FEATURES, 0)

        def add(seed, census):
            seeds.append(seed)
            for f in FEATURES:
                count[f] += census[f] > 0
        base = aov_scenes.random_graph_seeds(6)
        for s in base:
            add(s, random_scene_pair(s)[1].census()[0])
        seed = base[-1] + 1
        while len(seeds) < N_GRAPHS:
            prod, orac = random_scene_pair(seed)
            if prod.info()["n_nodes"] <= 64:
                census = orac.census()[0]
                short = [f for f in FEATURES if count[f] < 2]
                if not short or any(census[f] > 0 for f in short):
                    add(seed, census)
            seed += 1
        assert all(count[f] >= 2 for f in FEATURES), count
        _GRAPHS = seeds
    return _GRAPHS


def scene_names():
    return [f"arm{a}" for a in ARMS] + list(aov_scenes.HAND_BUILT) + [f"graph{k}" for k in range(N_GRAPHS)]


_PAIRS = {}


def scene_pair(name):
    """(product scene, oracle scene); the oracle of a scene built through Dual carries material_of and isotropic_of"""
    if name not in _PAIRS:
        if name == "exact":
            _PAIRS[name] = exact_scene()
        elif name.startswith("graph"):
            _PAIRS[name] = random_scene_pair(graph_seeds()[int(name[5:])])
        else:
            _PAIRS[name] = aov_scenes.scene_pair(name)
    return _PAIRS[name]


# ---------------------------------------------------------------------------------------------------------------- the sets --

def _unit(g, n):
    """n directions uniform on the sphere: the first n of 4 n points of the cube that lie in the unit ball (and outside a tenth of it),
    normalised.  Like everything here it takes +, *, / and sqrt only, which IEEE 754 rounds correctly: the sets are the same doubles on
    every machine, whatever its libm or numpy's vector paths make of exp, log or pow."""
    v = g.uniform(-1.0, 1.0, size=(4 * n, 3))
    m = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    v, m = v[(m <= 1.0) & (m > 0.01)][:n], m[(m <= 1.0) & (m > 0.01)][:n]
    assert len(v) == n
    return v / np.sqrt(m)[:, None]


def _octaves(g, lo, hi, n):
    """log-uniform by octaves over [2^lo, 2^hi): an integer exponent and a mantissa uniform in [1, 2), exactly"""
    return np.ldexp(g.uniform(1.0, 2.0, size=n), g.integers(lo, hi, size=n))


def _origins(g, lo, hi, n):
    """uniform in the box [lo, hi] scaled by 1.5 about its centre"""
    return 0.5 * (lo + hi) + g.uniform(-1.0, 1.0, size=(n, 3)) * (0.75 * (hi - lo))


def _leaf_targets(prod):
    """(points [m, 4] = centre and a radius, material id [m]) of the product's leaf records, in the leaf's own space"""
    nd = HR.nodes_of(prod)
    kind = nd["kind"] & 0xFF
    pts, mats = [], []
    for n in nd[(kind >= HR.SPHERE) & (kind <= HR.YZ)]:
        k, d = int(n["kind"] & 0xFF), n["d"]
        if k == HR.SPHERE:
            c, r = d[:3], abs(d[3])
        elif k == HR.MSPHERE:
            c, r = 0.5 * (d[:3] + d[3:]), abs(n["e"][2])
        else:
            fixed = {HR.XY: 2, HR.XZ: 1, HR.YZ: 0}[k]
            ab = [a for a in range(3) if a != fixed]
            c = np.zeros(3)
            c[fixed], c[ab[0]], c[ab[1]] = d[4], 0.5 * (d[0] + d[1]), 0.5 * (d[2] + d[3])
            r = 0.5 * min(d[1] - d[0], d[3] - d[2])
        pts.append([c[0], c[1], c[2], r])
        mats.append(int(n["mat"] & 0xFFFF))
    return np.array(pts), np.array(mats)


def _rays(o, d, time, t_min=0.001, t_max=INF):
    n = len(o)
    return np.ascontiguousarray(np.column_stack([o, d, time, np.broadcast_to(t_min, (n,)), np.broadcast_to(t_max, (n,))]), dtype=np.float64)


def generic(g, prod, orac):
    """Origins uniform in the root box scaled by 1.5; directions uniform on the sphere (the second half aimed, see the module's text)
    times a length log-uniform by octaves in [2^-10, 2^10) (1e-3 .. 1e3); time uniform in [-0.5, 1.5].  Ray r has the window (0.001, inf) if r % 3 == 0; a drawn
    t_min if r % 3 == 1: a distance of the set's own hits at (0.001, inf), times a factor in [0.2, 1.2], in units of the direction; a
    finite t_max if r % 3 == 2: for half of the rays that hit, a part in [0.25, 1) of their own t, which cuts the hit; for the others
    a distance of the set's own hits times a factor in [0.5, 1.5].  Returns (rays, the oracle's records at (0.001, inf))."""
    n = N_GENERIC
    lo, hi = orac.census()[1]
    o, d = _origins(g, lo, hi, n), _unit(g, n)
    pts, mats = _leaf_targets(prod)
    first = n - n // 2
    ids = np.unique(mats)
    for r in range(first, n):
        cand = np.flatnonzero(mats == g.choice(ids))
        p = pts[g.choice(cand)]
        to = p[:3] + g.uniform(-0.5, 0.5, size=3) * p[3] - o[r]
        m = to[0] * to[0] + to[1] * to[1] + to[2] * to[2]
        if m > 0.0:
            d[r] = to / np.sqrt(m)
    length = _octaves(g, -10, 10, n)
    d = d * length[:, None]
    rays = _rays(o, d, g.uniform(-0.5, 1.5, size=n))
    probe = orac.hit(rays, FIRST_STREAM)[0]
    hit = probe[:, 0] == 1.0
    pool = probe[hit, 1] * length[hit] if hit.any() else np.ones(1)
    draws = g.choice(pool, size=n), g.uniform(0.0, 1.0, size=n), g.uniform(0.0, 1.0, size=n)
    for r in range(n):
        if r % 3 == 1:
            rays[r, 7] = draws[0][r] * (0.2 + draws[1][r]) / length[r]
        elif r % 3 == 2:
            own = hit[r] and draws[2][r] < 0.5
            rays[r, 8] = probe[r, 1] * (0.25 + 0.749 * draws[1][r]) if own else draws[0][r] * (0.5 + draws[1][r]) / length[r]
    return rays, probe


def _classes(aux):
    tag = aux[:, 0]
    glass = (aux[:, 2] == orc.MAT_DIELECTRIC) & ((tag & orc.LEAF_MASK) == orc.LEAF_SPHERE)
    medium = (tag & orc.LEAF_MASK) == orc.LEAF_MEDIUM
    wbox = ((tag & orc.TAG_BOX) != 0) & ((tag & (orc.TAG_TRANSLATE | orc.TAG_ROTATE)) != 0)
    return glass, medium, wbox


def continuation(g, rec, aux):
    """From hit points of the generic set (`rec`, `aux`: the oracle's records of it): origin p, direction -normal (even rays: on through
    the surface, into the object the generic ray met from outside) or +normal (odd rays: back) plus a numpy vector shorter than 0.86,
    so the sign decides the side; window (0.001, inf).  PER_CLASS rays each start from the hits on glass spheres, in media and on boxes
    under a Translate / RotateY, where the set has such hits; the others from hits drawn uniformly.  Returns (rays, the parents)."""
    n = N_CONTINUATION
    hit = rec[:, 0] == 1.0
    assert hit.any()
    parents = [g.choice(np.flatnonzero(hit & c), size=PER_CLASS) for c in _classes(aux) if (hit & c).any()]
    parents = np.concatenate(parents + [g.choice(np.flatnonzero(hit), size=n - PER_CLASS * len(parents))])
    sign = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    d = sign[:, None] * rec[parents, 5:8] + 0.55 * g.uniform(-0.9, 0.9, size=(n, 3))
    return _rays(rec[parents, 2:5], d, g.uniform(-0.5, 1.5, size=n)), parents


def _outside_wrappers(nd):
    """per node record: no Translate / RotateY above it (the chain of `b`)"""
    kind, up = nd["kind"] & 0xFF, nd["b"]
    out = np.ones(len(nd), dtype=bool)
    for i in range(len(nd)):
        s, steps = up[i], 0
        while s != HR.NO_NODE and s < len(nd) and steps < 16:
            out[i] &= kind[s] not in (HR.TRANSLATE, HR.ROTATE_Y)
            s, steps = up[s], steps + 1
    return out


def axis_parallel(g, prod, orac):
    """One or two direction components +0.0 or -0.0, the rest a uniform direction times a length log-uniform by octaves in [2^-7, 2^7).  The first
    half has a generic origin.  The second half lies in a plane: three in four in a face of a BVH node's box (the coordinate on a zero axis
    equals the slab plane, the other two are drawn inside the box: aabb.rs's 0 * inf), one in four in the plane of a rect (0 / 0 in
    aarect.rs) -- planes read from the product's node table, of records under no Translate / RotateY where there are such."""
    n = N_AXIS
    lo, hi = orac.census()[1]
    o = _origins(g, lo, hi, n)
    d = _unit(g, n) * _octaves(g, -7, 7, n)[:, None]
    nd = HR.nodes_of(prod)
    kind = nd["kind"] & 0xFF
    free = _outside_wrappers(nd)
    boxes = nd[(kind <= HR.BVH1) & free]
    boxes = boxes if len(boxes) else nd[kind <= HR.BVH1]
    rects = nd[(kind >= HR.XY) & (kind <= HR.YZ) & free]
    rects = rects if len(rects) else nd[(kind >= HR.XY) & (kind <= HR.YZ)]
    for r in range(n):
        zero = g.permutation(3)[:g.integers(1, 3)]
        if r >= n // 2:
            if r % 4 == 3 and len(rects):
                rc = rects[g.integers(0, len(rects))]
                fixed = {HR.XY: 2, HR.XZ: 1, HR.YZ: 0}[int(rc["kind"] & 0xFF)]
                ab = [a for a in range(3) if a != fixed]
                e = rc["d"]
                o[r, fixed], o[r, ab[0]], o[r, ab[1]] = e[4], g.uniform(e[0] - 1.0, e[1] + 1.0), g.uniform(e[2] - 1.0, e[3] + 1.0)
                zero = np.array([fixed])
            else:
                b = boxes[g.integers(0, len(boxes))]["d"]
                o[r] = g.uniform(b[:3], np.maximum(b[3:], b[:3]))
                a = zero[0]
                o[r, a] = b[a] if g.random() < 0.5 else b[3 + a]
        for a in zero:
            d[r, a] = 0.0 if g.random() < 0.5 else -0.0
    return _rays(o, d, g.uniform(-0.5, 1.5, size=n))


def degenerate(g, orac, rec):
    """rt1w_hit only, a fifth each: a zero direction (signs mixed); one denormal component beside zeros or ordinary components;
    t_min > t_max; t_min = +inf; a negative t_min, finite or -inf (what lies behind the origin is inside the window: a medium whose
    boundary the ray entered at a negative t clamps its entry to 0, constant_medium.rs:79-81).  Half of the origins are generic, half
    are hit points of the generic set -- on surfaces and inside media."""
    n = N_DEGENERATE
    lo, hi = orac.census()[1]
    o = _origins(g, lo, hi, n)
    pts = rec[rec[:, 0] == 1.0, 2:5]
    o[1::2] = pts[g.integers(0, len(pts), size=len(o[1::2]))]
    d = _unit(g, n) * _octaves(g, -3, 3, n)[:, None]
    rays = _rays(o, d, g.uniform(-0.5, 1.5, size=n))
    q = n // 5
    rays[:q, 3:6] = np.where(g.random(size=(q, 3)) < 0.5, 0.0, -0.0)
    rays[:q:3, 7] = 0.0
    for r in range(q, 2 * q):
        a = g.integers(0, 3)
        if r % 2:
            rays[r, 3:6] = 0.0
        rays[r, 3 + a] = g.choice([5e-324, -5e-324, 1e-310, -2.5e-308])
    rays[2 * q:3 * q, 7] = _octaves(g, -3, 10, q)
    rays[2 * q:3 * q, 8] = rays[2 * q:3 * q, 7] * g.uniform(0.0, 0.999, size=q)
    rays[3 * q:4 * q, 7] = INF
    rays[3 * q:4 * q:2, 8] = _octaves(g, -3, 10, len(rays[3 * q:4 * q:2]))
    rays[4 * q:, 7] = -_octaves(g, -7, 10, n - 4 * q)
    rays[4 * q::3, 7] = -INF
    return rays


# ---------------------------------------------------------------------------------------------------------------- census --

def _wrapped(aux):
    return (aux[:, 0] & (orc.TAG_TRANSLATE | orc.TAG_ROTATE)) != 0


def on_slab_plane(rays, planes):
    """per ray: on an axis whose direction component is zero the origin's coordinate is a slab plane of the oracle's own graph"""
    out = np.zeros(len(rays), dtype=bool)
    for a in range(3):
        out |= (rays[:, 3 + a] == 0.0) & np.isin(rays[:, a], np.fromiter(planes[a], dtype=np.float64, count=len(planes[a])))
    return out


class Sets:
    """The sets of one scene and their census, from the numpy seed and the oracle alone."""

    def __init__(self, name, seed=None):
        self.name = name
        self.seed = SEEDS.get(name, 1) if seed is None else seed
        prod, orac = scene_pair(name)
        g = np.random.default_rng([self.seed, sum(name.encode())])
        self.rays, self.oracle, self.census = {}, {}, {}
        self.rays["generic"], probe = generic(g, prod, orac)
        self.oracle["generic"] = orac.hit(self.rays["generic"], FIRST_STREAM)
        grec, _, gaux = self.oracle["generic"]
        self.rays["continuation"], self.parents = continuation(g, grec, gaux)
        self.rays["axis_parallel"] = axis_parallel(g, prod, orac)
        self.rays["degenerate"] = degenerate(g, orac, grec)
        for which in HIT_SETS[1:]:
            self.oracle[which] = orac.hit(self.rays[which], FIRST_STREAM)
        planes = orac.planes()
        third = np.arange(N_GENERIC) % 3 == 2
        cut = third & (probe[:, 0] == 1.0) & (grec[:, 0] == 0.0)
        crec, _, caux = self.oracle["continuation"]
        parent_aux = gaux[self.parents]
        glass, medium, wbox = _classes(parent_aux)
        # a ray starts inside a convex object if it leaves from a hit on it and meets the same object again (a ray that leaves outwards
        # never does); a hit in a medium lies inside the medium's boundary as it is, whichever way the ray leaves
        same = (crec[:, 0] == 1.0) & (caux[:, 1] == parent_aux[:, 1])
        inside = {"inside_glass": glass & same & ((caux[:, 0] & orc.LEAF_MASK) == orc.LEAF_SPHERE) & (caux[:, 2] == orc.MAT_DIELECTRIC),
                  "inside_medium": medium, "inside_wrapped_box": wbox & same & ((caux[:, 0] & orc.TAG_BOX) != 0)}
        for which in HIT_SETS:
            rec, _, aux = self.oracle[which]
            row = {"rays": len(rec), "hits": int(rec[:, 0].sum()), "hits_under_a_wrapper": int((_wrapped(aux) & (rec[:, 0] == 1.0)).sum()),
                   "inside_glass": 0, "inside_medium": 0, "inside_wrapped_box": 0, "window_cuts": 0,
                   "finite_t_max": int(np.isfinite(self.rays[which][:, 8]).sum()),
                   "slab_plane_rays": int(on_slab_plane(self.rays[which], planes).sum()), "nan_records": int(np.isnan(rec).any(axis=1).sum()), "segments": 0}
            if which == "continuation":
                row.update({k: int(v.sum()) for k, v in inside.items()})
            if which == "generic":
                row["window_cuts"] = int(cut.sum())
            if which in RADIANCE_SETS:
                row["segments"] = int(orac.ray_color(self.rays[which], None, FIRST_STREAM, 0, 0, 50)[1].sum())
            row["mean_segments"] = round(row["segments"] / row["rays"], 4)
            self.census[which] = row
        self.has = orac.census()[0]

    def check_conditions(self):
        """the conditions of the sets, from the oracle's output alone; returns the list of those missed"""
        c, missed = self.census, []
        gen = c["generic"]
        if not (0.2 * gen["rays"] <= gen["hits"] <= 0.8 * gen["rays"]):
            missed.append(("generic: at least 20 % hits and 20 % misses", gen["hits"], gen["rays"]))
        if gen["window_cuts"] < 0.1 * gen["finite_t_max"]:
            missed.append(("generic: 10 % of the finite-t_max rays are misses that hit at (0.001, inf)", gen["window_cuts"], gen["finite_t_max"]))
        for feature, key in (("glass_spheres", "inside_glass"), ("media", "inside_medium"), ("wrapped_boxes", "inside_wrapped_box")):
            if self.has[feature] and c["continuation"][key] < 30:
                missed.append((f"continuation: 30 rays {key}", c["continuation"][key]))
        if c["axis_parallel"]["slab_plane_rays"] < 50:
            missed.append(("axis-parallel: 50 rays on a slab plane", c["axis_parallel"]["slab_plane_rays"]))
        return missed


_SETS = {}


def sets(name):
    if name not in _SETS:
        _SETS[name] = Sets(name)
    return _SETS[name]


def find_seed(name, tries=20):
    """the first seed from 1 on whose sets meet every condition -- the oracle alone is consulted"""
    for seed in range(1, tries + 1):
        missed = Sets(name, seed).check_conditions()
        if not missed:
            return seed
        print(name, "seed", seed, "misses", missed)
    raise AssertionError(f"{name}: no seed of 1..{tries} meets the conditions")


def start_words(name, which, n):
    """a drawn start word in 0 .. 40 per ray"""
    return np.random.default_rng([7, sum(name.encode()), len(which)]).integers(0, 41, size=n).astype(np.uint32)


def census_document():
    """what tests/golden/query_oracle_census.json holds: one row per scene and set, the graphs' seeds, the exact-window set, and under
    "ties" the rays whose seed was replaced because twin and oracle agreed to 1e-12 and a comparison fell on opposite sides: none so far"""
    doc = {"graph_seeds": [int(s) for s in graph_seeds()], "set_seeds": {}, "scenes": {}, "ties": []}
    for name in scene_names():
        s = sets(name)
        missed = s.check_conditions()
        assert not missed, (name, missed)
        doc["set_seeds"][name] = s.seed
        doc["scenes"][name] = s.census
    rays, _ = exact_window()
    rec, _, aux = scene_pair("exact")[1].hit(rays, FIRST_STREAM)
    doc["exact_window"] = {"rays": len(rays), "hits": int(rec[:, 0].sum()), "hits_under_a_wrapper": int((_wrapped(aux) & (rec[:, 0] == 1.0)).sum())}
    return doc


def load_census():
    return json.load(open(CENSUS_PATH))


# ---------------------------------------------------------------------------------------------------------------- comparisons --

def _agree(got, want, tol):
    """per element: within tol, or both NaN, or the same infinity"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want))


def _first(bad):
    k = np.flatnonzero(bad)
    return (int(k[0]), int(len(k))) if len(k) else None


def check_hit(name, which, rays, got, node, want, wmat, waux, what, exact_t=False):
    """the records `got`, `node` of a product entry against the oracle's `want`, `wmat`, `waux` of the same rays: every ray"""
    prod, orac = scene_pair(name)
    tag = (name, which) + tuple(what)
    hit = want[:, 0] == 1.0
    assert np.array_equal(got[:, 0], want[:, 0]), tag + ("hit", _first(got[:, 0] != want[:, 0]))
    miss_ok = np.all(got[~hit].view(np.uint64) == 0, axis=1) & (node[~hit] == HR.NO_NODE)
    assert np.all(miss_ok), tag + ("a miss is zeros and no node", _first(~miss_ok))
    assert np.all(node[hit] != HR.NO_NODE), tag + ("a hit names its node",)
    g, w, r = got[hit], want[hit], rays[hit]
    assert np.array_equal(g[:, 10], w[:, 10]), tag + ("front_face", _first(g[:, 10] != w[:, 10]))
    with np.errstate(invalid="ignore", over="ignore"):
        ok_t = HR.same_bits(g[:, 1], w[:, 1]) if exact_t else np.all(_agree(g[:, 1], w[:, 1], RTOL * np.abs(w[:, 1])))
        assert ok_t, tag + ("t", _first(~_agree(g[:, 1], w[:, 1], 0.0 if exact_t else RTOL * np.abs(w[:, 1]))))
        wrapped = (waux[hit, 0] & (orc.TAG_TRANSLATE | orc.TAG_ROTATE)) != 0
        size = np.maximum(np.abs(w[:, 2:5]).max(axis=1), np.maximum(np.abs(r[:, 0:3]).max(axis=1), np.abs(w[:, 1:2] * r[:, 3:6]).max(axis=1)))
        finite = np.isfinite(w[:, 2:5]).all(axis=1)
        extent = max(1.0, float(np.abs(w[finite & wrapped, 2:5]).max())) if (finite & wrapped).any() else 1.0
        size = np.where(wrapped, np.maximum(extent, size), size)
        size = np.where(np.isfinite(size), size, 0.0)
        ok_p = _agree(g[:, 2:5], w[:, 2:5], RTOL * size[:, None])
    assert np.all(ok_p), tag + ("p", _first(~ok_p.all(axis=1)))
    ok_n = _agree(g[:, 5:8], w[:, 5:8], RTOL)
    assert np.all(ok_n), tag + ("normal", _first(~ok_n.all(axis=1)))
    reads = waux[hit, 3] == 1
    ok_uv = np.where(reads[:, None], _agree(g[:, 8:10], w[:, 8:10], RTOL), g[:, 8:10] == 0.0)
    assert np.all(ok_uv), tag + ("u, v: the oracle's where an image texture reads them, else 0", _first(~ok_uv.all(axis=1)))
    nodes = HR.nodes_of(prod)
    leaf = nodes["kind"][node[hit]] & 0xFF
    assert np.all((leaf >= HR.SPHERE) & (leaf <= HR.YZ) | (leaf == HR.MEDIUM)), tag + ("the node is a leaf's or a medium's record",)
    assert np.array_equal(g[:, 11], (nodes["mat"][node[hit]] & 0xFFFF).astype(np.float64)), tag + ("material id against the node table",)
    if hasattr(orac, "material_of"):  # built through Dual: the oracle's material, mapped to the id the product's constructor returned
        m, medium = wmat[hit], (waux[hit, 0] & orc.LEAF_MASK) == orc.LEAF_MEDIUM
        assert np.array_equal(m == -1, medium), tag + ("only a medium's Isotropic is a material the builder did not hand out",)
        expect = np.array([orac.isotropic_of[int(a[1])] if a[0] & orc.LEAF_MASK == orc.LEAF_MEDIUM else orac.material_of[int(k)] for k, a in zip(m, waux[hit])],
                          dtype=np.float64)
        assert np.array_equal(g[:, 11], expect), tag + ("material id against the oracle's material", _first(g[:, 11] != expect))
    return int(hit.sum())


def check_radiance(tag, got, got_segments, want, want_segments):
    bad_seg = got_segments != want_segments
    assert not bad_seg.any(), tag + ("segments per ray", _first(bad_seg), int(got_segments[bad_seg][0]), int(want_segments[bad_seg][0]))
    ok = _agree(got, want, RTOL * np.abs(want))
    k = _first(~ok.all(axis=1))
    assert k is None, tag + ("radiance", k, got[k[0]].tolist(), want[k[0]].tolist())
