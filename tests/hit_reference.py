"""Helpers of tests/test_hit.py: the ray sets of the ray-query tests (camera rays with bounds, the fixed adversarial set), the reference's
hit formulas restated in numpy (sphere.rs:31-62, moving_sphere.rs:23-26, aarect.rs:46-72, hittable.rs:206-292), the first draw of a
Philox stream, and the comparisons.  Nothing of csrc/ is in the formulas.  Test infrastructure."""
import ctypes as C
import math

import numpy as np

import orc

RAY, RECORD = 9, 12
NO_NODE = 0xFFFFFFFF
INF = float("inf")
NODE = np.dtype([("kind", "<u4"), ("skip", "<u4"), ("d", "<f8", (6,)), ("b", "<u4"), ("mat", "<u4"), ("e", "<f8", (3,)), ("a", "<u4"), ("pad", "<u4")])
assert NODE.itemsize == 96
BVH2, BVH1, SPHERE, MSPHERE, XY, XZ, YZ, TRANSLATE, ROTATE_Y, FLIP, MEDIUM = range(11)


def valid_variants(info):
    """the kernel variants that cover a scene (csrc/rt_flat.h: rt_variant_valid)"""
    media, tex, ms, sd = info["has_media"], info["has_textures"], info["has_moving"], info["scope_depth"]
    v = [1, 3, 4]
    if not media and not tex and not ms and sd <= 2:
        v.append(0)
    if not media:
        v.append(2)
    if not media and sd == 0:
        v.append(5)
    return sorted(v)


def nodes_of(scene):
    """the flattened node array rt1w_scene_copy_flat(.., 0, ..) exports, as records"""
    return scene.flat(0).view(NODE)


def with_bounds(rays7, t_min=0.001, t_max=INF):
    r = np.ascontiguousarray(rays7, dtype=np.float64).reshape(-1, 7)
    return np.concatenate([r, np.full((len(r), 1), t_min), np.full((len(r), 1), t_max)], axis=1)


def camera_rays(rt, scene, w, h, spp, sample_offset=0, global_seed=0):
    """[h * w * spp, 9]: the camera rays of the frame (rt1w_lab_camera_rays_host) with the bounds of main.rs:62"""
    return with_bounds(rt.camera_rays_host(scene, w, h, spp, sample_offset=sample_offset, global_seed=global_seed).reshape(-1, 8)[:, :7])


def adversarial_rays(scene, max_nodes=24):
    """The fixed adversarial set of a scene, [n, 9], made from its own node records (the first max_nodes boxes and leaves) and nothing
    random: zero and denormal directions, huge magnitudes, t_min > t_max, t_max = +inf, origins exactly on surfaces and on box faces,
    rays along box edges and diagonals, and the non-finite rays the entry answers as misses."""
    nd = nodes_of(scene)
    kind = nd["kind"] & 0xFF
    boxes = nd[kind <= BVH1][:max_nodes]
    leaves = nd[(kind >= SPHERE) & (kind <= YZ)][:max_nodes]
    lo, hi = (boxes[0]["d"][:3], boxes[0]["d"][3:]) if len(boxes) else (np.full(3, -1.0), np.full(3, 1.0))
    c = 0.5 * (lo + hi)
    far = c + 3.0 * (hi - lo) + 1.0
    rows = []

    def add(o, d, t_min=0.001, t_max=INF, time=0.5):
        rows.append([o[0], o[1], o[2], d[0], d[1], d[2], time, t_min, t_max])
    tiny, sub = 5e-324, 1e-310
    for o in (c, far, lo):
        add(o, (0.0, 0.0, 0.0))
        add(o, (-0.0, 0.0, -0.0), 0.0)
        add(o, (tiny, 0.0, 0.0))
        add(o, (sub, -sub, 2.0 * sub))
        add(o, (0.0, -tiny, sub), -INF)
    unit = (c - far) / np.sqrt(np.sum((c - far) ** 2))
    for s in (1e150, 1e300, 1.7e308):
        add(far, unit * s)
        add(c + np.array([s, 0.0, 0.0]), (-s, 0.0, 0.0))
        add((s, s, -s), (-s, -s, s), 0.0)
        add(c, (s, 1.0, 1e-300))
    for t_min, t_max in ((5.0, 1.0), (INF, 0.0), (0.001, INF), (0.0, INF), (-INF, INF), (0.001, -INF), (1.0, 1.0), (-1.0, -0.5)):
        add(far, c - far, t_min, t_max)
        add(c, far - c, t_min, t_max)
    axes = np.eye(3)
    for n in leaves:
        k, d = int(n["kind"] & 0xFF), n["d"]
        if k in (SPHERE, MSPHERE):
            ctr, r = (d[:3], d[3]) if k == SPHERE else (0.5 * (d[:3] + d[3:]), n["e"][2])  # a MovingSphere at the middle of its shutter
            on = ctr + np.array([r, 0.0, 0.0])
            for dr in (axes[0], -axes[0], axes[1], axes[2], (1.0, 1.0, 0.0)):
                add(on, dr, 0.0)
                add(on, dr)
        else:
            fixed = {XY: 2, XZ: 1, YZ: 0}[k]
            ab = [a for a in range(3) if a != fixed]
            for u, v in ((0.5 * (d[0] + d[1]), 0.5 * (d[2] + d[3])), (d[0], d[2]), (d[1], d[3])):  # the middle and two corners, on the plane
                on = np.zeros(3)
                on[fixed], on[ab[0]], on[ab[1]] = d[4], u, v
                for dr in (axes[fixed], -axes[fixed], axes[ab[0]], axes[ab[1]], axes[ab[0]] + axes[ab[1]]):
                    add(on, dr, 0.0)
                    add(on, dr)
    for n in boxes:
        blo, bhi = n["d"][:3], n["d"][3:]
        mid = 0.5 * (blo + bhi)
        for a in range(3):
            face = mid.copy()
            face[a] = blo[a]
            add(face, axes[a], 0.0)            # from a face inwards, outwards and along it
            add(face, -axes[a], 0.0)
            add(face, axes[(a + 1) % 3])
            add(blo, axes[a], 0.0)             # along the three edges at the lower corner, and back along those at the upper one
            add(bhi, -axes[a])
            add(blo - axes[a], axes[a])        # the same edge's line, from outside
        add(blo, bhi - blo, 0.0)               # the diagonal, corner to corner
        add(bhi, blo - bhi)
    nan = float("nan")
    add((nan, 0.0, 0.0), c - far)              # answered as misses before any walk
    add(far, (0.0, INF, 0.0))
    add(far, (-INF, nan, 0.0))
    add((INF, 0.0, 0.0), c - far)
    add(far, c - far, time=nan)
    add(far, c - far, time=INF)
    add(far, c - far, t_min=nan)
    add(far, c - far, t_max=nan)
    add(far, c - far)                          # a plain ray last: a refused lane beside walking ones, and one after them
    return np.array(rows, dtype=np.float64)


def refused(rays):
    """the rays rt1w_hit answers as misses before any walk: a non-finite origin, direction or time, a NaN bound"""
    r = np.asarray(rays).reshape(-1, RAY)
    return ~np.all(np.isfinite(r[:, :7]), axis=1) | np.isnan(r[:, 7]) | np.isnan(r[:, 8])


def same_bits(a, b):
    """equal bit for bit; NaN against NaN counts as equal (the host's and the GPU's default NaN differ in the sign bit)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def checksum(records, nodes):
    """FNV-1a (64 bit) over the bytes of the records and then of the node indices: what tests/hit_driver.cpp prints"""
    h = 0xCBF29CE484222325
    for byte in np.ascontiguousarray(records, dtype=np.float64).tobytes() + np.ascontiguousarray(nodes, dtype=np.uint32).tobytes():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def first_f64(stream, sample=0, global_seed=0):
    """The first f64 draw of the stream of (pixel seed `stream`, sample, global_seed): block 0 of Philox4x32-10 with the key
    (seed low, seed high) and the counter (block, sample, global_seed, "REND"), words 0 and 1 as rand 0.8's Standard f64 takes them
    (tests/test_num_contract.py: test_word_stream_is_philox_blocks_in_order, test_draw_shapes)"""
    ctr = np.array([0, sample, global_seed, 0x52454E44], dtype=np.uint32)
    key = np.array([stream & 0xFFFFFFFF, stream >> 32], dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    orc.A.orc_philox(ctr.ctypes.data_as(C.c_void_p), key.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return float((int(out[1]) << 32 | int(out[0])) >> 11) * 2.0 ** -53


# ---- the reference's formulas, one ray at a time, in Python floats (IEEE doubles, no contraction) ----

def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _at(o, d, t):
    return [o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]]


def _record(t, p, outward, d, u=0.0, v=0.0):
    """HitRecord::new hittable.rs:21-46"""
    front = _dot(d, outward) < 0.0
    return {"t": t, "p": p, "n": list(outward) if front else [-x for x in outward], "u": u, "v": v, "front": front}


def sphere_hit(center, radius, o, d, t_min, t_max):
    """sphere.rs:31-62; None = no hit"""
    oc = [o[k] - center[k] for k in range(3)]
    a, half_b, c = _dot(d, d), _dot(oc, d), _dot(oc, oc) - radius * radius
    disc = half_b * half_b - a * c
    if disc < 0.0:
        return None
    sq = math.sqrt(disc)
    root = (-half_b - sq) / a
    if root < t_min or t_max < root:
        root = (-half_b + sq) / a
        if root < t_min or t_max < root:
            return None
    p = _at(o, d, root)
    out = [(p[k] - center[k]) / radius for k in range(3)]
    theta, phi = math.acos(-out[1]), math.atan2(-out[2], out[0]) + math.pi  # sphere_uv math.rs:67-71
    return _record(root, p, out, d, phi / (2.0 * math.pi), theta / math.pi)


def moving_center(c0, c1, t0, t1, time):
    """moving_sphere.rs:23-26"""
    f = (time - t0) / (t1 - t0)
    return [c0[k] + f * (c1[k] - c0[k]) for k in range(3)]


def rect_hit(axis, a0, a1, b0, b1, k, o, d, t_min, t_max):
    """aarect.rs:46-72 (axis 0 XYRect), :96-109 (1 XZRect), :164-177 (2 YZRect): the fixed axis z, y, x; (a, b) = (x, y), (x, z), (y, z)"""
    fixed, ia, ib = ((2, 0, 1), (1, 0, 2), (0, 1, 2))[axis]
    with np.errstate(all="ignore"):
        t = float(np.float64(k - o[fixed]) / np.float64(d[fixed]))  # IEEE division: a ray in the rect's plane gives an infinity or a NaN
    if t < t_min or t > t_max:
        return None
    a, b = o[ia] + t * d[ia], o[ib] + t * d[ib]
    if a < a0 or a > a1 or b < b0 or b > b1:
        return None
    out = [0.0, 0.0, 0.0]
    out[fixed] = 1.0
    return _record(t, _at(o, d, t), out, d, (a - a0) / (a1 - a0), (b - b0) / (b1 - b0))


def box_hit(p0, p1, o, d, t_min, t_max):
    """AABox aabox.rs:22-84: six rects, the closest hit (the list keeps the closest so far as t_max, hittable.rs:110-125)"""
    sides = [(0, p0[0], p1[0], p0[1], p1[1], p1[2]), (0, p0[0], p1[0], p0[1], p1[1], p0[2]),
             (1, p0[0], p1[0], p0[2], p1[2], p1[1]), (1, p0[0], p1[0], p0[2], p1[2], p0[1]),
             (2, p0[1], p1[1], p0[2], p1[2], p1[0]), (2, p0[1], p1[1], p0[2], p1[2], p0[0])]
    best = None
    for s in sides:
        h = rect_hit(*s, o, d, t_min, best["t"] if best else t_max)
        best = h or best
    return best


def translate_hit(offset, inner, o, d, t_min, t_max):
    """Translate::hit hittable.rs:206-226; inner(o, d, t_min, t_max) -> record"""
    moved = [o[k] - offset[k] for k in range(3)]
    h = inner(moved, d, t_min, t_max)
    return h and _record(h["t"], [h["p"][k] + offset[k] for k in range(3)], h["n"], d, h["u"], h["v"])


def rotate_y_ray(angle_deg, o, d):
    """the ray in a RotateY's space, hittable.rs:238-251; sin and cos of RotateY::new hittable.rs:158-161"""
    rad = math.radians(angle_deg)
    s, c = math.sin(rad), math.cos(rad)
    return [c * o[0] - s * o[2], o[1], s * o[0] + c * o[2]], [c * d[0] - s * d[2], d[1], s * d[0] + c * d[2]]


def rotate_y_hit(angle_deg, inner, o, d, t_min, t_max):
    """RotateY::hit hittable.rs:237-279"""
    rad = math.radians(angle_deg)
    s, c = math.sin(rad), math.cos(rad)
    ro, rd = rotate_y_ray(angle_deg, o, d)
    h = inner(ro, rd, t_min, t_max)
    if not h:
        return None
    p = [c * h["p"][0] + s * h["p"][2], h["p"][1], -s * h["p"][0] + c * h["p"][2]]
    n = [c * h["n"][0] + s * h["n"][2], h["n"][1], -s * h["n"][0] + c * h["n"][2]]
    return _record(h["t"], p, n, rd, h["u"], h["v"])


def flip_hit(inner, o, d, t_min, t_max):
    """FlipFace::hit hittable.rs:287-292: the flag only"""
    h = inner(o, d, t_min, t_max)
    return h and dict(h, front=not h["front"])
