"""Shared by test_slab_reuse.py (CPU) and test_slab_reuse_gpu.py: the reuse table of a scene's generated kernel unit
(Scene.kernel_source: the library's own text, not a re-implementation) and small hand-built scenes that put equal bounds
where the table may, and where it may not, take a slab product from a box above."""
import re

import numpy as np

NODE = np.dtype([('kind', '<u4'), ('skip', '<u4'), ('d', '<f8', 6), ('b', '<u4'), ('mat', '<u4'), ('e', '<f8', 3), ('a', '<u4'), ('pad', '<u4')])
BVH2, BVH1, TRANSLATE, ROTATE_Y, FLIP, MEDIUM = 0, 1, 7, 8, 9, 10


def nodes_of(sc):
    return np.frombuffer(sc.flat(0).tobytes(), dtype=NODE)


def root_of(sc):
    return int(np.frombuffer(sc.flat(6).tobytes()[-8:-4], dtype='<u4')[0])


def reuse_table(sc):
    src = sc.kernel_source()
    m = re.search(r"reuse\[(\d+)\]\[6\] = \{(.*)\};", src)
    rows = [[int(x) for x in re.findall(r"\d+", r)] for r in re.findall(r"\{([^}]*)\}", m.group(2))]
    assert len(rows) == int(m.group(1)) and all(len(r) == 6 for r in rows)
    return rows


def counts(table):
    """(entries that name another node, axes whose two planes name the same other node)"""
    other = sum(1 for i, r in enumerate(table) for x in r if x != i)
    pairs = sum(1 for i, r in enumerate(table) for a in range(3) if r[a] != i and r[a] == r[a + 3])
    return other, pairs


def kinds(nodes):
    return [int(k) & 0xFF for k in nodes['kind']]


def same_space_bvh_ancestors(nodes, root, i):
    """BVH nodes above i, nearest first, up to the first Translate / RotateY / ConstantMedium (FlipFace does not end the way)"""
    k = kinds(nodes)
    out = []
    for j in range(i - 1, root - 1, -1):
        if int(nodes['skip'][j]) <= i:
            continue
        if k[j] == FLIP:
            continue
        if k[j] > BVH1:
            break
        out.append(j)
    return out


def check_table(sc):
    """Every entry that names another node names a BVH node above it in the same ray space with the same 8 bytes; rows of other
    nodes name themselves.  Returns (table, nodes)."""
    nodes, root, table = nodes_of(sc), root_of(sc), reuse_table(sc)
    k = kinds(nodes)
    assert len(table) == len(nodes)
    for i, row in enumerate(table):
        up = same_space_bvh_ancestors(nodes, root, i) if i >= root else []
        for p, j in enumerate(row):
            if j == i:
                continue
            assert k[i] <= BVH1 and j in up, (i, p, j)
            assert nodes['d'][j][p].tobytes() == nodes['d'][i][p].tobytes(), (i, p, j)
    return table, nodes


def _finish(s, world, look_from=(0.5, 0.6, 6.0), look_at=(0.5, 0.5, 0.0), vfov=40.0):
    s.set_world(world)
    s.set_lights([])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera(look_from, look_at, (0, 1, 0), vfov, 1.0, 0.0, 6.0, 0.0, 1.0)
    s.commit()
    return s


def _grey(s):
    return s.lambertian(s.solid_color((0.6, 0.6, 0.6)))


def child_equals_parent(rt):
    """BVH1 over BVH1 over a sphere: the child's box is the parent's on all six planes"""
    s = rt.Scene(build_seed=1)
    inner = s.bvh_node([s.sphere((0.5, 0.5, 0.5), 0.5, s.metal((0.8, 0.8, 0.8), 0.0))])
    return _finish(s, s.bvh_node([s.bvh_node([inner]), s.sphere((2.0, 0.5, 0.5), 0.5, _grey(s))]))


def sibling_only(rt):
    """two one-sphere nodes with the same y and z bounds in different subtrees; the boxes above the second one are taller and deeper"""
    s = rt.Scene(build_seed=1)
    left = s.bvh_node([s.sphere((-2.0, 0.5, 0.5), 0.5, _grey(s))])
    b = s.bvh_node([s.sphere((0.5, 0.5, 0.5), 0.5, s.metal((0.7, 0.6, 0.5), 0.0))])
    c = s.bvh_node([s.sphere((3.0, 0.25, 0.25), 1.0, _grey(s))])
    return _finish(s, s.bvh_node([left, s.bvh_node([b, c])]))


def under_translate(rt):
    """a node below a Translate whose bounds are, as numbers, bounds of the box above the Translate"""
    s = rt.Scene(build_seed=1)
    inner = s.bvh_node([s.sphere((0.5, 0.5, 0.5), 0.5, s.dielectric(1.5))])
    return _finish(s, s.bvh_node([s.translate(inner, (1.0, 0.0, 0.0)), s.sphere((0.5, 0.5, 0.5), 0.5, _grey(s))]))


def under_flip(rt):
    """a BVH node below a FlipFace: the ray is the same, the box above the FlipFace is reused"""
    s = rt.Scene(build_seed=1)
    inner = s.bvh_node([s.sphere((0.0, 0.5, 0.5), 0.5, _grey(s)), s.sphere((1.0, 0.5, 0.5), 0.5, s.metal((0.8, 0.8, 0.8), 0.1))])
    return _finish(s, s.bvh_node([s.flip_face(inner)]))


def nan_best_t(rt):
    """vfov = 0: every camera ray is the same axis-parallel ray (0, 0, -f) from (0.5, 0.5, 5), lying IN the plane of an XZRect.  The
    rect's t = 0 / 0 is accepted (aarect.rs:84-94: no comparison with NaN is true), so the closest hit is NaN and the next box, `b`,
    is tested in the literal form.  Inside `b` the sphere `behind` (t = 12) is accepted against the NaN, and the box `c` after it is
    back in the fast form with both its x and y pairs taken from the frame the literal form left at `b`.  The spheres in `c` are
    in FRONT of `behind` (t = 7.5): if the literal form left that frame unfilled, `c` would be missed and the frame would show
    `behind`."""
    s = rt.Scene(build_seed=1)
    r = s.xz_rect(-0.5, 1.0, -10.0, -9.0, 0.5, _grey(s))
    behind = s.sphere((0.5, 0.5, -7.5), 0.5, s.metal((0.9, 0.3, 0.3), 0.0))
    c = s.bvh_node([s.sphere((0.5, 0.5, -4.0), 0.5, _grey(s)), s.sphere((0.5, 0.5, -3.0), 0.5, s.lambertian(s.solid_color((0.2, 0.8, 0.2))))])
    b = s.bvh_node([c, behind])
    return _finish(s, s.bvh_node([b, r]), look_from=(0.5, 0.5, 5.0), look_at=(0.5, 0.5, 0.0), vfov=0.0)


def nan_some_rays(rt):
    """A camera whose viewport is 1e-299 high and 0.7 wide (vfov and aspect_ratio chosen so): the rays are a fan in the plane y = 0.5
    exactly, spread in x.  The XZRect in that plane gives 0 / 0 to every ray that gets to test it -- the rays that pass the box of
    the left group -- and the others never see a NaN.  In a wave the lanes of the right group are then pulled into the literal form
    by a lane of the left group, and back out of it where that lane's sphere is accepted: boxes tested for real in either form
    over frames the other form filled."""
    s = rt.Scene(build_seed=1)
    left = s.bvh_node([s.sphere((-1.5, 0.5, -1.0), 0.5, s.metal((0.9, 0.9, 0.9), 0.0)), s.xz_rect(-2.0, -1.0, 0.0, 1.0, 0.5, _grey(s))])
    r1 = s.bvh_node([s.sphere((0.5, 0.5, -1.0), 0.5, _grey(s)), s.sphere((0.5, 0.5, 0.5), 0.5, s.lambertian(s.solid_color((0.2, 0.8, 0.2))))])
    r2 = s.bvh_node([s.sphere((2.0, 0.5, -1.0), 0.5, s.metal((0.8, 0.6, 0.2), 0.0)), s.sphere((2.0, 0.5, 0.5), 0.5, _grey(s))])
    right = s.bvh_node([s.bvh_node([r1]), r2])
    s.set_world(s.bvh_node([right, left]))
    s.set_lights([])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera((0.25, 0.5, 5.0), (0.25, 0.5, 0.0), (0, 1, 0), 1e-298, 4e299, 0.0, 6.0, 0.0, 1.0)
    s.commit()
    return s


HAND_BUILT = (child_equals_parent, sibling_only, under_translate, under_flip, nan_best_t, nan_some_rays)
