"""Shared by test_box_free.py (CPU) and test_box_free_gpu.py: the scenes whose specialised unit sweeps without box tests (rt_core.h:
rt_sweep_free), what their generated unit declares about it (Topo::vbox, Topo::box_free), and the same answered by an independent walk
of the flat nodes."""
import re

import numpy as np

import hit_scenes as H
import lambert_scenes as L
import slab_scenes as S

NONE = 0xFFFFFFFF
SPACES = 4      # rt_box_free.h: RT_VBOX_SPACES
MAX_NODES = 64  # rt_box_free.h: RT_BOX_FREE_MAX_NODES


def cornell(rt):
    return rt.Scene.reference(5, build_seed=1)


def arm4(rt):
    return rt.Scene.reference(4, build_seed=1)


def coplanar_pair(rt):
    """two XY rects in one plane that overlap in 1 <= x <= 2, in different subtrees of the BVH, and one more behind them: a ray through
    the overlap meets two leaves at equal t, and the later one in sweep order keeps the hit"""
    s = rt.Scene(build_seed=1)
    a = s.bvh_node([s.xy_rect(0.0, 2.0, 0.0, 2.0, 1.0, L._lam(s, (0.8, 0.2, 0.2))), s.sphere((-1.5, 1.0, 1.0), 0.5, L._lam(s, (0.5, 0.5, 0.5)))])
    b = s.bvh_node([s.xy_rect(1.0, 3.0, 0.0, 2.0, 1.0, L._lam(s, (0.2, 0.8, 0.2))), s.xy_rect(0.0, 3.0, 0.0, 2.0, 0.0, L._lam(s, (0.2, 0.2, 0.8)))])
    return S._finish(s, s.bvh_node([a, b]), look_from=(1.5, 1.0, 6.0), look_at=(1.5, 1.0, 0.0))


CANDIDATES = (cornell, arm4, coplanar_pair) + tuple(H.HAND_BUILT) + tuple(S.HAND_BUILT)


def has_rect(nodes):
    return any(H.XY <= k <= H.YZ for k in S.kinds(nodes))


def expected_box_free(sc):
    """the issue's conditions, from the flat nodes: no medium, a rect, at most 64 nodes"""
    nodes = S.nodes_of(sc)
    return not sc.info()["has_media"] and has_rect(nodes) and len(nodes) <= MAX_NODES


def declared(sc):
    """(vbox rows, box_free) of the generated unit"""
    src = sc.kernel_source()
    m = re.search(r"constexpr uint32_t vbox\[(\d+)\]\[(\d+)\] = \{(.*?)\};\n", src)
    rows = [[int(x) for x in re.findall(r"(\d+)u", r)] for r in re.findall(r"\{([^{}]*)\}", m.group(3))]
    assert len(rows) == int(m.group(1)) and all(len(r) == int(m.group(2)) == SPACES for r in rows)
    flag = re.search(r"constexpr bool box_free = (true|false);", src).group(1) == "true"
    return rows, flag


def scenes(rt):
    """name -> scene, for every candidate whose unit sweeps without boxes"""
    out = {}
    for f in CANDIDATES:
        sc = f(rt)
        if expected_box_free(sc):
            out[f.__name__] = sc
    return out


def vbox_by_descent(nodes, root):
    """Topo::vbox from the top: go down the tree carrying, per ray space entered so far, the innermost BVH node passed in it"""
    k, skip = S.kinds(nodes), [int(x) for x in nodes['skip']]
    rows = [[NONE] * SPACES for _ in nodes]

    def walk(i, end, boxes):
        while i < end:
            if k[i] <= S.BVH1:
                walk(i + 1, skip[i], boxes[:-1] + [i])
                i = skip[i]
            elif k[i] == S.FLIP:
                walk(i + 1, skip[i], boxes)
                i = skip[i]
            elif k[i] in (S.TRANSLATE, S.ROTATE_Y):
                walk(i + 1, skip[i], boxes + [NONE])
                i = skip[i]
            else:
                assert H.SPHERE <= k[i] <= H.YZ, (i, k[i])
                rows[i] = (boxes + [NONE] * SPACES)[:SPACES]
                i += 1

    walk(root, skip[root], [NONE])
    return rows


def to_world(nodes, wrap, leaf, p):
    """points `p` (n, 3) of the leaf's own space in world space: out through its wrappers, innermost first"""
    p = np.array(p, dtype=np.float64)
    w = wrap[leaf]
    while w != NONE:
        kind, d = int(nodes['kind'][w]) & 0xFF, nodes['d'][w]
        if kind == S.TRANSLATE:
            p = p + d[:3]
        elif kind == S.ROTATE_Y:
            sn, cs = d[0], d[1]
            p = np.stack([cs * p[:, 0] + sn * p[:, 2], p[:, 1], -sn * p[:, 0] + cs * p[:, 2]], axis=1)
        w = wrap[w]
    return p


def rect_points(nd, kind, u, v):
    """points of a rect leaf at parameters u, v in [0, 1] (arrays), in the leaf's own space"""
    d = nd['d']
    b = d[0] + u * (d[1] - d[0])
    c = d[2] + v * (d[3] - d[2])
    b, c = np.minimum(np.maximum(b, d[0]), d[1]), np.minimum(np.maximum(c, d[2]), d[3])
    k = np.full_like(b, d[4])
    return np.stack({H.XY: [b, c, k], H.XZ: [b, k, c], H.YZ: [k, b, c]}[kind], axis=1)


def world_bounds(nodes, root):
    """a box around everything: the root's own if it is a BVH node, else the hull of what the leaves say about themselves"""
    if (int(nodes['kind'][root]) & 0xFF) <= S.BVH1:
        d = nodes['d'][root]
        return d[:3].copy(), d[3:6].copy()
    return np.array([-1.0, -1.0, -1.0]), np.array([4.0, 4.0, 4.0])
