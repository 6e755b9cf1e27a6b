"""Shared by test_hit_static.py (CPU) and test_hit_static_gpu.py: what a scene's generated kernel unit (Scene.kernel_source: the
library's own text) says about the wrapper above every node and about the kind word of every leaf's material (Topo::wrap,
Topo::mat_kind; rt_core.h: RtHitShape), and small hand-built scenes, each named for the branch of the static hit record it pins.

Every scene function takes `omit`: None builds the scene, k builds it without its k-th pinned object (PINNED[name] says how many it
has).  A scene whose pinned object no ray reaches would prove nothing: test_hit_static.py renders both and wants different frames."""
import re

import lambert_scenes as L

NONE = 0xFFFFFFFF
SPHERE, MSPHERE, XY, XZ, YZ, TRANSLATE, ROTATE_Y, FLIP, MEDIUM = 2, 3, 4, 5, 6, 7, 8, 9, 10
NEW_MEMBERS = ("wrap", "mat_kind")
MAX_CHAINS = 8   # rt_core.h: RT_HIT_MAX_CHAINS


def _table(src, name):
    m = re.search(r"constexpr uint32_t " + name + r"\[(\d+)\] = \{([^}]*)\};", src)
    vals = [int(x) for x in re.findall(r"(\d+)u", m.group(2))]
    assert int(m.group(1)) == len(vals)
    return vals


def tables(sc):
    """(wrap, mat_kind) as the generated unit declares them"""
    src = sc.kernel_source()
    return _table(src, "wrap"), _table(src, "mat_kind")


def members_text(sc, f32=False):
    """the lines of the new members in the generated unit"""
    src = sc.kernel_source(f32=f32)
    return src[src.index("    static constexpr uint32_t wrap["):src.index("    static constexpr uint32_t n_lights")]


def strip_new_members(topo):
    """a Topo as the library generated it before it knew wrappers and material kinds: the lines of the new members taken out"""
    lines = [ln for ln in topo.splitlines(keepends=True) if not any(("constexpr uint32_t " + m + "[") in ln for m in NEW_MEMBERS)]
    out = "".join(lines)
    assert "wrap[" not in out and "mat_kind[" not in out and "reuse[" in out and "light_kind[" in out
    return out


def chains(nodes, wrap):
    """the distinct wrapper chains (outermost first) above the leaves and media of the scene, in the order of their first leaf"""
    out = []
    for i, k in enumerate(int(x) & 0xFF for x in nodes['kind']):
        if not (SPHERE <= k <= YZ or k == MEDIUM):
            continue
        c, w = [], wrap[i]
        while w != NONE:
            c.insert(0, w)
            w = wrap[w]
        if c and tuple(c) not in out:
            out.append(tuple(c))
    return out


def _build(s, objects, pinned, omit):
    keep = [make for k, make in enumerate(pinned) if k != omit]
    return L._finish(s, objects + [make() for make in keep], [lambda: L._xz_light(s)])


def _box(s, size, mat, angle, offset):
    return s.translate(s.rotate_y(s.aabox((0.0, 0.0, 0.0), size, mat), angle), offset)


def two_chains(rt, omit=None, variant=False):
    """two boxes under Translate(RotateY) with different angles next to plain walls: two chains, each with a block of its own, and
    the unwrapped leaves beside them.  `variant`: other angles, offsets and colours, the same topology"""
    s = rt.Scene(build_seed=1)
    d = 0.05 if variant else 0.0
    pinned = [lambda: _box(s, (1.0, 1.6 + d, 1.0), s.metal((0.8, 0.85 - d, 0.88), 0.0), 18.0 + 40 * d, (0.5 + d, 0.0, 1.2)),
              lambda: _box(s, (1.1, 1.0, 1.1 + d), L._lam(s, (0.8 - d, 0.7, 0.2)), -22.0 - 40 * d, (2.3, 0.0, 1.9 - d))]
    return _build(s, L._corner(s), pinned, omit)


def translate_only_rotate_only(rt, omit=None):
    """one rect under a bare Translate and one under a bare RotateY: chains of one wrapper, of either kind"""
    s = rt.Scene(build_seed=1)
    pinned = [lambda: s.translate(s.xy_rect(0.0, 1.3, 0.0, 1.3, 0.0, L._lam(s, (0.8, 0.7, 0.2))), (0.4, 0.3, 1.6)),
              lambda: s.rotate_y(s.xy_rect(2.0, 3.4, 0.3, 1.7, 2.0, s.metal((0.9, 0.6, 0.5), 0.1)), 15.0)]
    return _build(s, L._corner(s), pinned, omit)


def depth_three(rt, omit=None):
    """a rect under Translate(RotateY(Translate)): three nested wrappers, the deepest the flattener allows"""
    s = rt.Scene(build_seed=1)
    rect = lambda: s.yz_rect(0.0, 1.6, -0.8, 0.8, 0.0, L._lam(s, (0.3, 0.4, 0.8)))
    pinned = [lambda: s.translate(s.rotate_y(s.translate(rect(), (0.2, 0.1, 0.0)), 40.0), (1.8, 0.2, 1.8))]
    return _build(s, L._corner(s), pinned, omit)


def flip_above_bvh(rt, omit=None):
    """a FlipFace over a BVH of two emitting XZ rects (the wrapper stays a node: an RT_FLIP in the chain) beside an emitting rect
    flipped directly (folded into the leaf).  A DiffuseLight emits from its front face only: seen from below, these emit because
    they are flipped"""
    s = rt.Scene(build_seed=1)
    pinned = [lambda: s.flip_face(s.bvh_node([s.xz_rect(0.3, 1.2, 0.5, 1.5, 3.0, L._emit(s, 2.0)), s.xz_rect(1.5, 2.3, 0.5, 1.5, 3.1, L._emit(s, 3.0))])),
              lambda: s.flip_face(s.xz_rect(2.7, 3.6, 0.5, 1.5, 2.9, L._emit(s, 4.0)))]
    return _build(s, L._corner(s), pinned, omit)


def sphere_under_wrappers(rt, omit=None):
    """a sphere and a moving sphere below Translate(RotateY): their records are read, and their normals turned on the way out"""
    s = rt.Scene(build_seed=1)
    pinned = [lambda: s.translate(s.rotate_y(s.sphere((0.0, 0.0, 0.0), 0.7, s.dielectric(1.5)), 30.0), (1.0, 0.8, 2.2)),
              lambda: s.translate(s.rotate_y(s.moving_sphere((0.0, 0.0, 0.0), (0.2, 0.3, 0.0), 0.0, 1.0, 0.6, L._lam(s, (0.8, 0.3, 0.3))), -35.0), (2.8, 0.7, 1.6))]
    return _build(s, L._corner(s), pinned, omit)


N_MANY = 10


def many_chains(rt, omit=None):
    """ten wrapped boxes, each with an angle of its own: more chains than get a block (the leaves of the others walk their chain at
    run time) and more than 64 nodes (set tests by mask words)"""
    s = rt.Scene(build_seed=1)
    mats = [lambda k=k: (s.metal((0.9, 0.5 + 0.04 * k, 0.4), 0.05) if k % 3 == 0 else L._lam(s, (0.2 + 0.07 * k, 0.8 - 0.06 * k, 0.5))) for k in range(N_MANY)]
    pinned = [lambda k=k: _box(s, (0.5, 0.5 + 0.1 * (k % 3), 0.5), mats[k](), 8.0 * k - 30.0, (0.25 + 0.75 * (k % 5), 0.0, 2.6 - 1.3 * (k // 5)))
              for k in range(N_MANY)]
    return _build(s, L._corner(s), pinned, omit)


HAND_BUILT = (two_chains, translate_only_rotate_only, depth_three, flip_above_bvh, sphere_under_wrappers, many_chains)
PINNED = {"two_chains": 2, "translate_only_rotate_only": 2, "depth_three": 1, "flip_above_bvh": 2, "sphere_under_wrappers": 2, "many_chains": N_MANY}
