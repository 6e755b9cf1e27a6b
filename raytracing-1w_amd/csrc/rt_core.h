/* rt_core.h -- the per-pixel sample loop and the iterative `ray_color`, over the
 * flattened scene (rt_flat.h).  This is the text the HIP kernel is built from.
 * It is also compiled for the host by oracle/oracle_flat.cpp, as TEST
 * infrastructure only (sanitizer builds, CPU-side checks of the flattener);
 * the shipped library has no CPU render path.
 *
 * Reference map (paths under /root/reference/src):
 *   rt_path_begin   main.rs:964-971 (seed, jitter, Camera::get_ray camera.rs:61-73)
 *   rt_path_step    main.rs:51-116 / :118-190, recursion unrolled into
 *                   L += beta*emitted ; beta *= att*spdf/pdf (or att)
 *   rt_traverse     bvh.rs:25-50 + aabb.rs:13-32 + every leaf `hit`
 *   rt_finish_hit   HitRecord::new hittable.rs:21-46 and the wrapper fix-ups
 *                   hittable.rs:206-226 (Translate), :237-279 (RotateY), :287-292 (FlipFace)
 *   rt_scatter...   material.rs, constant_medium.rs:36-51, pdf.rs, onb.rs, math.rs
 *   rt_texture      texture.rs:40-89, perlin.rs:46-106
 *
 * Traversal order is the reference's: depth first, left child before right,
 * with the running closest t as t_max (bvh.rs:38-47 is exactly that, because
 * the t_max handed to the right child is the left child's hit).  This matters
 * for results, not only speed: ConstantMedium::hit draws a random number
 * inside the traversal (constant_medium.rs:85) and ties in t go to the child
 * tested later.
 */
#ifndef RT1W_CORE_H
#define RT1W_CORE_H

#include <type_traits>
#include "rt_flat.h"

#define RT_POP_FLAG 0x80000000u
/* diagnostic build only (-DRT_STAMPS, never shipped): RT_STAMP(k) charges the wave's cycles
 * since the previous stamp to bucket k */
#ifndef RT_STAMP
#define RT_STAMP(k) ((void)0)
#endif
#ifndef RT_STAT_MAT
#define RT_STAT_MAT(mk) ((void)0)
#endif
#ifndef RT_STAT_VISIT
#define RT_STAT_VISIT(kind) ((void)0) /* hook for offline visit statistics (tools only) */
#endif
#ifndef RT_STAT_SLAB
#define RT_STAT_SLAB(literal) ((void)0) /* hook of the CPU tests: which form a box test of the unrolled sweep took */
#endif

/* "does any lane of this wave want this?" -- a scalar branch on the GPU; the CPU test
 * build runs one lane at a time */
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_WAVE_ANY(p) (__ballot((p)) != 0ull)
/* make a wave-uniform loaded value "arrived" here, so that the waitcnt pass does not
 * carry a pending scalar load into the loop that follows */
#define RT_SCALAR_READY(x) asm volatile("" ::"s"(x))
#else
#define RT_WAVE_ANY(p) (p)
#define RT_SCALAR_READY(x) ((void)0)
#endif

struct RtRay { RtV3 o, d; double time; };
struct RtRayOD { RtV3 o, d; };

/* HitRecord, hittable.rs:10-18 (material as table index) */
struct RtHit {
    RtV3 p, n;
    double t, u, v;
    uint32_t mat;
    bool front;
};

struct RtPath {
    RtRay ray;
    RtV3 beta;      /* product of (attenuation*scattering_pdf/pdf) so far */
    RtV3 radiance;  /* sum of beta*emitted so far */
    RtRng rng;
    uint32_t depth_left;
    bool alive;
};

/* ------------------------------------------------------------ geometry -- */

RT_HD RtV3 rt_at(RtV3 o, RtV3 d, double t) { return o + t * d; } /* ray.rs:12-14 */

/* AABB::hit aabb.rs:13-32; inv = 1/direction is the same value at every node of
 * one ray, so it is computed once per ray-space instead of per node. */
RT_HD bool rt_aabb_hit(const double* bb, RtV3 o, RtV3 inv, double t_min, double t_max) {
#define RT_SLAB(minv, maxv, ov, iv)                      \
    {                                                    \
        double t0 = ((minv) - (ov)) * (iv);              \
        double t1 = ((maxv) - (ov)) * (iv);              \
        if ((iv) < RT_R(0.0)) { double s_ = t0; t0 = t1; t1 = s_; } \
        t_min = t0 > t_min ? t0 : t_min;                 \
        t_max = t1 < t_max ? t1 : t_max;                 \
        if (t_max <= t_min) return false;                \
    }
    RT_SLAB(bb[0], bb[3], o.x, inv.x)
    RT_SLAB(bb[1], bb[4], o.y, inv.y)
    RT_SLAB(bb[2], bb[5], o.z, inv.z)
#undef RT_SLAB
    return true;
}

/* The same test with the running interval kept by max/min instructions.  Identical result
 * whenever t_min and t_max are not NaN on entry: `t0 > t_min ? t0 : t_min` keeps t_min when t0
 * is NaN and so does maxNum; equal values or zeros of either sign give the same comparisons
 * afterwards (t_min, t_max are not outputs).  Callers take the literal form when a NaN bound
 * is present (a NaN root was accepted earlier -- reference behaviour, reproduced). */
#if defined(RT_F32)
RT_HD double rt_vmax(double a, double b) { return __builtin_fmaxf(a, b); }
RT_HD double rt_vmin(double a, double b) { return __builtin_fminf(a, b); }
#elif defined(__HIP_DEVICE_COMPILE__) && !defined(RT_NO_ASM_MINMAX)
/* the bare instructions: __builtin_fmax/fmin make the compiler canonicalise each operand first
 * (a v_max_f64 x,x,x apiece); every operand here is an arithmetic result or a previous max/min */
RT_HD double rt_vmax(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RT_HD double rt_vmin(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
#else
RT_HD double rt_vmax(double a, double b) { return __builtin_fmax(a, b); }
RT_HD double rt_vmin(double a, double b) { return __builtin_fmin(a, b); }
#endif
/* EARLY: leave at the first closed axis (pays when few lanes of the wave are in the test, e.g. inside a medium's
 * boundary walk: then the whole wave often leaves; chosen per scene -- kernels of scenes with media use it throughout).  !EARLY: no early return -- a full wave leaves early only if all of
 * its lanes do, which is rare, while the exits cost every box an exec-mask save/restore and a branch per axis; the
 * verdict is the conjunction of the three "interval still open" tests in either form (what the interval becomes after a
 * failed axis is never looked at).  Measured: Cornell +1.8 %, random_scene +2 % without the exits; cornel_smoke -2.8 %. */
template <bool EARLY>
RT_HD bool rt_aabb_hit_fast(const double* bb, RtV3 o, RtV3 inv, double t_min, double t_max) {
    bool open = true;
#define RT_SLAB(minv, maxv, ov, iv)                      \
    {                                                    \
        double t0 = ((minv) - (ov)) * (iv);              \
        double t1 = ((maxv) - (ov)) * (iv);              \
        if ((iv) < RT_R(0.0)) { double s_ = t0; t0 = t1; t1 = s_; } \
        t_min = rt_vmax(t0, t_min);                      \
        t_max = rt_vmin(t1, t_max);                      \
        if (EARLY) { if (t_max <= t_min) return false; } \
        else open = open & !(t_max <= t_min);            \
    }
    RT_SLAB(bb[0], bb[3], o.x, inv.x)
    RT_SLAB(bb[1], bb[4], o.y, inv.y)
    RT_SLAB(bb[2], bb[5], o.z, inv.z)
#undef RT_SLAB
    return open;
}

/* Sphere::hit sphere.rs:31-48 / MovingSphere::hit moving_sphere.rs:38-55: the root only */
RT_HD bool rt_sphere_root(RtV3 center, double radius, RtV3 o, RtV3 d, double t_min, double t_max,
                          double& root_out) {
    RtV3 oc = o - center;
    double a = rt_mag2(d);
    double half_b = rt_dot(oc, d);
    double c = rt_mag2(oc) - radius * radius;
    double discriminant = half_b * half_b - a * c;
    if (discriminant < RT_R(0.0)) return false;
    double sqrtd = rt_sqrt(discriminant);
    double root = (-half_b - sqrtd) / a;
    if (root < t_min || t_max < root) {
        root = (-half_b + sqrtd) / a;
        if (root < t_min || t_max < root) return false;
    }
    root_out = root;
    return true;
}
/* rt_sphere_root for a caller that holds oc2 = |center - o|^2 already (rt_sphere_cone): its statements, with that value for |o - center|^2.
 * The two are the same bits: x - y and y - x are each other's negation in round-to-nearest, a square does not see the sign, and the
 * three squares are added in the same order (tests/test_light_cone.py compares them on 10^5 random pairs and the specials). */
RT_HD bool rt_sphere_root_oc2(RtV3 center, double radius, double oc2, RtV3 o, RtV3 d, double t_min, double t_max, double& root_out) {
    RtV3 oc = o - center;
    double a = rt_mag2(d);
    double half_b = rt_dot(oc, d);
    double c = oc2 - radius * radius;
    double discriminant = half_b * half_b - a * c;
    if (discriminant < RT_R(0.0)) return false;
    double sqrtd = rt_sqrt(discriminant);
    double root = (-half_b - sqrtd) / a;
    if (root < t_min || t_max < root) {
        root = (-half_b + sqrtd) / a;
        if (root < t_min || t_max < root) return false;
    }
    root_out = root;
    return true;
}
#if defined(__HIP_DEVICE_COMPILE__)
/* rt_sphere_root for a leaf of the box-free sweep that hands out a token besides its verdict (rt_sweep_free, RT_AHEAD_WORD 2): its
 * statements, and in `tok` the low word of the wave mask of ONE compare they make anyway -- a compare writes its mask to a scalar
 * register pair, so taking it costs no instruction.  The sphere's: the discriminant's sign, its last compare outside the divergent
 * part (the roots are tested by the lanes that have some). */
__device__ __forceinline__ bool rt_sphere_root_tok(RtV3 center, double radius, RtV3 o, RtV3 d, double t_min, double t_max, double& root_out, uint32_t& tok) {
    RtV3 oc = o - center;
    double a = rt_mag2(d);
    double half_b = rt_dot(oc, d);
    double c = rt_mag2(oc) - radius * radius;
    double discriminant = half_b * half_b - a * c;
    tok = (uint32_t)__builtin_amdgcn_ballot_w64(discriminant < RT_R(0.0));
    if (discriminant < RT_R(0.0)) return false;
    double sqrtd = rt_sqrt(discriminant);
    double root = (-half_b - sqrtd) / a;
    if (root < t_min || t_max < root) {
        root = (-half_b + sqrtd) / a;
        if (root < t_min || t_max < root) return false;
    }
    root_out = root;
    return true;
}
#endif
/* MovingSphere::center moving_sphere.rs:23-26 */
RT_HD RtV3 rt_msphere_center(const RtNode& nd, double time) {
    RtV3 c0 = rt_v3(nd.d[0], nd.d[1], nd.d[2]), c1 = rt_v3(nd.d[3], nd.d[4], nd.d[5]);
    return c0 + ((time - nd.e[0]) / (nd.e[1] - nd.e[0])) * (c1 - c0);
}
/* XYRect/XZRect/YZRect::hit aarect.rs:46-56,84-94,152-162: t and the in-bounds test.
 * (oa,da) is the axis normal to the plane, (ob,db),(oc,dc) the two in-plane axes. */
RT_HD bool rt_rect_t(const RtNode& nd, double oa, double da, double ob, double db, double oc,
                     double dc, double t_min, double t_max, double& t_out) {
    double t = (nd.d[4] - oa) / da;
    if (t < t_min || t > t_max) return false;
    double b = ob + t * db;
    double c = oc + t * dc;
    if (b < nd.d[0] || b > nd.d[1] || c < nd.d[2] || c > nd.d[3]) return false;
    t_out = t;
    return true;
}
/* the three rect kinds as one code path: axis selection by value instead of a 3-way branch
 * (same operands reach the same operations as in rt_rect_t) */
RT_HD bool rt_rect_any_t(const RtNode& nd, uint32_t kind, RtV3 o, RtV3 d, double t_min, double t_max, double& t) {
    double oa = kind == RT_XY ? o.z : (kind == RT_XZ ? o.y : o.x);
    double da = kind == RT_XY ? d.z : (kind == RT_XZ ? d.y : d.x);
    double ob = kind == RT_YZ ? o.y : o.x;
    double db = kind == RT_YZ ? d.y : d.x;
    double oc = kind == RT_XY ? o.y : o.z;
    double dc = kind == RT_XY ? d.y : d.z;
    return rt_rect_t(nd, oa, da, ob, db, oc, dc, t_min, t_max, t);
}
template <class Cfg>
RT_HD bool rt_prim_t(const RtNode& nd, uint32_t kind, RtV3 o, RtV3 d, double time, double t_min, double t_max,
                     double& t) {
    if (kind >= RT_XY) return rt_rect_any_t(nd, kind, o, d, t_min, t_max, t);
    if (Cfg::msphere && kind == RT_MSPHERE)
        return rt_sphere_root(rt_msphere_center(nd, time), nd.e[2], o, d, t_min, t_max, t);
    return rt_sphere_root(rt_v3(nd.d[0], nd.d[1], nd.d[2]), nd.d[3], o, d, t_min, t_max, t);
}

/* Translate::hit hittable.rs:207-211 / RotateY::hit hittable.rs:238-251: ray into the wrapper's space */
template <class NodeT>
RT_HD RtRayOD rt_scope_in(const NodeT& s, RtRayOD r) {
    if (s.kind == RT_TRANSLATE) {
        r.o = r.o - rt_v3(s.d[0], s.d[1], s.d[2]);
    } else if (s.kind == RT_ROTATE_Y) {
        double sn = s.d[0], cs = s.d[1];
        RtV3 o = r.o, d = r.d;
        r.o.x = cs * o.x - sn * o.z;
        r.o.z = sn * o.x + cs * o.z;
        r.d.x = cs * d.x - sn * d.z;
        r.d.z = sn * d.x + cs * d.z;
    }
    return r;
}
/* the same for a wrapper whose kind the caller knows at compile time (the sweeps unrolled along a scene's own tree): the statements of
 * that kind and nothing else -- the record's kind word is not read, no arm is chosen at run time, the ray stays in its registers.
 * RT_SCOPE_STATIC 0 is the dispatch on the record (RT1W_JIT_EXTRA_OPTS=-DRT_SCOPE_STATIC=0: the A/B). */
#ifndef RT_SCOPE_STATIC
#define RT_SCOPE_STATIC 1
#endif
template <uint32_t KIND, class NodeT>
RT_HD RtRayOD rt_scope_in_k(const NodeT& s, RtRayOD r) {
#if RT_SCOPE_STATIC
    static_assert(KIND == RT_TRANSLATE || KIND == RT_ROTATE_Y, "a wrapper that moves the ray");
    if constexpr (KIND == RT_TRANSLATE) {
        r.o = r.o - rt_v3(s.d[0], s.d[1], s.d[2]);
    } else {
        double sn = s.d[0], cs = s.d[1];
        RtV3 o = r.o, d = r.d;
        r.o.x = cs * o.x - sn * o.z;
        r.o.z = sn * o.x + cs * o.z;
        r.d.x = cs * d.x - sn * d.z;
        r.d.z = sn * d.x + cs * d.z;
    }
    return r;
#else
    return rt_scope_in(s, r);
#endif
}
/* the way back out: hittable.rs:215-225, :255-278, :288-291.  `inner` is the ray in
 * the wrapper's space (`moved` / `rotated_r`): both re-run HitRecord::new with it,
 * taking the child's already-forwarded normal as "outward" (reference quirk Q5). */
template <class NodeT>
RT_HD void rt_scope_out(const NodeT& s, RtRayOD inner, RtHit& h) {
    if (s.kind == RT_TRANSLATE) {
        h.p = h.p + rt_v3(s.d[0], s.d[1], s.d[2]);
        bool front = rt_dot(inner.d, h.n) < RT_R(0.0);
        h.n = front ? h.n : -h.n;
        h.front = front;
    } else if (s.kind == RT_ROTATE_Y) {
        double sn = s.d[0], cs = s.d[1];
        RtV3 p = h.p, n = h.n;
        p.x = cs * h.p.x + sn * h.p.z;
        p.z = -sn * h.p.x + cs * h.p.z;
        n.x = cs * h.n.x + sn * h.n.z;
        n.z = -sn * h.n.x + cs * h.n.z;
        bool front = rt_dot(inner.d, n) < RT_R(0.0);
        h.p = p;
        h.n = front ? n : -n;
        h.front = front;
    } else { /* RT_FLIP */
        h.front = !h.front;
    }
}

/* wrapper chain above a primitive, outermost first (depth <= RT_MAX_SCOPE_DEPTH) */
struct RtChain { uint32_t s0, s1, s2; };
RT_HD RtChain rt_chain(const RtNode* nodes, uint32_t scope) {
    RtChain c; c.s0 = c.s1 = c.s2 = RT_NONE;
    while (scope != RT_NONE) {
        c.s2 = c.s1; c.s1 = c.s0; c.s0 = scope;
        scope = nodes[scope].b;
    }
    return c;
}
RT_HD RtRayOD rt_ray_in_scope(const RtNode* nodes, uint32_t scope, RtRayOD world) {
    if (scope == RT_NONE) return world;
    RtChain c = rt_chain(nodes, scope);
    RtRayOD r = rt_scope_in(nodes[c.s0], world);
    if (c.s1 != RT_NONE) r = rt_scope_in(nodes[c.s1], r);
    if (c.s2 != RT_NONE) r = rt_scope_in(nodes[c.s2], r);
    return r;
}
/* the same, also telling whether a RotateY is among the wrappers: if none is, the direction -- and 1/direction -- is the world's */
RT_HD RtRayOD rt_ray_in_scope_r(const RtNode* nodes, uint32_t scope, RtRayOD world, bool& rotated) {
    rotated = false;
    if (scope == RT_NONE) return world;
    RtChain c = rt_chain(nodes, scope);
    rotated = (nodes[c.s0].kind & RT_KIND_MASK) == RT_ROTATE_Y;
    RtRayOD r = rt_scope_in(nodes[c.s0], world);
    if (c.s1 != RT_NONE) { rotated |= (nodes[c.s1].kind & RT_KIND_MASK) == RT_ROTATE_Y; r = rt_scope_in(nodes[c.s1], r); }
    if (c.s2 != RT_NONE) { rotated |= (nodes[c.s2].kind & RT_KIND_MASK) == RT_ROTATE_Y; r = rt_scope_in(nodes[c.s2], r); }
    return r;
}

/* sphere_uv math.rs:67-71 */
RT_HD void rt_sphere_uv(RtV3 p, double& u, double& v) {
    double theta = rt_acos(-p.y);
    double phi = rt_atan2(-p.z, p.x) + RT_R(RT_PI);
    u = phi / (RT_R(2.0) * RT_R(RT_PI));
    v = theta / RT_R(RT_PI);
}

/* The leaf's own HitRecord (sphere.rs:50-62, moving_sphere.rs:57-69, aarect.rs:58-71,
 * 96-109,164-177, constant_medium.rs:98-106) in the leaf's space.  u,v are only
 * evaluated when the material's texture reads them (image texture); they are
 * unobservable otherwise. */
template <class Cfg>
RT_HD void rt_leaf_record(const RtNode& nd, RtRayOD r, double time, double t, bool want_uv,
                          RtHit& h) {
    h.t = t; h.u = RT_R(0.0); h.v = RT_R(0.0); h.mat = nd.mat;
    h.p = rt_at(r.o, r.d, t);
    RtV3 on;
    const uint32_t kind = nd.kind & RT_KIND_MASK;
    const bool flipped = (nd.kind & RT_LEAF_FLIPPED) != 0u;
    if (kind == RT_SPHERE || kind == RT_MSPHERE) {
        if (!Cfg::msphere || kind == RT_SPHERE) on = (h.p - rt_v3(nd.d[0], nd.d[1], nd.d[2])) / nd.d[3];
        else on = (h.p - rt_msphere_center(nd, time)) / nd.e[2];
        if (Cfg::tex && want_uv) rt_sphere_uv(on, h.u, h.v);
    } else if (Cfg::media && kind == RT_MEDIUM) {
        h.n = rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0));
        h.front = true;
        return;
    } else {
        double b, c;
        if (kind == RT_XY) { on = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(1.0)); b = r.o.x + t * r.d.x; c = r.o.y + t * r.d.y; }
        else if (kind == RT_XZ) { on = rt_v3(RT_R(0.0), RT_R(1.0), RT_R(0.0)); b = r.o.x + t * r.d.x; c = r.o.z + t * r.d.z; }
        else { on = rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0)); b = r.o.y + t * r.d.y; c = r.o.z + t * r.d.z; }
        if (Cfg::tex && want_uv) {
            h.u = (b - nd.d[0]) / (nd.d[1] - nd.d[0]);
            h.v = (c - nd.d[2]) / (nd.d[3] - nd.d[2]);
        }
    }
    /* HitRecord::new hittable.rs:30-35 */
    bool front = rt_dot(r.d, on) < RT_R(0.0);
    h.n = front ? on : -on;
    h.front = flipped ? !front : front; /* FlipFace::hit hittable.rs:288-291 flips the flag only */
}

/* Full hit record of the winning leaf: leaf record in its own space, then the
 * wrapper fix-ups innermost to outermost. */
template <class Cfg>
RT_HD void rt_finish_hit(const RtSceneView& sc, const RtRay& world, uint32_t prim, uint32_t scope,
                         double t, RtHit& h) {
    const RtNode* nodes = sc.nodes;
    const RtNode& nd = nodes[prim];
    bool want_uv = Cfg::tex && (RT_MAT_KINDF(nd.mat) & RT_MAT_NEEDS_UV) != 0u;
    RtRayOD r0; r0.o = world.o; r0.d = world.d;
    if (Cfg::scope_depth == 0 || scope == RT_NONE) {
        rt_leaf_record<Cfg>(nd, r0, world.time, t, want_uv, h);
        return;
    }
    RtChain c = rt_chain(nodes, scope);
    RtRayOD r1 = rt_scope_in(nodes[c.s0], r0);
    RtRayOD r2 = r1, r3 = r1;
    if (c.s1 != RT_NONE) { r2 = rt_scope_in(nodes[c.s1], r1); r3 = r2; }
    if (c.s2 != RT_NONE) r3 = rt_scope_in(nodes[c.s2], r2);
    rt_leaf_record<Cfg>(nd, r3, world.time, t, want_uv, h);
    if (c.s2 != RT_NONE) rt_scope_out(nodes[c.s2], r3, h);
    if (c.s1 != RT_NONE) rt_scope_out(nodes[c.s1], r2, h);
    rt_scope_out(nodes[c.s0], r1, h);
}

/* static sphere and the three rects, from the hot half of the record (same operations as
 * rt_prim_t).  `kind` is wave-uniform in the sweep, so the axis choice is a scalar branch. */
RT_HD bool rt_rect_hot_at(const RtNodeHot& nd, double t, bool in_t, double ob, double db, double oc, double dc, double& t_out) {
    const double b = ob + t * db;
    const double c = oc + t * dc;
    const bool in_rect = !((b < nd.d[0]) | (b > nd.d[1]) | (c < nd.d[2]) | (c > nd.d[3]));
    if (in_t & in_rect) { t_out = t; return true; }
    return false;
}
RT_HD bool rt_rect_hot_t(const RtNodeHot& nd, double oa, double da, double ob, double db, double oc, double dc,
                         double t_min, double t_max, double& t_out) {
    /* both of aarect.rs' rejections as one conjunction (no exec-mask region for the second half: the wave runs it
     * anyway unless every lane fails the first); a NaN passes each comparison exactly as it does there */
    const double t = (nd.d[4] - oa) / da;
    const bool in_t = !((t < t_min) | (t > t_max));
    return rt_rect_hot_at(nd, t, in_t, ob, db, oc, dc, t_out);
}
RT_HD bool rt_prim_hot_t(const RtNodeHot& nd, uint32_t kind, RtV3 o, RtV3 d, double t_min, double t_max, double& t_out) {
    if (kind == RT_XY) return rt_rect_hot_t(nd, o.z, d.z, o.x, d.x, o.y, d.y, t_min, t_max, t_out);
    if (kind == RT_XZ) return rt_rect_hot_t(nd, o.y, d.y, o.x, d.x, o.z, d.z, t_min, t_max, t_out);
    if (kind == RT_YZ) return rt_rect_hot_t(nd, o.x, d.x, o.y, d.y, o.z, d.z, t_min, t_max, t_out);
    return rt_sphere_root(rt_v3(nd.d[0], nd.d[1], nd.d[2]), nd.d[3], o, d, t_min, t_max, t_out);
}

/* static sphere / rects from the hot half when the kind differs per lane (stack walk): axis by select */
RT_HD bool rt_prim_hot_sel_t(const RtNodeHot& nd, uint32_t kind, RtV3 o, RtV3 d, double t_min, double t_max, double& t_out) {
    if (kind >= RT_XY) {
        double oa = kind == RT_XY ? o.z : (kind == RT_XZ ? o.y : o.x);
        double da = kind == RT_XY ? d.z : (kind == RT_XZ ? d.y : d.x);
        double ob = kind == RT_YZ ? o.y : o.x;
        double db = kind == RT_YZ ? d.y : d.x;
        double oc = kind == RT_XY ? o.y : o.z;
        double dc = kind == RT_XY ? d.y : d.z;
        return rt_rect_hot_t(nd, oa, da, ob, db, oc, dc, t_min, t_max, t_out);
    }
    return rt_sphere_root(rt_v3(nd.d[0], nd.d[1], nd.d[2]), nd.d[3], o, d, t_min, t_max, t_out);
}

/* Where the sweep gets the hot half of node n (n is wave-uniform):
 *  - RtGlobalNodes: from memory (scalar loads on the GPU);
 *  - a lane-resident source (context.hip, scenes of <= 64 nodes): lane i of every wave keeps
 *    node i's hot words in registers for the whole kernel and node n is read with
 *    v_readlane -- the traversal then touches no memory at all. */
struct RtGlobalNodes {
    static constexpr bool virt = false;
    const RtNode* p;
    RT_HD RtNodeHot hot(uint32_t n) const { return *reinterpret_cast<const RtNodeHot*>(p + n); }
};
/*  - RtWalkNodes (stack-walk kernels with the node cache): records of the WALK TABLE (rt_walk_table.h), addressed by a walk id
 *    instead of the node index -- the table lists the nodes most likely to be visited first, and its first `nc` records sit in
 *    LDS.  `virt`: stack entries are walk ids; a record names its children / itself by the fields below instead of e + 1 / e. */
struct RtWalkNodes {
    static constexpr bool virt = true;
    const RtNodeHot* lds;  /* records [0, nc) */
    const RtNodeHot* glob; /* the whole table */
    uint32_t nc;
    RT_HD RtNodeHot hot(uint32_t v) const { return v < nc ? lds[v] : glob[v]; }
};
/* where the context keeps the walk table: behind the node array and its spare record, at the next 128-byte boundary */
#define RT_WT_OFFSET(n_nodes) ((((size_t)(n_nodes) + 1u) * sizeof(RtNode) + 127u) & ~(size_t)127u)
#define RT_WT_INLINE_SPHERE 0x1000u /* walk-table record of a ConstantMedium: its boundary is a bare Sphere, centre in d[1..3], radius in d[4] */
/* what a record says about its neighbours.  Node arrays: the left / only child is the next node in pre-order and an entry IS the node
 * index.  Walk table: BVH node: skip = left / only child's walk id, b = right child's; wrapper: skip = child's walk id, mat = own node
 * index; leaf and medium: skip = own node index (medium: mat = walk id of the boundary's root) */
template <class NS> RT_HD uint32_t rt_ns_child(uint32_t e, const RtNodeHot& nd) { if constexpr (NS::virt) return nd.skip; else return e + 1u; }
template <class NS> RT_HD uint32_t rt_ns_leaf_id(uint32_t e, const RtNodeHot& nd) { if constexpr (NS::virt) return nd.skip; else return e; }
template <class NS> RT_HD uint32_t rt_ns_wrap_id(uint32_t e, const RtNodeHot& nd) { if constexpr (NS::virt) return nd.mat; else return e; }

/* ----------------------------------------------------------- traversal -- */

RT_HD RtV3 rt_inv3(RtV3 d) { return rt_v3(RT_R(1.0) / d.x, RT_R(1.0) / d.y, RT_R(1.0) / d.z); }

/* What the unrolled sweep knows about 1 / direction in one ray space: the three reciprocals (`inv`, a plain RtV3), or those and the
 * prepared divisors y of include/rt1w_num.h ("quotients of one divisor") from which they were made.  A rect's t = (k - o_a) / d_a
 * is then three instructions on y_a instead of a division, and the two Newton steps run once per axis and ray space instead of
 * once per quotient (Cornell: 18 divisions of the sweep share 6 divisors).  Speculate, then verify: every divisor and every quotient
 * that leaves the range where that is `/` bit for bit sets its lane in `bad`, a wave mask in scalar registers, and rt_closest_hit
 * runs the sweep again with `/` for a wave that has one.  f64 device code of the media-free specialised units only (in a
 * ConstantMedium's boundary sweeps t_min is -inf or NaN and a zero quotient can be accepted); everything else keeps `/`.
 * RT_DIV_SHARED: bit 1 the prepared divisors and the reciprocals made from them, bit 2 the rects' quotients (2 alone is 3); default 3.
 * RT1W_JIT_EXTRA_OPTS=-DRT_DIV_SHARED=0: the text without any of it.  -DRT_DIV_SHARED_FORCE_SLOW=1 (tests): every wave sweeps twice. */
#undef RT_DIV_SHARED_ON /* (a unit may take this header twice: f64 records, then the f32 build) */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RT_F32)
#ifndef RT_DIV_SHARED
#define RT_DIV_SHARED 3
#endif
#define RT_DIV_SHARED_ON (RT_DIV_SHARED)
#else
#define RT_DIV_SHARED_ON 0
#endif
#ifndef RT_DIV_SHARED_FORCE_SLOW
#define RT_DIV_SHARED_FORCE_SLOW 0
#endif
template <class Inv> struct RtInvIsShared { static constexpr bool value = false; };
RT_HD const RtV3& rt_inv_of(const RtV3& inv) { return inv; }
RT_HD RtV3 rt_inv_again(const RtV3&, RtV3 d, bool) { return rt_inv3(d); } /* the next ray space (below a RotateY) */
#if RT_DIV_SHARED_ON
struct RtInvShared {
    RtV3 inv, y;
    uint64_t& bad;
};
template <> struct RtInvIsShared<RtInvShared> { static constexpr bool value = true; };
RT_HD const RtV3& rt_inv_of(const RtInvShared& s) { return s.inv; }
/* `act`: the lanes whose ray this is (the others' directions are whatever they hold and must not send the wave to the slow sweep) */
RT_HD RtInvShared rt_inv3_shared(RtV3 d, bool act, uint64_t& bad) {
    const RtV3 y = rt_v3(rt_div_prep(d.x), rt_div_prep(d.y), rt_div_prep(d.z));
    bad |= __builtin_amdgcn_ballot_w64(act & !(rt_div_d_ok(d.x) & rt_div_d_ok(d.y) & rt_div_d_ok(d.z)));
    return RtInvShared{rt_v3(rt_div_inv(d.x, y.x), rt_div_inv(d.y, y.y), rt_div_inv(d.z, y.z)), y, bad};
}
/* a scene without a rect has no quotient to share with the box tests' reciprocals: its unit keeps one sweep, with `/` */
template <class Topo>
constexpr bool rt_topo_has_rect() {
    for (uint32_t i = 0; i < sizeof(Topo::kind) / sizeof(Topo::kind[0]); ++i)
        if ((Topo::kind[i] & RT_KIND_MASK) >= RT_XY && (Topo::kind[i] & RT_KIND_MASK) <= RT_YZ) return true;
    return false;
}
RT_HD RtInvShared rt_inv_again(const RtInvShared& s, RtV3 d, bool act) { return rt_inv3_shared(d, act, s.bad); }
/* rt_rect_hot_t with the quotient from the prepared divisor of its axis.  Every lane of the wave computes, `act` says whose verdict
 * counts: the range test is then one compare straight into the wave mask (taken under `if (act)` it would be a per-lane value that
 * has to be collected again), and a lane that is elsewhere in the tree tests its own, real ray -- at worst a sweep too many.
 * rt_closest_hit has made sure of t_min (rt_div_tmin_ok), so a quotient that passes it is above the lower bound as well. */
RT_HD bool rt_rect_hot_t(const RtNodeHot& nd, uint32_t kind, RtV3 o, RtV3 d, const RtInvShared& s, bool act, double t_min, double t_max, double& t_out) {
    const double oa = kind == RT_XY ? o.z : (kind == RT_XZ ? o.y : o.x), da = kind == RT_XY ? d.z : (kind == RT_XZ ? d.y : d.x);
    const double ya = kind == RT_XY ? s.y.z : (kind == RT_XZ ? s.y.y : s.y.x);
    const double t = rt_div_q(nd.d[4] - oa, da, ya);
    s.bad |= __builtin_amdgcn_ballot_w64(rt_div_q_big(t));
    const bool in_t = act & !((t < t_min) | (t > t_max));
    if (kind == RT_XY) return rt_rect_hot_at(nd, t, in_t, o.x, d.x, o.y, d.y, t_out);
    if (kind == RT_XZ) return rt_rect_hot_at(nd, t, in_t, o.x, d.x, o.z, d.z, t_out);
    return rt_rect_hot_at(nd, t, in_t, o.y, d.y, o.z, d.z, t_out);
}
/* the same with a token for the box-free sweep (rt_sphere_root_tok): the mask of the rect's last compare, `c > nd.d[3]`, said once more
 * behind the conjunction it is part of -- one value, one instruction */
__device__ __forceinline__ bool rt_rect_hot_at_tok(const RtNodeHot& nd, double t, bool in_t, double ob, double db, double oc, double dc, double& t_out, uint32_t& tok) {
    const double b = ob + t * db;
    const double c = oc + t * dc;
    const bool in_rect = !((b < nd.d[0]) | (b > nd.d[1]) | (c < nd.d[2]) | (c > nd.d[3]));
    tok = (uint32_t)__builtin_amdgcn_ballot_w64(c > nd.d[3]);
    if (in_t & in_rect) { t_out = t; return true; }
    return false;
}
__device__ __forceinline__ bool rt_rect_hot_t_tok(const RtNodeHot& nd, uint32_t kind, RtV3 o, RtV3 d, const RtInvShared& s, bool act, double t_min, double t_max, double& t_out, uint32_t& tok) {
    const double oa = kind == RT_XY ? o.z : (kind == RT_XZ ? o.y : o.x), da = kind == RT_XY ? d.z : (kind == RT_XZ ? d.y : d.x);
    const double ya = kind == RT_XY ? s.y.z : (kind == RT_XZ ? s.y.y : s.y.x);
    const double t = rt_div_q(nd.d[4] - oa, da, ya);
    s.bad |= __builtin_amdgcn_ballot_w64(rt_div_q_big(t));
    const bool in_t = act & !((t < t_min) | (t > t_max));
    if (kind == RT_XY) return rt_rect_hot_at_tok(nd, t, in_t, o.x, d.x, o.y, d.y, t_out, tok);
    if (kind == RT_XZ) return rt_rect_hot_at_tok(nd, t, in_t, o.x, d.x, o.z, d.z, t_out, tok);
    return rt_rect_hot_at_tok(nd, t, in_t, o.y, d.y, o.z, d.z, t_out, tok);
}
#endif

/* ConstantMedium::hit constant_medium.rs:58-113, given the two boundary roots t1, t2 */
RT_HD bool rt_medium_t(double neg_inv_density, RtV3 d, double t1, double t2, double t_min, double t_max, RtRng& rng,
                       double& t_out) {
    double rec1 = rt_max(t1, t_min);
    double rec2 = rt_min(t2, t_max);
    if (rec1 >= rec2) return false;
    rec1 = rt_max(rec1, RT_R(0.0));
    double ray_length = rt_mag(d);
    double distance_inside_boundary = (rec2 - rec1) * ray_length;
    rt_rng_reserve(rng, rt_rng_need_u64(rng));
    double hit_distance = neg_inv_density * rt_log(rt_take_f64(rng));
    if (hit_distance > distance_inside_boundary) return false;
    t_out = rec1 + hit_distance / ray_length;
    return true;
}
RT_HD bool rt_medium_t(const RtNode& nd, RtV3 d, double t1, double t2, double t_min, double t_max, RtRng& rng, double& t_out) {
    return rt_medium_t(nd.d[0], d, t1, t2, t_min, t_max, rng, t_out);
}

/* Closest hit of a subtree for a ray within [t_min, t_max], with an explicit per-lane stack (LDS
 * on the GPU), written as a resumable walk: rt_walk_begin pushes the root, rt_walk_step handles ONE
 * stack entry whatever its kind, rt_walk_done says when the stack is back to its base.  (A kernel
 * that ran one step per iteration and let finished lanes shade in batches while the others kept
 * walking was measured: it only ties the plain loop at equal occupancy and needs more registers.)
 * The walk is bound by the latency of the dependent node fetches, so the fewest iterations win (a
 * "while-while" split of box and leaf work was measured 0.6x).
 * Visiting order is the reference's (bvh.rs:38-47): left subtree, then right subtree with the
 * closest t so far as t_max. */
struct RtWalk {
    RtRayOD w;          /* the ray in the subtree's outer space */
    RtRayOD cur;        /* the ray in the current wrapper's space */
    RtV3 inv_w, inv;    /* 1/direction of w and of cur */
    double time, t_min, best_t;
    uint32_t scope, best_prim, best_scope;
    int base;           /* stack level at entry */
    bool tmin_nan;
};

/* `inv_known`: 1/direction of `world` if the caller has it already (a ConstantMedium's boundary is walked with the very ray the
 * outer walk holds, constant_medium.rs:62-69: the same three quotients, not computed again twice per medium) */
template <class Stack>
RT_HD void rt_walk_begin(RtWalk& k, uint32_t root, const RtRay& world, double t_min, double t_max, Stack& stk, const RtV3* inv_known = nullptr) {
    k.w.o = world.o; k.w.d = world.d;
    k.cur = k.w;
    k.inv_w = inv_known ? *inv_known : rt_inv3(k.w.d);
    k.inv = k.inv_w;
    k.time = world.time; k.t_min = t_min; k.best_t = t_max;
    k.scope = RT_NONE; k.best_prim = RT_NONE; k.best_scope = RT_NONE;
    k.tmin_nan = rt_isnan(t_min);
    k.base = stk.sp;
    stk.push(root);
}
template <class Stack>
RT_HD bool rt_walk_done(const RtWalk& k, const Stack& stk) { return stk.sp <= k.base; }

template <class Cfg, bool MEDIA, class Stack, class NS>
RT_HD bool rt_traverse_stack(const RtSceneView& sc, const NS& ns, uint32_t root, const RtRay& world, double t_min,
                             double t_max, RtRng& rng, Stack& stk, double& out_t, uint32_t& out_prim,
                             uint32_t& out_scope, const RtV3* inv_known = nullptr);

/* The walk's work, one piece per kind of stack entry (MEDIA=false is the flavour used for a ConstantMedium's
 * boundary, where only t is consumed, constant_medium.rs:62-69). */
enum { RT_WK_NONE = 0, RT_WK_BOX = 1, RT_WK_LEAF = 2, RT_WK_WRAP = 3, RT_WK_EXIT = 4, RT_WK_OTHER = 5 };
RT_HD uint32_t rt_walk_class(uint32_t kind) {
    return kind <= RT_BVH1 ? RT_WK_BOX : (kind <= RT_YZ ? RT_WK_LEAF : (kind <= RT_FLIP ? RT_WK_WRAP : RT_WK_OTHER));
}
/* leaving a wrapper: back to the parent's ray (recomputed from the outer ray by the same operations that
 * produced it, hence the same bits) */
RT_HD void rt_walk_exit(const RtSceneView& sc, RtWalk& k, uint32_t e) {
    const RtNode* nodes = sc.nodes;
    k.scope = nodes[e & ~RT_POP_FLAG].b;
    if (k.scope == RT_NONE) { k.cur = k.w; k.inv = k.inv_w; }
    else {
        bool rotated;
        k.cur = rt_ray_in_scope_r(nodes, k.scope, k.w, rotated);
        k.inv = k.inv_w; /* Translate / FlipFace leave the direction alone: the same three quotients (hittable.rs:207-211) */
        if (rotated) k.inv = rt_inv3(k.cur.d);
    }
}
#ifndef RT_BRANCHLESS_PUSH
#define RT_BRANCHLESS_PUSH 1
#endif
template <class Cfg, bool EARLY, class NS = RtGlobalNodes, class Stack>
RT_HD void rt_walk_box(RtWalk& k, uint32_t e, const RtNodeHot& nd, Stack& stk) {
    const uint32_t left = rt_ns_child<NS>(e, nd); /* the left / only child */
    bool hit;
    if (RT_WAVE_ANY(k.tmin_nan || rt_isnan(k.best_t))) hit = rt_aabb_hit(nd.d, k.cur.o, k.inv, k.t_min, k.best_t);
    else hit = rt_aabb_hit_fast<EARLY>(nd.d, k.cur.o, k.inv, k.t_min, k.best_t);
#if RT_BRANCHLESS_PUSH /* the CPU test build runs the same form: its stack bound-checks every poke (oracle_flat.cpp) */
    if constexpr (!Cfg::ordered) {
        /* both slots are written whatever the test said and the stack pointer moves by 0, 1 or 2: no nested exec-mask regions.
         * A miss, or a BVHChild::One, leaves dead words above the top: the flattener counts TWO slots for every BVH node
         * (scene.cpp, Flattener::emit), so the footprint of the pokes is inside stack_need */
        const bool two = (nd.kind & RT_KIND_MASK) == RT_BVH2;
        stk.poke(0, two ? nd.b : left); /* BVH2: the right child below the left one (bvh.rs:38-47); BVH1: its only child */
        stk.poke(1, left);
        stk.sp += hit ? (two ? 2 : 1) : 0;
        return;
    }
#endif
    if (hit) {
        if ((nd.kind & RT_KIND_MASK) == RT_BVH2) {
            uint32_t first = left, second = nd.b; /* left child (the next node in pre-order), then the right one: bvh.rs:38-47 */
            const uint32_t ord = Cfg::ordered ? (nd.kind >> RT_BVH_ORDER_SHIFT) & RT_BVH_ORDER_MASK : 0u;
            if (Cfg::ordered && ord != 0u) { /* opt-in near-far order (variant V4 only): the child on the ray's near side first */
                const double da = ord == 1u ? k.cur.d.x : (ord == 2u ? k.cur.d.y : k.cur.d.z);
                const bool left_lower = (nd.kind & RT_BVH_LEFT_LOWER) != 0u;
                if ((da < RT_R(0.0) && left_lower) || (da > RT_R(0.0) && !left_lower)) { first = nd.b; second = left; }
            }
            stk.push(second);
            stk.push(first);
        } else {
            stk.push(left); /* only child */
        }
    }
}
/* Ties in t go to the primitive the reference tests LATER (bvh.rs:40, sphere.rs:43, aarect.rs:48: `t_max < root` keeps an
 * equal root), i.e. to the larger pre-order index.  In the reference's own visiting order a later test always has the larger
 * index, so this never rejects anything there; under the opt-in near-far order it is what keeps equal-t hits the reference's. */
RT_HD bool rt_tie_ok(double t, uint32_t e, double best_t, uint32_t best_prim) {
    return !(t == best_t && best_prim != RT_NONE && e < best_prim);
}
template <class Cfg, class NS = RtGlobalNodes>
RT_HD void rt_walk_leaf(const RtSceneView& sc, RtWalk& k, uint32_t e_, const RtNodeHot& nd) {
    const uint32_t e = rt_ns_leaf_id<NS>(e_, nd); /* the node index: what the walk reports */
    const uint32_t kind = nd.kind & RT_KIND_MASK;
    double t;
    bool hit;
    if (Cfg::msphere && kind == RT_MSPHERE) hit = rt_prim_t<Cfg>(sc.nodes[e], kind, k.cur.o, k.cur.d, k.time, k.t_min, k.best_t, t);
    else hit = rt_prim_hot_sel_t(nd, kind, k.cur.o, k.cur.d, k.t_min, k.best_t, t);
    if (hit && (!Cfg::ordered || rt_tie_ok(t, e, k.best_t, k.best_prim))) { k.best_t = t; k.best_prim = e; k.best_scope = k.scope; }
}
template <class NS = RtGlobalNodes, class Stack>
RT_HD void rt_walk_wrap(RtWalk& k, uint32_t e_, const RtNodeHot& nd, Stack& stk) {
    const uint32_t kind = nd.kind & RT_KIND_MASK;
    const uint32_t e = rt_ns_wrap_id<NS>(e_, nd); /* scopes and exit entries are node indices in every form of the walk */
    stk.push(e | RT_POP_FLAG);
    k.scope = e;
    if (kind != RT_FLIP) {
        k.cur = rt_scope_in(nd, k.cur);
        if (kind == RT_ROTATE_Y) k.inv = rt_inv3(k.cur.d);
    }
    stk.push(rt_ns_child<NS>(e_, nd));
}
template <class Cfg, bool MEDIA, class Stack, class NS>
RT_HD void rt_walk_other(const RtSceneView& sc, const NS& ns, RtWalk& k, uint32_t e_, const RtNodeHot& nd, RtRng& rng, Stack& stk) {
    if (MEDIA && Cfg::media && (nd.kind & RT_KIND_MASK) == RT_MEDIUM) {
        /* ConstantMedium::hit constant_medium.rs:58-113: two complete boundary walks, then the free-flight draw */
        const uint32_t e = rt_ns_leaf_id<NS>(e_, nd);
        RtRay br; br.o = k.cur.o; br.d = k.cur.d; br.time = k.time;
        double t1, t2, t; uint32_t p_, s_;
        bool both;
        bool sphere; RtV3 c; double radius; uint32_t broot;
        if constexpr (NS::virt) {
            sphere = (nd.kind & RT_WT_INLINE_SPHERE) != 0u; c = rt_v3(nd.d[1], nd.d[2], nd.d[3]); radius = nd.d[4]; broot = nd.mat;
        } else {
            const RtNodeHot bn = ns.hot(e + 1u);
            sphere = (bn.kind & RT_KIND_MASK) == RT_SPHERE; c = rt_v3(bn.d[0], bn.d[1], bn.d[2]); radius = bn.d[3]; broot = e + 1u;
        }
        if (sphere) {
            /* the boundary is a bare Sphere (every medium of the reference's scenes): its walk is one stack entry, one leaf
             * test -- run the two tests (sphere.rs:31-48 with (-inf, inf), then (t1 + 0.0001, inf)) without the walk around them */
            both = rt_sphere_root(c, radius, br.o, br.d, -RT_INF, RT_INF, t1) && rt_sphere_root(c, radius, br.o, br.d, t1 + RT_R(0.0001), RT_INF, t2);
        } else if constexpr (Cfg::sphere_media) {
            both = false; (void)p_; (void)s_; (void)broot; /* not reached: the host gives these kernels only scenes without such a medium (RtCfgSphereMedia) */
        } else {
            both = rt_traverse_stack<Cfg, false>(sc, ns, broot, br, -RT_INF, RT_INF, rng, stk, t1, p_, s_, &k.inv) &&
                   rt_traverse_stack<Cfg, false>(sc, ns, broot, br, t1 + RT_R(0.0001), RT_INF, rng, stk, t2, p_, s_, &k.inv);
        }
        if (both && rt_medium_t(nd.d[0], k.cur.d, t1, t2, k.t_min, k.best_t, rng, t)) {
            k.best_t = t; k.best_prim = e; k.best_scope = k.scope;
        }
    }
}

#ifndef RT_MEDIUM_DEFER
#define RT_MEDIUM_DEFER 0 /* 0: media run where they are met; 1, 2: parked and run wave-wide (rt_traverse_stack): MEASURED slower,
                            final_scene 118 -> 106 / 114 Mpaths/s at 16 spp, bit-identical (profiles/r02_medium_defer.txt) */
#endif
/* what a popped node entry `e` does once its record `nd` is there */
template <class Cfg, bool MEDIA, class Stack, class NS>
RT_HD void rt_walk_visit(const RtSceneView& sc, const NS& ns, RtWalk& k, RtRng& rng, Stack& stk, uint32_t e, const RtNodeHot& nd) {
    const uint32_t km = nd.kind & RT_KIND_MASK;
    RT_STAT_VISIT(km);
    /* the kinds are numbered so that each class is a range: the most frequent one costs one compare */
    if (km <= RT_BVH1) rt_walk_box<Cfg, false, NS>(k, e, nd, stk); /* the slab test without early exits (they paid while media boundaries were walked) */
    else if (km <= RT_YZ) rt_walk_leaf<Cfg, NS>(sc, k, e, nd);
    else if (Cfg::scope_depth > 0 && km <= RT_FLIP) rt_walk_wrap<NS>(k, e, nd, stk); /* scope_depth 0: the scene has no wrapper node */
    else if (Cfg::media) rt_walk_other<Cfg, MEDIA>(sc, ns, k, e, nd, rng, stk);
}
/* one stack entry */
template <class Cfg, bool MEDIA, class Stack, class NS>
RT_HD void rt_walk_step(const RtSceneView& sc, const NS& ns, RtWalk& k, RtRng& rng, Stack& stk) {
    uint32_t e = stk.pop();
    if (Cfg::scope_depth > 0 && (e & RT_POP_FLAG)) { rt_walk_exit(sc, k, e); return; }
    const RtNodeHot nd = ns.hot(e); /* the hot 64 bytes, fetched in one go */
    rt_walk_visit<Cfg, MEDIA>(sc, ns, k, rng, stk, e, nd);
}

/* a step that only a BVH node takes: the lane pops its next entry and, if that is a BVH node, tests its box and pushes the children;
 * any other entry is put back untouched and waits for the next full step.  Same visits, same order per lane -- it only lets the
 * lanes that are between boxes (84 % of final_scene's visits) advance several nodes for each execution of the rare kinds' code
 * (media, wrappers, primitives), which a full step runs for two or three lanes of the wave. */
template <class Cfg, class Stack, class NS>
RT_HD bool rt_walk_box_step(const NS& ns, RtWalk& k, Stack& stk) {
    const uint32_t e = stk.pop();
    bool taken = false;
    if (!(Cfg::scope_depth > 0 && (e & RT_POP_FLAG))) {
        const RtNodeHot nd = ns.hot(e);
        if ((nd.kind & RT_KIND_MASK) <= RT_BVH1) { RT_STAT_VISIT(nd.kind & RT_KIND_MASK); rt_walk_box<Cfg, false, NS>(k, e, nd, stk); taken = true; }
    }
    if (!taken) stk.sp += 1; /* the entry is still where it was */
    return taken;
}

/* a full step that leaves a ConstantMedium where it is (the lane waits for the next step that takes media): everything else as
 * rt_walk_step.  A medium is the longest piece of the walk by far (two sphere roots, a logarithm, a draw) and runs for two or three
 * lanes of a wave: a kernel that alternates between the two kinds of step executes that code half as often. */
template <class Cfg, class Stack, class NS>
RT_HD void rt_walk_light_step(const RtSceneView& sc, const NS& ns, RtWalk& k, Stack& stk) {
    const uint32_t e = stk.pop();
    if (Cfg::scope_depth > 0 && (e & RT_POP_FLAG)) { rt_walk_exit(sc, k, e); return; }
    const RtNodeHot nd = ns.hot(e);
    const uint32_t km = nd.kind & RT_KIND_MASK;
    if (km <= RT_BVH1) { RT_STAT_VISIT(km); rt_walk_box<Cfg, false, NS>(k, e, nd, stk); }
    else if (km <= RT_YZ) { RT_STAT_VISIT(km); rt_walk_leaf<Cfg, NS>(sc, k, e, nd); }
    else if (Cfg::scope_depth > 0 && km <= RT_FLIP) { RT_STAT_VISIT(km); rt_walk_wrap<NS>(k, e, nd, stk); }
    else stk.sp += 1;
}

/* the same for a primitive (sphere, moving sphere, rect): a step that only a lane whose next entry is a primitive takes */
template <class Cfg, class Stack, class NS>
RT_HD bool rt_walk_prim_step(const RtSceneView& sc, const NS& ns, RtWalk& k, Stack& stk) {
    const uint32_t e = stk.pop();
    bool taken = false;
    if (!(Cfg::scope_depth > 0 && (e & RT_POP_FLAG))) {
        const RtNodeHot nd = ns.hot(e);
        const uint32_t km = nd.kind & RT_KIND_MASK;
        if (km > RT_BVH1 && km <= RT_YZ) { RT_STAT_VISIT(km); rt_walk_leaf<Cfg, NS>(sc, k, e, nd); taken = true; }
    }
    if (!taken) stk.sp += 1;
    return taken;
}

template <class Cfg, bool MEDIA, class Stack, class NS>
RT_HD bool rt_traverse_stack(const RtSceneView& sc, const NS& ns, uint32_t root, const RtRay& world, double t_min,
                             double t_max, RtRng& rng, Stack& stk, double& out_t, uint32_t& out_prim,
                             uint32_t& out_scope, const RtV3* inv_known) {
    RtWalk k;
    rt_walk_begin(k, root, world, t_min, t_max, stk, inv_known);
    if constexpr (MEDIA && Cfg::media && RT_MEDIUM_DEFER != 0) {
        /* A ConstantMedium costs two complete boundary walks, a logarithm and a draw (rt_walk_other), and the lanes of a wave
         * reach their media at different steps: run in place, that code executes once per lane with the other 63 waiting
         * (final_scene: every ray crosses the global fog, constant_medium.rs:58-113 -- 8.7 % of the lanes active, PMC).  So a
         * lane that pops a medium PARKS on it (it simply does not pop again) while the others walk on, and the wave runs the
         * medium code for all parked lanes together once no lane can step (RT_MEDIUM_DEFER 1) or once at least as many lanes
         * are parked as still walk (2).  A lane's own sequence of operations is untouched -- it only waits -- so every bit
         * of its result is; on the CPU build (one lane) "no lane can step" is true at once and this is the plain loop. */
        uint32_t parked = RT_NONE;
        for (;;) {
            const bool can_step = parked == RT_NONE && !rt_walk_done(k, stk);
#if defined(__HIP_DEVICE_COMPILE__)
            const unsigned long long stepping = __ballot(can_step), waiting = __ballot(parked != RT_NONE);
            if (stepping == 0ull && waiting == 0ull) break;
            const bool round = stepping == 0ull || (RT_MEDIUM_DEFER == 2 && __popcll(waiting) >= __popcll(stepping));
#else
            if (!can_step && parked == RT_NONE) break;
            const bool round = !can_step;
#endif
            if (round) {
                if (parked != RT_NONE) {
                    rt_walk_other<Cfg, MEDIA>(sc, ns, k, parked, ns.hot(parked), rng, stk);
                    parked = RT_NONE;
                }
                continue;
            }
            if (can_step) {
                const uint32_t e = stk.pop();
                if (e & RT_POP_FLAG) { rt_walk_exit(sc, k, e); continue; }
                const RtNodeHot nd = ns.hot(e);
                const uint32_t cls = rt_walk_class(nd.kind & RT_KIND_MASK);
                RT_STAT_VISIT(nd.kind & RT_KIND_MASK);
                if (cls == RT_WK_BOX) rt_walk_box<Cfg, false, NS>(k, e, nd, stk);
                else if (cls == RT_WK_LEAF) rt_walk_leaf<Cfg, NS>(sc, k, e, nd);
                else if (cls == RT_WK_WRAP) rt_walk_wrap<NS>(k, e, nd, stk);
                else parked = e;
            }
        }
    } else {
        while (!rt_walk_done(k, stk)) rt_walk_step<Cfg, MEDIA>(sc, ns, k, rng, stk);
    }
    out_t = k.best_t; out_prim = k.best_prim; out_scope = k.best_scope;
    return k.best_prim != RT_NONE;
}

/* The same walk with fewer steps: the lane keeps its CURRENT node in a register (stepping into the left child costs no stack
 * traffic), and a box node is visited together with its left child when that is a box too -- the reference tests the left
 * child immediately after the parent with the same closest hit (bvh.rs:36-39), so doing both in one step changes neither the
 * order nor any operand.  The left child's record is the next one in memory and is requested with the parent's (the node
 * array carries one spare record at its end).  The walk is paced by the latency and the bookkeeping of a step, not by the
 * slab arithmetic (PMC), so fewer, fatter steps pay: 48 -> 33 steps per segment on random_scene. */
/* RT_WALK_MODE: 0 = the classic loop (every visit is a pop), 1 = current node in a register (stepping into the first child
 * costs no stack traffic), 2 = 1 + the fused left child.  MEASURED (random_scene / final_scene, Mpaths/s): mode 0 475 / 117,
 * mode 2 395 / 105 -- the second record costs 16 registers in a kernel that already spills, and its loads compete with the
 * walk's own; mode 1: see DESIGN section 8.  Exactness of every mode is covered by the CPU tier (the tests build oracle B
 * with the library's default). */
#ifndef RT_WALK_MODE
#define RT_WALK_MODE 0
#endif
#define RT_FUSED_WALK (RT_WALK_MODE == 2)
template <class Cfg, class Stack>
RT_HD void rt_walk_push_children(RtWalk& k, uint32_t e, const RtNodeHot& nd, Stack& stk, uint32_t& first) {
    /* children of a BVH node whose box was hit: `first` is visited next, the other one (if any) is pushed */
    first = e + 1u;
    if ((nd.kind & RT_KIND_MASK) == RT_BVH2) {
        uint32_t second = nd.b;
        const uint32_t ord = Cfg::ordered ? (nd.kind >> RT_BVH_ORDER_SHIFT) & RT_BVH_ORDER_MASK : 0u;
        if (Cfg::ordered && ord != 0u) {
            const double da = ord == 1u ? k.cur.d.x : (ord == 2u ? k.cur.d.y : k.cur.d.z);
            const bool left_lower = (nd.kind & RT_BVH_LEFT_LOWER) != 0u;
            if ((da < RT_R(0.0) && left_lower) || (da > RT_R(0.0) && !left_lower)) { first = nd.b; second = e + 1u; }
        }
        stk.push(second);
    }
}
template <class Cfg, bool EARLY>
RT_HD bool rt_walk_slab(const RtWalk& k, const RtNodeHot& nd) {
    if (RT_WAVE_ANY(k.tmin_nan || rt_isnan(k.best_t))) return rt_aabb_hit(nd.d, k.cur.o, k.inv, k.t_min, k.best_t);
    return rt_aabb_hit_fast<EARLY>(nd.d, k.cur.o, k.inv, k.t_min, k.best_t);
}
template <class Cfg, bool MEDIA, class Stack, class NS>
RT_HD bool rt_traverse_stack_fused(const RtSceneView& sc, const NS& ns, uint32_t root, const RtRay& world, double t_min,
                                   double t_max, RtRng& rng, Stack& stk, double& out_t, uint32_t& out_prim, uint32_t& out_scope) {
    RtWalk k;
    k.w.o = world.o; k.w.d = world.d;
    k.cur = k.w;
    k.inv_w = rt_inv3(k.w.d);
    k.inv = k.inv_w;
    k.time = world.time; k.t_min = t_min; k.best_t = t_max;
    k.scope = RT_NONE; k.best_prim = RT_NONE; k.best_scope = RT_NONE;
    k.tmin_nan = rt_isnan(t_min);
    k.base = stk.sp;
    uint32_t e = root;
    for (;;) {
        bool do_pop = true;
        if (e & RT_POP_FLAG) {
            rt_walk_exit(sc, k, e);
        } else {
            const RtNodeHot nd = ns.hot(e);
            const RtNodeHot nl = RT_FUSED_WALK ? ns.hot(e + 1u) : nd; /* the next record in pre-order = the left child of a BVH node */
            const uint32_t cls = rt_walk_class(nd.kind & RT_KIND_MASK);
            RT_STAT_VISIT(nd.kind & RT_KIND_MASK);
            if (cls == RT_WK_BOX) {
                if (rt_walk_slab<Cfg, Cfg::media>(k, nd)) {
                    uint32_t first;
                    rt_walk_push_children<Cfg>(k, e, nd, stk, first);
                    const bool left_first = first == e + 1u;
                    e = first;
                    do_pop = false;
                    /* the left child in the same step when it is a box too (same closest hit: nothing happened in between) */
                    if (RT_FUSED_WALK && left_first && rt_walk_class(nl.kind & RT_KIND_MASK) == RT_WK_BOX) {
                        RT_STAT_VISIT(nl.kind & RT_KIND_MASK);
                        if (rt_walk_slab<Cfg, Cfg::media>(k, nl)) {
                            uint32_t f2;
                            rt_walk_push_children<Cfg>(k, e, nl, stk, f2);
                            e = f2;
                        } else {
                            do_pop = true;
                        }
                    }
                }
            } else if (cls == RT_WK_LEAF) {
                rt_walk_leaf<Cfg>(sc, k, e, nd);
            } else if (cls == RT_WK_WRAP) {
                const uint32_t kind = nd.kind & RT_KIND_MASK;
                stk.push(e | RT_POP_FLAG);
                k.scope = e;
                if (kind != RT_FLIP) {
                    k.cur = rt_scope_in(nd, k.cur);
                    if (kind == RT_ROTATE_Y) k.inv = rt_inv3(k.cur.d);
                }
                e = e + 1u;
                do_pop = false;
            } else {
                rt_walk_other<Cfg, MEDIA>(sc, ns, k, e, nd, rng, stk);
            }
        }
        if (do_pop) {
            if (stk.sp <= k.base) break;
            e = stk.pop();
        }
    }
    out_t = k.best_t; out_prim = k.best_prim; out_scope = k.best_scope;
    return k.best_prim != RT_NONE;
}

/* The same traversal without a stack, for small scenes.  Nodes are stored in
 * depth-first pre-order and every node knows where its subtree ends (`skip`), so
 * the reference's walk (left subtree, then right subtree) is "visit node n, then
 * either n+1 or skip[n]": each lane keeps only the index `cur` of the next node it
 * has to visit.  The loop index n is the same in all lanes of a wave, so the node
 * record comes in through SCALAR loads, the node kind is a scalar branch (no
 * divergence between node kinds), and lanes that do not visit node n just sit out
 * that step.  Every lane still visits exactly the nodes the stack walk would, in
 * the same order, with the same arithmetic. */
template <class Cfg, bool MEDIA, class NS>
RT_HD bool rt_traverse_sweep(const RtSceneView& sc, const NS& ns, uint32_t root, const RtRay& world, double t_min,
                             double t_max, RtRng& rng, double& out_t, uint32_t& out_prim, uint32_t& out_scope) {
    const RtNode* nodes = sc.nodes;
    RtRayOD w; w.o = world.o; w.d = world.d;
    RtRayOD cur_ray = w;
    const RtV3 inv_w = rt_inv3(w.d);
    RtV3 inv = inv_w;
    uint32_t scope = RT_NONE, scope_end = RT_NONE;
    double best_t = t_max;
    uint32_t best_prim = RT_NONE, best_scope = RT_NONE;
    const bool tmin_nan = rt_isnan(t_min);
    const uint32_t end = ns.hot(root).skip;
    uint32_t cur = root;
    for (uint32_t n = root; n < end; ++n) {
        const RtNodeHot nd = ns.hot(n);
        /* lanes whose wrapper's subtree ended before n go back to the parent's ray */
        if (RT_WAVE_ANY(scope_end <= n)) {
            if (scope_end <= n) {
                do {
                    scope = nodes[scope].b;
                    scope_end = (scope == RT_NONE) ? RT_NONE : nodes[scope].skip;
                } while (scope_end <= n);
                /* the parent's ray, recomputed from the outer ray by the operations that made it */
                if (scope == RT_NONE) { cur_ray = w; inv = inv_w; }
                else { cur_ray = rt_ray_in_scope(nodes, scope, w); inv = rt_inv3(cur_ray.d); }
            }
        }
        bool active = (cur == n);
        if (!RT_WAVE_ANY(active)) continue;
        const uint32_t kind = nd.kind & RT_KIND_MASK;
        if (active) {
            RT_STAT_VISIT(kind);
            if (kind <= RT_BVH1) {
                bool hit;
                if (RT_WAVE_ANY(tmin_nan || rt_isnan(best_t))) hit = rt_aabb_hit(nd.d, cur_ray.o, inv, t_min, best_t);
                else hit = rt_aabb_hit_fast<Cfg::media>(nd.d, cur_ray.o, inv, t_min, best_t);
                cur = hit ? n + 1u : nd.skip;
            } else if (kind <= RT_YZ) {
                double t;
                bool hit;
                if (Cfg::msphere && kind == RT_MSPHERE) hit = rt_prim_t<Cfg>(nodes[n], kind, cur_ray.o, cur_ray.d, world.time, t_min, best_t, t);
                else hit = rt_prim_hot_t(nd, kind, cur_ray.o, cur_ray.d, t_min, best_t, t);
                if (hit) { best_t = t; best_prim = n; best_scope = scope; }
                cur = n + 1u;
            } else if (kind <= RT_FLIP) {
                scope = n; scope_end = nd.skip;
                if (kind == RT_TRANSLATE) {
                    cur_ray.o = cur_ray.o - rt_v3(nd.d[0], nd.d[1], nd.d[2]);
                } else if (kind == RT_ROTATE_Y) {
                    double sn = nd.d[0], cs = nd.d[1];
                    RtV3 o = cur_ray.o, d = cur_ray.d;
                    cur_ray.o.x = cs * o.x - sn * o.z;
                    cur_ray.o.z = sn * o.x + cs * o.z;
                    cur_ray.d.x = cs * d.x - sn * d.z;
                    cur_ray.d.z = sn * d.x + cs * d.z;
                    inv = rt_inv3(cur_ray.d);
                }
                cur = n + 1u;
            } else {
                if (MEDIA && Cfg::media && kind == RT_MEDIUM) {
                    const RtNode& full = nodes[n];
                    RtRay br; br.o = cur_ray.o; br.d = cur_ray.d; br.time = world.time;
                    double t1, t2, t; uint32_t p_, s_;
                    if (rt_traverse_sweep<Cfg, false>(sc, ns, n + 1u, br, -RT_INF, RT_INF, rng, t1, p_, s_) &&
                        rt_traverse_sweep<Cfg, false>(sc, ns, n + 1u, br, t1 + RT_R(0.0001), RT_INF, rng, t2, p_, s_) &&
                        rt_medium_t(full, cur_ray.d, t1, t2, t_min, best_t, rng, t)) {
                        best_t = t; best_prim = n; best_scope = scope;
                    }
                }
                cur = nd.skip;
            }
        }
    }
    out_t = best_t; out_prim = best_prim; out_scope = best_scope;
    return best_prim != RT_NONE;
}

/* Slab products a box shares with its ancestors (the unrolled sweep only).  In a median-split tree a child box keeps most of its
 * parent's faces, and for one ray in one ray space equal bound bits give equal products `(bound - o) * inv`.  The generator (jit.cpp:
 * jit_slab_reuse) says which: Topo::reuse[I][k] names, for plane k of BVH node I (0-2 min x/y/z, 3-5 max x/y/z), the nearest ancestor
 * BVH node in the same ray space whose d[k] holds the same 8 bytes, or I itself.  Every box test leaves its six products and the three
 * swapped pairs in a frame; the frames of the boxes above it are found by node index at compile time (the chain is a type), and a lane
 * reads a frame only after it passed that box, i.e. after it filled it.  A Topo without the table reuses nothing. */
template <class T> struct RtVoid { typedef void type; };
template <class Topo, class = void>
struct RtSlabReuse { static constexpr uint32_t of(uint32_t i, uint32_t) { return i; } };
template <class Topo>
struct RtSlabReuse<Topo, typename RtVoid<decltype(Topo::reuse)>::type> { static constexpr uint32_t of(uint32_t i, uint32_t k) { return Topo::reuse[i][k]; } };
struct RtSlabNone {}; /* the empty chain: the root of a sweep, below a Translate / RotateY, inside a medium's boundary sweeps */
template <uint32_t J, class Up>
struct RtSlabFrame {
    double p[6];         /* (d[k] - o) * inv, before the swap */
    double lo[3], hi[3]; /* the pairs after the `inv < 0` swap */
    const Up& up;
    RT_HD explicit RtSlabFrame(const Up& u) : up(u) {}
};
template <uint32_t J, uint32_t K, class Up>
RT_HD const auto& rt_slab_find(const RtSlabFrame<K, Up>& f) {
    if constexpr (J == K) return f;
    else return rt_slab_find<J>(f.up); /* no overload for RtSlabNone: a table that names a node off the chain does not compile */
}
/* One box test of the unrolled sweep: rt_aabb_hit (LITERAL) or rt_aabb_hit_fast<EARLY> with the products taken from the chain where the
 * table allows it -- the same operands reach the same operations in the same order, so the same bits.  Both forms fill the frame: a
 * descendant may run the other one. */
template <class Topo, uint32_t I, bool LITERAL, bool EARLY, class Up>
RT_HD bool rt_aabb_hit_chain(const double* bb, RtV3 o, RtV3 inv, double t_min, double t_max, RtSlabFrame<I, Up>& fr) {
    bool open = true;
#define RT_SLAB(A, ov, iv)                                                                            \
    {                                                                                                 \
        constexpr uint32_t j0 = RtSlabReuse<Topo>::of(I, A), j1 = RtSlabReuse<Topo>::of(I, A + 3u);   \
        if constexpr (j0 != I && j0 == j1) { /* both planes from one box: its swapped pair as it is */ \
            const auto& a = rt_slab_find<j0>(fr.up);                                                  \
            fr.p[A] = a.p[A]; fr.p[A + 3] = a.p[A + 3]; fr.lo[A] = a.lo[A]; fr.hi[A] = a.hi[A];       \
        } else {                                                                                      \
            if constexpr (j0 != I) fr.p[A] = rt_slab_find<j0>(fr.up).p[A];                            \
            else fr.p[A] = (bb[A] - (ov)) * (iv);                                                     \
            if constexpr (j1 != I) fr.p[A + 3] = rt_slab_find<j1>(fr.up).p[A + 3];                    \
            else fr.p[A + 3] = (bb[A + 3] - (ov)) * (iv);                                             \
            double t0 = fr.p[A], t1 = fr.p[A + 3];                                                    \
            if ((iv) < RT_R(0.0)) { double s_ = t0; t0 = t1; t1 = s_; }                               \
            fr.lo[A] = t0; fr.hi[A] = t1;                                                             \
        }                                                                                             \
        if constexpr (LITERAL) {                                                                      \
            t_min = fr.lo[A] > t_min ? fr.lo[A] : t_min;                                              \
            t_max = fr.hi[A] < t_max ? fr.hi[A] : t_max;                                              \
            if (t_max <= t_min) return false;                                                         \
        } else {                                                                                      \
            t_min = rt_vmax(fr.lo[A], t_min);                                                         \
            t_max = rt_vmin(fr.hi[A], t_max);                                                         \
            if (EARLY) { if (t_max <= t_min) return false; }                                          \
            else open = open & !(t_max <= t_min);                                                     \
        }                                                                                             \
    }
    RT_SLAB(0, o.x, inv.x)
    RT_SLAB(1, o.y, inv.y)
    RT_SLAB(2, o.z, inv.z)
#undef RT_SLAB
    return open;
}

/* The same sweep for a scene whose node kinds and subtree ends are known at compile time (Topo::kind[], Topo::skip[]):
 * the loop over n is unrolled into straight-line code that follows the tree -- a subtree's code is guarded by "some
 * lane of the wave is at its root", node kinds need no dispatch, the node record of step I is fetched at a constant
 * offset, and a wrapper's subtree simply runs with the inner ray while the outer one stays live.  Every lane still
 * visits exactly the nodes of the reference's walk, in its order, with the same arithmetic.
 * No lane keeps a node index here: "the lane is at node J" is "the lane passed the box test of every BVH node above J", and after a
 * subtree every lane that entered it stands at its end -- so `act` goes down the recursion, a BVH node's children get `act && hit`,
 * and what follows the subtree gets `act` again.  `up` is the chain of slab frames of the BVH nodes above I in this ray space. */
template <class Topo, class Cfg, bool MEDIA, uint32_t I, uint32_t END, class Up, class NS, class Inv>
RT_HD void rt_sweep_static(const RtSceneView& sc, const NS& ns, const RtRayOD& ray, const Inv& inv, double time, double t_min,
                           bool tmin_nan, RtRng& rng, const bool act, const Up& up, double& best_t, uint32_t& best_prim) {
    if constexpr (I < END) {
        constexpr uint32_t kind = Topo::kind[I] & RT_KIND_MASK;
        constexpr uint32_t skip = Topo::skip[I];
        if constexpr (kind <= RT_BVH1) {
            if (RT_WAVE_ANY(act)) {
                const RtNodeHot nd = ns.hot(I);
                RtSlabFrame<I, Up> fr(up);
                bool hit = false;
                if (act) {
                    if (RT_WAVE_ANY(tmin_nan || rt_isnan(best_t))) { RT_STAT_SLAB(1); hit = rt_aabb_hit_chain<Topo, I, true, false>(nd.d, ray.o, rt_inv_of(inv), t_min, best_t, fr); }
                    else { RT_STAT_SLAB(0); hit = rt_aabb_hit_chain<Topo, I, false, Cfg::media>(nd.d, ray.o, rt_inv_of(inv), t_min, best_t, fr); }
                }
                rt_sweep_static<Topo, Cfg, MEDIA, I + 1u, skip>(sc, ns, ray, inv, time, t_min, tmin_nan, rng, act && hit, fr, best_t, best_prim);
            }
            rt_sweep_static<Topo, Cfg, MEDIA, skip, END>(sc, ns, ray, inv, time, t_min, tmin_nan, rng, act, up, best_t, best_prim);
        } else if constexpr (kind <= RT_YZ) {
            if (RT_WAVE_ANY(act)) {
                const RtNodeHot nd = ns.hot(I);
                if constexpr (RtInvIsShared<Inv>::value && (RT_DIV_SHARED_ON & 2) != 0 && kind >= RT_XY) {
                    double t;
                    if (rt_rect_hot_t(nd, kind, ray.o, ray.d, inv, act, t_min, best_t, t)) { best_t = t; best_prim = I; }
                } else if (act) {
                    double t;
                    bool hit;
                    if constexpr (Cfg::msphere && kind == RT_MSPHERE) hit = rt_prim_t<Cfg>(sc.nodes[I], kind, ray.o, ray.d, time, t_min, best_t, t);
                    else hit = rt_prim_hot_t(nd, kind, ray.o, ray.d, t_min, best_t, t);
                    if (hit) { best_t = t; best_prim = I; }
                }
            }
            rt_sweep_static<Topo, Cfg, MEDIA, I + 1u, END>(sc, ns, ray, inv, time, t_min, tmin_nan, rng, act, up, best_t, best_prim);
        } else if constexpr (kind <= RT_FLIP) {
            if (RT_WAVE_ANY(act)) {
                if constexpr (kind == RT_FLIP) {
                    rt_sweep_static<Topo, Cfg, MEDIA, I + 1u, skip>(sc, ns, ray, inv, time, t_min, tmin_nan, rng, act, up, best_t, best_prim);
                } else {
                    /* Translate::hit hittable.rs:207-211 / RotateY::hit :238-251: another ray space, the chain starts empty */
                    const RtNodeHot nd = ns.hot(I);
                    const RtRayOD inner = rt_scope_in_k<kind>(nd, ray);
                    const RtSlabNone none;
                    if constexpr (kind == RT_ROTATE_Y) {
                        const Inv inv_inner = rt_inv_again(inv, inner.d, act);
                        rt_sweep_static<Topo, Cfg, MEDIA, I + 1u, skip>(sc, ns, inner, inv_inner, time, t_min, tmin_nan, rng, act, none, best_t, best_prim);
                    } else {
                        rt_sweep_static<Topo, Cfg, MEDIA, I + 1u, skip>(sc, ns, inner, inv, time, t_min, tmin_nan, rng, act, none, best_t, best_prim);
                    }
                }
            }
            rt_sweep_static<Topo, Cfg, MEDIA, skip, END>(sc, ns, ray, inv, time, t_min, tmin_nan, rng, act, up, best_t, best_prim);
        } else {
            if (RT_WAVE_ANY(act)) {
                if (act) {
                    if constexpr (MEDIA && Cfg::media && kind == RT_MEDIUM) {
                        /* ConstantMedium::hit constant_medium.rs:58-113: the boundary is a sweep of its own subtree, from an empty chain */
                        const RtNode& full = sc.nodes[I];
                        double t1 = RT_INF, t2 = RT_INF, t;
                        uint32_t p1 = RT_NONE, p2 = RT_NONE;
                        const RtSlabNone none;
                        rt_sweep_static<Topo, Cfg, false, I + 1u, skip>(sc, ns, ray, inv, time, -RT_INF, false, rng, true, none, t1, p1);
                        if (p1 != RT_NONE) {
                            const double lo = t1 + RT_R(0.0001);
                            rt_sweep_static<Topo, Cfg, false, I + 1u, skip>(sc, ns, ray, inv, time, lo, rt_isnan(lo), rng, true, none, t2, p2);
                            if (p2 != RT_NONE && rt_medium_t(full, ray.d, t1, t2, t_min, best_t, rng, t)) { best_t = t; best_prim = I; }
                        }
                    }
                }
            }
            rt_sweep_static<Topo, Cfg, MEDIA, skip, END>(sc, ns, ray, inv, time, t_min, tmin_nan, rng, act, up, best_t, best_prim);
        }
    }
}

/* The unrolled sweep without box tests (RT_BOX_FREE; DESIGN.md "Sweep without boxes").  Since the rects' quotients come from one
 * prepared divisor per axis, every lane computes every rect whatever `act` says, and in a scene of a dozen leaves nearly every wave
 * has a lane in every subtree: the box tests gate verdicts, they save no work.  So: speculate, then verify, with the machinery of
 * the shared divisors (a wave mask `bad`, and the parent's own sweep once more for a wave that has a lane in it).
 *   rt_sweep_free: a BVH node tests nothing; every lane visits every leaf in the reference's order, leaf tests and wrapper entries
 *     statement for statement.  It ends on the smallest candidate t, among equal ones on the last in sweep order.
 *   rt_box_free_verify: in every ray space on the way to that leaf, the INNERMOST box above it (Topo::vbox) must pass the reference's
 *     own test with t_max = T, the closest candidate among the leaves BEFORE it in sweep order (or the caller's t_max): what the running
 *     t_max was when the hit was accepted.  The reference's t_max at any box on the way is a minimum over some of those leaves, hence at
 *     or above T.  The boxes of one space are nested bit for bit and `(bound - o) * inv` is monotone in the bound, so every box above
 *     passed as well, each at its own, larger t_max: the reference reached the leaf and accepted it.  (Not the final t itself: a box face
 *     in the plane of the rect that is hit -- the top of a rotated box and its own world box -- would tie with it on half of the rays.)
 *   Anything the argument does not cover -- a NaN candidate or product, a divisor out of range (inv is then finite and non-zero
 *     in every ray space) -- sets the lane's bit.
 * The world space is verified after the sweep; the space below a Translate / RotateY where its subtree ends, on the inner ray the sweep
 * holds there, for the lanes whose closest hit so far lies in the subtree (for a lane that ends elsewhere a verdict too many).
 * Which units: f64, scene-specialised, no media, a rect, and Topo::box_free (jit.cpp: nested boxes, at most 64 nodes).  On the device
 * by default where the divisors are shared; RT1W_JIT_EXTRA_OPTS=-DRT_BOX_FREE=0 is the text without it.  A host build takes it with
 * -DRT_BOX_FREE=1: a wave of one lane, the mask a bool, quotients by `/`. */
#undef RT_BOX_FREE_ON /* (a unit may take this header twice: f64 records, then the f32 build) */
#if defined(RT_F32)
#define RT_BOX_FREE_ON 0
#elif defined(__HIP_DEVICE_COMPILE__)
#ifndef RT_BOX_FREE
#define RT_BOX_FREE 1
#endif
#define RT_BOX_FREE_ON ((RT_BOX_FREE) != 0 && (RT_DIV_SHARED_ON) == 3)
#elif defined(RT_BOX_FREE)
#define RT_BOX_FREE_ON ((RT_BOX_FREE) != 0)
#else
#define RT_BOX_FREE_ON 0
#endif
#ifndef RT1W_WAVE_MASK
#define RT1W_WAVE_MASK
/* the lanes of the wave for which `p` holds: a scalar register pair on the GPU, the one lane's own answer on the host */
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint64_t RtWaveMask;
RT_HD RtWaveMask rt_wave_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); }
#else
typedef bool RtWaveMask;
RT_HD RtWaveMask rt_wave_mask(bool p) { return p; }
#endif
#endif
template <class Topo, class = void>
struct RtBoxFreeTopo { static constexpr bool value = false; };
template <class Topo>
struct RtBoxFreeTopo<Topo, typename RtVoid<decltype(Topo::vbox)>::type> { static constexpr bool value = Topo::box_free; };
#if RT_BOX_FREE_ON
/* the common entry of the leaves [LO, HI) in column D of Topo::vbox, RT_NONE if they have none, RT_VBOX_MIXED if they differ */
#define RT_VBOX_MIXED 0xFFFFFFFEu
template <class Topo, uint32_t D, uint32_t LO, uint32_t HI>
constexpr uint32_t rt_vbox_common() {
    uint32_t c = RT_NONE;
    bool first = true;
    for (uint32_t i = LO; i < HI; ++i) {
        const uint32_t k = Topo::kind[i] & RT_KIND_MASK, v = Topo::vbox[i][D];
        if (k < RT_SPHERE || k > RT_YZ) continue;
        if (!first && c != v) return RT_VBOX_MIXED;
        c = v; first = false;
    }
    return c;
}
/* AABB::hit aabb.rs:13-32 as rt_aabb_hit_fast has it, for a t_min and t_max that are no NaN; a NaN product fails */
RT_HD bool rt_box_free_test(const double* bb, RtV3 o, RtV3 inv, double t_min, double t_max) {
    bool ok = true;
#define RT_SLAB(minv, maxv, ov, iv)                                 \
    {                                                               \
        double t0 = ((minv) - (ov)) * (iv);                         \
        double t1 = ((maxv) - (ov)) * (iv);                         \
        if ((iv) < RT_R(0.0)) { double s_ = t0; t0 = t1; t1 = s_; } \
        ok = ok & (t0 <= t1);                                       \
        t_min = rt_vmax(t0, t_min);                                 \
        t_max = rt_vmin(t1, t_max);                                 \
        ok = ok & (t_max > t_min);                                  \
    }
    RT_SLAB(bb[0], bb[3], o.x, inv.x)
    RT_SLAB(bb[1], bb[4], o.y, inv.y)
    RT_SLAB(bb[2], bb[5], o.z, inv.z)
#undef RT_SLAB
    return ok;
}
/* What a lane keeps as its closest leaf while it sweeps: the leaf's index in bits 0-7 and its row of Topo::vbox behind it, a byte per
 * ray space (0xFF: none; the fourth space of a three-wrapper chain is read from the table) -- a constant per leaf, so accepting a hit
 * is the one move it always was and the verification starts from a register, not from a table in memory.  RT_NONE is RT_NONE. */
template <class Topo>
constexpr uint32_t rt_vbox_word(uint32_t i) {
    static_assert(Topo::n <= 127u, "a node index is a byte here, and the sign-extended 0xFF is RT_NONE");
    uint32_t w = i;
    for (uint32_t s = 0u; s < 3u; ++s) w |= (Topo::vbox[i][s] == RT_NONE ? 0xFFu : Topo::vbox[i][s]) << (8u + 8u * s);
    return w;
}
RT_HD uint32_t rt_vbox_word_leaf(uint32_t word) { return (uint32_t)(int32_t)(int8_t)(word & 0xFFu); }
/* ray space D, entered for the leaves [LO, HI): a lane whose closest hit `word` is one of them verifies its box there.  The bounds
 * differ per lane, so they are data: six doubles of the node array (a few dozen records, cache-resident) by vector loads; where the
 * leaves share one box the index is a constant and the loads are scalar */
template <class Topo, uint32_t D, uint32_t LO, uint32_t HI>
RT_HD void rt_box_free_verify(const RtSceneView& sc, const RtRayOD& r, RtV3 inv, double t_min, double t, uint32_t word, RtWaveMask& bad) {
    constexpr uint32_t common = rt_vbox_common<Topo, D, LO, HI>();
    if constexpr (common != RT_NONE) {
        const bool mine = D == 0u ? word != RT_NONE : ((word & 0xFFu) - LO) < (HI - LO);
        if (RT_WAVE_ANY(mine)) {
            if constexpr (common != RT_VBOX_MIXED) {
                bad |= rt_wave_mask(mine & !rt_box_free_test(sc.nodes[common].d, r.o, inv, t_min, t));
            } else {
                uint32_t vb;
                if constexpr (D < 3u) vb = (word >> (8u + 8u * D)) & 0xFFu;
                else { vb = Topo::vbox[mine ? (word & 0xFFu) : LO][D]; vb = vb == RT_NONE ? 0xFFu : vb; }
                const bool need = mine & (vb != 0xFFu);
                bad |= rt_wave_mask(need & !rt_box_free_test(sc.nodes[need ? vb : LO].d, r.o, inv, t_min, t));
            }
        }
    }
}
/* 1 / direction of a ray space and the range check on its divisors: with the prepared divisors where they are shared, else by `/` */
RT_HD RtV3 rt_inv_free(RtV3 d, RtWaveMask& bad) {
    bad |= rt_wave_mask(!(rt_div_d_ok(d.x) & rt_div_d_ok(d.y) & rt_div_d_ok(d.z)));
    return rt_inv3(d);
}
RT_HD RtV3 rt_inv_free_again(const RtV3&, RtV3 d, RtWaveMask& bad) { return rt_inv_free(d, bad); }
#if RT_DIV_SHARED_ON
RT_HD RtInvShared rt_inv_free_again(const RtInvShared& s, RtV3 d, RtWaveMask&) { return rt_inv3_shared(d, true, s.bad); }
#endif
/* How far ahead of the leaf being tested the records of later leaves may be fetched.  The sweep is straight-line code, and left alone
 * the scheduler starts every leaf's scalar loads at the top: a dozen records are some 130 SGPRs, most of them spilled to VGPR lanes and
 * read back one v_readlane at a time.  So leaf I takes its record at index I + z, where z is a zero the compiler cannot see through and
 * that is not there before the verdict of the leaf RT_BOX_FREE_AHEAD nodes earlier is: the loads run that far ahead and no further. */
#ifndef RT_BOX_FREE_AHEAD
#define RT_BOX_FREE_AHEAD 3
#endif
#if defined(__HIP_DEVICE_COMPILE__) && RT_BOX_FREE_AHEAD > 0
struct RtSweepAhead { uint32_t tok[RT_BOX_FREE_AHEAD]; };
template <uint32_t I>
RT_HD uint32_t rt_sweep_ahead_index(const RtSweepAhead& a) {
    uint32_t z;
    asm("s_and_b32 %0, %1, 0" : "=s"(z) : "s"(a.tok[I % RT_BOX_FREE_AHEAD]) : "scc");
    return I + z;
}
/* The token of a leaf's verdict.  The wave mask of `hit` is a mask the compiler has to rebuild: `hit` is an `and` of compares, so its
 * ballot is a 0 / 1 per lane (v_cndmask) compared with 0 again, two vector instructions a leaf.  RT_AHEAD_WORD 1 takes the first lane's
 * closest-hit word after the leaf has been accepted or not instead: as late as the verdict, one v_readfirstlane -- and twice the scalar
 * spills (docs/LAB_NOTES.md).  RT_AHEAD_WORD 2 takes the low word of the wave mask of one compare `hit` is made of, which the compare
 * has written to scalar registers anyway (rt_rect_hot_t_tok, rt_sphere_root_tok: a rect's last bound test, a sphere's discriminant
 * test): no instruction at all, the same spills, ten pairs fewer in the Cornell unit -- and +0.45 % measured, 2.5 times the spread
 * where the project asks for four, so it is not the default either.  The token only has to exist no sooner than the leaf's
 * arithmetic; its value is and-ed with 0.  (0, the default: the mask of `hit`.) */
#ifndef RT_AHEAD_WORD
#define RT_AHEAD_WORD 0
#endif
template <uint32_t I>
RT_HD void rt_sweep_ahead_done(RtSweepAhead& a, bool hit, uint32_t word) {
#if RT_AHEAD_WORD == 1
    a.tok[I % RT_BOX_FREE_AHEAD] = __builtin_amdgcn_readfirstlane(word);
#else
    a.tok[I % RT_BOX_FREE_AHEAD] = (uint32_t)rt_wave_mask(hit);
#endif
}
#else
struct RtSweepAhead {};
template <uint32_t I> RT_HD uint32_t rt_sweep_ahead_index(const RtSweepAhead&) { return I; }
template <uint32_t I> RT_HD void rt_sweep_ahead_done(RtSweepAhead&, bool, uint32_t) {}
#endif
#undef RT_AHEAD_TOKEN_ON
#if defined(__HIP_DEVICE_COMPILE__) && RT_BOX_FREE_AHEAD > 0 && RT_AHEAD_WORD == 2
#define RT_AHEAD_TOKEN_ON 1
#else
#define RT_AHEAD_TOKEN_ON 0
#endif
template <class Topo, class Cfg, uint32_t D, uint32_t I, uint32_t END, class NS, class Inv>
RT_HD void rt_sweep_free(const RtSceneView& sc, const NS& ns, const RtRayOD& ray, const Inv& inv, double time, double t_min,
                         RtWaveMask& bad, double& best_t, double& prev_t, uint32_t& best_word, RtSweepAhead& ahead) {
    if constexpr (I < END) {
        constexpr uint32_t kind = Topo::kind[I] & RT_KIND_MASK;
        constexpr uint32_t skip = Topo::skip[I];
        if constexpr (kind <= RT_BVH1 || kind == RT_FLIP) {
            /* pre-order: the subtree is what follows */
            rt_sweep_free<Topo, Cfg, D, I + 1u, END>(sc, ns, ray, inv, time, t_min, bad, best_t, prev_t, best_word, ahead);
        } else if constexpr (kind <= RT_YZ) {
            const RtNodeHot nd = ns.hot(rt_sweep_ahead_index<I>(ahead));
            double t;
            bool hit;
#if RT_AHEAD_TOKEN_ON
            /* the kinds whose test hands the token out itself (RT_AHEAD_WORD 2); every other leaf's is the mask of its verdict */
            if constexpr (RtInvIsShared<Inv>::value && kind >= RT_XY) {
                hit = rt_rect_hot_t_tok(nd, kind, ray.o, ray.d, inv, true, t_min, best_t, t, ahead.tok[I % RT_BOX_FREE_AHEAD]);
                if (hit) { prev_t = best_t; best_t = t; best_word = rt_vbox_word<Topo>(I); }
            } else if constexpr (kind == RT_SPHERE) {
                hit = rt_sphere_root_tok(rt_v3(nd.d[0], nd.d[1], nd.d[2]), nd.d[3], ray.o, ray.d, t_min, best_t, t, ahead.tok[I % RT_BOX_FREE_AHEAD]); /* rt_prim_hot_t's call */
                bad |= rt_wave_mask(hit && rt_isnan(t));
                if (hit) { prev_t = best_t; best_t = t; best_word = rt_vbox_word<Topo>(I); }
            } else
#endif
            {
#if RT_DIV_SHARED_ON
                if constexpr (RtInvIsShared<Inv>::value && kind >= RT_XY) hit = rt_rect_hot_t(nd, kind, ray.o, ray.d, inv, true, t_min, best_t, t); /* (a NaN quotient is `big`) */
                else
#endif
                {
                    if constexpr (Cfg::msphere && kind == RT_MSPHERE) hit = rt_prim_t<Cfg>(sc.nodes[I], kind, ray.o, ray.d, time, t_min, best_t, t);
                    else hit = rt_prim_hot_t(nd, kind, ray.o, ray.d, t_min, best_t, t);
                    bad |= rt_wave_mask(hit && rt_isnan(t)); /* accepted as the reference accepts it, and every later leaf after it: not verifiable */
                }
                if (hit) { prev_t = best_t; best_t = t; best_word = rt_vbox_word<Topo>(I); }
                rt_sweep_ahead_done<I>(ahead, hit, best_word);
            }
            rt_sweep_free<Topo, Cfg, D, I + 1u, END>(sc, ns, ray, inv, time, t_min, bad, best_t, prev_t, best_word, ahead);
        } else if constexpr (kind <= RT_ROTATE_Y) {
            /* Translate::hit hittable.rs:207-211 / RotateY::hit :238-251: another ray space */
            const RtNodeHot nd = ns.hot(I);
            const RtRayOD inner = rt_scope_in_k<kind>(nd, ray);
            if constexpr (kind == RT_ROTATE_Y) {
                const Inv inv_inner = rt_inv_free_again(inv, inner.d, bad);
                rt_sweep_free<Topo, Cfg, D + 1u, I + 1u, skip>(sc, ns, inner, inv_inner, time, t_min, bad, best_t, prev_t, best_word, ahead);
                rt_box_free_verify<Topo, D + 1u, I + 1u, skip>(sc, inner, rt_inv_of(inv_inner), t_min, prev_t, best_word, bad);
            } else {
                rt_sweep_free<Topo, Cfg, D + 1u, I + 1u, skip>(sc, ns, inner, inv, time, t_min, bad, best_t, prev_t, best_word, ahead);
                rt_box_free_verify<Topo, D + 1u, I + 1u, skip>(sc, inner, rt_inv_of(inv), t_min, prev_t, best_word, bad);
            }
            rt_sweep_free<Topo, Cfg, D, skip, END>(sc, ns, ray, inv, time, t_min, bad, best_t, prev_t, best_word, ahead);
        } else {
            static_assert(kind <= RT_ROTATE_Y, "a unit with a medium keeps its boxes");
        }
    }
}
/* the speculative closest hit and the lanes that must not trust theirs (rt_closest_hit; tests/test_box_free.py reads both) */
template <class Cfg, class NS>
RT_HD RtWaveMask rt_closest_hit_free(const RtSceneView& sc, const NS& ns, const RtRayOD& w, double time, double t_min, double t_max,
                                     double& t, uint32_t& prim) {
    typedef typename Cfg::Topo Topo;
    /* a tiny quotient is trusted to fail t_min as the division's would: not with a t_min down there (or NaN) */
    RtWaveMask bad = rt_wave_mask(!rt_div_tmin_ok(t_min) | rt_isnan(t_max)); /* (nor with a NaN for t_max: nothing is "at or above" it) */
    t = t_max;
#if RT_DIV_SHARED_ON
    const RtInvShared inv = rt_inv3_shared(w.d, true, bad);
#else
    const RtV3 inv = rt_inv_free(w.d, bad);
#endif
    uint32_t word = RT_NONE;
    RtSweepAhead ahead = {};
    double prev = t_max; /* the closest candidate of the leaves before the one that holds the hit: what the boxes are verified against */
    rt_sweep_free<Topo, Cfg, 0u, Topo::root, Topo::skip[Topo::root]>(sc, ns, w, inv, time, t_min, bad, t, prev, word, ahead);
    rt_box_free_verify<Topo, 0u, Topo::root, Topo::skip[Topo::root]>(sc, w, rt_inv_of(inv), t_min, prev, word, bad);
    prim = rt_vbox_word_leaf(word);
    return bad;
}
#endif

template <class Topo, class = void>
struct RtHitShape; /* below, with the static hit record */
template <class Cfg, class Stack, class NS>
RT_HD bool rt_closest_hit(const RtSceneView& sc, const NS& ns, const RtRay& ray, double t_min, double t_max, RtRng& rng,
                          Stack& stk, double& t, uint32_t& prim, uint32_t& scope) {
    if constexpr (Cfg::sweep && !std::is_void<typename Cfg::Topo>::value) {
        typedef typename Cfg::Topo Topo;
        RtRayOD w; w.o = ray.o; w.d = ray.d;
        const RtSlabNone none;
        t = t_max; prim = RT_NONE;
#if RT_BOX_FREE_ON
        if constexpr (!Cfg::media && RtBoxFreeTopo<Topo>::value) {
            RtWaveMask bad = rt_closest_hit_free<Cfg>(sc, ns, w, ray.time, t_min, t_max, t, prim);
#if RT_DIV_SHARED_FORCE_SLOW
#if defined(__HIP_DEVICE_COMPILE__)
            { uint64_t all = ~0ull; asm volatile("" : "+s"(all)); bad |= all; } /* opaque: the first sweep stays, the second always runs */
#else
            bad = true;
#endif
#endif
            if (bad != 0) { /* some lane could not be verified: the whole wave once more, with boxes and `/` */
                RT_STAMP(2);
                const RtV3 inv = rt_inv3(w.d);
                t = t_max; prim = RT_NONE;
                rt_sweep_static<Topo, Cfg, true, Topo::root, Topo::skip[Topo::root]>(sc, ns, w, inv, ray.time, t_min, rt_isnan(t_min), rng, true, none, t, prim);
                RT_STAMP(14);
            }
        } else
#endif
#if RT_DIV_SHARED_ON
        if constexpr (!Cfg::media && rt_topo_has_rect<Topo>()) {
            /* a tiny quotient is trusted to fail t_min as the division's would: not with a t_min down there (or NaN) */
            uint64_t bad = __builtin_amdgcn_ballot_w64(!rt_div_tmin_ok(t_min));
#if RT_DIV_SHARED_FORCE_SLOW
            { uint64_t all = ~0ull; asm volatile("" : "+s"(all)); bad |= all; } /* opaque: the first sweep stays, the second always runs */
#endif
            const RtInvShared shared = rt_inv3_shared(w.d, true, bad);
            rt_sweep_static<Topo, Cfg, true, Topo::root, Topo::skip[Topo::root]>(sc, ns, w, shared, ray.time, t_min, rt_isnan(t_min), rng, true, none, t, prim);
            if (bad != 0ull) { /* some lane left the range: the whole wave once more, with `/` (a lane that was good gets its bits again) */
                RT_STAMP(2); /* diagnostic builds: the first sweep is traversal as ever, the second is bucket 14 (tools/stamps.py --jit) */
                const RtV3 inv = rt_inv3(w.d);
                t = t_max; prim = RT_NONE;
                rt_sweep_static<Topo, Cfg, true, Topo::root, Topo::skip[Topo::root]>(sc, ns, w, inv, ray.time, t_min, rt_isnan(t_min), rng, true, none, t, prim);
                RT_STAMP(14);
            }
        } else
#endif
        {
            const RtV3 inv = rt_inv3(w.d);
            rt_sweep_static<Topo, Cfg, true, Topo::root, Topo::skip[Topo::root]>(sc, ns, w, inv, ray.time, t_min, rt_isnan(t_min), rng, true, none, t, prim);
        }
        if constexpr (RtHitShape<Topo>::trace || RtHitShape<Topo>::carry) scope = RtHitShape<Topo>::scope_of(prim); /* a compile-time function of the leaf: no record is read */
        else scope = prim == RT_NONE ? RT_NONE : ns.hot(prim).b; /* leaves keep their innermost wrapper in `b` */
        return prim != RT_NONE;
    } else if constexpr (Cfg::sweep) return rt_traverse_sweep<Cfg, true>(sc, ns, sc.root, ray, t_min, t_max, rng, t, prim, scope);
    else if constexpr (RT_WALK_MODE != 0) return rt_traverse_stack_fused<Cfg, true>(sc, ns, sc.root, ray, t_min, t_max, rng, stk, t, prim, scope);
    else return rt_traverse_stack<Cfg, true>(sc, ns, sc.root, ray, t_min, t_max, rng, stk, t, prim, scope);
}

/* ------------------------------------------------------------ textures -- */

/* Perlin::noise perlin.rs:46-72 + perlin_interp :88-106 */
RT_HD double rt_perlin_noise(const RtPerlin& pl, RtV3 p) {
    double fx = rt_floor(p.x), fy = rt_floor(p.y), fz = rt_floor(p.z);
    double u = p.x - fx, v = p.y - fy, w = p.z - fz;
    /* `as isize` saturates where Rust does (perlin.rs:51-53): at 2^63 and below -2^63 (-2^63 itself converts exactly), NaN -> 0; & 255
     * afterwards.  Both constants are exact as floats too.  A floor in [9.2e18, 2^63) converts exactly: it is a multiple of 1024, so the
     * corners read perm[0] and perm[1] (tests/test_texture_kats.py) */
    int64_t i = (fx >= RT_R(9223372036854775808.0)) ? INT64_MAX : (fx < -RT_R(9223372036854775808.0)) ? INT64_MIN : (fx != fx ? 0 : (int64_t)fx);
    int64_t j = (fy >= RT_R(9223372036854775808.0)) ? INT64_MAX : (fy < -RT_R(9223372036854775808.0)) ? INT64_MIN : (fy != fy ? 0 : (int64_t)fy);
    int64_t k = (fz >= RT_R(9223372036854775808.0)) ? INT64_MAX : (fz < -RT_R(9223372036854775808.0)) ? INT64_MIN : (fz != fz ? 0 : (int64_t)fz);
    double uu = u * u * (RT_R(3.0) - RT_R(2.0) * u);
    double vv = v * v * (RT_R(3.0) - RT_R(2.0) * v);
    double ww = w * w * (RT_R(3.0) - RT_R(2.0) * w);
    double accum = RT_R(0.0);
    for (int di = 0; di < 2; ++di)
        for (int dj = 0; dj < 2; ++dj)
            for (int dk = 0; dk < 2; ++dk) {
                /* wrapping add like the release build of the reference */
                uint32_t ii = (uint32_t)(((uint64_t)i + (uint64_t)di) & 255u);
                uint32_t jj = (uint32_t)(((uint64_t)j + (uint64_t)dj) & 255u);
                uint32_t kk = (uint32_t)(((uint64_t)k + (uint64_t)dk) & 255u);
                uint32_t idx = pl.perm_x[ii] ^ pl.perm_y[jj] ^ pl.perm_z[kk];
                RtV3 c = rt_v3(pl.ranvec[idx * 3 + 0], pl.ranvec[idx * 3 + 1], pl.ranvec[idx * 3 + 2]);
                double fi = (double)di, fj = (double)dj, fk = (double)dk;
                RtV3 weight_v = rt_v3(u - fi, v - fj, w - fk);
                accum += (fi * uu + (RT_R(1.0) - fi) * (RT_R(1.0) - uu)) * (fj * vv + (RT_R(1.0) - fj) * (RT_R(1.0) - vv)) *
                         (fk * ww + (RT_R(1.0) - fk) * (RT_R(1.0) - ww)) * rt_dot(c, weight_v);
            }
    return accum;
}
/* Perlin::turb perlin.rs:74-86 */
RT_HD double rt_perlin_turb(const RtPerlin& pl, RtV3 p, int depth) {
    double accum = RT_R(0.0), weight = RT_R(1.0);
    RtV3 temp_p = p;
    for (int i = 0; i < depth; ++i) {
        accum += weight * rt_perlin_noise(pl, temp_p);
        weight *= RT_R(0.5);
        temp_p = temp_p * RT_R(2.0);
    }
    return rt_abs(accum);
}
/* `x as u32` of Rust: saturating, NaN -> 0 */
RT_HD uint32_t rt_as_u32(double x) {
    if (!(x > RT_R(0.0))) return 0u;
    if (x >= RT_R(4294967295.0)) return 4294967295u;
    return (uint32_t)x;
}
/* Texture::value texture.rs:40-89 */
template <class Cfg>
RT_HD RtV3 rt_texture(const RtSceneView& sc, uint32_t tex, double u, double v, RtV3 p) {
    if (!Cfg::tex) { /* every texture of the scene is a SolidColor */
        const RtTexture& t = sc.textures[tex];
        return rt_v3(t.d[0], t.d[1], t.d[2]);
    }
    for (;;) {
        const RtTexture& t = sc.textures[tex];
        if (t.kind == RT_TEX_CHECKER) {
            double sines = rt_sin(RT_R(10.0) * p.x) * rt_sin(RT_R(10.0) * p.y) * rt_sin(RT_R(10.0) * p.z);
            tex = (sines < RT_R(0.0)) ? t.a : t.b;
            continue;
        }
        if (t.kind == RT_TEX_SOLID) return rt_v3(t.d[0], t.d[1], t.d[2]);
        if (t.kind == RT_TEX_NOISE) {
            double s = RT_R(1.0) * RT_R(0.5) * (RT_R(1.0) + rt_sin(t.d[0] * p.z + RT_R(10.0) * rt_perlin_turb(sc.perlin[t.a], p, 7)));
            return rt_v3(s, s, s);
        }
        /* RT_TEX_IMAGE texture.rs:67-88 */
        double uc = u < RT_R(0.0) ? RT_R(0.0) : (u > RT_R(1.0) ? RT_R(1.0) : u);
        double vc = RT_R(1.0) - (v < RT_R(0.0) ? RT_R(0.0) : (v > RT_R(1.0) ? RT_R(1.0) : v));
        uint32_t i = rt_as_u32(uc * (double)t.a);
        uint32_t j = rt_as_u32(vc * (double)t.b);
        i = i < t.a - 1u ? i : t.a - 1u;
        j = j < t.b - 1u ? j : t.b - 1u;
        const uint8_t* px = sc.images + t.c + ((size_t)j * t.a + i) * 3u;
        const double COLOR_SCALE = RT_R(1.0) / RT_R(255.0);
        return rt_v3((double)px[0] * COLOR_SCALE, (double)px[1] * COLOR_SCALE, (double)px[2] * COLOR_SCALE);
    }
}

/* texture.value(u, v, p) of a material: a SolidColor's value is kept in the material record itself */
template <class Cfg>
RT_HD RtV3 rt_mat_colour(const RtSceneView& sc, const RtMaterial& m, double u, double v, RtV3 p) {
    if (!Cfg::tex || (m.kind & RT_MAT_SOLID) != 0u) return rt_v3(m.d[0], m.d[1], m.d[2]);
    return rt_texture<Cfg>(sc, m.tex, u, v, p);
}

/* ------------------------------------------------------------ samplers -- */

/* math.rs:6-18.  gen_range(-1.0..1.0) as rt_take_pm1: the same words and values as rt_take_range with those bounds, whose retry
 * (and the generator block it holds) can never run (include/rt1w_num.h) */
RT_HD RtV3 rt_random_in_unit_sphere(RtRng& rng) {
    for (;;) {
        rt_rng_reserve(rng, rt_rng_need_2u64(rng));
        double x = rt_take_pm1(rng);
        double y = rt_take_pm1(rng);
        rt_rng_reserve(rng, rt_rng_need_u64(rng));
        double z = rt_take_pm1(rng);
        RtV3 v = rt_v3(x, y, z);
        if (rt_mag2(v) < RT_R(1.0)) return v;
    }
}
/* math.rs:30-37 */
RT_HD RtV3 rt_random_in_unit_disk(RtRng& rng) {
    for (;;) {
        rt_rng_reserve(rng, rt_rng_need_2u64(rng));
        double x = rt_take_pm1(rng);
        double y = rt_take_pm1(rng);
        RtV3 p = rt_v3(x, y, RT_R(0.0));
        if (rt_mag2(p) < RT_R(1.0)) return p;
    }
}
/* ---- the two rejection samplers, a wave at a time ----
 * A wave pays every round of these loops in full while any one of its lanes is still rejecting: with 14 Metal lanes in a wave the
 * sphere loop runs 4.6 times where a lane needs 1.9 rounds, and each round generates up to two Philox blocks for a handful of
 * lanes.  Round r of a loop is a function of the stream's key and of where the loop was entered (include/rt1w_num.h:
 * rt_sphere_round / rt_disk_round), so here the lanes of the wave that want nothing evaluate further rounds of the loops of those
 * that do: K rounds of every loop in one pass, each loop stopping at its first accepted round -- the words, the values and the
 * stream position of the looped sampler, in fewer passes.  Every lane of the wave calls the function, `want` says whether it samples.
 *   K = the largest power of two with K <= RT_WAVE_ROUNDS_CAP and K x (lanes that want) <= 64, chosen anew for every pass; where
 * most of the wave wants a sample K is 1 and every lane takes its own loop's next round, nothing travels.  Otherwise the lanes find
 * each other with a ballot and mbcnt, and the key, the position and the accepted round travel by ds_permute / ds_bpermute: no LDS is
 * allocated.  Those instructions read nothing from a lane that is switched off, so a wave that is not whole here (the last passes of
 * a frame, where lanes have retired) keeps K = 1.  The stream is touched once, when its loop stops (rt_rng_after_round).
 * Device code of the f64 reordering kernels only (rt_kernel_sorted.h), where a wave mostly holds one class of paths and the others
 * are idle in these loops.  Parts (RT1W_JIT_EXTRA_OPTS=-DRT_WAVE_ROUNDS=k builds any mix of them into the kernels compiled at run
 * time, 0 the loops; every mix gives the same bits).  Measured on the Cornell kernel, ms per launch at 600x600x1000
 * (profiles/wave_rounds_bench.json): none 111.3; 1: 106.2; 2: 121.3; both: 115.8 -- the camera's loop is short (1.27 rounds a lane), most
 * of a regenerating wave wants a sample, and the hand-over costs more than the passes it saves: it stays behind the switch.
 *   1  the unit sphere of the Metal scatter (rt_path_shade_wave)      2  the unit disk of the camera ray (rt_path_begin_wave)
 * The cap on K, with part 1: 2: 110.6; 4: 106.8; 8: 106.3; 16: 106.3. */
#ifndef RT_WAVE_ROUNDS
#define RT_WAVE_ROUNDS 1
#endif
#ifndef RT_WAVE_ROUNDS_CAP
#define RT_WAVE_ROUNDS_CAP 8u
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RT_RNG_REFSTREAM) && !defined(RT_F32)
#define RT_WAVE_ROUNDS_ON (RT_WAVE_ROUNDS)
template <bool SPHERE>
__device__ __forceinline__ RtV3 rt_wave_rounds(RtRng& rng, bool want) {
    RtV3 out = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const bool whole = __ballot(1) == ~0ull;
    const RtRngPos start = rt_rng_pos_even(rng);
#define RT_FROM(l, v) ((uint32_t)__builtin_amdgcn_ds_bpermute((l), (int)(v)))
    for (uint32_t base = 0u;;) {
        const unsigned long long wm = __ballot(want);
        if (wm == 0ull) break;
        const uint32_t nw = (uint32_t)__popcll(wm);
        const uint32_t kl = whole ? rt_wave_rounds_log2(64u, nw, RT_WAVE_ROUNDS_CAP) : 0u;
        const uint32_t wr = __builtin_amdgcn_mbcnt_hi((uint32_t)(wm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wm, 0u));
        /* K = 1: every lane that wants takes its own loop's round `base` */
        uint32_t k0 = rng.k0, k1 = rng.k1, c1 = rng.c1, c2 = rng.c2, c3 = rng.c3, round = base;
        RtRngPos from = start;
        bool valid = want;
        if (kl != 0u) {
            /* lane q of `tab`: the q-th lane that wants a sample (behind those, the others: every lane is written once) */
            const uint32_t nr = __builtin_amdgcn_mbcnt_hi((uint32_t)(~wm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)~wm, 0u));
            const uint32_t tab = (uint32_t)__builtin_amdgcn_ds_permute((int)((want ? wr : nw + nr) << 2), (int)lane);
            const RtWaveSlot s = rt_wave_slot(lane, kl, nw, base);
            const int src = (int)(RT_FROM((int)(s.loop << 2), tab) << 2);
            k0 = RT_FROM(src, rng.k0); k1 = RT_FROM(src, rng.k1); c1 = RT_FROM(src, rng.c1); c2 = RT_FROM(src, rng.c2); c3 = RT_FROM(src, rng.c3);
            from.blk = RT_FROM(src, start.blk); from.off = RT_FROM(src, start.off);
            round = s.round; valid = s.valid;
        }
        RtRound o;
        if (SPHERE) o = rt_sphere_round(k0, k1, c1, c2, c3, from, round);
        else o = rt_disk_round(k0, k1, c1, c2, c3, from, round);
        bool got = want && o.accept;
        if (kl != 0u) { /* every loop stops at the first of its K rounds that accepted, and fetches it */
            const unsigned long long accepted = __ballot(valid && o.accept);
            const uint32_t first = rt_wave_first(accepted, want ? wr : 0u, kl);
            got = want && first < 64u;
            const int win = (int)((got ? first : lane) << 2);
            const uint64_t ux = rt_d2u(o.v.x), uy = rt_d2u(o.v.y), uz = rt_d2u(o.v.z);
            o.v.x = rt_u2d(((uint64_t)RT_FROM(win, (uint32_t)(ux >> 32)) << 32) | RT_FROM(win, (uint32_t)ux));
            o.v.y = rt_u2d(((uint64_t)RT_FROM(win, (uint32_t)(uy >> 32)) << 32) | RT_FROM(win, (uint32_t)uy));
            if (SPHERE) o.v.z = rt_u2d(((uint64_t)RT_FROM(win, (uint32_t)(uz >> 32)) << 32) | RT_FROM(win, (uint32_t)uz));
            o.blk = RT_FROM(win, o.blk); o.left = RT_FROM(win, o.left); o.a0 = RT_FROM(win, o.a0); o.a1 = RT_FROM(win, o.a1);
        }
        if (got) { out = o.v; rt_rng_after_round(rng, o); want = false; }
        base += 1u << kl;
    }
#undef RT_FROM
    return out;
}
#else
#define RT_WAVE_ROUNDS_ON 0
#endif

/* math.rs:39-49 (caller has reserved two 64-bit draws) */
RT_HD RtV3 rt_random_cosine_direction(RtRng& rng) {
    double r1 = rt_take_f64(rng);
    double r2 = rt_take_f64(rng);
    double z = rt_sqrt(RT_R(1.0) - r2);
    double phi = RT_R(2.0) * RT_R(RT_PI) * r1;
    double s, c;
    rt_sincos(phi, s, c);
    double sr2 = rt_sqrt(r2);
    return rt_v3(c * sr2, s * sr2, z);
}
/* math.rs:51-65 (caller has reserved two 64-bit draws) */
RT_HD RtV3 rt_random_to_sphere(double radius, double distance_squared, RtRng& rng) {
    double r1 = rt_take_f64(rng);
    double r2 = rt_take_f64(rng);
    double z = RT_R(1.0) + r2 * (rt_sqrt(RT_R(1.0) - radius * radius / distance_squared) - RT_R(1.0));
    double phi = RT_R(2.0) * RT_R(RT_PI) * r1;
    double s, c;
    rt_sincos(phi, s, c);
    double q = rt_sqrt(RT_R(1.0) - z * z);
    return rt_v3(c * q, s * q, z);
}

/* Onb onb.rs:13-28 */
struct RtOnb { RtV3 u, v, w; };
RT_HD RtOnb rt_onb_from_w(RtV3 n) {
    RtOnb o;
    o.w = rt_normalize(n);
    RtV3 a = (rt_abs(o.w.x) > RT_R(0.9)) ? rt_v3(RT_R(0.0), RT_R(1.0), RT_R(0.0)) : rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0));
    o.v = rt_normalize(rt_cross(o.w, a));
    o.u = rt_cross(o.w, o.v);
    return o;
}
RT_HD RtV3 rt_onb_local(const RtOnb& o, RtV3 a) { return o.u * a.x + o.v * a.y + o.w * a.z; }

/* ---------------------------------------------------------------- lights -- */

/* Hittable::pdf_value of one light: XZRect aarect.rs:119-138, Sphere sphere.rs:72-90,
 * anything else the trait default 0.0 (hittable.rs:66-68) */
RT_HD double rt_xz_light_pdf_value(const RtNode& l, RtV3 o, RtV3 v) {
    double t;
    if (!rt_rect_t(l, o.y, v.y, o.x, v.x, o.z, v.z, RT_R(0.001), RT_INF, t)) return RT_R(0.0);
    RtV3 on = rt_v3(RT_R(0.0), RT_R(1.0), RT_R(0.0));
    RtV3 normal = (rt_dot(v, on) < RT_R(0.0)) ? on : -on;
    double area = (l.d[1] - l.d[0]) * (l.d[3] - l.d[2]);
    double distance_squared = t * t * rt_mag2(v);
    double cosine = rt_abs(rt_dot(v, normal) / rt_mag(v));
    return distance_squared / (cosine * area);
}
RT_HD double rt_sphere_light_pdf_value(const RtNode& l, RtV3 o, RtV3 v) {
    double t;
    RtV3 center = rt_v3(l.d[0], l.d[1], l.d[2]);
    if (!rt_sphere_root(center, l.d[3], o, v, RT_R(0.001), RT_INF, t)) return RT_R(0.0);
    double cos_theta_max = rt_sqrt(RT_R(1.0) - l.d[3] * l.d[3] / rt_mag2(center - o));
    double solid_angle = RT_R(2.0) * RT_R(RT_PI) * (RT_R(1.0) - cos_theta_max);
    return RT_R(1.0) / solid_angle;
}
/* What the sphere light's sampling lobe (rt_random_to_sphere's caller, sphere.rs:92-99) and its pdf (above, sphere.rs:72-90) both compute
 * from the light and the shaded point o alone: the direction to the centre, its squared length, and the cosine of the cone the sphere
 * fills -- the statements of the two, in their order.  A Lambertian bounce under a light list with one sphere in it (RtLightShape:
 * `cone`) evaluates this once for both; in the kernel the two copies sat in different divergent regions and both ran for nearly every wave.
 * RT_LIGHT_CONE 0 (RT1W_JIT_EXTRA_OPTS=-DRT_LIGHT_CONE=0) is the text without it.  f64 builds with the library's own stream only. */
#ifndef RT_LIGHT_CONE
#define RT_LIGHT_CONE 1
#endif
#undef RT_LIGHT_CONE_ON
#if defined(RT_F32) || defined(RT_RNG_REFSTREAM)
#define RT_LIGHT_CONE_ON 0
#else
#define RT_LIGHT_CONE_ON ((RT_LIGHT_CONE) != 0)
#endif
/* Where the cone is (`cone`), the cosine lobe and the sphere lobe build their direction alike: a square root, and a frame applied to
 * (cos * q, sin * q, z).  A wave that holds lanes of both -- nearly every Lambertian one -- ran the two copies one after the other;
 * with RT_LOBE_SHARED each lobe leaves its frame, its z and its radicand (r2, or 1 - z * z), and one sqrt and one rt_onb_local serve
 * both: per lane the operations and operands of before.  RT1W_JIT_EXTRA_OPTS=-DRT_LOBE_SHARED=0 is the text with the two copies. */
#ifndef RT_LOBE_SHARED
#define RT_LOBE_SHARED 1
#endif
struct RtSphereCone { RtV3 direction; double distance_squared, cos_theta_max; };
struct RtNoCone {};
RT_HD RtSphereCone rt_sphere_cone(const RtNode& l, RtV3 o) {
    RtSphereCone k;
    k.direction = rt_v3(l.d[0], l.d[1], l.d[2]) - o;
    k.distance_squared = rt_mag2(k.direction);
    k.cos_theta_max = rt_sqrt(RT_R(1.0) - l.d[3] * l.d[3] / k.distance_squared);
    return k;
}
/* RT_LOBE_SHARED: the scattered direction of a lane that drew the one sphere light's lobe (`sphere`) or the cosine lobe about `uvw`,
 * from r2 and the sine and cosine of 2 pi r1.  Each lobe hands over its frame, its z and its radicand; the square root and the
 * frame's product stand once.  The sphere lobe: sphere.rs:92-99 -> math.rs:51-65; the cosine lobe: math.rs:39-49. */
RT_HD RtV3 rt_lobe_dir_shared(bool sphere, const RtOnb& uvw, const RtSphereCone& cone, double r2, double sn, double cs) {
    RtOnb fr = uvw;
    double z, rad = r2;
    if (sphere) {
        fr = rt_onb_from_w(cone.direction);
        z = RT_R(1.0) + r2 * (cone.cos_theta_max - RT_R(1.0));
        rad = RT_R(1.0) - z * z;
    } else {
        z = rt_sqrt(RT_R(1.0) - r2);
    }
    const double q = rt_sqrt(rad);
    return rt_onb_local(fr, rt_v3(cs * q, sn * q, z));
}
/* rt_sphere_light_pdf_value with the cone of (l, o) at hand */
RT_HD double rt_sphere_light_pdf_value(const RtNode& l, const RtSphereCone& k, RtV3 o, RtV3 v) {
    double t;
    RtV3 center = rt_v3(l.d[0], l.d[1], l.d[2]);
    if (!rt_sphere_root_oc2(center, l.d[3], k.distance_squared, o, v, RT_R(0.001), RT_INF, t)) return RT_R(0.0);
    double solid_angle = RT_R(2.0) * RT_R(RT_PI) * (RT_R(1.0) - k.cos_theta_max);
    return RT_R(1.0) / solid_angle;
}
RT_HD double rt_light_pdf_value(const RtNode& l, RtV3 o, RtV3 v) {
    if (l.kind == RT_XZ) return rt_xz_light_pdf_value(l, o, v);
    if (l.kind == RT_SPHERE) return rt_sphere_light_pdf_value(l, o, v);
    return RT_R(0.0);
}
/* Hittable::random of one light: aarect.rs:140-147, sphere.rs:92-99, default (1,0,0)
 * (caller has reserved two 64-bit draws) */
RT_HD RtV3 rt_light_random(const RtNode& l, RtV3 o, RtRng& rng) {
    if (l.kind == RT_XZ) {
        double x = rt_take_range(rng, l.d[0], l.d[1]);
        double z = rt_take_range(rng, l.d[2], l.d[3]);
        return rt_v3(x, l.d[4], z) - o;
    }
    if (l.kind == RT_SPHERE) {
        RtV3 direction = rt_v3(l.d[0], l.d[1], l.d[2]) - o;
        double distance_squared = rt_mag2(direction);
        RtOnb uvw = rt_onb_from_w(direction);
        return rt_onb_local(uvw, rt_random_to_sphere(l.d[3], distance_squared, rng));
    }
    return rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0));
}
/* impl Hittable for [T]: pdf_value hittable.rs:144-150 */
RT_HD double rt_lights_pdf_value(const RtSceneView& sc, RtV3 o, RtV3 v) {
    double weight = RT_R(1.0) / (double)sc.n_lights;
    double sum = RT_R(0.0);
    for (uint32_t i = 0; i < sc.n_lights; ++i) sum = sum + weight * rt_light_pdf_value(sc.lights[i], o, v);
    return sum;
}

/* The light list's shape as the scene-specialised kernel knows it (jit.cpp: Topo::n_lights, Topo::light_kind -- the kind word of
 * every sc.lights[i], in order; the records' values still come from sc.lights).  The walk over the list, the choice of a lobe and
 * the tests for an empty list are then unrolled at compile time: every lane performs the operations of the loops above in their
 * order, the compiler leaves out the kinds the list does not hold.  A Topo without the members (and void) leaves all of it to
 * run time. */
template <class Topo, class = void>
struct RtLightShape {
    static constexpr bool fixed = false, may_xz = true, may_sphere = true, may_default = true, cone = false;
    RT_HD static bool any(const RtSceneView& sc) { return sc.n_lights > 0u; }
    RT_HD static uint32_t choose(const RtSceneView& sc, RtRng& rng) { return rt_gen_below(rng, sc.n_lights); }
    RT_HD static uint32_t kind(const RtSceneView& sc, uint32_t li) { return sc.lights[li].kind; }
    RT_HD static uint32_t index(uint32_t, uint32_t li) { return li; }
    RT_HD static double pdf_value(const RtSceneView& sc, RtV3 o, RtV3 v) { return rt_lights_pdf_value(sc, o, v); }
};
/* lights of `kind` in Topo's list from entry i on, and the index of the first of them (n_lights if there is none) */
template <class Topo>
constexpr uint32_t rt_light_count(uint32_t kind, uint32_t i = 0u) { return i < Topo::n_lights ? (Topo::light_kind[i] == kind ? 1u : 0u) + rt_light_count<Topo>(kind, i + 1u) : 0u; }
template <class Topo>
constexpr uint32_t rt_light_first(uint32_t kind, uint32_t i = 0u) { return i < Topo::n_lights && Topo::light_kind[i] != kind ? rt_light_first<Topo>(kind, i + 1u) : i; }
template <class Topo>
struct RtLightShape<Topo, typename RtVoid<decltype(Topo::light_kind)>::type> {
    static constexpr uint32_t n = Topo::n_lights;
    static constexpr bool fixed = true, may_xz = rt_light_count<Topo>(RT_XZ) > 0u, may_sphere = rt_light_count<Topo>(RT_SPHERE) > 0u,
                          may_default = rt_light_count<Topo>(RT_XZ) + rt_light_count<Topo>(RT_SPHERE) < n,
                          cone = RT_LIGHT_CONE_ON && rt_light_count<Topo>(RT_SPHERE) == 1u; /* exactly one sphere light: one cone per shaded point (rt_sphere_cone) */
    RT_HD static bool any(const RtSceneView&) { return n > 0u; }
    RT_HD static uint32_t choose(const RtSceneView&, RtRng& rng) { return rt_gen_below(rng, n); }
    template <uint32_t I = 0u>
    RT_HD static uint32_t kind(const RtSceneView& sc, uint32_t li) {
        if constexpr (I + 1u < n) return li == I ? Topo::light_kind[I] : kind<I + 1u>(sc, li);
        else return Topo::light_kind[I];
    }
    /* the record of the chosen light of `kind`: where the list holds one light of that kind its index is a constant and the
     * record is read once for the wave */
    RT_HD static uint32_t index(uint32_t kind, uint32_t li) { return rt_light_count<Topo>(kind) == 1u ? rt_light_first<Topo>(kind) : li; }
    template <uint32_t I>
    RT_HD static double pdf_sum(const RtSceneView& sc, RtV3 o, RtV3 v, double sum) {
        if constexpr (I < n) {
            constexpr double weight = RT_R(1.0) / (double)n; /* the same correctly rounded quotient as at run time */
            double value = RT_R(0.0);
            if constexpr (Topo::light_kind[I] == RT_XZ) value = rt_xz_light_pdf_value(sc.lights[I], o, v);
            else if constexpr (Topo::light_kind[I] == RT_SPHERE) value = rt_sphere_light_pdf_value(sc.lights[I], o, v);
            return pdf_sum<I + 1u>(sc, o, v, sum + weight * value);
        } else return sum;
    }
    RT_HD static double pdf_value(const RtSceneView& sc, RtV3 o, RtV3 v) { return pdf_sum<0u>(sc, o, v, RT_R(0.0)); }
    /* the same sum where the one sphere light's cone at o is at hand (`cone`) */
    template <uint32_t I>
    RT_HD static double pdf_sum(const RtSceneView& sc, const RtSphereCone& k, RtV3 o, RtV3 v, double sum) {
        if constexpr (I < n) {
            constexpr double weight = RT_R(1.0) / (double)n;
            double value = RT_R(0.0);
            if constexpr (Topo::light_kind[I] == RT_XZ) value = rt_xz_light_pdf_value(sc.lights[I], o, v);
            else if constexpr (Topo::light_kind[I] == RT_SPHERE) value = rt_sphere_light_pdf_value(sc.lights[I], k, o, v);
            return pdf_sum<I + 1u>(sc, k, o, v, sum + weight * value);
        } else return sum;
    }
    RT_HD static double pdf_value(const RtSceneView& sc, const RtSphereCone& k, RtV3 o, RtV3 v) { return pdf_sum<0u>(sc, k, o, v, RT_R(0.0)); }
};

/* Where Lambertian materials sit, as the scene-specialised kernel knows it (jit.cpp: Topo::lambert_xy / _xz / _yz: some XY / XZ /
 * YZ rect outside every wrapper carries one; Topo::lambert_general: something else does).  The normal of such a rect is +-(0,0,1),
 * +-(0,1,0) or +-(1,0,0) -- HitRecord::new's `-on`, so with the zeros' signs -- and its shading frame is rt_onb_from_w of that
 * literal, which the compiler evaluates: six constant frames, selected by the rect's kind and the sign of the normal's own
 * component.  The frames are not written out by hand: the signs of their zeros reach the scattered direction, 1 / d of the next
 * segment and the slab swap. */
template <class Topo, class = void>
struct RtLambertWalls { static constexpr bool walls = false, general = true, xy = false, xz = false, yz = false; };
template <class Topo>
struct RtLambertWalls<Topo, typename RtVoid<decltype(Topo::lambert_general)>::type> {
    static constexpr bool general = Topo::lambert_general, xy = Topo::lambert_xy, xz = Topo::lambert_xz, yz = Topo::lambert_yz, walls = xy || xz || yz;
};
RT_HD RtOnb rt_onb_select(bool c, const RtOnb& a, const RtOnb& b) {
    RtOnb o;
    o.u = rt_v3(c ? a.u.x : b.u.x, c ? a.u.y : b.u.y, c ? a.u.z : b.u.z);
    o.v = rt_v3(c ? a.v.x : b.v.x, c ? a.v.y : b.v.y, c ? a.v.z : b.v.z);
    o.w = rt_v3(c ? a.w.x : b.w.x, c ? a.w.y : b.w.y, c ? a.w.z : b.w.z);
    return o;
}
/* the frame of an unwrapped axis rect (an XZ one, an XY one, else a YZ one) whose normal is n; for any other lane one of the frames, which
 * nobody uses */
template <class LW>
RT_HD RtOnb rt_wall_frame(bool is_xz, bool is_xy, RtV3 n) {
    const RtV3 ex = rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0)), ey = rt_v3(RT_R(0.0), RT_R(1.0), RT_R(0.0)), ez = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(1.0));
    RtOnb o = rt_onb_from_w(ex);
    if (LW::yz) o = rt_onb_select(n.x < RT_R(0.0), rt_onb_from_w(-ex), rt_onb_from_w(ex));
    if (LW::xz) { RtOnb f = rt_onb_select(n.y < RT_R(0.0), rt_onb_from_w(-ey), rt_onb_from_w(ey)); o = LW::yz ? rt_onb_select(is_xz, f, o) : f; }
    if (LW::xy) { RtOnb f = rt_onb_select(n.z < RT_R(0.0), rt_onb_from_w(-ez), rt_onb_from_w(ez)); o = (LW::yz || LW::xz) ? rt_onb_select(is_xy, f, o) : f; }
    return o;
}

/* ------------------------------------------------------------ materials -- */

RT_HD RtV3 rt_reflect(RtV3 v, RtV3 n) { return v - RT_R(2.0) * rt_dot(v, n) * n; } /* material.rs:94-96 */
RT_HD RtV3 rt_refract(RtV3 uv, RtV3 n, double etai_over_etat) {               /* material.rs:114-119 */
    double cos_theta = rt_min(rt_dot(-uv, n), RT_R(1.0));
    RtV3 r_out_perp = etai_over_etat * (uv + cos_theta * n);
    RtV3 r_out_parallel = -rt_sqrt(rt_abs(RT_R(1.0) - rt_mag2(r_out_perp))) * n;
    return r_out_perp + r_out_parallel;
}
RT_HD double rt_reflectance_r0(double cosine, double r0) {                    /* material.rs:124: the statement behind r0 */
    return r0 + (RT_R(1.0) - r0) * rt_pow5(RT_R(1.0) - cosine);
}
RT_HD double rt_reflectance(double cosine, double ref_idx) {                  /* material.rs:121-125 */
    return rt_reflectance_r0(cosine, rt_schlick_r0(ref_idx));
}
/* A Dielectric's refraction ratios and their r0 are the material's alone: the record carries them (rt_flat.h: rt_material_derive) and a
 * bounce selects by the face instead of dividing twice per lane.  RT1W_JIT_EXTRA_OPTS=-DRT_MAT_DERIVED=0: the text that computes them.
 * f64 records only (the f32 build's records are conversions, and the conversion of a quotient is not the quotient of conversions). */
#ifndef RT_MAT_DERIVED
#define RT_MAT_DERIVED 1
#endif
#undef RT_MAT_DERIVED_ON /* (a unit may take this header twice: f64 records, then the f32 build) */
#if defined(RT_F32)
#define RT_MAT_DERIVED_ON false
#else
#define RT_MAT_DERIVED_ON ((RT_MAT_DERIVED) != 0)
#endif

/* --------------------------------------------------------------- camera -- */

/* main.rs:964-971 + Camera::get_ray camera.rs:61-73 */
RT_HD void rt_path_begin_cam(const RtCamera& c, const RtFrame& f, uint32_t i, uint32_t j,
                         uint32_t sample, RtPath& p);
RT_HD void rt_path_begin(const RtSceneView& sc, const RtFrame& f, uint32_t i, uint32_t j,
                         uint32_t sample, RtPath& p) { rt_path_begin_cam(sc.camera, f, i, j, sample, p); }
RT_HD void rt_path_begin_cam(const RtCamera& c, const RtFrame& f, uint32_t i, uint32_t j,
                         uint32_t sample, RtPath& p) {
#if defined(RT_RNG_REFSTREAM)
    /* main.rs:964-967: the pixel's stream is seeded once, before its sample loop, and every sample draws on from where
     * the previous one stopped (a lane runs all samples of its pixel in order: chunk = spp, sample_offset = 0) */
    if (sample == 0u) p.rng = rt_rng_make((uint32_t)((uint64_t)j * f.width + i), (uint32_t)(((uint64_t)j * f.width + i) >> 32), 0u, 0u, 0u);
#else
    p.rng = rt_rng_pixel_sample((uint64_t)j * f.width + i, sample, f.global_seed);
#endif
    rt_rng_reserve(p.rng, 4u);
    double u = ((double)i + rt_take_f64(p.rng)) / (double)(f.width - 1u);
    double v = ((double)j + rt_take_f64(p.rng)) / (double)(f.height - 1u);
    RtV3 rd = c.lens_radius * rt_random_in_unit_disk(p.rng);
    RtV3 offset = c.u * rd.x + c.v * rd.y;
    p.ray.o = c.origin + offset;
    p.ray.d = c.lower_left_corner + u * c.horizontal + v * c.vertical - c.origin - offset;
    rt_rng_reserve(p.rng, rt_rng_need_u64(p.rng));
    p.ray.time = rt_take_range(p.rng, c.time0, c.time1);
    p.beta = rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0));
    p.radiance = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
    p.depth_left = f.max_depth;
    p.alive = true;
}
#if RT_WAVE_ROUNDS_ON
/* rt_path_begin_cam for the lanes of a wave that `begin` a path, called by every lane of the wave: its statements, with the unit
 * disk's rounds spread over the lanes that begin nothing (rt_wave_rounds) */
__device__ __forceinline__ void rt_path_begin_wave(const RtCamera& c, const RtFrame& f, uint32_t i, uint32_t j, uint32_t sample, RtPath& p, bool begin) {
    double u = RT_R(0.0), v = RT_R(0.0);
    if (begin) {
        p.rng = rt_rng_pixel_sample((uint64_t)j * f.width + i, sample, f.global_seed);
        rt_rng_reserve(p.rng, 4u);
        u = ((double)i + rt_take_f64(p.rng)) / (double)(f.width - 1u);
        v = ((double)j + rt_take_f64(p.rng)) / (double)(f.height - 1u);
    }
    const RtV3 disk = rt_wave_rounds<false>(p.rng, begin);
    if (begin) {
        RtV3 rd = c.lens_radius * disk;
        RtV3 offset = c.u * rd.x + c.v * rd.y;
        p.ray.o = c.origin + offset;
        p.ray.d = c.lower_left_corner + u * c.horizontal + v * c.vertical - c.origin - offset;
        rt_rng_reserve(p.rng, rt_rng_need_u64(p.rng));
        p.ray.time = rt_take_range(p.rng, c.time0, c.time1);
        p.beta = rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0));
        p.radiance = rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
        p.depth_left = f.max_depth;
        p.alive = true;
    }
}
#endif

/* ------------------------------------------------------------ integrator -- */

/* One level of ray_color (main.rs:51-116; with no lights :118-190).  The
 * recursion  L = emitted + W (.) L'/pdf  is carried as  radiance += beta (.) emitted,
 * beta = beta (.) W / pdf.  Every terminal adds beta (.) value -- including the zero
 * of depth exhaustion (main.rs:59-61) -- so a non-finite beta poisons the sample
 * exactly as it does through the reference's multiplications. */
/* The closest hit found by the first half of a step, and what the second half will do with
 * it: the class is the sort key of the workgroup-level reordering (context.hip). */
struct RtTrace {
    double t;
    uint32_t prim, scope;
    uint32_t cls; /* RT_CLS_* */
};
/* order = position in the sorted workgroup: Lambertian paths fill the first waves, the paths that end
 * (and will regenerate) the last one; other orders were measured 0.5-4 % slower */
enum { RT_CLS_LAMBERT = 0, RT_CLS_DIELECTRIC = 1, RT_CLS_METAL = 2, RT_CLS_OTHER = 3, RT_CLS_TERMINAL = 4, RT_CLS_IDLE = 5, RT_N_CLS = 6 };

/* the class of a hit on a material of kind mk */
RT_HD constexpr uint32_t rt_class_of(uint32_t mk) {
    return mk == RT_MAT_LAMBERTIAN ? RT_CLS_LAMBERT
         : mk == RT_MAT_DIELECTRIC ? RT_CLS_DIELECTRIC
         : mk == RT_MAT_METAL ? RT_CLS_METAL
         : mk == RT_MAT_ISOTROPIC ? RT_CLS_OTHER : RT_CLS_TERMINAL;
}

/* ------------------------------------------------------ static hit record -- */

/* What the scene-specialised kernel knows about the node a path hit (jit.cpp: Topo::wrap -- the wrapper above every leaf, wrapper and
 * medium -- and Topo::mat_kind -- the kind word of a leaf's material).  In the unrolled sweep the closest leaf is one of a set the
 * compiler knows, so its kind, its RT_LEAF_FLIPPED flag, its wrapper chain, whether its material reads (u, v) and the class its path
 * sorts under are compile-time functions of `prim`: "is the lane's leaf one of these" replaces the node record, the walk up the chain
 * and every dispatch on a loaded kind.  Values -- a wrapper's offset and angle, a sphere's centre -- still come from the records, read
 * at constant indices (scalar loads).  A Topo without the members (and void) keeps rt_finish_hit.
 * The leaves a path can hit are the leaves and media of the world outside every medium's boundary (a boundary is swept for its two
 * roots only). */
template <uint32_t N>
struct RtHitTab {
    bool leaf[N];       /* a path's closest hit can be this node */
    uint32_t chain[N];  /* which of the distinct wrapper chains stands above it; RT_NONE outside every wrapper */
    uint32_t s[N][3];   /* the distinct chains, outermost wrapper first (rt_chain), in the order of their first leaf */
    uint32_t n_chains;
};
template <class Topo>
constexpr RtHitTab<Topo::n> rt_hit_tab() {
    RtHitTab<Topo::n> T{};
    uint32_t medium_end = 0u;
    for (uint32_t i = 0u; i < Topo::n; ++i) {
        const uint32_t k = Topo::kind[i] & RT_KIND_MASK;
        T.chain[i] = RT_NONE;
        const bool hittable = i >= Topo::root && i < Topo::skip[Topo::root] && i >= medium_end && ((k >= RT_SPHERE && k <= RT_YZ) || k == RT_MEDIUM);
        if (hittable) {
            T.leaf[i] = true;
            uint32_t c[3] = {RT_NONE, RT_NONE, RT_NONE};
            for (uint32_t w = Topo::wrap[i]; w != RT_NONE; w = Topo::wrap[w]) { c[2] = c[1]; c[1] = c[0]; c[0] = w; }
            if (c[0] != RT_NONE) {
                uint32_t j = 0u;
                while (j < T.n_chains && !(T.s[j][0] == c[0] && T.s[j][1] == c[1] && T.s[j][2] == c[2])) ++j;
                if (j == T.n_chains) { T.s[j][0] = c[0]; T.s[j][1] = c[1]; T.s[j][2] = c[2]; ++T.n_chains; }
                T.chain[i] = j;
            }
        }
        if (hittable && k == RT_MEDIUM) medium_end = Topo::skip[i];
    }
    return T;
}
#ifndef RT_HIT_STATIC
/* which parts are on (RT1W_JIT_EXTRA_OPTS=-DRT_HIT_STATIC=k builds any other mix; every mix gives the same bits).  Measured on the Cornell
 * kernel, ms per launch at 600x600x1000 (profiles/hit_static_bench.json): none 115.6; the shipped 1 + 4: 111.6.  The class from the leaf
 * (2) and the material word in the exchange (8) execute fewer instructions still and run slower: 1 + 2 + 4 + 8: 118.2, 1 + 4 + 8: 119.0,
 * 1 + 2 + 8: 114.8, 2 alone 114.7 -- they stay behind the switch.
 *   1  the static hit record (rt_finish_hit_static)
 *   2  class and wrapper of a hit from its leaf: rt_path_trace reads no record in front of the sort
 *   4  the Lambertian branch asks the leaf sets for "an unwrapped axis rect, and of which kind"
 *   8  (with 1) the node's material word travels in the exchange where the wrapper did: no node record is read after it for a rect */
#define RT_HIT_STATIC 5
#endif
#ifndef RT_HIT_MAX_CHAINS
#define RT_HIT_MAX_CHAINS 8u /* distinct chains that get a block of their own; the leaves of the others walk their chain at run time */
#endif
/* groups of leaves: a chain's index, or */
#define RT_HG_ANY 0xFFFFFFFEu       /* every leaf a path can hit */
#define RT_HG_UNWRAPPED RT_NONE     /* the leaves outside every wrapper */
#define RT_HG_WALKED 0xFFFFFFFDu    /* the leaves of the chains beyond RT_HIT_MAX_CHAINS */
/* flags a set can ask for */
enum { RT_HF_NONE = 0, RT_HF_FLIPPED = 1, RT_HF_UV = 2, RT_HF_CLASS = 3 /* arg: RT_CLS_* */ };
#define RT_HK_ALL 0xFFFFFFFFu /* kinds as a mask of 1 << RT_SPHERE ... 1 << RT_MEDIUM */
template <uint32_t I, uint32_t END, class F>
RT_HD void rt_static_for(F&& f) {
    if constexpr (I < END) { f(std::integral_constant<uint32_t, I>()); rt_static_for<I + 1u, END>(f); }
}
template <class Topo, class>
struct RtHitShape { static constexpr bool fixed = false, record = false, trace = false, walls = false, carry = false; };
template <class Topo>
struct RtHitShape<Topo, typename RtVoid<decltype(Topo::wrap)>::type> {
    static constexpr bool fixed = RT_HIT_STATIC != 0, record = (RT_HIT_STATIC & 1) != 0, trace = (RT_HIT_STATIC & 2) != 0, walls = (RT_HIT_STATIC & 4) != 0,
                          carry = record && (RT_HIT_STATIC & 8) != 0;
    static constexpr uint32_t n = Topo::n;
    static constexpr RtHitTab<Topo::n> tab = rt_hit_tab<Topo>();
    static constexpr uint32_t n_chains = tab.n_chains, n_blocks = n_chains < RT_HIT_MAX_CHAINS ? n_chains : RT_HIT_MAX_CHAINS;
    static constexpr bool in_group(uint32_t g, uint32_t i) {
        return tab.leaf[i] && (g == RT_HG_ANY || (g == RT_HG_WALKED ? (tab.chain[i] != RT_NONE && tab.chain[i] >= n_blocks) : tab.chain[i] == g));
    }
    /* the set (KINDS, FLAG, ARG, GROUP): leaves of GROUP whose kind is in KINDS and that have the flag */
    static constexpr bool has(uint32_t kinds, uint32_t flag, uint32_t arg, uint32_t group, uint32_t i) {
        return in_group(group, i) && ((kinds >> (Topo::kind[i] & RT_KIND_MASK)) & 1u) != 0u &&
               (flag == RT_HF_NONE || (flag == RT_HF_FLIPPED ? (Topo::kind[i] & RT_LEAF_FLIPPED) != 0u
                                       : flag == RT_HF_UV ? (Topo::mat_kind[i] & RT_MAT_NEEDS_UV) != 0u
                                                          : rt_class_of(Topo::mat_kind[i] & 0xFFu) == arg));
    }
    static constexpr uint32_t count(uint32_t kinds, uint32_t flag, uint32_t arg, uint32_t group) {
        uint32_t c = 0u;
        for (uint32_t i = 0u; i < n; ++i) c += has(kinds, flag, arg, group, i) ? 1u : 0u;
        return c;
    }
    /* the k-th member of the set, or of the rest of KNOWN (`other`) */
    static constexpr uint32_t nth(uint32_t kinds, uint32_t flag, uint32_t arg, uint32_t group, uint32_t known, bool other, uint32_t k) {
        for (uint32_t i = 0u; i < n; ++i)
            if (in_group(known, i) && has(kinds, flag, arg, group, i) != other && k-- == 0u) return i;
        return RT_NONE;
    }
    static constexpr uint64_t mask(uint32_t kinds, uint32_t flag, uint32_t arg, uint32_t group, uint32_t first, uint32_t bits) {
        uint64_t m = 0u;
        for (uint32_t i = 0u; i < bits && first + i < n; ++i) m |= has(kinds, flag, arg, group, first + i) ? (uint64_t)1u << i : (uint64_t)0u;
        return m;
    }
    /* "is the lane's leaf in the set?", for a lane whose leaf is known to be in the group KNOWN.  A set that is empty or all of KNOWN
     * is answered by the compiler; one or two leaves (or all but one or two) by comparing; anything else by a bit of a constant mask:
     * one 32-bit word up to 32 nodes, one 64-bit word up to 64, and above that the non-zero 32-bit words, each behind the test for
     * its word */
    template <uint32_t KINDS, uint32_t FLAG, uint32_t ARG, uint32_t GROUP, uint32_t KNOWN = RT_HG_ANY>
    RT_HD static bool in(uint32_t prim) {
        static_assert(GROUP == KNOWN || KNOWN == RT_HG_ANY, "the set lies in the group the lane is known to be in");
        constexpr uint32_t G = GROUP, cnt = count(KINDS, FLAG, ARG, G), tot = count(RT_HK_ALL, RT_HF_NONE, 0u, KNOWN);
        if constexpr (cnt == 0u) return false;
        else if constexpr (cnt == tot) return true;
        else if constexpr (cnt <= 2u) {
            constexpr uint32_t a = nth(KINDS, FLAG, ARG, G, KNOWN, false, 0u), b = nth(KINDS, FLAG, ARG, G, KNOWN, false, cnt - 1u);
            return (prim == a) | (prim == b);
        } else if constexpr (tot - cnt <= 2u) {
            constexpr uint32_t a = nth(KINDS, FLAG, ARG, G, KNOWN, true, 0u), b = nth(KINDS, FLAG, ARG, G, KNOWN, true, tot - cnt - 1u);
            return !((prim == a) | (prim == b));
        } else if constexpr (n <= 32u) {
            constexpr uint32_t m = (uint32_t)mask(KINDS, FLAG, ARG, G, 0u, 32u);
            return ((m >> (prim & 31u)) & 1u) != 0u;
        } else if constexpr (n <= 64u) {
            constexpr uint64_t m = mask(KINDS, FLAG, ARG, G, 0u, 64u);
            return ((m >> (prim & 63u)) & 1u) != 0u;
        } else {
            bool r = false;
            rt_static_for<0u, (n + 31u) / 32u>([&](auto wi) {
                constexpr uint32_t W = decltype(wi)::value, m = (uint32_t)mask(KINDS, FLAG, ARG, G, W * 32u, 32u);
                if constexpr (m != 0u) r = r | (((prim >> 5) == W) & (((m >> (prim & 31u)) & 1u) != 0u));
            });
            return r;
        }
    }
    /* the sort class of a hit on `prim` */
    RT_HD static uint32_t cls(uint32_t prim) {
        uint32_t c = RT_CLS_TERMINAL;
        if (in<RT_HK_ALL, RT_HF_CLASS, RT_CLS_OTHER, RT_HG_ANY>(prim)) c = RT_CLS_OTHER;
        if (in<RT_HK_ALL, RT_HF_CLASS, RT_CLS_METAL, RT_HG_ANY>(prim)) c = RT_CLS_METAL;
        if (in<RT_HK_ALL, RT_HF_CLASS, RT_CLS_DIELECTRIC, RT_HG_ANY>(prim)) c = RT_CLS_DIELECTRIC;
        if (in<RT_HK_ALL, RT_HF_CLASS, RT_CLS_LAMBERT, RT_HG_ANY>(prim)) c = RT_CLS_LAMBERT;
        return c;
    }
    /* the innermost wrapper above `prim` (what the node keeps in `b`), for the callers of rt_closest_hit that want it */
    RT_HD static uint32_t scope_of(uint32_t prim) {
        uint32_t scope = RT_NONE;
        if (prim == RT_NONE) return scope;
        rt_static_for<0u, n_chains>([&](auto ci) {
            constexpr uint32_t C = decltype(ci)::value;
            constexpr uint32_t innermost = tab.s[C][2] != RT_NONE ? tab.s[C][2] : (tab.s[C][1] != RT_NONE ? tab.s[C][1] : tab.s[C][0]);
            if (in<RT_HK_ALL, RT_HF_NONE, 0u, C>(prim)) scope = innermost;
        });
        return scope;
    }
    /* record of wrapper J, its kind word from the topology: rt_scope_in / rt_scope_out need no dispatch */
    template <uint32_t J>
    RT_HD static RtNodeHot wrapper(const RtSceneView& sc) {
        constexpr uint32_t k = Topo::kind[J];
        RtNodeHot w = RtGlobalNodes{sc.nodes}.hot(J);
        w.kind = k;
        return w;
    }
};

/* A sphere's outward normal, (p - c) / r, is three divisions by one divisor: with the divisor prepared once (rt1w_num.h: rt_div_prep)
 * the three quotients are rt_div_q's, 5 + 9 instructions for 33.  The guards are the header's: the divisor's range, and every quotient's
 * as one that is used (a zero or tiny component would take div_fixup's sign and div_scale's scaling, which rt_div_q does not
 * reproduce).  rt_div_q3 is the three quotients and `bad`, whether a guard failed; a wave with a failing lane divides with `/`
 * (rt_sphere_normal; diagnostic builds charge that to bucket 15).  The static hit record's Sphere case, f64 device code only.
 * NOT SHIPPED: exact (tests/test_glass_terms.py, test_glass_terms_gpu.py), but on the Cornell kernel it gains 0.2-0.4 %, one parent
 * spread where the bar is four, alone and on top of the two other parts (docs/LAB_NOTES.md section 5; profiles/glass_terms_bench.json):
 * the guards cost eight compares of the nineteen instructions saved, and the fallback's text is 24 more static VALU.  The default is the
 * text with the three divisions; RT1W_JIT_EXTRA_OPTS=-DRT_NORMAL_SHARED=1 builds the part. */
#ifndef RT_NORMAL_SHARED
#define RT_NORMAL_SHARED 0
#endif
#undef RT_NORMAL_SHARED_ON /* (a unit may take this header twice: f64 records, then the f32 build) */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RT_F32)
#define RT_NORMAL_SHARED_ON ((RT_NORMAL_SHARED) != 0)
#else
#define RT_NORMAL_SHARED_ON 0
#endif
#if !defined(RT_F32)
RT_HD RtV3 rt_div_q3(RtV3 n, double d, double y, bool& bad) {
    const RtV3 q = rt_v3(rt_div_q(n.x, d, y), rt_div_q(n.y, d, y), rt_div_q(n.z, d, y));
    bad = !rt_div_d_ok(d) | rt_div_q_bad(q.x, true) | rt_div_q_bad(q.y, true) | rt_div_q_bad(q.z, true);
    return q;
}
#endif
RT_HD RtV3 rt_sphere_normal(RtV3 n, double r) {
#if RT_NORMAL_SHARED_ON
    bool bad;
    RtV3 on = rt_div_q3(n, r, rt_div_prep(r), bad);
    if (RT_WAVE_ANY(bad)) {
        on = n / r;
        RT_STAMP(15);
    }
    return on;
#else
    return n / r;
#endif
}

/* rt_leaf_record for a lane whose leaf is in GROUP: the same statements on the same operands; which of them a lane runs is decided by
 * set tests, and a record is read only where a value is needed -- a sphere's centre and radius (one scalar load where GROUP has one
 * sphere), a moving sphere's, a rect's bounds where its texture reads (u, v) */
template <class Cfg, uint32_t GROUP>
RT_HD void rt_leaf_record_static(const RtSceneView& sc, RtRayOD r, double time, uint32_t prim, uint32_t mat, double t, RtHit& h) {
    typedef RtHitShape<typename Cfg::Topo> HS;
    constexpr uint32_t SPH = 1u << RT_SPHERE, MSPH = 1u << RT_MSPHERE, MED = 1u << RT_MEDIUM;
    h.t = t; h.u = RT_R(0.0); h.v = RT_R(0.0); h.mat = mat;
    h.p = rt_at(r.o, r.d, t);
    const bool want_uv = Cfg::tex && HS::template in<RT_HK_ALL, RT_HF_UV, 0u, GROUP, GROUP>(prim);
    if (Cfg::media && HS::template in<MED, RT_HF_NONE, 0u, GROUP, GROUP>(prim)) {
        h.n = rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0));
        h.front = true;
        return;
    }
    RtV3 on;
    if (HS::template in<SPH | MSPH, RT_HF_NONE, 0u, GROUP, GROUP>(prim)) {
        if (Cfg::msphere && HS::template in<MSPH, RT_HF_NONE, 0u, GROUP, GROUP>(prim)) {
            const RtNode& nd = sc.nodes[prim];
            on = (h.p - rt_msphere_center(nd, time)) / nd.e[2];
        } else if constexpr (HS::count(Cfg::msphere ? SPH : SPH | MSPH, RT_HF_NONE, 0u, GROUP) == 1u) {
            constexpr uint32_t J = HS::nth(Cfg::msphere ? SPH : SPH | MSPH, RT_HF_NONE, 0u, GROUP, GROUP, false, 0u);
            const RtNodeHot nd = RtGlobalNodes{sc.nodes}.hot(J);
            on = rt_sphere_normal(h.p - rt_v3(nd.d[0], nd.d[1], nd.d[2]), nd.d[3]);
        } else {
            const RtNode& nd = sc.nodes[prim];
            on = rt_sphere_normal(h.p - rt_v3(nd.d[0], nd.d[1], nd.d[2]), nd.d[3]);
        }
        if (Cfg::tex && want_uv) rt_sphere_uv(on, h.u, h.v);
    } else {
        const bool is_xy = HS::template in<1u << RT_XY, RT_HF_NONE, 0u, GROUP, GROUP>(prim), is_xz = HS::template in<1u << RT_XZ, RT_HF_NONE, 0u, GROUP, GROUP>(prim);
        on = rt_v3((is_xy | is_xz) ? RT_R(0.0) : RT_R(1.0), is_xz ? RT_R(1.0) : RT_R(0.0), is_xy ? RT_R(1.0) : RT_R(0.0));
        if (Cfg::tex && want_uv) {
            const RtNode& nd = sc.nodes[prim];
            double b, c;
            if (is_xy) { b = r.o.x + t * r.d.x; c = r.o.y + t * r.d.y; }
            else if (is_xz) { b = r.o.x + t * r.d.x; c = r.o.z + t * r.d.z; }
            else { b = r.o.y + t * r.d.y; c = r.o.z + t * r.d.z; }
            h.u = (b - nd.d[0]) / (nd.d[1] - nd.d[0]);
            h.v = (c - nd.d[2]) / (nd.d[3] - nd.d[2]);
        }
    }
    /* HitRecord::new hittable.rs:30-35 */
    bool front = rt_dot(r.d, on) < RT_R(0.0);
    h.n = front ? on : -on;
    h.front = HS::template in<RT_HK_ALL, RT_HF_FLIPPED, 0u, GROUP, GROUP>(prim) ? !front : front; /* FlipFace::hit hittable.rs:288-291 flips the flag only */
}

/* rt_finish_hit with the leaf sets known: the leaves outside every wrapper take their record in the world's ray; every distinct chain
 * has one block, entered when a lane of the wave hit one of its leaves, with the wrappers' records at constant indices -- ray in,
 * leaf record in the innermost ray, fix-ups innermost to outermost, as rt_finish_hit orders them.  Every lane performs the operations
 * rt_finish_hit performs for it, on the same operands, in the same order.  `mat` is the node's material word.  Chains
 * beyond RT_HIT_MAX_CHAINS are walked by rt_finish_hit itself. */
template <class Cfg>
RT_HD void rt_finish_hit_static(const RtSceneView& sc, const RtRay& world, uint32_t prim, uint32_t mat, double t, RtHit& h) {
    typedef RtHitShape<typename Cfg::Topo> HS;
    RtRayOD r0; r0.o = world.o; r0.d = world.d;
    const bool plain = HS::template in<RT_HK_ALL, RT_HF_NONE, 0u, RT_HG_UNWRAPPED>(prim);
    if (RT_WAVE_ANY(plain)) {
        if (plain) rt_leaf_record_static<Cfg, RT_HG_UNWRAPPED>(sc, r0, world.time, prim, mat, t, h);
    }
    rt_static_for<0u, HS::n_blocks>([&](auto ci) {
        constexpr uint32_t C = decltype(ci)::value, s0 = HS::tab.s[C][0], s1 = HS::tab.s[C][1], s2 = HS::tab.s[C][2];
        const bool mine = HS::template in<RT_HK_ALL, RT_HF_NONE, 0u, C>(prim);
        if (RT_WAVE_ANY(mine)) {
            if (mine) {
                const RtRayOD r1 = rt_scope_in(HS::template wrapper<s0>(sc), r0);
                RtRayOD r2 = r1, r3 = r1;
                if constexpr (s1 != RT_NONE) { r2 = rt_scope_in(HS::template wrapper<s1>(sc), r1); r3 = r2; }
                if constexpr (s2 != RT_NONE) r3 = rt_scope_in(HS::template wrapper<s2>(sc), r2);
                rt_leaf_record_static<Cfg, C>(sc, r3, world.time, prim, mat, t, h);
                if constexpr (s2 != RT_NONE) rt_scope_out(HS::template wrapper<s2>(sc), r3, h);
                if constexpr (s1 != RT_NONE) rt_scope_out(HS::template wrapper<s1>(sc), r2, h);
                rt_scope_out(HS::template wrapper<s0>(sc), r1, h);
            }
        }
    });
    if constexpr (HS::n_chains > HS::n_blocks) {
        const bool walked = HS::template in<RT_HK_ALL, RT_HF_NONE, 0u, RT_HG_WALKED>(prim);
        if (RT_WAVE_ANY(walked)) {
            if (walked) rt_finish_hit<Cfg>(sc, world, prim, sc.nodes[prim].b, t, h);
        }
    }
}

/* first half of one level of ray_color: depth check (main.rs:59-61) and world.hit (main.rs:62) */
template <class Cfg, class Stack, class NS>
RT_HD RtTrace rt_path_trace(const RtSceneView& sc, const NS& ns, RtPath& p, Stack& stk) {
    RtTrace tr;
    tr.t = RT_R(0.0); tr.prim = RT_NONE; tr.scope = RT_NONE; tr.cls = RT_CLS_TERMINAL;
    if (p.depth_left == 0u) return tr;
    bool found = rt_closest_hit<Cfg>(sc, ns, p.ray, RT_R(0.001), RT_INF, p.rng, stk, tr.t, tr.prim, tr.scope);
    if (!found) { tr.prim = RT_NONE; return tr; }
    if constexpr (Cfg::sweep && RtHitShape<typename Cfg::Topo>::trace) {
        /* the class is a function of the leaf, so no load stands in front of the sort */
        tr.cls = RtHitShape<typename Cfg::Topo>::cls(tr.prim);
    } else {
        uint32_t mk = RT_MAT_KINDF(ns.hot(tr.prim).mat) & 0xFFu; /* the node carries its material's kind word */
        tr.cls = rt_class_of(mk);
    }
    /* the node's material word, which the second half wants for the material's index, where the wrapper was: the static hit record knows the chain */
    if constexpr (Cfg::sweep && RtHitShape<typename Cfg::Topo>::carry) tr.scope = ns.hot(tr.prim).mat;
    return tr;
}

/* second half: emitted / scatter / the next ray (main.rs:63-115).  The recursion
 * L = emitted + W (.) L'/pdf  is carried as  radiance += beta (.) emitted,
 * beta = beta (.) W / pdf.  Every terminal adds beta (.) value -- including the zero
 * of depth exhaustion (main.rs:59-61) -- so a non-finite beta poisons the sample
 * exactly as it does through the reference's multiplications. */
/* `later`: by default the Metal scatter draws its unit-sphere sample where it stands.  Given an RtSphereLater, the lane only says
 * that it wants one, keeps the fuzz and parks the reflected direction in p.ray.d: the sample is then drawn by the whole wave behind
 * the other materials (rt_path_shade_wave). */
struct RtSphereNow {};
struct RtSphereLater { bool* want; double* fuzz; };
template <class Cfg, class Sphere = RtSphereNow>
RT_HD void rt_path_shade(const RtSceneView& sc, RtPath& p, const RtTrace& tr, Sphere later = Sphere()) {
    if (p.depth_left == 0u) {
        p.radiance = p.radiance + rt_mul(p.beta, rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0)));
        p.alive = false;
        return;
    }
    if (tr.prim == RT_NONE) {
        p.radiance = p.radiance + rt_mul(p.beta, sc.background);
        p.alive = false;
        return;
    }
    const double t = tr.t;
    const uint32_t prim = tr.prim, scope = tr.scope;
    typedef RtHitShape<typename Cfg::Topo> HS;
    RtHit h;
    if constexpr (Cfg::sweep && HS::carry) rt_finish_hit_static<Cfg>(sc, p.ray, prim, scope /* the node's material word: rt_path_trace */, t, h);
    else if constexpr (Cfg::sweep && HS::record) rt_finish_hit_static<Cfg>(sc, p.ray, prim, sc.nodes[prim].mat, t, h);
    else rt_finish_hit<Cfg>(sc, p.ray, prim, scope, t, h);
    RT_STAMP(3);
    const RtMaterial& m = sc.materials[RT_MAT_INDEX(h.mat)];
    uint32_t mk = RT_MAT_KINDF(h.mat) & 0xFFu;
    RT_STAT_MAT(mk);

    /* emitted: DiffuseLight material.rs:168-181 (front face only); every other
     * material returns the default (0,0,0) (material.rs:40-49), whose addition in
     * main.rs:92 changes nothing, so it is not carried.  In this reference the
     * emitting material never scatters, so a path's radiance is beta (.) its
     * terminal value (light, background, or the zero of depth exhaustion). */
    if (mk == RT_MAT_DIFFUSE_LIGHT) {
        RtV3 emitted = h.front ? rt_mat_colour<Cfg>(sc, m, h.u, h.v, h.p) : rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0));
        p.radiance = p.radiance + rt_mul(p.beta, emitted);
        p.alive = false; /* DiffuseLight::scatter -> None, main.rs:110-112 */
        return;
    }

    if (mk == RT_MAT_LAMBERTIAN) {
        /* Lambertian::scatter material.rs:71-80 -> ScatterKind::Pdf(CosinePdf) */
        RtV3 attenuation = rt_mat_colour<Cfg>(sc, m, h.u, h.v, h.p);
        typedef RtLightShape<typename Cfg::Topo> LS;
        typedef RtLambertWalls<typename Cfg::Topo> LW;
        /* an axis rect outside every wrapper: its frame is one of six constants (rt_wall_frame); every other path computes it */
        bool wall, is_xz, is_xy;
        if constexpr (Cfg::sweep && HS::walls) { /* which leaf it is says all three */
            constexpr uint32_t WK = (LW::xy ? 1u << RT_XY : 0u) | (LW::xz ? 1u << RT_XZ : 0u) | (LW::yz ? 1u << RT_YZ : 0u);
            wall = LW::walls && (!LW::general || HS::template in<WK, RT_HF_NONE, 0u, RT_HG_UNWRAPPED>(prim));
            is_xz = HS::template in<1u << RT_XZ, RT_HF_NONE, 0u, RT_HG_ANY>(prim);
            is_xy = HS::template in<1u << RT_XY, RT_HF_NONE, 0u, RT_HG_ANY>(prim);
        } else {
            const uint32_t pk = LW::walls ? sc.nodes[prim].kind & RT_KIND_MASK : (uint32_t)RT_NONE;
            bool outside;
            if constexpr (Cfg::sweep && HS::carry) outside = HS::template in<RT_HK_ALL, RT_HF_NONE, 0u, RT_HG_UNWRAPPED>(prim); /* `scope` carries the material word */
            else outside = scope == RT_NONE;
            wall = LW::walls && (!LW::general || (outside && ((LW::xy && pk == RT_XY) || (LW::xz && pk == RT_XZ) || (LW::yz && pk == RT_YZ))));
            is_xz = pk == RT_XZ; is_xy = pk == RT_XY;
        }
        RtOnb uvw = rt_wall_frame<LW>(is_xz, is_xy, h.n);
        if (!LW::walls || (LW::general && RT_WAVE_ANY(!wall))) {
            RtOnb g = rt_onb_from_w(h.n);
            uvw = rt_onb_select(wall, uvw, g);
        }
        RtV3 dir;
        double pdf;
        /* MixturePdf::generate pdf.rs:62-68 (p0 = HittablePdf{lights}, p1 = CosinePdf), or CosinePdf alone.
         * The cosine lobe (math.rs:39-49), the sphere light (sphere.rs:92-99 -> math.rs:51-65) and the
         * rect light (aarect.rs:140-147) each consume two 64-bit draws, so the draws are taken once for
         * the three cases and only the conversion differs; cosine and sphere share one sincos. */
        uint32_t lk = RT_NONE; /* RT_NONE: cosine lobe */
        uint32_t li = 0u;
        if (LS::any(sc)) {
            rt_rng_fill(p.rng);
            if (rt_take_bool(p.rng)) {
                li = LS::choose(sc, p.rng); /* choose, hittable.rs:153 */
                lk = LS::kind(sc, li);
            }
        }
        /* the one sphere light's cone at h.p, for the lobe and for the pdf below: every Lambertian lane, whichever lobe it drew */
        typename std::conditional<LS::cone, RtSphereCone, RtNoCone>::type cone;
        if constexpr (LS::cone) cone = rt_sphere_cone(sc.lights[LS::index(RT_SPHERE, 0u)], h.p);
        if (!LS::may_default || lk == RT_NONE || lk == RT_XZ || lk == RT_SPHERE) {
            rt_rng_reserve(p.rng, rt_rng_need_2u64(p.rng));
            uint64_t q1 = rt_take_u64(p.rng);
            uint64_t q2 = rt_take_u64(p.rng);
            if (LS::may_xz && lk == RT_XZ) {
                const RtNode& l = sc.lights[LS::index(RT_XZ, li)];
                double x = rt_range_from_bits(q1, l.d[0], l.d[1]);
                if (!(x < l.d[1])) { /* rounding onto `high`: the retry takes the next draw (rand 0.8 sample_single) */
                    x = rt_range_from_bits(q2, l.d[0], l.d[1]);
                    while (!(x < l.d[1])) x = rt_range_from_bits(rt_next_u64(p.rng), l.d[0], l.d[1]);
                    q2 = rt_next_u64(p.rng);
                }
                double z = rt_range_from_bits(q2, l.d[2], l.d[3]);
                while (!(z < l.d[3])) z = rt_range_from_bits(rt_next_u64(p.rng), l.d[2], l.d[3]);
                dir = rt_v3(x, l.d[4], z) - h.p;
            } else {
                double r1 = rt_f64_from_bits(q1);
                double r2 = rt_f64_from_bits(q2);
                double phi = RT_R(2.0) * RT_R(RT_PI) * r1;
                double sn, cs;
                rt_sincos(phi, sn, cs);
                if constexpr (LS::cone && (RT_LOBE_SHARED) != 0) {
                    dir = rt_lobe_dir_shared(lk == RT_SPHERE, uvw, cone, r2, sn, cs);
                } else if (LS::may_sphere && lk == RT_SPHERE) {
                    if constexpr (LS::cone) {
                        RtOnb lw = rt_onb_from_w(cone.direction);
                        double z = RT_R(1.0) + r2 * (cone.cos_theta_max - RT_R(1.0));
                        double q = rt_sqrt(RT_R(1.0) - z * z);
                        dir = rt_onb_local(lw, rt_v3(cs * q, sn * q, z));
                    } else {
                        const RtNode& l = sc.lights[LS::index(RT_SPHERE, li)];
                        RtV3 direction = rt_v3(l.d[0], l.d[1], l.d[2]) - h.p;
                        double distance_squared = rt_mag2(direction);
                        RtOnb lw = rt_onb_from_w(direction);
                        double z = RT_R(1.0) + r2 * (rt_sqrt(RT_R(1.0) - l.d[3] * l.d[3] / distance_squared) - RT_R(1.0));
                        double q = rt_sqrt(RT_R(1.0) - z * z);
                        dir = rt_onb_local(lw, rt_v3(cs * q, sn * q, z));
                    }
                } else {
                    double z = rt_sqrt(RT_R(1.0) - r2);
                    double sr2 = rt_sqrt(r2);
                    dir = rt_onb_local(uvw, rt_v3(cs * sr2, sn * sr2, z));
                }
            }
        } else {
            dir = rt_v3(RT_R(1.0), RT_R(0.0), RT_R(0.0)); /* Hittable::random default, hittable.rs:69-71 */
        }
        double p1 = rt_max(rt_dot(rt_normalize(dir), uvw.w) / RT_R(RT_PI), RT_R(0.0)); /* CosinePdf::value pdf.rs:37-40 */
        if (LS::any(sc)) {
            double p0;
            if constexpr (LS::cone) p0 = LS::pdf_value(sc, cone, h.p, dir);
            else p0 = LS::pdf_value(sc, h.p, dir);
            pdf = RT_R(0.5) * p0 + RT_R(0.5) * p1; /* MixturePdf::value pdf.rs:58-60 */
        } else {
            pdf = p1;
        }
        /* Lambertian::scattering_pdf material.rs:82-91.  On a wall uvw.w is h.n bit for bit (an axis unit vector has magnitude exactly
         * 1 and n * (1.0 / 1.0) is n, signed zeros included), and so this is p1, the same operations on the same operands. */
        double spdf = p1;
        if (!LW::walls || (LW::general && RT_WAVE_ANY(!wall))) {
            double g = rt_max(rt_dot(h.n, rt_normalize(dir)) / RT_R(RT_PI), RT_R(0.0));
            spdf = wall ? p1 : g;
        }
        p.beta = rt_mul(p.beta, attenuation * spdf) / pdf;
        p.ray.o = h.p; p.ray.d = dir;
        p.ray.time = h.t; /* main.rs:86: time = hit_record.t (reference quirk Q1) */
        RT_STAMP(4);
    } else if (mk == RT_MAT_METAL) {
        /* Metal::scatter material.rs:99-111 */
        RtV3 reflected = rt_reflect(rt_normalize(p.ray.d), h.n);
        RtV3 dir;
        if constexpr (std::is_same<Sphere, RtSphereLater>::value) { *later.want = true; *later.fuzz = m.d[3]; dir = reflected; }
        else dir = reflected + m.d[3] * rt_random_in_unit_sphere(p.rng);
        p.beta = rt_mul(p.beta, rt_v3(m.d[0], m.d[1], m.d[2]));
        p.ray.o = h.p; p.ray.d = dir;
    } else if (mk == RT_MAT_DIELECTRIC) {
        /* Dielectric::scatter material.rs:133-160 */
        double refraction_ratio, r0 = RT_R(0.0);
        if constexpr (RT_MAT_DERIVED_ON) { refraction_ratio = h.front ? m.d[1] : m.d[0]; r0 = h.front ? m.d[2] : m.d[3]; }
        else refraction_ratio = h.front ? RT_R(1.0) / m.d[0] : m.d[0];
        RtV3 unit_direction = rt_normalize(p.ray.d);
        double cos_theta = rt_min(rt_dot(-unit_direction, h.n), RT_R(1.0));
        double sin_theta = rt_sqrt(RT_R(1.0) - cos_theta * cos_theta);
        bool cannot_refract = refraction_ratio * sin_theta > RT_R(1.0);
        RtV3 dir;
        if (cannot_refract || (RT_MAT_DERIVED_ON ? rt_reflectance_r0(cos_theta, r0) : rt_reflectance(cos_theta, refraction_ratio)) > rt_gen_f64(p.rng)) /* checked draw: rarely-run site */
            dir = rt_reflect(unit_direction, h.n);
        else
            dir = rt_refract(unit_direction, h.n, refraction_ratio);
        p.beta = rt_mul(p.beta, rt_v3(RT_R(1.0), RT_R(1.0), RT_R(1.0)));
        p.ray.o = h.p; p.ray.d = dir;
    } else if (Cfg::media && mk == RT_MAT_ISOTROPIC) {
        /* Isotropic::scatter constant_medium.rs:37-50 */
        RtV3 attenuation = rt_mat_colour<Cfg>(sc, m, h.u, h.v, h.p);
        RtV3 dir = rt_random_in_unit_sphere(p.rng);
        p.beta = rt_mul(p.beta, attenuation);
        p.ray.o = h.p; p.ray.d = dir;
    } else {
        /* impl Material for (): scatter -> None, emitted (0,0,0): main.rs:110-112 */
        p.radiance = p.radiance + rt_mul(p.beta, rt_v3(RT_R(0.0), RT_R(0.0), RT_R(0.0)));
        p.alive = false;
        return;
    }
    p.depth_left -= 1u;
    RT_STAMP(5);
}
#if RT_WAVE_ROUNDS_ON
/* rt_path_shade for the reordering kernels, called by every lane of the region: materials exclude each other per lane, so the Metal
 * lanes' sample can come last, behind a wave-uniform test, where the lanes of every other material -- and those whose path just ended
 * -- take rounds of it (rt_wave_rounds) and the sample is live across no other branch.  dir = reflected + fuzz * sample, as above. */
template <class Cfg>
__device__ __forceinline__ void rt_path_shade_wave(const RtSceneView& sc, RtPath& p, const RtTrace& tr) {
    bool sphere = false;
    double fuzz = RT_R(0.0);
    RtSphereLater later;
    later.want = &sphere; later.fuzz = &fuzz;
    rt_path_shade<Cfg>(sc, p, tr, later);
    if (RT_WAVE_ANY(sphere)) {
        const RtV3 v = rt_wave_rounds<true>(p.rng, sphere);
        if (sphere) p.ray.d = p.ray.d + fuzz * v;
    }
}
#endif

/* One level of ray_color (main.rs:51-116; with no lights :118-190) */
template <class Cfg, class Stack, class NS>
RT_HD void rt_path_step(const RtSceneView& sc, const NS& ns, RtPath& p, Stack& stk) {
    RtTrace tr = rt_path_trace<Cfg>(sc, ns, p, stk);
    rt_path_shade<Cfg>(sc, p, tr);
}

/* ----------------------------------------------------------------- color -- */

/* Color::into_sampled color.rs:14-21 */
RT_HD RtV3 rt_into_sampled(RtV3 sum, uint32_t samples_per_pixel) {
    double scale = RT_R(1.0) / (double)samples_per_pixel;
    double r = rt_isnan(sum.x) ? RT_R(0.0) : sum.x;
    double g = rt_isnan(sum.y) ? RT_R(0.0) : sum.y;
    double b = rt_isnan(sum.z) ? RT_R(0.0) : sum.z;
    return rt_v3(r, g, b) * scale;
}
/* Display for SampledColor color.rs:56-65: (256 * sqrt(c).clamp(0, 0.999)) as usize */
RT_HD uint32_t rt_quantize(double c) {
    double s = rt_sqrt(c);
    if (s < RT_R(0.0)) s = RT_R(0.0);
    if (s > RT_R(0.999)) s = RT_R(0.999);
    double q = RT_R(256.0) * s;
    return (q != q) ? 0u : (uint32_t)q;
}

/* work item -> (pixel, chunk): items are numbered so that 64 consecutive items
 * are an 8x8 pixel block of one chunk (rays of one wave start coherent). */
RT_HD void rt_item_decode(const RtFrame& f, uint64_t item, uint32_t& px, uint32_t& py, uint32_t& chunk) {
#if !defined(RT_NO_PROBE)
    if (f.probe) item = ((item >> 6) << 6) | ((item >> 6) & 63u); /* RtFrame::probe: 64 consecutive ids (one wave's) -> one item, one pixel per 8x8 block */
#endif
    uint32_t bw = (f.tile_w + 7u) >> 3, bh = (f.tile_h + 7u) >> 3;
    uint64_t per_chunk = (uint64_t)bw * bh * 64u;
    chunk = (uint32_t)(item / per_chunk);
    uint64_t r = item % per_chunk;
    uint32_t blk = (uint32_t)(r >> 6), in = (uint32_t)(r & 63u);
    px = (blk % bw) * 8u + (in & 7u);
    py = (blk / bw) * 8u + (in >> 3);
}
RT_HD uint64_t rt_item_count(const RtFrame& f) {
    uint32_t bw = (f.tile_w + 7u) >> 3, bh = (f.tile_h + 7u) >> 3;
    return (uint64_t)bw * bh * 64u * f.n_chunks;
}

#endif
