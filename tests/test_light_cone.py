"""The sphere light's cone, evaluated once per Lambertian bounce (rt_core.h: RtSphereCone, rt_sphere_cone, RtLightShape::cone,
rt_sphere_root_oc2; RT_LIGHT_CONE).  On the CPU: the flat core built around the library's own generated Topo of every scene of
bounce_scenes.py, once with the part and once with -DRT_LIGHT_CONE=0, against each other and against the generic core, bit for bit;
and the part's own functions against the ones they stand for on random operands.

Condition, not a statistic: every frame equal in every bit (a NaN where the other has a NaN), the segment counts equal, every pair
of squared distances and every pdf value equal in every bit."""
import ctypes as C

import numpy as np
import pytest

import bounce_scenes as Bn
import core_builds as CB
import orc


@pytest.fixture(scope="module")
def cases(rt):
    return [(f.__name__, f(rt)) for f in Bn.SCENES]


def _command(work, cases, tag, extra):
    census = lambda k, name, sc: (f"static_assert(RtLightShape<Topo_{tag}_{k}>::cone == {'true' if Bn.ELIGIBLE[name] and not extra else 'false'}, "
                                  "\"which units build the part\");\n")
    return CB.static_command(work, tag, [(name, sc, CB.topo_text(sc, "Topo")) for name, sc in cases], extra, per_unit=census)


@pytest.fixture(scope="module")
def libs(cases, tmp_path_factory):
    """(the core with the cone, the core built with -DRT_LIGHT_CONE=0): the static_assert in each unit's text is the census -- which
    Topo builds the part is checked by the compiler, in both builds"""
    work = tmp_path_factory.mktemp("light_cone")
    builds = [_command(work / "on", cases, "light_cone_on", []), _command(work / "off", cases, "light_cone_off", ["-DRT_LIGHT_CONE=0"])]
    CB.build_all([cmd for _, cmd in builds])
    return tuple(orc.declare_flat(C.CDLL(so)) for so, _ in builds)


def test_the_generated_units_say_which_build_the_part(cases):
    for name, sc in cases:
        assert Bn.eligible(sc) == Bn.ELIGIBLE[name], name
    by_name = dict(cases)
    # the rect-only room and arm 6 hold no sphere light, two_spheres holds two: their text is the parent's
    import lambert_scenes as L
    assert L.shape(by_name["rect_only"])[0] == [L.XZ] and L.shape(by_name["cornel_smoke"])[0] == [L.XZ]
    assert L.shape(by_name["two_spheres"])[0] == [L.SPHERE, L.SPHERE]
    assert L.shape(by_name["cornell"])[0] == [L.XZ, L.SPHERE] and L.shape(by_name["radius_zero"])[0] == [L.SPHERE, L.XZ]


@pytest.mark.parametrize("W,H,chunk,depth", Bn.FRAMES, ids=lambda v: str(v))
def test_frames_with_and_without_the_cone(libs, cases, W, H, chunk, depth):
    on, off = libs
    assert on.orcflat_n_static() == off.orcflat_n_static() == len(cases)
    for k, (name, sc) in enumerate(cases):
        g, sg = orc.flat_render(sc, W, H, 8, max_depth=depth, chunk=chunk)
        a, sa = orc.flat_render(sc, W, H, 8, max_depth=depth, chunk=chunk, variant=100 + k, lib=on)
        b, sb = orc.flat_render(sc, W, H, 8, max_depth=depth, chunk=chunk, variant=100 + k, lib=off)
        assert sa["segments"] == sb["segments"] == sg["segments"], name
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name + ": the cone changes a bit of the frame"
        assert np.array_equal(a, g, equal_nan=True), name + ": the specialised core differs from the generic one"
        assert np.any(a > 0.0), name


SHIM = r"""
#include <cstddef>
#include <cstring>
#include "rt_core.h"
extern "C" {
/* o, c: cnt x 3.  |o - c|^2 as rt_sphere_root forms it, |c - o|^2 as the lobe and the pdf form it, component squares included */
void lc_dist(const double* o, const double* c, uint64_t cnt, double* root_form, double* cone_form) {
    for (uint64_t i = 0; i < cnt; ++i) {
        const RtV3 O = rt_v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), Cc = rt_v3(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
        const RtV3 a = O - Cc, b = Cc - O;
        root_form[4 * i] = a.x * a.x; root_form[4 * i + 1] = a.y * a.y; root_form[4 * i + 2] = a.z * a.z; root_form[4 * i + 3] = rt_mag2(a);
        cone_form[4 * i] = b.x * b.x; cone_form[4 * i + 1] = b.y * b.y; cone_form[4 * i + 2] = b.z * b.z; cone_form[4 * i + 3] = rt_mag2(b);
    }
}
/* the pdf of a sphere light (centre c, radius r) at o towards v: the function itself, and the form that takes the cone */
void lc_pdf(const double* o, const double* c, const double* r, const double* v, uint64_t cnt, double* plain, double* with_cone, double* cone_out) {
    for (uint64_t i = 0; i < cnt; ++i) {
        RtNode l = {};
        l.kind = RT_SPHERE;
        l.d[0] = c[3 * i]; l.d[1] = c[3 * i + 1]; l.d[2] = c[3 * i + 2]; l.d[3] = r[i];
        const RtV3 O = rt_v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V = rt_v3(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
        const RtSphereCone k = rt_sphere_cone(l, O);
        plain[i] = rt_sphere_light_pdf_value(l, O, V);
        with_cone[i] = rt_sphere_light_pdf_value(l, k, O, V);
        cone_out[2 * i] = k.distance_squared; cone_out[2 * i + 1] = k.cos_theta_max;
    }
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return CB.shim_lib(tmp_path_factory.mktemp("light_cone_shim"), "light_cone", SHIM, csrc=True)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _points(g, n):
    """n points: a scene's coordinates, every exponent, and pairs that nearly cancel"""
    k = n // 4
    room = g.uniform(-600.0, 600.0, (k, 3))
    wide = np.ldexp(g.uniform(1.0, 2.0, (k, 3)) * g.choice([-1.0, 1.0], (k, 3)), g.integers(-500, 500, (k, 3)).astype(np.int32))
    tiny = np.ldexp(g.uniform(1.0, 2.0, (k, 3)), g.integers(-1074, -1000, (k, 3)).astype(np.int32))
    rest = g.uniform(-3.0, 3.0, (n - 3 * k, 3))
    return np.ascontiguousarray(np.concatenate([room, wide, tiny, rest]))


def test_squared_distances_agree_bit_for_bit(shim):
    """|o - c|^2 (rt_sphere_root's `oc`) and |c - o|^2 (the lobe's `direction`): the same bits component by component -- 10^5 random
    pairs, pairs a few ulps apart, and the specials (zeros of both signs, infinities, NaN, the largest and smallest doubles)"""
    g = np.random.default_rng(20261019)
    o, c = _points(g, 100_000), _points(g, 100_000)
    near = o[:20_000] * (1.0 + g.integers(-4, 5, (20_000, 3)) * 2.0 ** -52)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0, 2.2250738585072014e-308])
    so, sc = (x.ravel() for x in np.meshgrid(sp, sp))
    o = np.ascontiguousarray(np.concatenate([o, o[:20_000], np.stack([so, sc, so], axis=1)]))
    c = np.ascontiguousarray(np.concatenate([c, near, np.stack([sc, so, np.ones_like(so)], axis=1)]))
    a, b = np.empty((o.shape[0], 4)), np.empty((o.shape[0], 4))
    with np.errstate(all="ignore"):
        shim.lc_dist(_p(o), _p(c), C.c_uint64(o.shape[0]), _p(a), _p(b))
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])
    assert (~nan).all(axis=1).sum() >= 120_000


def test_pdf_with_the_cone_is_the_pdf(shim):
    """rt_sphere_light_pdf_value through rt_sphere_cone and rt_sphere_root_oc2 against the function itself: points outside, on and
    inside the sphere, radius 0, directions that hit and miss"""
    g = np.random.default_rng(7)
    n = 100_000
    c = g.uniform(-5.0, 5.0, (n, 3))
    r = np.abs(g.normal(0.0, 1.5, n))
    r[:1000] = 0.0
    o = c + g.normal(0.0, 1.0, (n, 3)) * r[:, None] * g.choice([0.3, 1.0, 3.0], n)[:, None]   # inside, about the surface, outside
    o[:1000] = c[:1000] + g.normal(0.0, 2.0, (1000, 3))
    o[1000:1100] = c[1000:1100]                                                              # at the centre: d2 = 0
    v = (c - o) + g.normal(0.0, 1.0, (n, 3)) * r[:, None] * g.choice([0.1, 1.0, 4.0], n)[:, None]
    o, c, v, r = (np.ascontiguousarray(x) for x in (o, c, v, r))
    plain, cone, k = np.empty(n), np.empty(n), np.empty((n, 2))
    with np.errstate(all="ignore"):
        shim.lc_pdf(_p(o), _p(c), _p(r), _p(v), C.c_uint64(n), _p(plain), _p(cone), _p(k))
    nan = np.isnan(plain)
    assert np.array_equal(nan, np.isnan(cone))
    assert np.array_equal(plain.view(np.uint64)[~nan], cone.view(np.uint64)[~nan])
    # the cases are all there: hits and misses, the NaN of a point inside, the infinity of radius 0
    assert (plain == 0.0).sum() > 1000 and np.isfinite(plain[plain > 0.0]).sum() > 1000 and nan.sum() > 1000 and np.isinf(plain).sum() > 0


def test_inside_light_shades_points_inside_the_light(shim):
    """the scene `inside_light` does what its name says: the floor point straight below the light's centre is inside the light, inside
    the floor rect, inside the camera's field of view and not hidden by the ball -- a first hit there is a Lambertian point whose cone,
    by the part's own function, has a NaN cosine and whose pdf is NaN in both forms"""
    (c, r), (bc, br), (frm, at, vfov) = Bn.INSIDE_LIGHT, Bn.INSIDE_BALL, Bn.INSIDE_CAMERA
    pt = np.array([c[0], 0.0, c[2]])
    assert 0.0 < pt[0] < 4.0 and 0.0 < pt[2] < 4.0 and np.linalg.norm(pt - np.array(c)) < r           # on the floor, inside the light
    frm, view, to = np.array(frm), np.array(at) - np.array(frm), pt - np.array(frm)
    cos_angle = view @ to / (np.linalg.norm(view) * np.linalg.norm(to))
    assert np.degrees(np.arccos(cos_angle)) < 0.5 * vfov - 5.0                                        # well inside the (square) frame
    oc = frm - np.array(bc)
    d = to / np.linalg.norm(to)
    assert (oc @ d) ** 2 - (oc @ oc - br * br) < 0.0                                                  # the line of sight misses the ball
    o = np.ascontiguousarray(pt[None, :])
    cc, rr, v = np.ascontiguousarray(np.array(c)[None, :]), np.array([r]), np.ascontiguousarray(np.array([[0.0, 1.0, 0.0]]))
    plain, cone, k = np.empty(1), np.empty(1), np.empty((1, 2))
    with np.errstate(all="ignore"):
        shim.lc_pdf(_p(o), _p(cc), _p(rr), _p(v), C.c_uint64(1), _p(plain), _p(cone), _p(k))
    assert k[0, 0] < r * r and np.isnan(k[0, 1]) and np.isnan(plain[0]) and np.isnan(cone[0])
