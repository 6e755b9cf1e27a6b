"""The glass and light bounces without their scene-only terms (rt_core.h: RT_MAT_DERIVED, RT_NORMAL_SHARED, RT_LOBE_SHARED), on the CPU.

A  a Dielectric record carries 1 / ir and the two r0 (rt_flat.h: rt_material_derive): the stored fields against the expressions a bounce
   evaluates, bit for bit, and frames of the host core built with and without the switch.
B  a sphere's outward normal from one prepared divisor (rt_div_q3 and the wave fallback of rt_sphere_normal): a 64-lane model on the
   host.  The one thing the CPU does not have is the seed v_rcp_f64 returns; as in test_div_shared.py the model takes it as a parameter,
   RN(1 / r) perturbed by up to 2^-24 relative.  The real seed is tested on the GPU (test_glass_terms_gpu.py).
C  one direction build for the cosine lobe and the sphere lobe (rt_lobe_dir_shared) against the two branches it stands for.

Condition, not a statistic: equal in every bit (a NaN where the other has a NaN), segment counts equal."""
import ctypes as C

import numpy as np
import pytest

import core_builds as CB
import glass_scenes as G
import orc

IRS = [1.5, 1.0, 0.5, 1.0 / 3.0, 2.4, 1.7976931348623157e308, 5e-324]

SHIM = r"""
#include <cstddef>
#include <cstring>
#include "rt_core.h"
extern "C" {
/* what a Dielectric bounce computes from ir when the record does not carry it (the text under RT_MAT_DERIVED=0): the front face's ratio,
 * and rt_reflectance's r0 of either face's ratio -- at cosine 1 the function returns r0 + (1 - r0) * 0, which is r0 in every bit
 * unless r0 is not finite (then both are NaN or the infinity itself is not reached: the caller compares NaN to NaN) */
void gt_fields(const double* ir, uint64_t cnt, double* out) {
    for (uint64_t i = 0; i < cnt; ++i) {
        const double ratio = RT_R(1.0) / ir[i];
        out[3 * i] = ratio;
        out[3 * i + 1] = rt_reflectance(1.0, ratio);
        out[3 * i + 2] = rt_reflectance(1.0, ir[i]);
    }
}
/* what rt_material_derive writes */
void gt_derive(const double* ir, uint64_t cnt, double* out) {
    for (uint64_t i = 0; i < cnt; ++i) {
        RtMaterial m;
        memset(&m, 0, sizeof m);
        m.kind = RT_MAT_DIELECTRIC; m.d[0] = ir[i];
        rt_material_derive(m);
        out[3 * i] = m.d[1]; out[3 * i + 1] = m.d[2]; out[3 * i + 2] = m.d[3];
    }
}
/* the reflectance of a bounce, both forms: from the ratio, and from the r0 the record carries */
void gt_reflectance(const double* cosine, const double* ri, const double* r0, uint64_t cnt, double* from_ratio, double* from_r0) {
    for (uint64_t i = 0; i < cnt; ++i) { from_ratio[i] = rt_reflectance(cosine[i], ri[i]); from_r0[i] = rt_reflectance_r0(cosine[i], r0[i]); }
}
/* B: waves of 64 lanes.  n: cnt x 3, r, y0 (the seed): cnt; cnt a multiple of 64.  fast: rt_div_q3's quotients; bad: its guard per lane;
 * fell: per wave, whether rt_sphere_normal's fallback ran; out: what the wave's lanes end with; slow: n / r */
void gt_normal(const double* n, const double* r, const double* y0, uint64_t cnt, double* fast, uint8_t* bad, uint8_t* fell, double* out, double* slow) {
    for (uint64_t w = 0; w < cnt / 64; ++w) {
        bool any = false;
        for (uint64_t i = 64 * w; i < 64 * w + 64; ++i) {
            bool b;
            const RtV3 q = rt_div_q3(rt_v3(n[3 * i], n[3 * i + 1], n[3 * i + 2]), r[i], rt_div_refine(r[i], y0[i]), b);
            fast[3 * i] = q.x; fast[3 * i + 1] = q.y; fast[3 * i + 2] = q.z;
            bad[i] = b; any = any | b;
        }
        fell[w] = any;
        for (uint64_t i = 64 * w; i < 64 * w + 64; ++i) {
            const RtV3 s = rt_v3(n[3 * i], n[3 * i + 1], n[3 * i + 2]) / r[i];
            slow[3 * i] = s.x; slow[3 * i + 1] = s.y; slow[3 * i + 2] = s.z;
            for (int k = 0; k < 3; ++k) out[3 * i + k] = any ? slow[3 * i + k] : fast[3 * i + k];
        }
    }
}
double gt_lo() { return RT_DIV_LO; }
double gt_hi() { return RT_DIV_HI; }
/* C: the direction of a Lambertian lane that drew the sphere lobe (`sphere`) or the cosine lobe about the frame of `normal`: the two
 * branches as rt_path_shade states them without the part, and the shared build */
void gt_lobe(const double* r1, const double* r2, const double* normal, const double* cone_dir, const double* cos_theta_max, const uint8_t* sphere,
             uint64_t cnt, double* two, double* shared) {
    for (uint64_t i = 0; i < cnt; ++i) {
        const RtOnb uvw = rt_onb_from_w(rt_v3(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]));
        RtSphereCone cone;
        cone.direction = rt_v3(cone_dir[3 * i], cone_dir[3 * i + 1], cone_dir[3 * i + 2]);
        cone.distance_squared = rt_mag2(cone.direction);
        cone.cos_theta_max = cos_theta_max[i];
        double phi = RT_R(2.0) * RT_R(RT_PI) * r1[i];
        double sn, cs;
        rt_sincos(phi, sn, cs);
        RtV3 dir;
        if (sphere[i]) {
            RtOnb lw = rt_onb_from_w(cone.direction);
            double z = RT_R(1.0) + r2[i] * (cone.cos_theta_max - RT_R(1.0));
            double q = rt_sqrt(RT_R(1.0) - z * z);
            dir = rt_onb_local(lw, rt_v3(cs * q, sn * q, z));
        } else {
            double z = rt_sqrt(RT_R(1.0) - r2[i]);
            double sr2 = rt_sqrt(r2[i]);
            dir = rt_onb_local(uvw, rt_v3(cs * sr2, sn * sr2, z));
        }
        two[3 * i] = dir.x; two[3 * i + 1] = dir.y; two[3 * i + 2] = dir.z;
        const RtV3 s = rt_lobe_dir_shared(sphere[i] != 0, uvw, cone, r2[i], sn, cs);
        shared[3 * i] = s.x; shared[3 * i + 1] = s.y; shared[3 * i + 2] = s.z;
    }
}
}
"""


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same_bits(a, b):
    """equal in every bit; where one is a NaN the other is"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = CB.shim_lib(tmp_path_factory.mktemp("glass_terms_shim"), "glass_terms", SHIM, csrc=True)
    L.gt_lo.restype = L.gt_hi.restype = C.c_double
    return L


# ------------------------------------------------------------------------------------------------------------------ A: the fields

def _glass_scene(rt, irs):
    """one sphere per ir; returns the committed scene's material records as (n, 6) doubles (d[0..3], kind | tex, pads)"""
    s = rt.Scene(build_seed=1)
    objs = [s.sphere((2.5 * k, 0.0, -3.0), 1.0, s.dielectric(ir)) for k, ir in enumerate(irs)]
    s.set_world(s.bvh_node(objs))
    s.set_lights([])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), (0, 1, 0), 60.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    s.commit()
    rec = s.flat(2)
    assert rec.size == 48 * len(irs)
    return rec.view(np.float64).reshape(len(irs), 6)[:, :4], rec.view(np.uint32).reshape(len(irs), 12)[:, 8]


def test_the_record_carries_what_a_bounce_computes(rt, shim):
    """d[1], d[2], d[3] of every Dielectric record the library writes against 1 / ir and rt_reflectance's r0 of the front and the back
    face's ratio as the core evaluates them; ir 1.5, 1, 0.5, 1/3, 2.4, the largest finite double and a subnormal"""
    irs = np.array(IRS)
    d, kind = _glass_scene(rt, IRS)
    assert np.all((kind & 0xFF) == 3) and _same_bits(d[:, 0], irs)
    want, derived = np.empty((irs.size, 3)), np.empty((irs.size, 3))
    with np.errstate(all="ignore"):
        shim.gt_fields(_p(irs), C.c_uint64(irs.size), _p(want))
        shim.gt_derive(_p(irs), C.c_uint64(irs.size), _p(derived))
    assert _same_bits(d[:, 1:], want), "a stored field is not the value the bounce computes"
    assert _same_bits(derived, want)
    # the cases are what they are meant to be: ratio 1 has r0 = 0 on both faces; 1 / max is a subnormal, 1 / subnormal an infinity whose r0 is a NaN
    assert d[1, 1] == 1.0 and d[1, 2] == 0.0 and d[1, 3] == 0.0
    assert 0.0 < d[5, 1] < 2.2250738585072014e-308 and np.isinf(d[6, 1]) and np.isnan(d[6, 2]) and d[6, 3] == 1.0
    assert d[0, 1] == 1.0 / 1.5 and abs(d[0, 2] - 0.04) < 1e-15 and abs(d[0, 3] - 0.04) < 1e-15


def test_reflectance_from_the_stored_r0_is_reflectance(rt, shim):
    """rt_reflectance_r0 on the stored r0 against rt_reflectance on the ratio, 10^5 cosines per ir and face (the range a bounce can
    see and a little beyond), the specials among them"""
    g = np.random.default_rng(20261020)
    d, _ = _glass_scene(rt, IRS)
    for row in d:
        for ri, r0 in ((row[1], row[2]), (row[0], row[3])):
            cos = np.concatenate([g.uniform(-1.0, 1.0, 100_000), [1.0, 0.0, -0.0, -1.0, 1.0 - 2.0 ** -53, np.nan, 5e-324]])
            a, b = np.empty(cos.size), np.empty(cos.size)
            with np.errstate(all="ignore"):
                shim.gt_reflectance(_p(cos), _p(np.full(cos.size, ri)), _p(np.full(cos.size, r0)), C.c_uint64(cos.size), _p(a), _p(b))
            assert _same_bits(a, b), (ri, r0)


def test_other_materials_keep_their_fields(rt):
    """rt_material_derive touches Dielectric records only: a Metal's d[0..3] are its albedo and fuzz"""
    s = rt.Scene(build_seed=1)
    m = s.metal((0.25, 0.5, 0.75), 0.125)
    s.set_world(s.bvh_node([s.sphere((0.0, 0.0, -3.0), 1.0, m)]))
    s.set_lights([])
    s.set_background((0.5, 0.7, 1.0))
    s.set_camera((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), (0, 1, 0), 60.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    s.commit()
    assert list(s.flat(2).view(np.float64)[:4]) == [0.25, 0.5, 0.75, 0.125]


# ------------------------------------------------------------------------------------------------------------------ frames

@pytest.fixture(scope="module")
def cases(rt):
    return [(f.__name__, f(rt)) for f in G.SPECIALISED]


# host builds of the core: as shipped, each switch that reaches host code alone at its other setting, and all three out (RT_NORMAL_SHARED
# is device code only: the host core divides three times under either setting, its switch is in the last build for the record)
BUILDS = ([], [G.OFF["A"]], [G.OFF["C"]], G.ALL_OFF.split())


def _command(work, cases, tag, extra):
    shared, derived = ("true" if G.OFF[part] not in extra else "false" for part in "CA")
    census = lambda k, name, sc: (f"static_assert(RtLightShape<Topo_{tag}_{k}>::cone, \"one sphere light: the unit builds the lobes' part\");\n"
                                  f"static_assert(((RT_LOBE_SHARED) != 0) == {shared} && (RT_MAT_DERIVED_ON) == {derived}, \"the switches reach the core\");\n")
    return CB.static_command(work, tag, [(name, sc, CB.topo_text(sc, "Topo")) for name, sc in cases], extra, per_unit=census)


@pytest.fixture(scope="module")
def libs(cases, tmp_path_factory):
    work = tmp_path_factory.mktemp("glass_terms")
    builds = [_command(work / f"b{k}", cases, f"glass_terms_b{k}", extra) for k, extra in enumerate(BUILDS)]
    CB.build_all([cmd for _, cmd in builds])
    return [orc.declare_flat(C.CDLL(so)) for so, _ in builds]


@pytest.mark.parametrize("W,H,chunk", G.FRAMES, ids=lambda v: str(v))
def test_frames_under_every_switch(libs, cases, W, H, chunk):
    """arm 5 and the hand-built scene through their specialised host units, every build against the shipped one and against the generic core"""
    for k, (name, sc) in enumerate(cases):
        g, sg = orc.flat_render(sc, W, H, 8, chunk=chunk)
        a, sa = orc.flat_render(sc, W, H, 8, chunk=chunk, variant=100 + k, lib=libs[0])
        assert sa["segments"] == sg["segments"] and np.array_equal(a, g, equal_nan=True), name + ": the specialised core differs from the generic one"
        for extra, lib in zip(BUILDS[1:], libs[1:]):
            assert lib.orcflat_n_static() == len(cases)
            b, sb = orc.flat_render(sc, W, H, 8, chunk=chunk, variant=100 + k, lib=lib)
            assert sb["segments"] == sa["segments"], (name, extra)
            assert _same_bits(a, b), f"{name}: {' '.join(extra)} changes a bit of the frame"
        assert np.any(a > 0.0), name


def test_generic_frames_under_every_switch(rt, libs, cases):
    """the generic units read the same records: arm 0 cropped (glass on the stack walk), arm 5 and the hand-built scene through the
    variant the library picks, every build against the shipped oracle library"""
    W, H = G.ARM0_FRAME
    todo = [("random_scene", G.random_scene(rt), W, H, G.ARM0_TILE)] + [(n, sc, 32, 32, None) for n, sc in cases]
    for name, sc, w, h, tile in todo:
        g, sg = orc.flat_render(sc, w, h, 8, tile=tile)
        for extra, lib in zip(BUILDS, libs):
            b, sb = orc.flat_render(sc, w, h, 8, tile=tile, lib=lib)
            assert sb["segments"] == sg["segments"], (name, extra)
            assert _same_bits(g, b), f"{name}: {' '.join(extra)} changes a bit of the generic frame"


def test_the_hand_built_scene_is_what_it_says():
    """nested_and_aligned: the aligned sphere's centre lies in the wall's plane and at the camera's height, the inner sphere of ir 1 inside
    the outer one; and a camera ray from z = 0 meets the plane z = k at a z that is k exactly in most cases, (k / d) * d == k -- from
    such a point the default lobe (1, 0, 0) reaches the aligned sphere with an exact zero in p - c"""
    (c, r), k = G.ALIGNED, G.WALL_K
    assert c[2] == k and c[1] == G.CAMERA[0][1] and G.CAMERA[0][2] == 0.0
    assert G.NESTED[2] < G.NESTED[1]
    g = np.random.default_rng(3)
    d = -g.uniform(0.5, 1.0, 100_000)                        # the z of a normalised-or-not direction towards the wall
    assert np.mean((k / d) * d == k) > 0.5


# ------------------------------------------------------------------------------------------------------------------ B: the normal

SEED_ERR = 2.0 ** -24


def _seeds(r, g):
    with np.errstate(all="ignore"):
        y = 1.0 / r
        e = g.uniform(-SEED_ERR, SEED_ERR, r.size)
        e[0::7] = SEED_ERR
        e[1::7] = -SEED_ERR
        return y * (1.0 + e)


def _normal_samples(g):
    """10^6 lanes (15625 waves) of (p - c, r): scene-sized numbers for most, so that whole waves pass; every exponent; and the specials
    -- zeros of both signs, subnormals, huge values, infinities, NaN -- one to a wave in some waves, many to a wave in others"""
    n_lanes = 1_000_000
    n = g.uniform(-1.0, 1.0, (n_lanes, 3)) * g.choice([1.0, 90.0, 1000.0], (n_lanes, 1))
    r = g.choice([90.0, 0.5, 1.0, 1000.0, 0.2], n_lanes) * g.choice([1.0, 1.0, 1.0 + 2.0 ** -30], n_lanes)
    wide = slice(700_000, 900_000)                          # every exponent a double has
    m = lambda shape: g.uniform(1.0, 2.0, shape) * g.choice([-1.0, 1.0], shape)
    n[wide] = np.ldexp(m((200_000, 3)), g.integers(-1070, 1023, (200_000, 3)).astype(np.int32))
    r[wide] = np.ldexp(m(200_000), g.integers(-1070, 1023, 200_000).astype(np.int32))
    mid = slice(900_000, 1_000_000)                         # inside the guards' range by construction
    n[mid] = np.ldexp(m((100_000, 3)), g.integers(-140, 140, (100_000, 3)).astype(np.int32))
    r[mid] = np.ldexp(m(100_000), g.integers(-140, 140, 100_000).astype(np.int32))
    sp = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 2.0 ** -301 * 90.0, 2.0 ** 301, 1.7976931348623157e308, np.inf, -np.inf, np.nan])
    # one special numerator component in one lane of each of the first 2000 waves
    lanes = 64 * np.arange(2000) + g.integers(0, 64, 2000)
    n[lanes, g.integers(0, 3, 2000)] = g.choice(sp, 2000)
    # a special divisor in one lane of each of the next 500 waves; the radius 0 of a degenerate sphere among them
    lanes = 64 * np.arange(2000, 2500) + g.integers(0, 64, 500)
    r[lanes] = g.choice(np.concatenate([sp, [2.0 ** -300, 2.0 ** 300]]), 500)
    # waves full of zeros: the aligned sphere's case for every lane
    n[64 * 2500:64 * 2600, 2] = g.choice([0.0, -0.0], 6400)
    return np.ascontiguousarray(n), np.ascontiguousarray(r)


def test_normal_from_one_prepared_divisor(shim):
    g = np.random.default_rng(20261021)
    n, r = _normal_samples(g)
    cnt = r.size
    assert cnt % 64 == 0 and cnt == 1_000_000
    y0 = _seeds(r, g)
    fast, out, slow = np.empty((cnt, 3)), np.empty((cnt, 3)), np.empty((cnt, 3))
    bad, fell = np.empty(cnt, dtype=np.uint8), np.empty(cnt // 64, dtype=np.uint8)
    with np.errstate(all="ignore"):
        shim.gt_normal(_p(n), _p(r), _p(y0), C.c_uint64(cnt), _p(fast), _p(bad), _p(fell), _p(out), _p(slow))
        want = n / r[:, None]
    assert _same_bits(slow, want)
    # every lane of every wave ends with the division's bits
    assert _same_bits(out, want), "a lane's normal differs from (p - c) / r"
    # the fallback runs exactly in the waves that hold a lane whose guard failed ...
    assert np.array_equal(fell.astype(bool), bad.reshape(-1, 64).astype(bool).any(axis=1))
    # ... and a lane's guard is the header's: the divisor's range, every quotient's range as one that is used
    lo, hi = shim.gt_lo(), shim.gt_hi()
    with np.errstate(all="ignore"):
        guard = ~((np.abs(r) > lo) & (np.abs(r) < hi)) | ~((np.abs(fast) > lo) & (np.abs(fast) < hi)).all(axis=1)
    assert np.array_equal(bad.astype(bool), guard)
    # wherever the guards pass, the quotients alone are the division's bits (no help from the fallback of a neighbour)
    good = ~bad.astype(bool)
    assert _same_bits(fast[good], want[good])
    # what the guards must catch, from the division's own operands and results
    with np.errstate(all="ignore"):
        special = ~(np.abs(r) > lo) | ~(np.abs(r) < hi) | ~((np.abs(want) > lo) & (np.abs(want) < hi)).all(axis=1)
    assert not np.any(special & good), "a zero, infinity, NaN, denormal or out-of-range value passed the guards"
    # the census: whole waves pass, whole waves fall back, and the zeros' waves all do
    assert (fell == 0).sum() > 5000 and (fell == 1).sum() > 3000 and fell[2500:2600].all()
    assert good[900_000:].all()
    # the zero's sign is what the guard is for: somewhere among the zero components rt_div_q's sign is not the division's
    z = (want == 0.0) & np.isfinite(fast)
    assert np.any(np.signbit(fast[z]) != np.signbit(want[z]))


# ------------------------------------------------------------------------------------------------------------------ C: the lobes

def test_one_direction_build_for_both_lobes(shim):
    """10^5 (r1, r2, cone) triples, each as a sphere-lobe lane and as a cosine-lobe lane: cones of every width, the cosine 1 of radius 0,
    the NaN cosine of a point inside the light, r2 at both ends, frames about every kind of normal"""
    g = np.random.default_rng(20261022)
    cnt = 100_000
    r1, r2 = g.uniform(0.0, 1.0, cnt), g.uniform(0.0, 1.0, cnt)
    r2[:200] = 0.0
    r2[200:400] = 1.0 - 2.0 ** -53
    r1[400:500] = 0.0
    ctm = np.sqrt(1.0 - g.uniform(0.0, 1.0, cnt))
    ctm[1000:2000] = np.nan
    ctm[2000:2500] = 1.0
    ctm[2500:3000] = 0.0
    normal = g.normal(0.0, 1.0, (cnt, 3))
    axes = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, -0.0], [0.0, 0.0, 1.0], [-0.0, 0.0, -1.0]])
    normal[3000:9000] = axes[g.integers(0, 6, 6000)]
    cone_dir = g.normal(0.0, 200.0, (cnt, 3))
    cone_dir[9000:9500] = axes[g.integers(0, 6, 500)] * 300.0
    cone_dir[9500:9600] = 0.0                                  # the shaded point at the light's centre: a NaN frame
    r1, r2, ctm, normal, cone_dir = (np.ascontiguousarray(x) for x in (r1, r2, ctm, normal, cone_dir))
    for sphere in (1, 0):
        flag = np.full(cnt, sphere, dtype=np.uint8)
        two, shared = np.empty((cnt, 3)), np.empty((cnt, 3))
        with np.errstate(all="ignore"):
            shim.gt_lobe(_p(r1), _p(r2), _p(normal), _p(cone_dir), _p(ctm), _p(flag), C.c_uint64(cnt), _p(two), _p(shared))
        assert _same_bits(two, shared), "the shared build differs from the " + ("sphere" if sphere else "cosine") + " lobe"
        assert np.isfinite(two).all(axis=1).sum() > 90_000
        if sphere:
            assert np.isnan(two[1000:2000]).any(axis=1).all() and np.isnan(two[9500:9600]).all()
    # mixed lanes, as a wave holds them
    flag = g.integers(0, 2, cnt).astype(np.uint8)
    two, shared = np.empty((cnt, 3)), np.empty((cnt, 3))
    with np.errstate(all="ignore"):
        shim.gt_lobe(_p(r1), _p(r2), _p(normal), _p(cone_dir), _p(ctm), _p(flag), C.c_uint64(cnt), _p(two), _p(shared))
    assert _same_bits(two, shared)
