"""Quotients of one divisor on the GPU (include/rt1w_num.h: rt_div_prep / rt_div_q / rt_div_inv and their guards; rt_core.h: the
unrolled sweep over RtInvShared, the second sweep with `/` for a wave that left the range).

Part one, the arithmetic with the real seed (v_rcp_f64): rt1w_debug_eval 14 (the quotient), 15 (the guards) and 16 (1/d) against
`/` on the device (selector 0) and on the CPU, 2^20 pairs of the input classes of test_div_shared.py.  Condition: every pair whose
guards pass has the division's bits; every zero, infinity, NaN, denormal and out-of-range operand or result raises a guard.

Part two, frames: the scene-specialised kernel as shipped = the same kernel built with -DRT_DIV_SHARED=0 (`/` everywhere) = built
with -DRT_DIV_SHARED_FORCE_SLOW=1 (every wave runs the second sweep) = the generic kernel = the CPU build of the core, byte for byte."""
import numpy as np
import pytest

import core_builds as CB
import hit_scenes as H
import orc
import slab_scenes as S

pytestmark = pytest.mark.gpu

LO, HI = 2.0 ** -300, 2.0 ** 300


# ------------------------------------------------------------------ part one

def pairs():
    """2^20 (n, d): random over every exponent, random in the sweep's range, next to rounding midpoints, the specials, the bounds"""
    g = np.random.default_rng(20241019)
    m = lambda k: g.uniform(1.0, 2.0, k) * g.choice([-1.0, 1.0], k)
    e = lambda k, lo, hi: g.integers(lo, hi, k).astype(np.int32)
    k = 1 << 18
    n = [np.ldexp(m(k), e(k, -1070, 1023)), np.ldexp(m(k), e(k, -140, 140)), np.ldexp(m(k), e(k, -10, 10))]
    d = [np.ldexp(m(k), e(k, -1070, 1023)), np.ldexp(m(k), e(k, -140, 140)), np.ldexp(m(k), e(k, -10, 10))]
    # next to midpoints: n = d x (q +- half an ulp), rounded
    k4 = (1 << 18) - 4096
    q, dd = np.ldexp(g.uniform(1.0, 2.0, k4), e(k4, -60, 60)), np.ldexp(m(k4), e(k4, -60, 60))
    n.append(q * dd + (g.choice([0.5, -0.5, 0.0], k4) * np.spacing(q)) * dd)
    d.append(dd)
    # specials and the bounds, every combination (64 x 64 = 4096)
    up, dn = lambda x: np.nextafter(x, np.inf), lambda x: np.nextafter(x, 0.0)
    sp = [0.0, np.inf, np.nan, 5e-324, 1e-310, 2.2250738585072014e-308, 1.7976931348623157e308, LO, up(LO), dn(LO), HI, up(HI), dn(HI),
          2 * LO, HI / 2, 1.0, 3.0, 0.001, 555.0, 2.0 ** 200, 2.0 ** -200, 2.0 ** 150, 2.0 ** -150, 1.5 * LO, 1.5 * HI, 0.75 * HI, 2.0 ** 599, 2.0 ** -599,
          2.0 ** -969, 2.0 ** -970, 2.0 ** 768, 7.0]
    sp = np.array(sp + [-x for x in sp])
    assert sp.size == 64
    a, b = (x.ravel() for x in np.meshgrid(sp, sp))
    n.append(a)
    d.append(b)
    n, d = np.concatenate(n), np.concatenate(d)
    assert n.size == 1 << 20
    return n, d


def test_quotient_and_guards_with_the_real_seed(rt, gpu_ctx_factory):
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    n, d = pairs()
    q_fast = ctx.debug_eval(14, n, d)
    verdict = ctx.debug_eval(15, n, d).astype(np.int64)
    inv_fast = ctx.debug_eval(16, n, d)
    q_dev = ctx.debug_eval(0, n, d)
    inv_dev = ctx.debug_eval(0, np.ones_like(d), d)
    with np.errstate(all="ignore"):
        q_cpu, inv_cpu = n / d, 1.0 / d
    bits = lambda x: x.view(np.uint64)
    nan = np.isnan(q_cpu)
    assert np.array_equal(bits(q_dev)[~nan], bits(q_cpu)[~nan]) and np.all(np.isnan(q_dev[nan]))   # the yardstick: `/` is `/` on both sides
    good = (verdict & 3) == 0
    print(f"in range: {good.sum()} of {good.size}; quotient mismatches among them: {(bits(q_fast)[good] != bits(q_dev)[good]).sum()}")
    assert good.sum() > 700_000
    assert np.array_equal(bits(q_fast)[good], bits(q_dev)[good]), "an in-range quotient differs from n / d"
    dok = (verdict & 1) == 0
    assert np.array_equal(bits(inv_fast)[dok], bits(inv_dev)[dok]) and np.array_equal(bits(inv_fast)[dok], bits(inv_cpu)[dok]), "1/d differs from 1.0 / d"
    with np.errstate(all="ignore"):
        special = ~(np.abs(d) > LO) | ~(np.abs(d) < HI) | ~(np.abs(q_cpu) > LO) | ~(np.abs(q_cpu) < HI)
        too_big = ((verdict & 1) == 0) & ~(np.abs(q_cpu) < HI)
    assert not np.any(special & good), "a zero, infinity, NaN, denormal or out-of-range value passed the guards"
    assert np.all((verdict[too_big] & 4) != 0), "a quotient at or above the upper bound, or a NaN, was not called too large"
    # the guards on the device are the guards on the CPU: the divisor's from d, and nothing in range is called bad
    with np.errstate(all="ignore"):
        assert np.array_equal((verdict & 1) != 0, ~((np.abs(d) > LO) & (np.abs(d) < HI)))
        inside = ((verdict & 1) == 0) & (np.abs(q_cpu) > 2 * LO) & (np.abs(q_cpu) < HI / 2)
    assert np.all((verdict[inside] & 6) == 0)


# ------------------------------------------------------------------ part two

def cornell(rt):
    return rt.Scene.reference(5, build_seed=1)


# Cornell, every scene of hit_scenes.py (all six stand in L._corner's three walls under a rect light; many_chains: ten RotateY spaces,
# more than 64 nodes, chains without a block; sphere_under_wrappers: sphere leaves swept under the shared divisors of a RotateY space)
# and the two scenes of slab_scenes.py that hold a rect (the other four are spheres only: their units keep one sweep)
SCENES = {f.__name__: f for f in (cornell,) + tuple(H.HAND_BUILT) + (S.nan_best_t, S.nan_some_rays)}
BUILDS = (None, "-DRT_DIV_SHARED=0", "-DRT_DIV_SHARED_FORCE_SLOW=1")


@pytest.fixture(scope="module")
def kernels(rt, gpu_ctx_factory, tmp_path_factory):
    """name -> (scene, context with the kernel as shipped, with `/` everywhere, with the second sweep forced); built once per scene"""
    cache = str(tmp_path_factory.mktemp("div_shared_kcache"))
    made = {}

    def get(name):
        if name not in made:
            sc = SCENES[name](rt)
            made[name] = (sc,) + tuple(CB.specialised(gpu_ctx_factory, sc, cache, o) for o in BUILDS)
        return made[name]

    return get


# scene, width, height, spp, chunk (0: the library's), max_depth: every scene at 32x32 with depth 50 and depth 3 and at 8x4 (32 work
# items: half of the only wave that works has retired from the start), 8 spp.  A case renders in about 0.1 s; the first case of a scene
# compiles its three kernels as well: 2.6-5.8 s measured on an MI355X host, and 22.7 s for many_chains (169 nodes, about 7 s a build) --
# the four-way equality needs all three builds, and the issue names the scene.
# nan_best_t: vfov = 0, every ray is (0, 0, -f): two divisors of three are zero and the rect's quotient is 0 / 0 -- the guards send
# every wave to the second sweep; nan_some_rays: d.y == 0 in every lane, 0 / 0 in some
FRAMES = [(name, W, H, 8, chunk, depth) for name in SCENES for (W, H, chunk, depth) in ((32, 32, 0, 50), (32, 32, 0, 3), (8, 4, 8, 50), (8, 4, 8, 3))]


@pytest.mark.parametrize("name,W,H,spp,chunk,depth", FRAMES, ids=lambda v: str(v))
def test_frames_equal_the_division(kernels, name, W, H, spp, chunk, depth):
    sc, on, off, slow = kernels(name)
    a, sa = on.render(W, H, spp, max_depth=depth, chunk=chunk)
    o, so = off.render(W, H, spp, max_depth=depth, chunk=sa["chunk"])
    w, sw = slow.render(W, H, spp, max_depth=depth, chunk=sa["chunk"])
    g, sg = on.render(W, H, spp, max_depth=depth, chunk=sa["chunk"], generic=True)
    f, sf = orc.flat_render(sc, W, H, spp, max_depth=depth, chunk=sa["chunk"])
    assert all(s["sorted"] & 4 for s in (sa, so, sw)) and not (sg["sorted"] & 4)   # three specialised kernels, one generic
    assert sa["segments"] == so["segments"] == sw["segments"] == sg["segments"] == sf["segments"]
    assert np.array_equal(a, f, equal_nan=True), "specialised kernel with shared divisors differs from the CPU build of the core"
    assert np.array_equal(a, o, equal_nan=True), "shared divisors and `/` differ in the same kernel"
    assert np.array_equal(w, o, equal_nan=True), "the second sweep differs from `/`"
    assert np.array_equal(g, f, equal_nan=True), "generic kernel differs from the CPU build of the core"
    assert np.any(a > 0.0)


def test_the_three_builds_are_three_kernels(kernels):
    """the switches reach the run-time compiler: three different code objects"""
    sc, on, off, slow = kernels("cornell")
    keys = {c.specialise()["key"] for c in (on, off, slow)}
    assert len(keys) == 3
