"""Ray and radiance queries against the literal oracle on the caller's own rays -- GPU tier.

Context.hit and Context.ray_color (the host entries rt1w_hit and rt1w_ray_color) on the sets of tests/query_rays.py: against the
literal oracle directly, at the bounds of tests/test_query_oracle.py, and against the CPU twins bit for bit.  One context per scene.
The oracle library is the one build() makes from oracle/."""
import time

import numpy as np
import pytest

import hit_reference as HR
import query_rays as Q

SORTED, JIT, PW, SS, HC = 1, 4, 128, 512, 1024  # rt1w_stats.sorted (include/rt1w.h)
# what must have run on the reference arms (test_ray_color_gpu.py: FAMILY): (all of these bits, none of these)
FAMILY = {"arm5": (SORTED, JIT | PW | SS), "arm6": (SORTED, JIT | PW | SS), "arm0": (PW | SS, JIT | SORTED), "arm7": (SS | HC, JIT | SORTED | PW)}
pytestmark = pytest.mark.gpu


def _hit(rt, ctx, name, which, rays, exact_t=False):
    prod, orac = Q.scene_pair(name)
    for sample, gs in Q.PAIRS:
        want, wmat, waux = orac.hit(rays, Q.FIRST_STREAM, sample, gs)
        for v in HR.valid_variants(prod.info()):
            kw = dict(first_stream=Q.FIRST_STREAM, sample=sample, global_seed=gs, variant=v)
            got, node, st = ctx.hit(rays, with_stats=True, **kw)
            Q.check_hit(name, which, rays, got, node, want, wmat, waux, ("gpu", sample, gs, "variant", v), exact_t=exact_t)
            twin, twin_node = rt.hit_host(prod, rays, **kw)
            assert HR.same_bits(got, twin) and np.array_equal(node, twin_node), (name, which, sample, gs, v, int((node != twin_node).sum()))
            assert st["paths"] == st["segments"] == len(rays) and st["variant"] == v


@pytest.mark.parametrize("name", Q.scene_names())
def test_gpu_hit_against_the_oracle_and_the_twin(rt, gpu_ctx_factory, name):
    """Context.hit on the four sets, every variant that covers the scene, two (sample, global_seed) pairs, in the default I/O form."""
    ctx = gpu_ctx_factory(Q.scene_pair(name)[0])
    t0 = time.perf_counter()
    for which in Q.HIT_SETS:
        _hit(rt, ctx, name, which, Q.sets(name).rays[which])
    print(name, "hit: %.2f s" % (time.perf_counter() - t0))
    ctx.close()


def test_gpu_hit_on_the_exact_windows(rt, gpu_ctx_factory):
    """roots on the window's ends and one ulp to either side: the oracle's verdicts and the oracle's bits of t"""
    ctx = gpu_ctx_factory(Q.scene_pair("exact")[0])
    _hit(rt, ctx, "exact", "exact_window", Q.exact_window()[0], exact_t=True)
    ctx.close()


@pytest.mark.parametrize("name", Q.scene_names())
def test_gpu_radiance_against_the_oracle_and_the_twin(rt, gpu_ctx_factory, name):
    """Context.ray_color on the generic, continuation and axis-parallel sets at 1 spp, raw sums: samples 0 and 7, start words none and
    drawn, max_depth 1, 2 and 50.  Against the oracle 1e-12 relative with the oracle's segments in total (per ray they are the twin's,
    whose values the kernels equal bit for bit); the kernel family from stats.sorted."""
    prod, orac = Q.scene_pair(name)
    ctx = gpu_ctx_factory(prod)
    s = Q.sets(name)
    t0 = time.perf_counter()
    for which in Q.RADIANCE_SETS:
        rays = s.rays[which]
        for sample in Q.SAMPLES:
            for word in (None, Q.start_words(name, which, len(rays))):
                for depth in Q.DEPTHS:
                    kw = dict(spp=1, sample_offset=sample, first_stream=Q.FIRST_STREAM, global_seed=3, max_depth=depth, out_sum=True)
                    tag = (name, which, sample, "start words" if word is not None else "word 0", depth, "gpu")
                    want, wseg = orac.ray_color(rays, word, Q.FIRST_STREAM, sample, 3, depth)
                    twin, tst = rt.ray_color_host(prod, rays, word, with_stats=True, **kw)
                    got, st = ctx.ray_color(rays, word, with_stats=True, **kw)
                    assert HR.same_bits(got, twin), tag + (int((got != twin).any(axis=1).sum()),)
                    assert st["segments"] == tst["segments"] == int(wseg.sum()) and st["paths"] == len(rays), tag + (st["segments"], int(wseg.sum()))
                    Q.check_radiance(tag, got, tst["ray_segments"], want, wseg)
                    need, never = FAMILY.get(name, (SORTED, JIT | PW | SS))  # the hand-built scenes and graphs are small: the reordering kernel
                    assert st["sorted"] & need == need and not st["sorted"] & never, tag + (st["sorted"],)
    print(name, "radiance: %.2f s" % (time.perf_counter() - t0), "sorted", st["sorted"])
    ctx.close()
