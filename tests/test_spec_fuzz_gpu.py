"""The scene-specialised kernels on 24 graphs of the fuzz corpus (spec_graphs.py: 12 random, 12 lattice, none above 64 nodes, so a
run-time compile takes a few seconds): the kernel compiled for the graph == the generic kernel == the CPU build of the core, bit for bit
with equal segment counts, at 32 x 32 x 8 and at 8 x 4 x 8 with chunk 8 -- 32 work items, less than a wave: lanes are retired from the
start, which the wave-wide rejection rounds and the box-free sweep's votes must survive.  On eight graphs also the f32 kernels and a tile
with a sample offset and raw sums; on the four box-free graphs with the most coincident bounds also the kernel built with
-DRT_BOX_FREE=0 and with -DRT_DIV_SHARED_FORCE_SLOW=1.  One context alive at a time, each closed when its case is done."""
import json
import os

import numpy as np
import pytest

import box_free_scenes as BF
import core_builds as CB
import orc
import spec_graphs as G

pytestmark = pytest.mark.gpu

RECORDED = json.load(open(os.path.join(orc.ROOT, "tests", "golden", "spec_fuzz_census.json")))
# the 24 cover on their own what the corpus is for ("at least four" scaled to two): a condition on the list, checked where it is read
_MISSING = [what for what, ok in G.coverage([RECORDED[n] for n in G.GPU_NAMES], few=2).items() if not ok]
assert not _MISSING, _MISSING
assert len(G.GPU) == 24 and sum(e[0] == "random" for e in G.GPU) == 12 and all(RECORDED[n]["n_nodes"] <= 64 for n in G.GPU_NAMES)
assert set(G.GPU_F32_AND_TILES) <= set(G.GPU_NAMES) and len(G.GPU_F32_AND_TILES) == 8
_FREE = sorted((n for n in G.GPU_NAMES if RECORDED[n]["box_free"]), key=lambda n: -RECORDED[n]["reuse_entries"])
assert tuple(sorted(_FREE[:4])) == tuple(sorted(G.GPU_BOX_FREE_BUILDS))

FRAMES = ((32, 32, 8, 0), (8, 4, 8, 8))   # width, height, spp, chunk


@pytest.mark.parametrize("entry", G.GPU, ids=G.name_of)
def test_specialised_equals_generic_equals_cpu_core(gpu_ctx_factory, tmp_path, monkeypatch, entry):
    name = G.name_of(entry)
    prod, _ = G.build(entry)
    assert G.census(prod) == RECORDED[name]
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path))
    monkeypatch.delenv("RT1W_JIT_EXTRA_OPTS", raising=False)
    ctx = gpu_ctx_factory(prod)
    try:
        info = ctx.specialise()
        assert info["active"] and not info["from_cache"], info
        for W, H, spp, chunk in FRAMES:
            a, sa = ctx.render(W, H, spp, max_depth=50, chunk=chunk)
            g, sg = ctx.render(W, H, spp, max_depth=50, chunk=sa["chunk"], generic=True)
            f, sf = orc.flat_render(prod, W, H, spp, max_depth=50, chunk=sa["chunk"])
            assert (sa["sorted"] & 4) and not (sg["sorted"] & 4), (name, W, H)
            assert sa["segments"] == sg["segments"] == sf["segments"], (name, W, H)
            assert np.array_equal(g, f, equal_nan=True), (name, W, H, "the generic kernel differs from the CPU build of the core")
            assert np.array_equal(a, g, equal_nan=True), (name, W, H, "the specialised kernel differs from the generic kernel")
            assert np.any(a > 0.0), (name, W, H)
        if name in G.GPU_F32_AND_TILES:
            for W, H, spp, chunk in FRAMES:
                a, sa = ctx.render(W, H, spp, max_depth=50, chunk=chunk, f32=True)
                g, sg = ctx.render(W, H, spp, max_depth=50, chunk=sa["chunk"], f32=True, generic=True)
                assert (sa["sorted"] & 4) and (sa["sorted"] & 32) and not (sg["sorted"] & 4), (name, "f32", W, H)
                assert sa["segments"] == sg["segments"] and np.array_equal(a, g, equal_nan=True), (name, "f32", W, H)
            tile = dict(tile=(5, 3, 17, 11), sample_offset=5, out_sum=True, max_depth=50)
            a, sa = ctx.render(32, 32, 8, **tile)
            g, sg = ctx.render(32, 32, 8, chunk=sa["chunk"], generic=True, **tile)
            assert (sa["sorted"] & 4) and not (sg["sorted"] & 4), (name, "tile")
            assert sa["segments"] == sg["segments"] and np.array_equal(a, g, equal_nan=True), (name, "tile")
            assert np.any(a > 0.0), (name, "tile")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", G.GPU_BOX_FREE_BUILDS)
def test_box_free_builds_have_the_shipped_bits(gpu_ctx_factory, tmp_path, name):
    """as test_box_free_gpu.py does for its scenes: every box tested, and the second sweep forced for every wave"""
    prod, _ = G.build(G.GPU[G.GPU_NAMES.index(name)])
    assert BF.declared(prod)[1]
    shipped = {}
    keys = set()
    for opts in (None, "-DRT_BOX_FREE=0", "-DRT_DIV_SHARED_FORCE_SLOW=1"):
        ctx = CB.specialised(gpu_ctx_factory, prod, str(tmp_path), opts)
        try:
            keys.add(ctx.specialise()["key"])
            for W, H, spp, chunk in FRAMES:
                a, sa = ctx.render(W, H, spp, max_depth=50, chunk=chunk)
                assert sa["sorted"] & 4, (name, opts)
                if opts is None:
                    shipped[(W, H)] = (a, sa)
                    continue
                b, sb = shipped[(W, H)]
                assert sa["chunk"] == sb["chunk"] and sa["segments"] == sb["segments"], (name, opts, W, H)
                assert np.array_equal(a, b, equal_nan=True), (name, opts, W, H)
        finally:
            ctx.close()
    assert len(keys) == 3   # three different code objects


def test_one_node_too_many_is_refused_on_the_device(rt, gpu_ctx_factory, tmp_path, monkeypatch):
    """257 nodes: specialise() refuses, and the context renders with the generic kernels what the CPU build of the core renders"""
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path))
    prod, _ = G.build(G.REFUSED)
    ctx = gpu_ctx_factory(prod)
    try:
        with pytest.raises(rt.Rt1wError) as e:
            ctx.specialise()
        assert e.value.code == rt.ERR_UNSUPPORTED
        a, sa = ctx.render(32, 32, 8)
        f, sf = orc.flat_render(prod, 32, 32, 8, chunk=sa["chunk"])
        assert not (sa["sorted"] & 4) and sa["segments"] == sf["segments"] and np.array_equal(a, f, equal_nan=True)
    finally:
        ctx.close()
