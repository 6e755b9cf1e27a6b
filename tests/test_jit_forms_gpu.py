"""The three forms of the scene-specialised kernel on one context (csrc/jit.h: JitForm; csrc/context.h: rt1w_context::jit): every form's
render runs its own slot's kernel, and the lazy cache lookups of the f32 and the tile-list form (context.hip: specialised_lookup) do not
depend on the order in which renders ask for them.  Arms 5 and 6 at build_seed 1: the build has precompiled all three forms of both, so
nothing is compiled and no user cache is written."""
import os

import numpy as np
import pytest

from test_render_tiles_gpu import _same

pytestmark = pytest.mark.gpu

W = H = 32
SPP, DEPTH, T, CHUNK = 4, 8, 16, 2
LIST = [(0, 0, 0), (16, 0, 4), (0, 16, 8), (16, 16, 12)]   # the frame's four tiles, a sample offset each


def _f64(ctx):
    """a) the rectangle render and, from the same kernel, the raw sums of every tile's rectangle at its sample offset"""
    img, st = ctx.render(W, H, SPP, max_depth=DEPTH)
    assert st["sorted"] & 4 and not (st["sorted"] & 32), st
    rects = []
    for x0, y0, off in LIST:
        r, sr = ctx.render(W, H, SPP, max_depth=DEPTH, tile=(x0, y0, T, T), sample_offset=off, out_sum=True, chunk=CHUNK)
        assert sr["sorted"] & 4 and not (sr["sorted"] & 32), sr
        rects.append(r)
    return img, np.stack(rects)


def _f32(ctx):
    """b) the f32 form, against the generic f32 kernel of the same context"""
    img, st = ctx.render(W, H, SPP, max_depth=DEPTH, f32=True)
    assert st["sorted"] & 36 == 36, st
    gen, sg = ctx.render(W, H, SPP, max_depth=DEPTH, f32=True, generic=True)
    assert sg["sorted"] & 32 and not (sg["sorted"] & 4), sg
    assert _same(img, gen)
    return img


def _tiles(ctx, specialised):
    """c) the tile-list form, d) the generic tile form"""
    tiles, st = ctx.render_tiles(W, H, SPP, T, LIST, max_depth=DEPTH, out_sum=True, chunk=CHUNK, specialised=specialised)
    assert (st["sorted"] & 5 == 5) if specialised else not (st["sorted"] & 4), st
    return tiles


@pytest.mark.parametrize("arm", [5, 6])
def test_gpu_three_forms_on_one_context_in_any_order(rt, gpu_ctx_factory, tmp_path, monkeypatch, arm):
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path))   # empty, and still empty afterwards: everything comes from the install cache
    monkeypatch.delenv("RT1W_JIT_EXTRA_OPTS", raising=False)
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=W / H)

    ctx = gpu_ctx_factory(sc)
    a, rects = _f64(ctx)
    b = _f32(ctx)
    c = _tiles(ctx, True)
    d = _tiles(ctx, False)
    for k in range(len(LIST)):
        assert _same(c[k], rects[k]), k
    assert _same(c, d)
    assert not _same(a, b)   # two precisions, two pictures: the slots were not mixed up

    other = gpu_ctx_factory(sc)
    c2 = _tiles(other, True)
    b2 = _f32(other)
    d2 = _tiles(other, False)
    a2, rects2 = _f64(other)
    assert _same(c2, c) and _same(b2, b) and _same(d2, d) and _same(a2, a) and _same(rects2, rects)
    assert os.listdir(tmp_path) == []
