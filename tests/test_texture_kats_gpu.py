"""The points of tests/test_texture_kats.py through rt1w_debug_texture ON THE DEVICE: every output equals the CPU twin
(rt.texture_host) bit for bit, NaN payloads aside, and meets the reference (tests/tex_reference.py) within the CPU tier's bounds on
its own account; image colours bit for bit.  Lists of 1, 255, 256 and 257 points reach a lone lane, a partial workgroup, a full one and
the first lane of a second; the full sets run many workgroups.

With TEXTURE_KATS_RECORD naming a file, the device's measured maxima are written there (the `device` row of
tests/golden/texture_kats.json: recorded, not asserted)."""
import json
import os

import numpy as np
import pytest

import texture_kats as tk

pytestmark = pytest.mark.gpu
MAXIMA = {}


@pytest.fixture(scope="module")
def rig(rt, gpu_ctx_factory):
    sc, ids = tk.build_scene(rt)
    return sc, ids, gpu_ctx_factory(sc)


def same_bits(dev, twin):
    """bit for bit, a NaN equalling a NaN whatever its payload"""
    nan = np.isnan(twin)
    return np.array_equal(np.isnan(dev), nan) and np.array_equal(dev[~nan].view(np.uint64), twin[~nan].view(np.uint64))


def record(**kv):
    MAXIMA.update(kv)
    path = os.environ.get("TEXTURE_KATS_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(MAXIMA, f, indent=1)


@pytest.mark.parametrize("count", [1, 255, 256, 257, None], ids=["1", "255", "256", "257", "all"])
@pytest.mark.parametrize("name", ["random", "revealing"])
def test_noise_and_turb_on_the_device(rt, rig, name, count):
    sc, ids, ctx = rig
    k = ["random", "revealing"].index(name)
    q = tk.uvp(tk.all_noise_points()[:count])
    dev = ctx.debug_texture(1, k, q)
    assert same_bits(dev, rt.texture_host(sc, 1, k, q))
    dn, dt = tk.check_noise(dev, tk.tables()[name], name)
    if count is None:
        record(**{f"noise_{name}_e": round(dn, 3), f"turb_{name}_e": round(dt, 3)})


@pytest.mark.parametrize("count", [1, 255, 256, 257, None], ids=["1", "255", "256", "257", "all"])
def test_noise_texture_value_on_the_device(rt, rig, count):
    sc, ids, ctx = rig
    for k, name in enumerate(("random", "revealing")):
        q = tk.uvp(tk.value_points(), u=0.3, v=0.8)[:count]
        dev = ctx.debug_texture(0, ids[f"noise_{name}"], q)
        assert same_bits(dev, rt.texture_host(sc, 0, ids[f"noise_{name}"], q))
        if count is None:
            record(**{f"value_{name}_e": round(tk.check_value(dev, tk.tables()[name], tk.SCALES[k], name), 3)})
    if count is None:   # the texture of rt1w_texture_noise, its tables read back
        table = tk.perlin_record(sc, 2)
        dev = ctx.debug_texture(1, 2, tk.uvp(tk.all_noise_points()))
        assert same_bits(dev, rt.texture_host(sc, 1, 2, tk.uvp(tk.all_noise_points())))
        tk.check_noise(dev, table, "own")
        tk.check_value(ctx.debug_texture(0, ids["noise_own"], q), table, tk.SCALES[2], "own")


@pytest.mark.parametrize("k", range(len(tk.IMAGE_SIZES)), ids=[f"{w}x{h}" for w, h in tk.IMAGE_SIZES])
def test_image_texture_on_the_device(rt, rig, k):
    sc, ids, ctx = rig
    w, h = tk.IMAGE_SIZES[k]
    q = tk.image_queries(w, h)
    dev = ctx.debug_texture(0, ids["images"][k], q)
    tk.check_image(dev, w, h, q)
    assert same_bits(dev, rt.texture_host(sc, 0, ids["images"][k], q))
    for count in (1, 255, 256, 257):
        assert np.array_equal(ctx.debug_texture(0, ids["images"][k], q[:count]), dev[:count])


def test_checkers_and_sphere_uv_on_the_device(rt, rig):
    sc, ids, ctx = rig
    g = np.random.default_rng(80)
    n = 20000
    q = tk.uvp(g.uniform(-20.0, 20.0, size=(n, 3)))
    q[:, 0], q[:, 1] = g.uniform(-0.2, 1.2, size=n), g.uniform(-0.2, 1.2, size=n)
    for tex in ("checker_solids", "checker_image_noise", "checker_checkers"):
        for count in (257, None):
            assert same_bits(ctx.debug_texture(0, ids[tex], q[:count]), rt.texture_host(sc, 0, ids[tex], q[:count])), tex
    pts, _ = tk.uv_points()
    for count in (1, 255, 256, 257, None):
        dev = ctx.debug_texture(2, 0xFFFFFFFF, tk.uvp(pts[:count]))   # mode 2 ignores `tex`
        assert same_bits(dev, rt.texture_host(sc, 2, 0, tk.uvp(pts[:count])))
    eu, ev = tk.check_sphere_uv(dev)
    record(sphere_uv_u_abs=eu, sphere_uv_v_abs=ev)


def test_the_probe_refuses_a_table_it_does_not_have(rt, rig):
    """mode 1 with `tex` at or beyond the scene's Perlin tables is refused before anything is launched, as the twin refuses it"""
    sc, ids, ctx = rig
    q = tk.uvp(np.zeros((2, 3)))
    n_perlin = sc.info()["n_perlin"]
    for mode, tex, text in ((1, n_perlin, "bad Perlin table index"), (1, ids["noise_own"], "bad Perlin table index"),
                            (1, 0xFFFFFFFF, "bad Perlin table index"), (0, sc.info()["n_textures"], "bad texture id"), (3, 0, "unknown mode")):
        with pytest.raises(rt.Rt1wError) as why:
            ctx.debug_texture(mode, tex, q)
        assert why.value.code == rt.ERR_INVALID and text in str(why.value)
        with pytest.raises(rt.Rt1wError) as twin:
            rt.texture_host(sc, mode, tex, q)
        assert str(twin.value) == str(why.value)
