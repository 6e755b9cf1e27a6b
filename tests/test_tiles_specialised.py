"""The tile-list form of the scene-specialised kernels, host side (csrc/jit.cpp: jit_source of JIT_TILES; include/rt1w.h:
rt1w_scene_kernel_key_tiles, rt1w_scene_kernel_source_tiles): the generated text, its key, the code objects the build leaves in
<package>/kernels and the refusals.  No GPU."""
import os
import re
import subprocess
import sys

import pytest

import orc

ARMS = (1, 2, 3, 4, 5, 6)
TOPO = re.compile(r"struct TopoJit \{.*?\n\};\n", re.S)


@pytest.mark.parametrize("arm", ARMS)
def test_the_build_leaves_the_tile_form_of_every_eligible_arm(rt, arm):
    """another text, so another key and another sweep_<key>.hsaco, compiled by the build (rt1w_precompile) next to the rectangle form's"""
    sc = rt.Scene.reference(arm, build_seed=1)
    key, rect = sc.kernel_key(tiles=True), sc.kernel_key()
    assert re.fullmatch(r"[0-9a-f]{16}", key) and key != rect
    assert sc.kernel_key(tiles=False) == rect
    kdir = os.path.join(os.path.dirname(rt.LIB_PATH), "kernels")
    for k in (key, rect):
        path = os.path.join(kdir, f"sweep_{k}.hsaco")
        assert os.path.exists(path), f"arm {arm}: {path} missing -- run the build (make -C raytracing-1w_amd/csrc)"
        assert open(path, "rb").read(4) == b"\x7fELF"
    # the default BVH build chooses its split axes: the tree, and the kernel made for it, do not depend on the build seed
    assert rt.Scene.reference(arm, build_seed=2).kernel_key(tiles=True) == key


@pytest.mark.parametrize("arm", ARMS)
def test_the_tile_source_is_the_rectangle_source_around_a_tile_list(rt, arm):
    sc = rt.Scene.reference(arm, build_seed=1)
    src, tile = sc.kernel_source(), sc.kernel_source(tiles=True)
    first_include = tile.index("#include")
    assert 0 <= tile.find("#define RT_TILE_LIST 1\n") < first_include and 0 <= tile.find("#define RT_NO_PROBE 1\n") < first_include
    assert "RT_TILE_LIST" not in src and "RtTileList" not in src
    # the same tables ...
    assert len(TOPO.findall(src)) == len(TOPO.findall(tile)) == 1 and TOPO.findall(src) == TOPO.findall(tile)
    # ... the same configuration and the same wave / exchange-parts choice ...
    cfg = re.compile(r"typedef RtCfg<[^\n]*> CfgJit;\n")
    assert cfg.findall(src) == cfg.findall(tile) and len(cfg.findall(src)) == 1
    assert ("#define RT_SORT_WAVES_OVERRIDE 4" in src) == ("#define RT_SORT_WAVES_OVERRIDE 4" in tile)
    assert ("#define RT_XCH_PARTS 2" in src) == ("#define RT_XCH_PARTS 2" in tile)
    # ... and a kernel of the same name and launch bounds that hands the list on
    assert re.search(r"void rt_jit_sorted\([^)]*unsigned long long\* __restrict__ counters, RtTileList tl\) \{\n"
                     r"    rt_render_sorted_body<CfgJit>\(sc, f, partial, counters, tl\);\n\}", tile)
    assert tile.count("__launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES(CfgJit))") == src.count("__launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES(CfgJit))") == 1
    # everything but the two switches, the kernel's signature and what follows it is the rectangle text
    head = tile.replace("#define RT_TILE_LIST 1\n#define RT_NO_PROBE 1\n", "", 1)
    cut = src.index("extern \"C\" __global__")
    assert head[:cut] == src[:cut]


def test_the_two_existing_forms_are_untouched_by_the_keyword(rt):
    sc = rt.Scene.reference(5, build_seed=1)
    assert sc.kernel_source(tiles=False) == sc.kernel_source()
    assert sc.kernel_source(f32=True, tiles=False) == sc.kernel_source(f32=True)
    assert "RT_TILE_LIST" not in sc.kernel_source(f32=True)
    n = rt._lib.rt1w_scene_kernel_source(sc._h, 0, None, 0)
    assert n == len(sc.kernel_source().encode()) and rt._lib.rt1w_scene_kernel_source_tiles(sc._h, None, 0) == len(sc.kernel_source(tiles=True).encode())
    with pytest.raises(ValueError):
        sc.kernel_source(f32=True, tiles=True)


def test_refusals_are_those_of_the_rectangle_entries(rt):
    for arm in (0, 7):   # more than 256 nodes
        sc = rt.Scene.reference(arm, build_seed=1)
        for ask in (lambda: sc.kernel_key(tiles=True), lambda: sc.kernel_source(tiles=True)):
            with pytest.raises(rt.Rt1wError) as e:
                ask()
            assert e.value.code == rt.ERR_UNSUPPORTED
    sc = rt.Scene()
    sc.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    for ask in (lambda: sc.kernel_key(tiles=True), lambda: sc.kernel_source(tiles=True)):
        with pytest.raises(rt.Rt1wError) as e:
            ask()
        assert e.value.code == rt.ERR_STATE
    import ctypes as C
    assert rt._lib.rt1w_scene_kernel_key_tiles(None, (C.c_char * 24)()) == rt.ERR_INVALID
    assert rt._lib.rt1w_scene_kernel_source_tiles(None, None, 0) == rt.ERR_INVALID
    five = rt.Scene.reference(5, build_seed=1)
    assert rt._lib.rt1w_scene_kernel_source_tiles(five._h, C.create_string_buffer(8), 8) == rt.ERR_INVALID   # buffer too small


def test_the_host_entries_need_neither_compiler_nor_cache(rt, tmp_path):
    """a host without libhiprtc and with an empty user cache still names the kernels and finds the build's code objects"""
    code = ("import importlib, sys; sys.path.insert(0, %r); rt = importlib.import_module('raytracing-1w_amd')\n"
            "for arm in (2, 5, 6):\n"
            "    sc = rt.Scene.reference(arm, build_seed=1)\n"
            "    print(arm, sc.kernel_key(), sc.kernel_key(tiles=True), len(sc.kernel_source(tiles=True)))\n" % orc.ROOT)
    env = dict(os.environ, RT1W_NO_HIPRTC="1", RT1W_KERNEL_CACHE=str(tmp_path))
    out = subprocess.check_output([sys.executable, "-c", code], env=env).decode().split("\n")
    for line, arm in zip(out, (2, 5, 6)):
        sc = rt.Scene.reference(arm, build_seed=1)
        assert line.split() == [str(arm), sc.kernel_key(), sc.kernel_key(tiles=True), str(len(sc.kernel_source(tiles=True)))]
    assert os.listdir(tmp_path) == []


def test_refusals_that_need_no_context(rt):
    """what the parameters alone decide is decided before the context is looked at: RT1W_TILES_SPECIALISED passes the flag checks of the
    tile entries and of the adaptive entries on its own or with RT1W_OUT_SUM, and is refused with today's texts in any other company"""
    import ctypes as C
    import numpy as np
    p = rt.RenderParams()
    for k, v in dict(width=40, height=24, tile_w=40, tile_h=24, spp=3, max_depth=8).items():
        setattr(p, k, v)
    rec, n = rt._tile_list([(0, 0, 0)])
    ptr = np.zeros(16 * 16 * 8).ctypes.data_as(C.c_void_p)
    a = rt.adaptive_params(tile=16, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16)

    def tiles(flags):
        p.flags = flags
        return rt._lib.rt1w_render_tiles_device(None, C.byref(p), 16, rec, n, ptr, None), rt.last_error()

    def filtered(flags):
        p.flags = flags
        return rt._lib.rt1w_render_adaptive_filtered(None, C.byref(p), C.byref(a), None, 0.0, ptr, None, None, None), rt.last_error()

    # a null context is what is left to refuse once the flags have passed
    assert filtered(rt.TILES_SPECIALISED) == filtered(0) == filtered(rt.GENERIC) == (rt.ERR_INVALID, "null argument")
    today = "rt1w_render_adaptive_filtered: p->flags must be 0 or RT1W_GENERIC (the rounds go through rt1w_render_tiles, which runs the generic kernels)"
    for bad in (rt.TILES_SPECIALISED | rt.UNSORTED, rt.TILES_SPECIALISED | rt.GENERIC, rt.UNSORTED):
        assert filtered(bad) == (rt.ERR_INVALID, today)
    assert tiles(rt.TILES_SPECIALISED) == (rt.ERR_INVALID, "null argument")
    p.flags = rt.TILES_SPECIALISED
    assert rt._lib.rt1w_render_aov_tiles(None, C.byref(p), 16, rec, n, ptr, None) == rt.ERR_INVALID
    assert rt.last_error() == "rt1w_render_aov_tiles: flags 0 or RT1W_FORCE_VARIANT only"
    assert rt.TILES_SPECIALISED == 0x40000 and rt.SPECIALISE_TILES == 2
    hdr = open(os.path.join(orc.ROOT, "include", "rt1w.h")).read()
    assert "#define RT1W_TILES_SPECIALISED 0x40000u" in hdr and "#define RT1W_SPECIALISE_TILES 2u" in hdr
