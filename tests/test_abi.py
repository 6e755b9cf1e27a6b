"""The C-ABI library: loads, exports every symbol include/rt1w.h declares, and the host-side
error behaviour (the reference's panics become error codes).  No compute here (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc

ROOT = orc.ROOT


def declared_functions():
    src = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rt1w_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(rt):
    lib = C.CDLL(rt.LIB_PATH)
    names = declared_functions()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), f"{n} is declared in include/rt1w.h but not exported"


def test_library_exports_nothing_else(rt):
    """librt1w.so is built with -fvisibility=hidden and a linker version script (csrc/librt1w.map): its dynamic symbol table holds the
    entries include/rt1w.h declares plus the four hooks of csrc/rt1w_internal.h (for the diagnostics library librt1w_lab.so) and
    nothing else -- no C++ internals, no kernel host stubs, no unprefixed helpers, no laboratory (`rt1w_lab_*` and the wavefront form's kernels live in librt1w_lab.so)."""
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", rt.LIB_PATH]).decode()
    exported = sorted({line.split()[-1] for line in out.splitlines() if line.strip()})
    internal = ["rt1w_internal_device", "rt1w_internal_register_f32_kernels", "rt1w_internal_register_wavefront", "rt1w_internal_set_error", "rt1w_internal_view"]
    assert exported == sorted(set(declared_functions()) | set(internal)), sorted(set(exported) ^ (set(declared_functions()) | set(internal)))
    lab = os.path.join(os.path.dirname(rt.LIB_PATH), "librt1w_lab.so")
    lab_syms = subprocess.check_output(["nm", "-D", "--defined-only", lab]).decode()
    assert "rt1w_lab_trace" in lab_syms and "rt1w_lab_" not in out


def test_lab_prototype_table_matches_the_header(rt):
    """The binding declares the rt1w_lab_* functions it calls once, in its _LAB_SIGS table: csrc/walk_lab.h declares every one of them
    with as many parameters as the table gives it argtypes, and the binding names no rt1w_lab_* function the table lacks.  The table
    is read, not the live function objects: other tests re-type those."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raytracing-1w_amd", "csrc", "walk_lab.h")).read(), flags=re.S)
    assert len(rt._LAB_SIGS) >= 24
    for name, argtypes in rt._LAB_SIGS.items():
        assert "int " + name + "(" in hdr, f"{name} is not declared in csrc/walk_lab.h"
        decl = hdr[hdr.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(argtypes), name
    src = open(os.path.join(ROOT, "raytracing-1w_amd", "__init__.py")).read()
    called = set(re.findall(r"\"(rt1w_lab_[a-z0-9_]+)\"", src)) | set(re.findall(r"\.(rt1w_lab_[a-z0-9_]+)\(", src))
    assert called == set(rt._LAB_SIGS), called ^ set(rt._LAB_SIGS)


def test_integration_rust_block_declares_every_entry_of_the_header():
    """INTEGRATION.md section 2 claims to mirror include/rt1w.h one to one: the `extern "C"` block must name exactly the
    functions the header declares, and its #[repr(C)] structs must have the header's fields in the header's order."""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("## 2."):md.index("## 3.")]
    rust = sorted(set(re.findall(r"pub fn (rt1w_[a-z0-9_]+)\(", block)))
    assert rust == declared_functions(), (set(declared_functions()) - set(rust), set(rust) - set(declared_functions()))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt1w.h")).read(), flags=re.S)
    for name in ("rt1w_render_params", "rt1w_stats", "rt1w_scene_info", "rt1w_specialise_info"):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                c_fields += [re.sub(r"\[.*?\]", "", f).strip().split()[-1] for f in decl.split(",")]
        rs = re.search(r"pub struct " + name + r" \{(.*?)\n\}", block, flags=re.S).group(1)
        rs = re.sub(r"//[^\n]*", "", rs)
        r_fields = re.findall(r"pub ([a-z0-9_]+):", rs)
        assert r_fields == c_fields, (name, r_fields, c_fields)


def test_every_declared_entry_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "rt1w.h")).read()
    for fn in ("rt1w_hittable_sphere", "rt1w_hittable_bvh", "rt1w_render", "rt1w_scene_set_camera", "rt1w_quantize"):
        line = [l for l in src.splitlines() if fn + "(" in l][0]
        block = src[src.index(line) - 600: src.index(line) + 400]
        assert re.search(r"\.rs:\d+", block), f"no reference citation near {fn}"


def test_struct_layouts_match_between_python_and_c_with_stats_passes(rt):
    """rt1w_stats is 64 bytes: the 56 of its first layout, then `passes` and a reserved word."""
    assert C.sizeof(rt.RenderParams) == 64 and C.sizeof(rt.Stats) == 64 and C.sizeof(rt.SceneInfo) == 56
    assert rt.Stats.sorted.offset == 52 and rt.Stats.passes.offset == 56 and rt.Stats.reserved.offset == 60
    assert C.sizeof(rt.SpecialiseInfo) == 48
    for i, t in enumerate((rt.RenderParams, rt.Stats, rt.SceneInfo, rt.SpecialiseInfo)):
        assert rt._lib.rt1w_abi_sizeof(i) == C.sizeof(t)
    assert orc.B.orcflat_sizeof(0) == 96 and orc.B.orcflat_sizeof(1) == 48 and orc.B.orcflat_sizeof(2) == 48
    assert orc.B.orcflat_sizeof(3) == 9216 and orc.B.orcflat_sizeof(5) == C.sizeof(orc.Frame)


def test_error_behaviour(rt):
    s = rt.Scene(build_seed=1)
    with pytest.raises(rt.Rt1wError) as e:            # BVHNode::new panics on empty (bvh.rs:61)
        s.bvh_node([])
    assert e.value.code == rt.ERR_INVALID and "empty" in str(e.value)
    with pytest.raises(rt.Rt1wError):
        s.lambertian(99)                             # bad texture id
    with pytest.raises(rt.Rt1wError):
        s.sphere((0, 0, 0), 1.0, 5)                  # bad material id
    m = s.lambertian(s.solid_color((0.5, 0.5, 0.5)))
    a = s.sphere((0, 0, 0), 1.0, m)
    t = s.translate(a, (1, 0, 0))
    with pytest.raises(rt.Rt1wError):                # Box ownership: a child is owned once
        s.flip_face(a)
    with pytest.raises(rt.Rt1wError) as e:
        s.commit()                                   # no world / camera yet
    assert e.value.code == rt.ERR_STATE
    w = s.bvh_node([t])
    s.set_world(w)
    s.set_lights([])
    s.set_background((0, 0, 0))
    with pytest.raises(rt.Rt1wError):                # gen_range(time0..time1) needs a non-empty range (camera.rs:71)
        s.set_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), 40, 1.0, 0.0, 10.0, 1.0, 1.0)
    s.set_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), 40, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.commit()
    with pytest.raises(rt.Rt1wError) as e:           # immutable after commit
        s.solid_color((1, 1, 1))
    assert e.value.code == rt.ERR_STATE
    info = s.info()
    assert info["n_nodes"] == 3 and info["scope_depth"] == 1 and info["n_lights"] == 0


def test_unsupported_graph_shapes_are_reported(rt):
    s = rt.Scene(build_seed=1)
    m = s.lambertian(s.solid_color((0.5, 0.5, 0.5)))
    h = s.sphere((0, 0, 0), 1.0, m)
    for _ in range(5):                               # innermost FlipFace folds into the leaf; 4 more wrappers > RT_MAX_SCOPE_DEPTH
        h = s.flip_face(h)
    s.set_world(s.bvh_node([h]))
    s.set_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), 40, 1.0, 0.0, 10.0, 0.0, 1.0)
    with pytest.raises(rt.Rt1wError) as e:
        s.commit()
    assert e.value.code == rt.ERR_UNSUPPORTED


def test_no_cpu_render_path(rt):
    """Without a GPU the product refuses to render instead of falling back."""
    if rt.device_count() > 0:
        pytest.skip("a GPU is present")
    sc = rt.Scene.reference(5)
    with pytest.raises(rt.Rt1wError) as e:
        rt.Context(sc, 0)
    assert e.value.code == rt.ERR_DEVICE and "no CPU render path" in str(e.value)


def test_flattened_cornell_structure(rt):
    """Sizes derived from the source: 13 primitives, 14 BVH nodes, 3 wrappers; 2 lights."""
    sc = rt.Scene.reference(5, build_seed=1)
    info = sc.info()
    nodes = sc.flat(0).view(np.uint32).reshape(-1, 24)
    kinds = nodes[:, 0] & 0xFF
    flipped = (nodes[:, 0] & 0x100) != 0
    assert info["n_nodes"] == 29 and info["n_lights"] == 2 and info["has_media"] == 0
    assert (kinds <= 1).sum() == 14                  # BVH nodes: 7 top + 7 in the box
    assert ((kinds >= 2) & (kinds <= 6)).sum() == 13 # 5 walls + light + 6 box sides + sphere
    assert sorted(kinds[kinds >= 7]) == [7, 8]       # Translate, RotateY; FlipFace(light rect) is folded into the leaf
    assert flipped.sum() == 1 and kinds[flipped][0] == 5
    assert sc.defaults == (600, 600, 100)            # main.rs:868-870
    # camera block: origin = look_from
    cam = sc.flat(6).view(np.float64)
    assert tuple(cam[0:3]) == (278.0, 278.0, -800.0)


def test_reference_defaults_table(rt):
    # main.rs:798-800,817,856,870,898,918-919,939
    assert rt.Scene.reference(0).defaults == (400, 225, 500)
    assert rt.Scene.reference(1).defaults == (400, 225, 100)
    assert rt.Scene.reference(4).defaults == (400, 225, 400)
    assert rt.Scene.reference(6).defaults == (600, 600, 200)
    assert rt.Scene.reference(7).defaults == (800, 800, 10000)
    assert rt.Scene.reference(5, aspect_ratio=16.0 / 9.0).defaults[1] == 337


def test_format_ppm_matches_reference_layout(rt):
    img = np.zeros((2, 3, 3))
    img[1, 0] = (1.0, 0.25, 0.0)                     # j = 1 is the TOP row (main.rs:957-960)
    txt = rt.format_ppm(img)
    lines = txt.split("\n")
    assert lines[:3] == ["P3", "3 2", "255"]
    assert lines[3] == "255 128 0" and lines[4] == "0 0 0" and len(lines) == 3 + 6 + 1 and lines[-1] == ""


def test_specialised_kernels_of_the_reference_arms_are_built(rt):
    """Host side of the scene-specialised kernels (jit.cpp), no GPU: the cache key is a function of the scene's
    topology and of the library's own source; the build has compiled the reference's eligible arms (build_seed 1)
    into <package>/kernels; big scenes are refused."""
    import os
    kdir = os.path.join(os.path.dirname(rt.LIB_PATH), "kernels")
    keys = {}
    for arm in (1, 2, 3, 4, 5, 6):
        key = rt.Scene.reference(arm, build_seed=1).kernel_key()
        assert len(key) == 16 and int(key, 16) >= 0
        path = os.path.join(kdir, f"sweep_{key}.hsaco")
        assert os.path.exists(path), f"arm {arm}: {path} missing -- run the build (make -C raytracing-1w_amd/csrc)"
        assert open(path, "rb").read(4) == b"\x7fELF"
        keys[arm] = key
    assert keys[5] != keys[6] and keys[5] != keys[4]
    assert rt.Scene.reference(5, build_seed=1).kernel_key() == keys[5]          # deterministic
    # the default build chooses its split axes (RT1W_BVH_BEST_AXIS): the tree -- and the kernel made for it -- no longer depends on what
    # the build seed draws; with the axes drawn (RT1W_BVH_REFERENCE) another seed is another tree, another kernel
    assert rt.Scene.reference(5, build_seed=2).kernel_key() == keys[5]
    assert rt.Scene.reference(5, build_seed=2).set_bvh_build("reference").kernel_key() != rt.Scene.reference(5, build_seed=1).set_bvh_build("reference").kernel_key()
    for arm in (0, 7):
        with pytest.raises(rt.Rt1wError) as e:
            rt.Scene.reference(arm, build_seed=1).kernel_key()
        assert e.value.code == rt.ERR_UNSUPPORTED
