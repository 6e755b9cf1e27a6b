"""Builds shared by the tests of the scene-specialised kernels.  Test infrastructure only.

Host side: the flat core (oracle/oracle_flat.cpp) compiled around generated Topo structs -- one header, one command line -- and the small
shim libraries over rt_core.h / rt1w_num.h.  GPU side: a context whose run-time-compiled kernel is built under other -D switches, and the
three test bodies the parts' GPU modules have in common.

Every library built here is loaded into the one pytest process.  A `static constexpr` array member such as Topo::kind is emitted as a GNU
unique symbol: the process holds one object per NAME, whichever library defined it first, RTLD_LOCAL or not.  So the type names of a
library carry its tag (Topo_<tag>_<k>, Cfg_<tag>_<k>), and a tag is given out once per process."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import orc

# what every host build of the core shares; the optimisation level, -pthread, -include and -D switches are the caller's
FLAGS = ["-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
         "-I" + os.path.join(orc.ROOT, "include"), "-I" + os.path.join(orc.ROOT, "raytracing-1w_amd", "csrc")]
_tags = set()


def claim_tag(tag):
    """a tag names the types of one library; asking for it twice would put two libraries' tables under one name"""
    if not re.fullmatch(r"\w+", tag) or tag in _tags:
        raise ValueError(f"tag {tag!r} is taken or is not an identifier")
    _tags.add(tag)


def small_frame(name):
    """(width, height, spp) of a host frame: the Cornell rooms need more pixels to show their boxes"""
    return (48, 48, 6) if "cornel" in name else (28, 20, 4)


def topo_text(sc, name, f32=False):
    """`struct TopoJit { ... };` of the generated unit (Scene.kernel_source, of either precision), renamed"""
    src = sc.kernel_source(f32=f32)
    body = src[src.index("struct TopoJit {"):]
    body = body[:body.index("};\n};\n") + len("};\n};\n")]
    assert "reuse[" in body
    return body.replace("struct TopoJit", "struct " + name)


def unit_text(sc, topo, tag, k):
    """the Topo text as Topo_<tag>_<k>, and the configuration the library derives from the scene as Cfg_<tag>_<k>"""
    b = lambda key: "true" if sc.info()[key] else "false"
    text, n = re.subn(r"^struct \w+", f"struct Topo_{tag}_{k}", topo, count=1)
    assert n == 1
    return text + (f"typedef RtCfg<{b('has_media')}, {b('has_textures')}, {b('has_moving')}, true, {max(2, sc.info()['scope_depth'])}, "
                   f"Topo_{tag}_{k}> Cfg_{tag}_{k};\n")


def static_header(work, tag, units, per_unit=None, prologue=""):
    """writes <work>/topo_gen.h for `units`, a list of (name, scene, Topo text): unit k is variant 100 + k of the flat core.
    per_unit(k, name, scene) is text put after unit k (in it, Topo_<tag>_<k> is the unit's type); `prologue` comes first"""
    claim_tag(tag)
    os.makedirs(work, exist_ok=True)
    hdr = [unit_text(sc, topo, tag, k) + (per_unit(k, name, sc) if per_unit else "") for k, (name, sc, topo) in enumerate(units)]
    sw = [f"case {100 + k}: run_path<Cfg_{tag}_{k}>(sc, f, px, py, s, stk, sum, segs, path); break;" for k in range(len(units))]
    with open(os.path.join(work, "topo_gen.h"), "w") as f:
        f.write(prologue + "".join(hdr) + f"#define ORC_N_STATIC {len(units)}\n#define ORC_STATIC_CASES " + " ".join(sw) + "\n")


def command(out, source, *flags, level="-O1", pthread=True, work=None, csrc=True):
    """the compiler's command line for `source`; `work` is one more include directory"""
    return ["g++", level, *(["-pthread"] if pthread else []), *(FLAGS if csrc else FLAGS[:-1]), *(["-I" + str(work)] if work else []),
            *flags, str(source), "-o", str(out)]


def static_command(work, tag, units, flags=(), f32=False, **header):
    """writes the header (static_header) and returns (library path, command line) of the flat core, or its f32 twin, built around it"""
    static_header(work, tag, units, **header)
    so = os.path.join(work, f"lib{tag}.so")
    return so, command(so, os.path.join(orc.ROOT, "oracle", "oracle_flat_f32.cpp" if f32 else "oracle_flat.cpp"), *flags,
                       "-DRT_RNG_CHECK", '-DORC_STATIC_TOPO_H="topo_gen.h"', "-shared", work=work)


def build_all(commands):
    """runs the command lines, at most 16 at a time; the first that fails raises"""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(subprocess.check_call, commands))


def static_lib(work, tag, units, flags=(), **header):
    """one flat core built around `units` and loaded"""
    so, cmd = static_command(work, tag, units, flags, **header)
    subprocess.check_call(cmd)
    return orc.declare_flat(C.CDLL(so))


def shim_lib(work, name, source, csrc=False):
    """lib<name>.so from the text `source` over the project's headers (csrc: rt_core.h's directory too), loaded"""
    cpp, so = os.path.join(work, "shim.cpp"), os.path.join(work, f"lib{name}.so")
    with open(cpp, "w") as f:
        f.write(source)
    subprocess.check_call(command(so, cpp, "-shared", pthread=False, csrc=csrc))
    return C.CDLL(so)


# ------------------------------------------------------------------------------------------------------------------ on the GPU

def specialised(ctx_factory, sc, cache, opts):
    """a context whose scene-specialised kernel is built with `opts` (RT1W_JIT_EXTRA_OPTS is part of a kernel's key)"""
    keys = ("RT1W_KERNEL_CACHE", "RT1W_JIT_EXTRA_OPTS")
    old = {k: os.environ.get(k) for k in keys}
    os.environ["RT1W_KERNEL_CACHE"] = cache
    os.environ.pop("RT1W_JIT_EXTRA_OPTS", None)
    if opts:
        os.environ["RT1W_JIT_EXTRA_OPTS"] = opts
    try:
        ctx = ctx_factory(sc)
        assert ctx.specialise()["active"]
        return ctx
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def agree_specialised_generic_core(ctx, sc, W, H, spp):
    """the precompiled specialised kernel, the generic kernel and the CPU build of the core: the same frame and segment count"""
    assert ctx.specialised(), "no precompiled kernel found next to the library"
    a, sa = ctx.render(W, H, spp)
    b, sb = ctx.render(W, H, spp, generic=True)
    f, sf = orc.flat_render(sc, W, H, spp, chunk=sa["chunk"])
    assert (sa["sorted"] & 4) and not (sb["sorted"] & 4)
    assert sa["segments"] == sb["segments"] == sf["segments"]
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, f, equal_nan=True)


def agree_compiled_at_run_time(ctx, sc):
    """the same for a scene without a precompiled kernel (the caller points RT1W_KERNEL_CACHE at an empty directory): generic first,
    then the kernel the run-time compiler builds.  Returns the frame"""
    b, sb = ctx.render(32, 32, 4)
    assert not (sb["sorted"] & 4)
    info = ctx.specialise()
    assert info["active"] and not info["from_cache"]
    a, sa = ctx.render(32, 32, 4)
    f, sf = orc.flat_render(sc, 32, 32, 4, chunk=sa["chunk"])
    assert (sa["sorted"] & 4) and sa["segments"] == sb["segments"] == sf["segments"]
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, f, equal_nan=True)
    return a


def agree_f32_specialised_generic(ctx):
    """single precision: the specialised and the generic f32 kernels agree"""
    a, sa = ctx.render(64, 64, 8, f32=True)
    b, sb = ctx.render(64, 64, 8, f32=True, generic=True)
    assert (sa["sorted"] & 4) and not (sb["sorted"] & 4)
    assert sa["segments"] == sb["segments"] and np.array_equal(a, b, equal_nan=True)
