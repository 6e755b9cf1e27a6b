"""What the entries of features.hip refuse, with which code and text, and in which order (include/rt1w.h: rt1w_render_aov*, rt1w_denoise*,
rt1w_render_denoised*, rt1w_batch_variance*, rt1w_accum_*, rt1w_adaptive_select, rt1w_render_adaptive).  A characterisation test: the
expected (return code, rt1w_last_error text) of every case is the recording tests/golden/feature_refusals.json, made by
`python tests/test_feature_refusals.py --record` on a GPU.  Every entry has a call that would run and an ordered chain of defects, one per
check in the order the entry performs them; extra defects are further ways to fail one of those checks.
  single cases: every defect alone;
  pair cases:   defects i and i + 1 of the chain at once -- the text is then defect i's, which pins the order.
Every case returns before any launch.  A device form takes the same (host) pointers and is only called once its host form has refused the
case, so no pointer is ever followed on the device."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "feature_refusals.json")
W = 32      # frame 32 x 32
T = 16      # render tile, accumulator tile
NAN, INF = float("nan"), float("inf")
NAMED_FLAGS = {"RT1W_OUT_SUM": 1, "RT1W_UNSORTED": 2, "RT1W_LDS_NODES": 4, "RT1W_GENERIC": 8, "RT1W_WAVEFRONT": 16, "RT1W_OUT_FRAME": 32,
               "RT1W_RNG_REFERENCE": 64, "RT1W_CLASSIC_WALK": 128, "RT1W_NO_NODE_CACHE": 0x10000, "RT1W_PROBE_COHERENT": 0x40000000}
DENOISED_FLAGS = ("RT1W_OUT_SUM", "RT1W_OUT_FRAME", "RT1W_RNG_REFERENCE", "RT1W_PROBE_COHERENT")  # the ones rt1w_render_denoised refuses
UNKNOWN_FLAG = 0x20000


def arg(**kw):
    """defect: replace whole arguments"""
    return lambda a: a.update(kw)


def member(key, **kw):
    """defect: replace members of the struct argument `key` (nothing to do where another defect made it null)"""
    def f(a):
        if a[key] is not None:
            a[key] = dict(a[key], **kw)
    return f


RENDER = dict(width=W, height=W, x0=0, y0=0, tile_w=T, tile_h=T, spp=4, sample_offset=0, max_depth=8, global_seed=0, chunk=0, flags=0,
              strip_rows=0, strip_period=0, precision=0, partial_mib=0)
DENOISE = dict(width=W, height=W, iterations=2, flags=0, sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0)
ADAPTIVE = dict(tile=T, batch_spp=2, pilot_batches=2, budget_spp=8, max_spp=16, target_error=0.0, round_share=0.0, flags=0)

# chains shared by several entries: (case name, defect) in the order of the checks
NULL_RENDER = [("null context", arg(ctx=None)), ("null params", arg(p=None)), ("width 1", member("p", width=1))]
DEEP = [("max_specular 65", arg(max_specular=65))]
DENOISE_CHECKS = [("width 0", member("d", width=0)), ("iterations 9", member("d", iterations=9)), ("unknown denoise flag", member("d", flags=2)),
                  ("sigma NaN", member("d", sigma_colour=NAN))]
DENOISE_MORE = [("height 0", member("d", height=0)), ("sigma negative", member("d", sigma_colour=-1.0)),
                ("sigma infinite", member("d", sigma_colour=INF)), ("sigma_normal NaN", member("d", sigma_normal=NAN)),
                ("sigma_depth NaN", member("d", sigma_depth=NAN))]
SIGMA_VARIANCE = [("sigma_variance NaN", arg(sigma_variance=NAN))]
SIGMA_VARIANCE_MORE = [("sigma_variance negative", arg(sigma_variance=-1.0)), ("sigma_variance infinite", arg(sigma_variance=INF))]
# the preamble of the render-then-filter entries, then their denoise parameters against the tile
DENOISED = [("RT1W_OUT_SUM", member("p", flags=1)), ("strip_rows 4", member("p", strip_rows=4, strip_period=4)), ("f32", member("p", precision=1))]
DENOISED_MORE = [(n, member("p", flags=NAMED_FLAGS[n])) for n in DENOISED_FLAGS[1:]]
TILE_DENOISE = [("denoise width 24", member("d", width=24)), ("iterations 9", member("d", iterations=9)),
                ("unknown denoise flag", member("d", flags=2)), ("sigma NaN", member("d", sigma_colour=NAN))]
TILE_DENOISE_MORE = [("denoise height 24", member("d", height=24)), ("sigma negative", member("d", sigma_colour=-1.0)),
                     ("sigma infinite", member("d", sigma_colour=INF))]


def nulls(*keys):
    return [("null " + k, arg(**{k: None})) for k in keys]


def tiles_defect(what):
    def f(a):
        t = [tuple(x) for x in a["tiles"]]
        if not t:
            return  # another defect emptied the list
        if what == "unaligned":
            t[0] = (8, 0, 0, 0)
        elif what == "duplicate":
            t.append(t[-1])
        elif what == "outside":
            t[0] = (W, 0, 0, 0)
        elif what == "reserved":
            t[0] = t[0][:3] + (1,)
        a["tiles"] = t
    return f


AOV_CHAIN = NULL_RENDER + [("null out", arg(out=None)), ("RT1W_OUT_SUM", member("p", flags=1)), ("f32", member("p", precision=1))]
AOV_MORE = [(n, member("p", flags=v)) for n, v in NAMED_FLAGS.items() if n != "RT1W_OUT_SUM"] + [("unknown flag", member("p", flags=UNKNOWN_FLAG))]
FRAME = [("null context", arg(ctx=None)), ("width 0", arg(w=0))]

# entry -> (its device form or None, the call that would run, the names of its arguments in order, chain, extra single defects)
ENTRIES = {
    "rt1w_render_aov": ("rt1w_render_aov_device", dict(p=RENDER), ("ctx", "p", "out", "stats"), AOV_CHAIN, AOV_MORE),
    "rt1w_render_aov_deep": ("rt1w_render_aov_deep_device", dict(p=RENDER, max_specular=8, max_fuzz=0.0),
                             ("ctx", "p", "max_specular", "max_fuzz", "out", "stats"), DEEP + AOV_CHAIN,
                             [("max_fuzz negative", arg(max_fuzz=-1.0))] + AOV_MORE),
    "rt1w_denoise": ("rt1w_denoise_device", dict(d=DENOISE), ("ctx", "d", "frame", "aov", "out", "stats"),
                     [("null context", arg(ctx=None)), ("null params", arg(d=None))] + DENOISE_CHECKS + nulls("frame"),
                     DENOISE_MORE + nulls("aov", "out")),
    "rt1w_render_denoised": (None, dict(p=RENDER, d=dict(DENOISE, width=T, height=T)), ("ctx", "p", "d", "out", "stats"),
                             NULL_RENDER + [("null out", arg(out=None))] + DENOISED + TILE_DENOISE, DENOISED_MORE + TILE_DENOISE_MORE),
    "rt1w_render_denoised_deep": (None, dict(p=RENDER, d=dict(DENOISE, width=T, height=T), max_specular=8, max_fuzz=0.0),
                                  ("ctx", "p", "d", "max_specular", "max_fuzz", "out", "stats"),
                                  DEEP + NULL_RENDER + [("null out", arg(out=None))] + DENOISED + TILE_DENOISE,
                                  [("max_fuzz negative", arg(max_fuzz=-1.0))] + DENOISED_MORE + TILE_DENOISE_MORE),
    "rt1w_batch_variance": ("rt1w_batch_variance_device", dict(w=W, h=W, batches=4, batch_spp=2, flags=0),
                            ("ctx", "w", "h", "batches", "batch_spp", "flags", "sums", "aov", "frame", "var", "stats"),
                            FRAME + [("unknown denoise flag", arg(flags=2)), ("batches 1", arg(batches=1))] + nulls("sums"),
                            [("height 0", arg(h=0)), ("batches 17", arg(batches=17)), ("batch_spp 0", arg(batch_spp=0))] + nulls("aov", "frame", "var")),
    "rt1w_denoise_var": ("rt1w_denoise_var_device", dict(d=DENOISE, sigma_variance=0.0),
                         ("ctx", "d", "frame", "aov", "var", "sigma_variance", "out", "stats"),
                         [("null context", arg(ctx=None)), ("null params", arg(d=None))] + DENOISE_CHECKS + SIGMA_VARIANCE + nulls("frame"),
                         DENOISE_MORE + SIGMA_VARIANCE_MORE + nulls("aov", "var", "out")),
    "rt1w_render_denoised_var": (None, dict(p=RENDER, d=dict(DENOISE, width=T, height=T), batches=4, sigma_variance=0.0, max_specular=8, max_fuzz=0.0),
                                 ("ctx", "p", "d", "batches", "sigma_variance", "max_specular", "max_fuzz", "out", "stats"),
                                 DEEP + SIGMA_VARIANCE + NULL_RENDER + [("null out", arg(out=None))] + DENOISED + [("batches 1", arg(batches=1))] + TILE_DENOISE,
                                 [("max_fuzz negative", arg(max_fuzz=-1.0)), ("batches 17", arg(batches=17)),
                                  ("spp 6 in 4 batches", member("p", spp=6))] + SIGMA_VARIANCE_MORE + DENOISED_MORE + TILE_DENOISE_MORE),
    "rt1w_accum_merge": ("rt1w_accum_merge_device", dict(w=W, h=W, x0=T, y0=T, tw=T, th=T, batch_spp=2, flags=0),
                         ("ctx", "w", "h", "x0", "y0", "tw", "th", "batch_spp", "flags", "sums", "aov", "acc", "stats"),
                         FRAME + [("rectangle outside", arg(x0=24))] + nulls("sums"),
                         [("height 0", arg(h=0)), ("rectangle origin outside", arg(y0=W)), ("batch_spp 0", arg(batch_spp=0)),
                          ("unknown flag", arg(flags=2))] + nulls("aov", "acc")),
    "rt1w_accum_merge_tiles": ("rt1w_accum_merge_tiles_device", dict(w=W, h=W, tile=T, tiles=[(0, 0, 0, 0), (T, T, 0, 0)], batch_spp=2, flags=0),
                               ("ctx", "w", "h", "tile", "tiles", "n_tiles", "batch_spp", "flags", "sums", "aov", "acc", "stats"),
                               FRAME + [("tile 8", arg(tile=8)), ("batch_spp 0", arg(batch_spp=0)), ("no tiles", arg(tiles=[])),
                                        ("unaligned tile", tiles_defect("unaligned")), ("duplicate tile", tiles_defect("duplicate"))] + nulls("sums"),
                               [("tile 24", arg(tile=24)), ("unknown flag", arg(flags=2)), ("null tiles", arg(tiles=None)),
                                ("tile outside", tiles_defect("outside")), ("tile reserved 1", tiles_defect("reserved"))] + nulls("aov", "acc")),
    "rt1w_accum_resolve": ("rt1w_accum_resolve_device", dict(w=W, h=W, batch_spp=2), ("ctx", "w", "h", "batch_spp", "acc", "frame", "var", "spp", "stats"),
                           FRAME + [("batch_spp 0", arg(batch_spp=0))] + nulls("acc"), [("height 0", arg(h=0))] + nulls("frame", "var", "spp")),
    "rt1w_accum_tile_error": ("rt1w_accum_tile_error_device", dict(w=W, h=W, tile=T), ("ctx", "w", "h", "tile", "acc", "err", "stats"),
                              FRAME + [("tile 8", arg(tile=8))] + nulls("acc"), [("height 0", arg(h=0)), ("tile 24", arg(tile=24))] + nulls("err")),
    "rt1w_adaptive_select": (None, dict(a=ADAPTIVE, ntx=2, nty=2, w=W, h=W, capacity=4), ("a", "ntx", "nty", "w", "h", "err", "m", "out", "capacity"),
                             [("null params", arg(a=None)), ("size 4", member("a", size=4)), ("tile 8", member("a", tile=8)),
                              ("wrong tile grid", arg(ntx=3))] + nulls("err"),
                             [("tile 24", member("a", tile=24)), ("pilot 1", member("a", pilot_batches=1)), ("max_spp 2", member("a", max_spp=2)),
                              ("budget_spp 2", member("a", budget_spp=2)), ("target_error NaN", member("a", target_error=NAN)),
                              ("round_share 2", member("a", round_share=2.0)), ("unknown adaptive flag", member("a", flags=2)),
                              ("width 0", arg(w=0)), ("wrong tile rows", arg(nty=1))] + nulls("m", "out")),
    "rt1w_render_adaptive": (None, dict(p=dict(RENDER, tile_w=W, tile_h=W), a=ADAPTIVE, d=DENOISE, sigma_variance=0.0),
                             ("ctx", "p", "a", "d", "sigma_variance", "out", "out_spp", "stats"),
                             SIGMA_VARIANCE + [("null adaptive params", arg(a=None)), ("tile 8", member("a", tile=8))] + NULL_RENDER +
                             [("null out", arg(out=None))] + DENOISED +
                             [("sub-frame tile", member("p", tile_w=T)), ("one launch and RT1W_UNSORTED", lambda a: (member("a", flags=0x100)(a), member("p", flags=2)(a))),
                              ("sample_offset and max_spp overflow", member("p", sample_offset=0xFFFFFFFF - 2))] + TILE_DENOISE,
                             SIGMA_VARIANCE_MORE + DENOISED_MORE + TILE_DENOISE_MORE +
                             [("tile 24", member("a", tile=24)), ("size 4", member("a", size=4)), ("sub-frame origin", member("p", x0=T, tile_w=T))]),
}


def cases_of(entry):
    """[(case name, [defects])]: the singles, then the pairs of neighbours in the chain"""
    _, _, _, chain, more = ENTRIES[entry]
    singles = [(n, [f]) for n, f in chain + more]
    assert len({n for n, _ in singles}) == len(singles), entry
    pairs = [(f"{a[0]} + {b[0]}", [a[1], b[1]]) for a, b in zip(chain, chain[1:])]
    return singles + pairs


def case_names():
    names = {}
    for entry, spec in ENTRIES.items():
        for e in (entry, spec[0]):
            if e:
                names[e] = [n for n, _ in cases_of(entry)]
    return names


def run_cases(rt, ctx):
    """{entry: [[case, return code, error text]]} of this library; a device form gets the cases its host form refused"""
    buf = np.zeros(W * W * 3 * 17)  # as large as the largest buffer of any call here; no case gets as far as reading it
    keep = []

    def marshal(name, v, a):
        if name == "ctx":
            return ctx._h if v == "ctx" else None
        if name == "stats":
            return None
        if name == "n_tiles":
            return len(a["tiles"] or ())
        if name == "tiles":
            if v is None:
                return None
            keep.append(rt._tile_list(v)[0])
            return C.cast(keep[-1], C.c_void_p)
        if name in ("p", "d", "a"):
            if v is None:
                return None
            s = {"p": rt.RenderParams, "d": rt.DenoiseParams}[name](**v) if name != "a" else rt.adaptive_params(**v)
            keep.append(s)
            return C.byref(s)
        if isinstance(v, (int, float)):
            return v
        return None if v is None else buf.ctypes.data  # a buffer

    def call(fn_name, order, a):
        fn = getattr(rt._lib, fn_name)
        rc = fn(*[marshal(k, a.get(k, "buffer"), a) for k in order])
        return [int(rc), rt.last_error() if rc < 0 else ""]

    out = {}
    for entry, (device, good, order, _, _) in ENTRIES.items():
        out[entry] = []
        if device:
            out[device] = []
        for name, defects in cases_of(entry):
            a = dict(good, ctx="ctx")
            for f in defects:
                f(a)
            got = call(entry, order, a)
            out[entry].append([name] + got)
            if device:
                out[device].append([name] + (call(device, order, a) if got[0] < 0 else [0, "not called: the host form did not refuse"]))
    return out


@pytest.mark.gpu
def test_feature_refusals(rt, gpu_ctx_factory):
    with open(GOLDEN) as f:
        want = json.load(f)
    names = case_names()
    assert {e: [c[0] for c in cs] for e, cs in want.items()} == names, "the recording's cases are not the cases of this file: record again"
    got = run_cases(rt, gpu_ctx_factory(rt.Scene.reference(0, build_seed=1)))
    wrong = [(e, g, w) for e in names for g, w in zip(got[e], want[e]) if g != w]
    assert not wrong, f"{len(wrong)} refusals differ from the recording, (entry, got, recorded): {wrong[:8]}"
    assert all(c[1] < 0 for cs in want.values() for c in cs), "a recorded case was not refused"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_feature_refusals.py --record   (on a GPU, with the library whose refusals are to be pinned)")
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import orc
    _rt = orc.rt()
    assert _rt.device_count() >= 1, "recording needs a GPU"
    _ctx = _rt.Context(_rt.Scene.reference(0, build_seed=1), 0)
    _got = run_cases(_rt, _ctx)
    _ctx.close()
    _open = [(e, c) for e, cs in _got.items() for c in cs if c[1] >= 0]
    assert not _open, f"cases that were not refused: {_open}"
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(_got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(c) for c in _got.values())} cases of {len(_got)} entries")
