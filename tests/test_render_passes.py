"""Renders that run as several sample passes, and the device entry rt1w_render_device (GPU tier).

A render whose chunk partial sums exceed the budget (rt1w_render_params.partial_mib, default 8 GiB) runs as several launches of the
trace kernel over consecutive chunk ranges; the resolve kernel adds each pass onto the running sums in order, so the frame must not
change by a bit.  rt1w_stats.passes reports how many launches ran; every render here asserts it against expected_passes, a plain
restatement of chunks_per_pass (csrc/context.hip).

Expected sides: the CPU build of the kernel core (orc.flat_render) with the same chunking for the f64 Philox kernels; the same kernel's
one-pass frame for the f32 kernels (their CPU twin, orc.flat_f32_render, is compared with the exact build of the same kernels in
test_f32_twin.py: the product's own f32 frame differs from it in five elementary functions); the reference-stream CPU core for the reference stream.
"""
import ctypes as C
import json

import numpy as np
import pytest

import orc
from test_kernel_choice import FIXTURE, MODES, SIZES

pytestmark = pytest.mark.gpu

DEFAULT_BUDGET = 8 << 30
# 128 x 96 pixels are 294 912 B of partial sums per chunk: 3 chunks per 1 MiB pass, so 10 samples at chunk 1 run as 3 + 3 + 3 + 1
W, H, SPP = 128, 96, 10
# 256 x 160 pixels are 983 040 B per chunk: one chunk per 1 MiB pass
ONE_W, ONE_H = 256, 160


def expected_passes(tile_w, tile_h, spp, chunk, mib):
    """chunks_per_pass restated: chunks of `chunk` samples, as many per pass as the budget holds but at least one."""
    chunk = min(chunk, spp)
    n_chunks = -(-spp // chunk)
    per_chunk = tile_w * tile_h * 3 * 8
    budget = (mib << 20) if mib else DEFAULT_BUDGET
    per_pass = min(max(1, budget // per_chunk), n_chunks)
    return -(-n_chunks // per_pass)


def test_expected_passes_restatement():
    assert expected_passes(W, H, SPP, 1, 1) == 4
    assert expected_passes(W, H, SPP, 3, 1) == 2                   # chunks of 3, 3, 3, 1 samples: 3 chunks, then 1
    assert expected_passes(ONE_W, ONE_H, 3, 1, 1) == 3
    assert expected_passes(256, 256, 5, 5, 1) == 1                 # one chunk larger than the budget still runs, in one pass
    assert expected_passes(W, H, SPP, 1, 0) == 1


_SCENES = {}
_CPU = {}


def scene(rt, arm):
    if arm not in _SCENES:
        _SCENES[arm] = rt.Scene.reference(arm, build_seed=1)
    return _SCENES[arm]


def cpu(rt, arm, width, height, spp, chunk, variant=None, **kw):
    """orc.flat_render of one (arm, variant, shape, chunk), computed once for the module"""
    key = (arm, width, height, spp, chunk, variant, tuple(sorted(kw.items())))
    if key not in _CPU:
        _CPU[key] = orc.flat_render(scene(rt, arm), width, height, spp, chunk=chunk, variant=variant, **kw)
    return _CPU[key]


def same(img, st, ref):
    """bit for bit, equal segment counts"""
    want, sw = ref
    return st["segments"] == sw["segments"] and np.array_equal(img, want, equal_nan=True)


def test_every_kernel_of_the_table_across_sample_passes(rt, tmp_path, monkeypatch):
    """Every row of tests/golden/kernel_choice.json that renders with the Philox streams, at 128 x 96 x 10 spp, chunk 1 and a 1 MiB
    budget: 4 passes.  The row's variant and stats.sorted bits equal the fixture's (the intended kernel ran); f64 frames equal the
    CPU core, f32 frames the kernel's own one-pass frame.  Reference-stream rows are one chunk, hence one pass.  The wavefront form
    renders in one pass only: refused when the budget forces passes, equal to the CPU core when it fits."""
    monkeypatch.setenv("RT1W_KERNEL_CACHE", str(tmp_path))
    want = json.load(open(FIXTURE))
    n_pass = expected_passes(W, H, SPP, 1, 1)
    assert n_pass >= 3
    philox = sorted(k for k, v in want.items() if "error" not in v and not v["sorted"] & (8 | 16))
    covered, wavefront, refstream = [], [], []
    for arm in SIZES:
        ctx = rt.Context(scene(rt, arm), 0)
        try:
            for name, kw in MODES:
                key = f"{arm}/{name}"
                row = want[key]
                if "error" in row:
                    continue
                if row["sorted"] & 16:             # reference stream: one chunk per pixel, one pass whatever the budget
                    img, st = ctx.render(W, H, SPP, partial_mib=1, **kw)
                    one, so = ctx.render(W, H, SPP, **kw)
                    assert st["passes"] == so["passes"] == 1 and st["n_chunks"] == 1, key
                    assert (st["variant"], st["sorted"]) == (row["variant"], row["sorted"]), key
                    assert same(img, st, (one, so)), key
                    refstream.append(key)
                    continue
                if row["sorted"] & 8:              # wavefront form
                    with pytest.raises(rt.Rt1wError) as e:
                        ctx.render(W, H, SPP, chunk=1, partial_mib=1, **kw)
                    assert e.value.code == rt.ERR_UNSUPPORTED, key
                    img, st = ctx.render(W, H, SPP, chunk=1, **kw)
                    assert st["passes"] == 1 and (st["variant"], st["sorted"]) == (row["variant"], row["sorted"]), key
                    assert same(img, st, cpu(rt, arm, W, H, SPP, 1, st["variant"])), key
                    wavefront.append(key)
                    continue
                if kw is None:                     # render_rows: one strip of the whole tile
                    img, st = ctx.render_rows(W, H, SPP, strip_rows=H, chunk=1, partial_mib=1)
                else:
                    img, st = ctx.render(W, H, SPP, chunk=1, partial_mib=1, **kw)
                assert (st["variant"], st["sorted"]) == (row["variant"], row["sorted"]), key
                assert st["passes"] == n_pass and st["chunk"] == 1 and st["n_chunks"] == SPP, (key, st["passes"])
                if st["sorted"] & 32:              # f32: the same kernel in one pass
                    one, so = ctx.render(W, H, SPP, chunk=1, **kw)
                    assert so["passes"] == 1 and so["sorted"] == st["sorted"], key
                    assert same(img, st, (one, so)), key
                else:
                    assert same(img, st, cpu(rt, arm, W, H, SPP, 1, st["variant"])), key
                covered.append(key)
            # the default kernel with a sample offset on a tile, raw sums, one chunk per pass and a ragged chunk of 3
            tile = (16, 8, 96, 80)                 # 184 320 B per chunk: 5 chunks per pass
            img, st = ctx.render(W, H, SPP, tile=tile, sample_offset=7, chunk=1, partial_mib=1)
            assert st["passes"] == expected_passes(96, 80, SPP, 1, 1) == 2, arm
            assert same(img, st, cpu(rt, arm, W, H, SPP, 1, tile=tile, sample_offset=7)), arm
            raw, sr = ctx.render(W, H, SPP, out_sum=True, chunk=1, partial_mib=1)
            assert sr["passes"] == n_pass and same(raw, sr, cpu(rt, arm, W, H, SPP, 1, out_sum=True)), arm
            img, st = ctx.render(ONE_W, ONE_H, 3, chunk=1, partial_mib=1)
            assert st["passes"] == expected_passes(ONE_W, ONE_H, 3, 1, 1) == 3, arm
            assert same(img, st, cpu(rt, arm, ONE_W, ONE_H, 3, 1)), arm
            img, st = ctx.render(W, H, SPP, chunk=3, partial_mib=1)
            assert st["passes"] == expected_passes(W, H, SPP, 3, 1) == 2 and st["n_chunks"] == 4, arm
            assert same(img, st, cpu(rt, arm, W, H, SPP, 3)), arm
        finally:
            ctx.close()
    print(f"\nsample passes: {len(covered)} rows at {n_pass} passes: {' '.join(covered)}")
    print(f"one pass: reference stream {' '.join(refstream)}; wavefront {' '.join(wavefront)}")
    assert sorted(covered) == philox, sorted(set(philox) ^ set(covered))
    assert wavefront == ["0/wavefront", "7/wavefront"]


@pytest.mark.parametrize("arm", (5, 7))
def test_reference_stream_chunk_larger_than_the_budget(rt, gpu_ctx_factory, arm):
    """One chunk of 1.5 MiB under a 1 MiB budget: the pass cannot be split, it still renders, in one pass."""
    ctx = gpu_ctx_factory(scene(rt, arm))
    img, st = ctx.render(256, 256, 3, reference_stream=True, partial_mib=1)
    assert st["passes"] == expected_passes(256, 256, 3, 3, 1) == 1 and st["n_chunks"] == 1
    assert same(img, st, orc.flat_render(scene(rt, arm), 256, 256, 3, chunk=3, lib=orc.flat_ref_lib(), variant=st["variant"]))


@pytest.mark.parametrize("arm", (7, 0))
def test_render_rows_and_u8_across_sample_passes(rt, gpu_ctx_factory, arm):
    """render_rows with a 1 MiB budget: strips of 56 rows (2 passes each, one per lane) and of 40 rows (2 passes; the third strip,
    16 rows, is ragged and runs in 1 pass on lane 0 again); render_u8 with 4 passes.  Equal to render and to the CPU core."""
    ctx = gpu_ctx_factory(scene(rt, arm))
    ref = cpu(rt, arm, W, H, SPP, 1)
    full, sf = ctx.render(W, H, SPP, chunk=1, partial_mib=1)
    assert same(full, sf, ref)
    for strip in (56, 40):
        heights = [min(strip, H - top) for top in range(0, H, strip)]
        want = sum(expected_passes(W, h, SPP, 1, 1) for h in heights)
        img, st = ctx.render_rows(W, H, SPP, strip_rows=strip, chunk=1, partial_mib=1)
        assert st["passes"] == want and all(expected_passes(W, h, SPP, 1, 1) >= 2 for h in heights[:2]), (strip, st["passes"])
        assert same(img, st, ref), strip
        u8, su = ctx.render_rows(W, H, SPP, strip_rows=strip, u8=True, chunk=1, partial_mib=1)
        assert su["passes"] == want and np.array_equal(u8, rt.quantize(ref[0])[::-1]), strip
    u8, su = ctx.render_u8(W, H, SPP, chunk=1, partial_mib=1)
    assert su["passes"] == expected_passes(W, H, SPP, 1, 1) and np.array_equal(u8, rt.quantize(full)[::-1])


def test_lane_buffer_reuse_across_budgets(rt, gpu_ctx_factory):
    """One context: default budget, 1 MiB, default again.  Each frame and pass count equals a fresh context's."""
    ctx = gpu_ctx_factory(scene(rt, 7))
    for mib in (0, 1, 0, 1):
        img, st = ctx.render(W, H, SPP, chunk=1, partial_mib=mib)
        fresh = gpu_ctx_factory(scene(rt, 7))
        want, sw = fresh.render(W, H, SPP, chunk=1, partial_mib=mib)
        fresh.close()
        assert st["passes"] == sw["passes"] == expected_passes(W, H, SPP, 1, mib), mib
        assert same(img, st, (want, sw)) and same(img, st, cpu(rt, 7, W, H, SPP, 1)), mib


class DeviceBuffer:
    """device memory from the HIP runtime librt1w.so itself uses (what a torch tensor's data_ptr() would hand over)"""
    hip = None

    def __init__(self, nbytes):
        if DeviceBuffer.hip is None:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipFree.argtypes = [C.c_void_p]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventDestroy.argtypes = [C.c_void_p]
            DeviceBuffer.hip = hip
        self.nbytes = nbytes
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        self.ptr = p.value

    def to_host(self, shape):
        out = np.empty(shape, dtype=np.float64)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0  # DeviceToHost
        return out

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


def same_stats(a, b):
    return {k: v for k, v in a.items() if not k.endswith("_ms")} == {k: v for k, v in b.items() if not k.endswith("_ms")}


@pytest.mark.parametrize("arm", (5, 7, 0))
def test_render_device_equals_render_and_the_cpu_core(rt, gpu_ctx_factory, arm):
    """rt1w_render_device into caller device memory: full frame, tile, packed interleaved strips, raw sums with a sample offset, f32
    and a 1 MiB budget, each equal to render and to the CPU core bit for bit, with the same stats.  RT1W_OUT_FRAME and a null
    pointer are refused."""
    ctx = gpu_ctx_factory(scene(rt, arm))
    ref = cpu(rt, arm, W, H, SPP, 1)
    cases = [({}, (H, W), ref[0]),
             ({"tile": (16, 8, 64, 40)}, (40, 64), ref[0][8:48, 16:80]),
             ({"tile": (0, 0, W, 32), "strips": (16, 48)}, (32, W), np.concatenate([ref[0][0:16], ref[0][48:64]])),
             ({"partial_mib": 1}, (H, W), ref[0]),
             ({"tile": (8, 16, 32, 24), "out_sum": True, "sample_offset": 3}, (24, 32),
              cpu(rt, arm, W, H, SPP, 1, tile=(8, 16, 32, 24), out_sum=True, sample_offset=3)[0]),
             ({"f32": True, "partial_mib": 1}, (H, W), None)]
    for kw, (th, tw), want in cases:
        host, sh = ctx.render(W, H, SPP, chunk=1, **kw)
        dev = DeviceBuffer(th * tw * 3 * 8)
        try:
            sd = ctx.render_device(dev.ptr, W, H, SPP, chunk=1, **kw)
            got = dev.to_host((th, tw, 3))
        finally:
            dev.free()
        assert same_stats(sd, sh), (kw, sd, sh)
        assert sd["passes"] == expected_passes(tw, th, SPP, 1, kw.get("partial_mib", 0)), kw
        assert np.array_equal(got, host, equal_nan=True), kw
        if want is not None:
            assert np.array_equal(got, want, equal_nan=True), kw
    dev = DeviceBuffer(H * W * 3 * 8)
    try:
        p = ctx._params(W, H, SPP, 50, None, 0, 0, 1, False)
        p.flags = rt.OUT_FRAME
        assert rt._lib.rt1w_render_device(ctx._h, C.byref(p), C.c_void_p(dev.ptr), None) == rt.ERR_INVALID and rt.last_error()
        p.flags = 0
        assert rt._lib.rt1w_render_device(ctx._h, C.byref(p), None, None) == rt.ERR_INVALID and rt.last_error()
    finally:
        dev.free()


def test_render_device_runs_after_work_queued_on_the_null_stream(rt, gpu_ctx_factory):
    """include/rt1w.h / context.hip: the lanes' streams are blocking streams, so a render into caller memory runs after what the caller
    queued on the null stream.  Queued on stream 0: long memsets of a scratch buffer, then a memset of the output buffer to 0xFF;
    then render_device and one device-wide wait.  If the render did not wait, the 0xFF memset would land after it and the buffer
    would hold no frame.  The check is one-sided: it only means something while the scratch memsets outlast the render, which the
    test measures and asserts (events on stream 0 against stats.kernel_ms).  Measured on an MI355X: 10.8 ms for the eight 8 GiB
    memsets, 0.9 ms for the render."""
    ctx = gpu_ctx_factory(scene(rt, 5))
    w, h, spp = 64, 64, 4
    want, sw = ctx.render(w, h, spp)
    out, scratch = DeviceBuffer(h * w * 3 * 8), DeviceBuffer(8 << 30)
    hip = DeviceBuffer.hip
    ev = [C.c_void_p(), C.c_void_p()]
    try:
        for e in ev:
            assert hip.hipEventCreate(C.byref(e)) == 0
        assert hip.hipEventRecord(ev[0], None) == 0
        for _ in range(8):
            assert hip.hipMemsetAsync(scratch.ptr, 0x5A, scratch.nbytes, None) == 0
        assert hip.hipEventRecord(ev[1], None) == 0
        assert hip.hipMemsetAsync(out.ptr, 0xFF, out.nbytes, None) == 0
        sd = ctx.render_device(out.ptr, w, h, spp)
        assert hip.hipDeviceSynchronize() == 0
        got = out.to_host((h, w, 3))
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    finally:
        for e in ev:
            if e.value:
                hip.hipEventDestroy(e)
        out.free()
        scratch.free()
    print(f"\nnull-stream memsets of 8 x 8 GiB: {ms.value:.3f} ms; render: {sd['kernel_ms']:.3f} ms")
    assert np.array_equal(got, want, equal_nan=True) and sd["segments"] == sw["segments"]
    assert ms.value > 2 * sd["kernel_ms"], (ms.value, sd["kernel_ms"])
