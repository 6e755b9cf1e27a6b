"""The one skeleton of the four a-trous filters (csrc/rt_atrous_kernels.h: work mapping, staged tile, level kernel, enqueue loop) under each
of its four policies: rt1w_denoise, rt1w_denoise_var, rt1w_denoise_var_halves and rt1w_denoise_cross on the GPU against their CPU twins
(csrc/denoise_host.cpp), bit for bit, at the sizes where the skeleton takes another path.  Synthetic inputs, no render."""
import numpy as np
import pytest

import test_adaptive_filtered as TF

_same = TF._same

# (w, h): a single lane; exactly one workgroup tile; one pixel over and under the tile edge; an interior tile with a halo on every side at
# steps 1 and 2; the two degenerate strips
SHAPES = [(1, 1), (16, 16), (17, 15), (37, 21), (1, 300), (300, 1)]
# the last level is the step-1 staged form, the step-2 staged form, the direct form; steps up to 128, larger than every image here
ITERATIONS = [1, 2, 3, 8]

# name: (the buffers the filter takes after frame and aov, whether it writes err_px, the device entry, the twin)
FILTERS = {
    "denoise": ((), False, "denoise_device", "denoise_host"),
    "denoise_var": (("var",), False, "denoise_var_device", "denoise_var_host"),
    "denoise_var_halves": (("var", "half_a", "half_b"), True, "denoise_var_halves_device", "denoise_var_halves_host"),
    "denoise_cross": (("var", "half_a", "half_b"), True, "denoise_cross_device", "denoise_cross_host"),
}


def _inputs(w, h, seed):
    """a seeded frame as the mean of its two halves, a variance, and feature buffers with unit normals"""
    rng = np.random.default_rng(seed)
    aov = TF._guides(h, w, rng)
    n = rng.normal(size=(h, w, 3))
    aov[..., 3:6] = n / np.sqrt((n * n).sum(axis=2, keepdims=True))
    aov[..., 6] = rng.uniform(1.0, 9.0, (h, w))
    aov[..., 7] = rng.uniform(0.0, 1.0, (h, w))
    half_a, half_b = rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 2.0, (h, w, 3))
    return dict(frame=(half_a + half_b) * 0.5, aov=aov, var=rng.uniform(0.0, 0.3, (h, w)), half_a=half_a, half_b=half_b)


def _hostile(w, h, seed):
    """the same with a block of miss pixels, and one NaN and one inf in the frame and in a half"""
    b = _inputs(w, h, seed)
    b["aov"][5:9, 10:20, 3:6] = 0.0
    b["aov"][5:9, 10:20, 6] = np.inf
    b["aov"][5:9, 10:20, 7] = 0.0
    b["frame"][15, 15] = np.nan
    b["half_a"][15, 15] = np.nan
    b["frame"][16, 16, 1] = np.inf
    b["half_b"][16, 16, 1] = np.inf
    return b


class _Case:
    """one filter on one set of buffers, uploaded once: run(**kw) compares the device form with the twin"""

    def __init__(self, rt, ctx, dev, name, buffers):
        extra, self.has_err, entry, twin = FILTERS[name]
        self.name, self.dev, self.entry, self.twin = name, dev, getattr(ctx, entry), getattr(rt, twin)
        self.host = [buffers[k] for k in ("frame", "aov") + extra]
        self.h, self.w = buffers["frame"].shape[:2]
        self.d_in = [dev.put(x) for x in self.host]
        self.d_out, self.d_err = dev.alloc(self.host[0].nbytes), dev.alloc(8 * self.w * self.h)

    def run(self, in_place=False, **kw):
        expect = self.twin(*self.host, **kw)
        t_out, t_err = expect if self.has_err else (expect, None)
        d_out = self.d_in[0] if in_place else self.d_out
        st = self.entry(*self.d_in, d_out, *((self.d_err,) if self.has_err else ()), self.w, self.h, **kw)
        what = (self.name, self.w, self.h, in_place, kw)
        assert st["block"] == 256 and st["grid"] == ((self.w + 15) // 16) * ((self.h + 15) // 16), what
        assert _same(self.dev.fetch(d_out, t_out.shape), t_out), what
        if self.has_err:
            assert _same(self.dev.fetch(self.d_err, t_err.shape), t_err), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FILTERS))
def test_gpu_skeleton_equals_twin(rt, gpu_ctx_factory, name):
    """out (and err_px where the filter has one) of the device entry == the twin, bit for bit: SHAPES x ITERATIONS x keep_albedo off and on;
    then at 37 x 21 the hostile pixels, and on them the device form in place (out == frame), last, as it consumes the frame."""
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    dev = TF._DeviceBuffers()
    try:
        for w, h in SHAPES:
            case = _Case(rt, ctx, dev, name, _inputs(w, h, 1000 * w + h))
            for iterations in ITERATIONS:
                for keep_albedo in (False, True):
                    case.run(iterations=iterations, keep_albedo=keep_albedo)
        case = _Case(rt, ctx, dev, name, _hostile(37, 21, 7))
        case.run()
        case.run(in_place=True)
    finally:
        dev.free()
