"""Radiance queries (rt1w_ray_color, rt1w_ray_color_device; csrc/context_rays.hip: the render kernels' ray-list form) -- GPU tier.

The kernels against the CPU twin (test_ray_color.py holds the twin to the CPU build of the render core and to the literal oracle), the
entry against rt1w_render_device on the camera's own rays, sample passes, the device entry between guard bands, the rays that are not
traced and the refusal table on the real entries, and the command-line tool's panorama.  Everything is bit for bit (a NaN equals a NaN),
with equal segment counts; every ray is compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import ray_color_reference as RC
import spec_graphs as G

ROOT = orc.ROOT
W, H = RC.W, RC.H
SORTED, JIT, PW, SS, HC = 1, 4, 128, 512, 1024  # rt1w_stats.sorted (include/rt1w.h)
pytestmark = pytest.mark.gpu


def _scene(rt, name):
    return G.build(("random", 3047, None))[0] if name == "random3047" else rt.Scene.reference(name, build_seed=1, aspect_ratio=1.5)


# what must have run: arm 5 the reordering kernel, 6 the same with media, 0 the pair walk with slice-end reordering, 7 the sliced stack
# walk with the node cache, the random wrapper graph the reordering kernel; never a scene-specialised kernel
FAMILY = {5: (SORTED, JIT | PW | SS), 6: (SORTED, JIT | PW | SS), 0: (PW | SS, JIT | SORTED), 7: (SS | HC, JIT | SORTED | PW), "random3047": (SORTED, JIT | PW | SS)}


@pytest.mark.parametrize("name", list(FAMILY))
def test_kernels_equal_the_twin(rt, gpu_ctx_factory, name):
    """Every n of COUNTS on camera rays (with their stream positions) and on incoherent bounce rays (with made-up positions), spp 1 and
    5, work items of the default size, 1 and 2: values and segments of the twin, and the kernel family in stats.sorted."""
    sc = _scene(rt, name)
    ctx = gpu_ctx_factory(sc)
    cam, cam_word = RC.camera_list(rt, sc, 40, 25, 3, 2)  # 1000 rays in pixel-seed order
    bounce = RC.bounce_rays(rt, sc, max(RC.COUNTS))
    bounce_word = (np.arange(len(bounce), dtype=np.uint32) * 7) % 29
    want_bits, never = FAMILY[name]
    for what, rays, word in (("camera", cam, cam_word), ("bounce", bounce, bounce_word)):
        for n in RC.COUNTS:
            for spp in (1, 5):
                for chunk in (0, 1, 2):
                    kw = dict(spp=spp, chunk=chunk, sample_offset=3, first_stream=0 if what == "camera" else 77, global_seed=2)
                    want, wst = rt.ray_color_host(sc, rays[:n], word[:n], with_stats=True, **kw)
                    got, st = ctx.ray_color(rays[:n], word[:n], with_stats=True, **kw)
                    tag = (name, what, n, spp, chunk)
                    assert RC.same_bits(got, want), (tag, int((got != want).any(axis=1).sum()))
                    assert st["segments"] == wst["segments"] and st["paths"] == n * spp, (tag, st["segments"], wst["segments"])
                    assert st["sorted"] & want_bits == want_bits and not st["sorted"] & never, (tag, st["sorted"])
                    eff = min(sc.default_chunk(n, 1, spp) if chunk == 0 else chunk, spp)
                    assert st["chunk"] == eff and st["n_chunks"] == (spp + eff - 1) // eff and st["passes"] == 1 and st["variant"] == sc.info()["variant"], (tag, st)
    ctx.close()


@pytest.fixture()
def dev():
    d = RC.Device()
    yield d
    d.free()


def _to_device(dev, a):
    a = np.ascontiguousarray(a)
    ptr, _ = dev.alloc(a.nbytes)
    dev.upload(ptr, a)
    return ptr


@pytest.mark.parametrize("arm", [0, 5, 6, 7])
def test_entry_equals_render_device(rt, gpu_ctx_factory, dev, arm):
    """The camera rays and stream positions of a 24 x 16 frame: ray_color_device(spp 1, RT1W_OUT_SUM) is render_device(spp 1, the same
    sample_offset, RT1W_OUT_SUM), with RT1W_GENERIC and with the context's default kernel, bit for bit with equal segments."""
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=1.5)
    ctx = gpu_ctx_factory(sc)
    specialised = 0
    for s, gs in ((0, 0), (7, 2)):
        rays, word = RC.camera_list(rt, sc, W, H, s, gs)
        n = len(rays)
        d_out = _to_device(dev, np.full((n, 3), -1.0))
        st = ctx.ray_color_device(_to_device(dev, rays), d_out, n, _to_device(dev, word), spp=1, sample_offset=s, global_seed=gs, out_sum=True)
        got = dev.download(d_out, (H, W, 3), np.float64)
        for generic in (True, False):
            d_img = _to_device(dev, np.full((H, W, 3), -2.0))
            rst = ctx.render_device(d_img, W, H, 1, sample_offset=s, global_seed=gs, out_sum=True, generic=generic)
            img = dev.download(d_img, (H, W, 3), np.float64)
            assert RC.same_bits(got, img), (arm, s, gs, generic, int((got != img).any(axis=2).sum()))
            assert st["segments"] == rst["segments"] and st["paths"] == rst["paths"], (arm, s, gs, generic)
            if generic:
                assert st["sorted"] == rst["sorted"] and st["variant"] == rst["variant"] and st["block"] == rst["block"], (arm, st, rst)
            else:
                specialised += (rst["sorted"] & JIT) != 0
    print("arm", arm, "default kernel scene-specialised in", specialised, "of 2 renders")
    ctx.close()


def test_sample_passes(rt, gpu_ctx_factory):
    """The 20 000 camera rays of a 200 x 100 Cornell frame, spp 5 in work items of 1 with a budget of 1 MiB for the partial sums: at
    480 000 B per chunk that is two chunks per pass, three passes, and the bits of the one-pass result."""
    sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=2.0)
    ctx = gpu_ctx_factory(sc)
    rays, word = RC.camera_list(rt, sc, 200, 100, 0, 1)
    kw = dict(spp=5, chunk=1, global_seed=1)
    one, st1 = ctx.ray_color(rays, word, with_stats=True, **kw)
    three, st3 = ctx.ray_color(rays, word, with_stats=True, partial_mib=1, **kw)
    assert st1["passes"] == 1 and st3["passes"] == 3 and st3["n_chunks"] == 5
    assert RC.same_bits(three, one) and st3["segments"] == st1["segments"] and np.all(np.isfinite(one)) and one.max() > 0.0
    ctx.close()


def test_device_entry_between_guard_bands(rt, gpu_ctx_factory, dev):
    """d_out inside a larger buffer filled with a sentinel: nothing outside [n][3] is written; d_start_word null and non-null; records of
    nine doubles; the values are the twin's."""
    sc = rt.Scene.reference(6, build_seed=1, aspect_ratio=1.5)
    ctx = gpu_ctx_factory(sc)
    guard, sentinel = 512, -12345.0
    for n in (1, 65, 257):
        rays = RC.bounce_rays(rt, sc, n)
        word = (np.arange(n, dtype=np.uint32) * 3) % 17
        for stride in (7, 9):
            r = rays if stride == 7 else np.concatenate([rays, np.full((n, 2), 9.0)], axis=1)
            d_rays = _to_device(dev, r)
            for w in (None, word):
                big = _to_device(dev, np.full((guard + n + guard, 3), sentinel))
                st = ctx.ray_color_device(d_rays, big + guard * 24, n, None if w is None else _to_device(dev, w), stride=stride, spp=3, chunk=2,
                                          first_stream=5, global_seed=4)
                host = dev.download(big, (guard + n + guard, 3), np.float64)
                assert np.all(host[:guard] == sentinel) and np.all(host[guard + n:] == sentinel), (n, stride, w is None)
                want, wst = rt.ray_color_host(sc, rays, w, spp=3, chunk=2, first_stream=5, global_seed=4, with_stats=True)
                assert RC.same_bits(host[guard:guard + n], want) and st["segments"] == wst["segments"], (n, stride, w is None)
                assert RC.same_bits(dev.download(d_rays, r.shape, np.float64), r), "the rays are read only"
    ctx.close()


_TORCH_CHILD = r"""
import sys, importlib
import numpy as np
import torch
root = sys.argv[1]
sys.path.insert(0, root)
rt = importlib.import_module("raytracing-1w_amd")
sc = rt.Scene.reference(5, build_seed=1, aspect_ratio=1.5)
rays, word = rt.camera_rays_pos_host(sc, 24, 16, 1, sample_offset=1, global_seed=3)
rays, word = np.ascontiguousarray(rays.reshape(-1, 8)), np.ascontiguousarray(word.reshape(-1))
t_rays, t_word = torch.from_numpy(rays).cuda(), torch.from_numpy(word.view(np.int32)).cuda()
t_out = torch.zeros((len(rays), 3), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
ctx = rt.Context(sc, 0)
host = ctx.ray_color(rays, word, spp=2, sample_offset=1, global_seed=3)
ctx.ray_color_device(t_rays.data_ptr(), t_out.data_ptr(), len(rays), t_word.data_ptr(), stride=8, spp=2, sample_offset=1, global_seed=3)
got = t_out.cpu().numpy()
assert np.array_equal(got.view(np.uint64), host.view(np.uint64)) and got.max() > 0.0, "tensors differ from the host form"
assert np.array_equal(t_rays.cpu().numpy().view(np.uint64), rays.view(np.uint64)), "the rays were written"
ctx.close()
print("TORCH-RAYS-OK")
"""


def test_device_entry_on_torch_tensors(rt):
    """ray_color_device on torch tensors of the context's GPU (records of eight doubles as camera_rays_pos_host returns them) equals the
    host form.  torch has to initialise the HIP runtime before librt1w.so does, so the tensors live in a process of their own."""
    import sys
    child = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert child.returncode == 0 and "TORCH-RAYS-OK" in child.stdout, child.stdout[-3000:]


def test_nonfinite_rays_and_the_refusal_table_on_the_entries(rt, gpu_ctx_factory):
    """The rays that are not traced, among good ones, through the kernels (arm 1: a sky; arm 6: black, media) against the rule and the
    twin; and every case of tests/golden/ray_color_refusals.json through rt1w_ray_color on host memory and rt1w_ray_color_device on
    device memory, with its text."""
    for arm in (1, 6):
        sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=1.5)
        ctx = gpu_ctx_factory(sc)
        got = RC.check_nonfinite(rt, sc, lambda rays, fs, depth: ctx.ray_color(rays, spp=3, first_stream=fs, global_seed=2, max_depth=depth))
        rays, bad = RC.nonfinite_lists()
        want, wst = rt.ray_color_host(sc, rays, spp=3, first_stream=40, global_seed=2, with_stats=True)
        _, st = ctx.ray_color(rays, spp=3, first_stream=40, global_seed=2, with_stats=True)
        assert RC.same_bits(got, want) and st["segments"] == wst["segments"] and st["paths"] == 3 * len(rays)
        if arm == 1:
            ctx.close()
    lib = rt._lib

    def host_call(p, rays, word, out):
        return lib.rt1w_ray_color(ctx._h, None if p is None else C.byref(p), rays, word, out, None)

    def host_alloc(nbytes):
        a = np.zeros(nbytes + 16, dtype=np.uint8)
        return (a.ctypes.data + 15) & ~15, a

    def host_download(ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        C.memmove(out.ctypes.data, ptr, out.nbytes)
        return out
    RC.run_table(rt, host_call, host_alloc, lambda ptr, a: C.memmove(ptr, a.ctypes.data, a.nbytes), host_download)
    dev = RC.Device()
    try:
        RC.run_table(rt, lambda p, rays, word, out: lib.rt1w_ray_color_device(ctx._h, None if p is None else C.byref(p), rays, word, out, None),
                     dev.alloc, dev.upload, dev.download)
    finally:
        dev.free()
    ctx.close()


def test_cli_panorama(rt, gpu_ctx_factory, tmp_path):
    """`rt1w --scene 5 --panorama 64 32 --spp 4` writes the bytes the binding produces for the same rays through ray_color and the PPM
    writer: the tool's camera is the few lines of host code its header states (longitude and latitude of the pixel centres, turned so that the middle column looks at look_at; C's sin,
    cos and atan2: Python's math module calls the same functions)."""
    import math
    pw, ph = 64, 32
    out = tmp_path / "pano.ppm"
    tool = os.path.join(ROOT, "raytracing-1w_amd", "rt1w")
    p = subprocess.run([tool, "--scene", "5", "--panorama", str(pw), str(ph), "--spp", "4", "--out", str(out)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    cam = rt.reference_camera(5)
    lf, la = cam["look_from"], cam["look_at"]
    phi0 = math.atan2(la[0] - lf[0], -(la[2] - lf[2]))  # the middle column looks towards look_at
    rays = np.zeros((ph, pw, 7))
    for j in range(ph):
        for i in range(pw):
            phi, theta = 2.0 * math.pi * ((i + 0.5) / pw) - math.pi + phi0, math.pi * ((j + 0.5) / ph) - 0.5 * math.pi
            rays[j, i] = (*lf, math.cos(theta) * math.sin(phi), math.sin(theta), -(math.cos(theta) * math.cos(phi)), 0.0)
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1))
    means = ctx.ray_color(rays.reshape(-1, 7), spp=4, max_depth=50)
    ctx.close()
    text = rt.format_ppm(means.reshape(ph, pw, 3))
    assert out.read_text() == text
    body = np.array(text.split()[4:], dtype=np.int64)
    assert text.startswith(f"P3\n{pw} {ph}\n255\n") and body.max() > 100 and len(set(body.tolist())) > 16, "a picture, not a flat field"
