"""Path states (rt1w_path_step[_device], rt1w_path_begin[_device]; csrc/path_step.hip) -- GPU tier.

The kernels against the CPU twins (test_path_step.py holds the twins to rt.ray_color_host, to the CPU build of the render core and to
the literal oracle): all 128 bytes of every state and out_node (D); split, order and compaction on the device (A); carried to its end
against rt1w_ray_color_device (B) and, from the camera, against rt1w_render_device (C); the refusals on the real entries, a misaligned
device pointer and a partial overlap among them (F).  Everything is bit for bit -- the radiance against the other entries `==` as
numbers, a NaN equals a NaN -- with equal segment counts; every state is compared."""
import ctypes as C

import numpy as np
import pytest

import hit_reference as HR
import path_reference as P
import query_rays as Q
import ray_color_reference as RC

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65, 1000)  # a lone lane; a wave short of, at and past 64; a last workgroup that is partly filled
STEPS = (1, 3, 64)


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


def _graph_with_wrappers_and_a_medium():
    for k in range(Q.N_GRAPHS):
        has = Q.scene_pair(f"graph{k}")[1].census()[0]
        if has["media"] > 0 and has["translates"] + has["rotates"] > 0:
            return f"graph{k}"
    raise AssertionError("no random graph with wrappers and a medium")


def _scene(rt, name):
    return Q.scene_pair(_graph_with_wrappers_and_a_medium())[0] if name == "graph" else rt.Scene.reference(name, build_seed=1, aspect_ratio=1.5)


def _states(rt, sc, n):
    """n fresh states: camera rays at their stream positions in front, incoherent bounce rays with made-up positions behind them, some
    rays that are not finite, some states dead on arrival"""
    cam, cam_word = RC.camera_list(rt, sc, 40, 25, 3, 2)
    half = n // 2
    rays = np.concatenate([cam[:half], RC.bounce_rays(rt, sc, n - half)])
    word = np.concatenate([cam_word[:half], (np.arange(n - half, dtype=np.uint32) * 7) % 29])
    s = P.fresh(rt, rays, 0, 3, word, 50)
    s["stream"][half:] += 5000
    s["ray"][9::16, 4] = -np.inf
    s["status"][13::32] = 0x300  # dead, with an event
    return s


# ---------------------------------------------------------------------------------------------------------------- D --

@pytest.mark.parametrize("name", [5, 6, 0, 7, "graph"])
def test_kernels_equal_the_twin(rt, gpu_ctx_factory, dev, name):
    """n in COUNTS, steps in STEPS, every variant that covers the scene: the host entry and the device entry, out of place and in place,
    give the twin's 128 bytes per state, its out_node and its segments."""
    sc = _scene(rt, name)
    ctx = gpu_ctx_factory(sc)
    all_states = _states(rt, sc, max(COUNTS))
    for n in COUNTS:
        s0 = all_states[:n]
        d_in = _to_device(dev, s0)
        for steps in STEPS:
            for v in HR.valid_variants(sc.info()):
                tag = (name, n, steps, v)
                want, wnode, wst = rt.path_step_host(sc, s0, steps, global_seed=2, variant=v, with_stats=True)
                got, node, st = ctx.path_step(s0, steps, global_seed=2, variant=v, with_stats=True)
                assert P.same_states(got, want), (tag, "host entry", P.first_difference(got, want))
                assert np.array_equal(node, wnode), (tag, "host entry: out_node")
                assert st["segments"] == wst["segments"] and st["paths"] == n and st["variant"] == v and st["block"] == 256 and st["grid"] == (n + 255) // 256, (tag, st)
                d_out, d_node = _to_device(dev, np.zeros(n, dtype=rt.PATH_STATE)), _to_device(dev, np.zeros(n, dtype=np.uint32))
                dst = ctx.path_step_device(d_in, d_out, d_node, n, steps, global_seed=2, variant=v)
                assert P.same_states(dev.download(d_out, (n,), rt.PATH_STATE), want), (tag, "device entry")
                assert np.array_equal(dev.download(d_node, (n,), np.uint32), wnode) and dst["segments"] == wst["segments"], (tag, "device entry")
                assert P.same_states(dev.download(d_in, (n,), rt.PATH_STATE), s0), (tag, "the input is only read")
                d_place = _to_device(dev, s0)
                ctx.path_step_device(d_place, d_place, None, n, steps, global_seed=2, variant=v)
                assert P.same_states(dev.download(d_place, (n,), rt.PATH_STATE), want), (tag, "in place")
        dev.free()
    ctx.close()


def test_device_entry_writes_its_states_only(rt, gpu_ctx_factory, dev):
    """d_out and d_out_node inside larger buffers filled with a sentinel: nothing outside [n] is written"""
    sc = _scene(rt, 6)
    ctx = gpu_ctx_factory(sc)
    for n in (1, 65, 257):
        s0 = _states(rt, sc, n)
        big = np.full((n + 8) * 16, -12345.0)
        nodes = np.full(n + 64, 0xDEADBEEF, dtype=np.uint32)
        d_big, d_nodes = _to_device(dev, big), _to_device(dev, nodes)
        ctx.path_step_device(_to_device(dev, s0), d_big + 4 * 128, d_nodes + 32 * 4, n, 3, global_seed=2)
        out = dev.download(d_big, (n + 8, 16), np.float64)
        nd = dev.download(d_nodes, (n + 64,), np.uint32)
        want, wnode = rt.path_step_host(sc, s0, 3, global_seed=2)
        assert np.all(out[:4] == -12345.0) and np.all(out[n + 4:] == -12345.0) and P.same_states(out[4:n + 4].copy().view(rt.PATH_STATE).reshape(-1), want)
        assert np.all(nd[:32] == 0xDEADBEEF) and np.all(nd[n + 32:] == 0xDEADBEEF) and np.array_equal(nd[32:n + 32], wnode)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- A --

def test_split_order_and_compaction_on_the_device(rt, gpu_ctx_factory):
    """torch tensors [n, 16] taken by pointer and advanced in place: 64 levels in one call; in 64 calls; as 3 + 61; shuffled and compacted
    by torch between calls and matched back by stream; cut into two calls -- the same 128 bytes for every state, the twin's.  (Most of
    this test's time is torch bringing up its own device context, once per process; the calls themselves take milliseconds.)"""
    import torch
    sc = _scene(rt, 5)
    ctx = gpu_ctx_factory(sc)
    s0 = _states(rt, sc, 1000)
    s0["stream"] = np.arange(1000, dtype=np.uint64) + 100  # distinct keys
    want, _ = rt.path_step_host(sc, s0, 64, global_seed=2)

    def tensor(s):
        return torch.from_numpy(np.ascontiguousarray(s).view(np.float64).reshape(-1, 16).copy()).cuda()

    def states(t):
        return t.cpu().numpy().copy().view(rt.PATH_STATE).reshape(-1)
    one = tensor(s0)
    st = ctx.path_step(one, 64, global_seed=2, device=True)
    assert P.same_states(states(one), want) and st["paths"] == 1000
    t = tensor(s0)
    for _ in range(64):
        ctx.path_step(t, 1, global_seed=2, device=True)
    assert P.same_states(states(t), want)
    t = tensor(s0)
    ctx.path_step(t, 3, global_seed=2, device=True)
    ctx.path_step(t, 61, global_seed=2, device=True)
    assert P.same_states(states(t), want)
    g = torch.Generator(device="cpu").manual_seed(4)
    live, done = tensor(s0), []
    for _ in range(64):
        live = live[torch.randperm(live.shape[0], generator=g).cuda()].contiguous()
        ctx.path_step(live, 1, global_seed=2, device=True)
        is_alive = (live[:, 15].view(torch.int64) >> 32) & 1 == 1  # status: the high word of the last double
        done.append(states(live[~is_alive]))
        live = live[is_alive].contiguous()
        if live.shape[0] == 0:
            break
    assert live.shape[0] == 0
    done = np.concatenate(done)
    assert P.same_states(done[np.argsort(done["stream"])], want)
    lo, hi = tensor(s0[:300]), tensor(s0[300:])
    ctx.path_step(lo, 64, global_seed=2, device=True)
    ctx.path_step(hi, 64, global_seed=2, device=True)
    assert P.same_states(np.concatenate([states(lo), states(hi)]), want)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- B --

@pytest.mark.parametrize("arm", [5, 7])
def test_carried_to_its_end_it_is_ray_color_device(rt, gpu_ctx_factory, dev, arm):
    """1000 rays -- the continuation set of the arm, filled up from its generic set -- with drawn start words: fresh states advanced by
    max_depth + 1 levels hold rt1w_ray_color_device's raw sums of that sample (`==`, a NaN equals a NaN), and the levels that traced a
    ray are its segments; samples 0 and 7, max_depth 1, 2 and 50."""
    name = f"arm{arm}"
    sc = Q.scene_pair(name)[0]
    ctx = gpu_ctx_factory(sc)
    sets = Q.sets(name)
    rays = np.ascontiguousarray(np.concatenate([sets.rays["continuation"], sets.rays["generic"]])[:1000, :7])
    word = np.random.default_rng(5).integers(0, 41, size=1000).astype(np.uint32)
    d_rays, d_word = _to_device(dev, rays), _to_device(dev, word)
    for sample in (0, 7):
        for depth in (1, 2, 50):
            d_rgb = _to_device(dev, np.full((1000, 3), -1.0))
            rst = ctx.ray_color_device(d_rays, d_rgb, 1000, d_word, spp=1, sample_offset=sample, first_stream=Q.FIRST_STREAM, global_seed=3, max_depth=depth,
                                       out_sum=True)
            want = dev.download(d_rgb, (1000, 3), np.float64)
            d_s = _to_device(dev, P.fresh(rt, rays, Q.FIRST_STREAM, sample, word, depth))
            st = ctx.path_step_device(d_s, d_s, None, 1000, depth + 1, global_seed=3)
            end = dev.download(d_s, (1000,), rt.PATH_STATE)
            assert not P.alive(end).any()
            assert P.radiance_equal(end["radiance"], want), (arm, sample, depth, int((end["radiance"] != want).any(axis=1).sum()))
            assert st["segments"] == rst["segments"], (arm, sample, depth, st["segments"], rst["segments"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- C --

CAMERA = ((300.0, 250.0, -700.0), (270.0, 280.0, 0.0), (0.0, 1.0, 0.0), 35.0, 4.0 / 3.0, 0.5, 600.0, 0.0, 1.0)


@pytest.mark.parametrize("arm", [0, 5, 6])
def test_from_the_camera_it_is_render_device(rt, gpu_ctx_factory, dev, arm):
    """rt1w_path_begin_device + levels to the end against rt1w_render_device(spp 1, sample_offset s, chunk 1, RT1W_OUT_SUM) of the same
    32 x 24 pixels, s in {0, 7}; then again after rt1w_context_set_camera.  The begin kernel's states are the begin twin's bits (the
    twin sees the moved camera through rt1w_lab_scene_set_camera)."""
    w, h = 32, 24
    sc = rt.Scene.reference(arm, build_seed=1, aspect_ratio=4.0 / 3.0)
    ctx = gpu_ctx_factory(sc)
    for moved in (False, True):
        if moved:
            ctx.set_camera(*CAMERA)
            rt.scene_set_camera_host(sc, *CAMERA)
        for s in (0, 7):
            px = np.array([[i, j, s] for j in range(h) for i in range(w)], dtype=np.uint32)
            d_s = _to_device(dev, np.zeros(len(px), dtype=rt.PATH_STATE))
            bst = ctx.path_begin_device(_to_device(dev, px), d_s, len(px), w, h, global_seed=2, max_depth=50)
            begun = dev.download(d_s, (len(px),), rt.PATH_STATE)
            assert P.same_states(begun, rt.path_begin_host(sc, w, h, px, global_seed=2, max_depth=50)) and bst["paths"] == len(px)
            assert P.same_states(ctx.path_begin(w, h, px, global_seed=2, max_depth=50), begun)
            st = ctx.path_step_device(d_s, d_s, None, len(px), 51, global_seed=2)
            end = dev.download(d_s, (len(px),), rt.PATH_STATE)
            d_img = _to_device(dev, np.full((h, w, 3), -2.0))
            rst = ctx.render_device(d_img, w, h, 1, sample_offset=s, global_seed=2, chunk=1, out_sum=True)
            img = dev.download(d_img, (h, w, 3), np.float64)
            assert not P.alive(end).any()
            assert P.radiance_equal(end["radiance"].reshape(h, w, 3), img), (arm, moved, s, int((end["radiance"].reshape(h, w, 3) != img).any(axis=2).sum()))
            assert st["segments"] == rst["segments"], (arm, moved, s, st["segments"], rst["segments"])
        dev.free()
    ctx.close()


def test_begin_on_tensors(rt, gpu_ctx_factory):
    import torch
    sc = _scene(rt, 5)
    ctx = gpu_ctx_factory(sc)
    px = np.array([[i, j, 3] for j in range(5) for i in range(13)], dtype=np.int32)
    t = ctx.path_begin(13, 5, torch.from_numpy(px).cuda(), global_seed=1, max_depth=9, device=True)
    assert P.same_states(t.cpu().numpy().copy().view(rt.PATH_STATE).reshape(-1), rt.path_begin_host(sc, 13, 5, px, global_seed=1, max_depth=9))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- F --

def test_refusals_on_the_entries(rt, gpu_ctx_factory, dev):
    """Every RT1W_ERR_INVALID through rt1w_path_step (host buffers) and rt1w_path_step_device (device buffers); on the device also a
    state pointer that is not 16-byte aligned; the begin entries' refusals, a pixel outside the frame among them (seen by the lanes).
    Unknown status bits come back 0 and a dead state comes back unchanged through the kernels: test_kernels_equal_the_twin's lists hold
    both, test_path_step.py holds the twin to it."""
    sc = _scene(rt, 6)
    ctx = gpu_ctx_factory(sc)
    n = 8
    s0 = _states(rt, sc, n)
    h_in, h_out, h_node = np.zeros(n + 2, dtype=rt.PATH_STATE), np.zeros(n + 2, dtype=rt.PATH_STATE), np.zeros(n * 40, dtype=np.uint32)
    h_in[:n] = s0
    P.step_refusals(rt, lambda p, a, b, c: rt._lib.rt1w_path_step(ctx._h, None if p is None else C.byref(p), a, b, c, None),
                  h_in.ctypes.data, h_out.ctypes.data, h_node.ctypes.data, n)
    d_in, d_out, d_node = _to_device(dev, h_in), _to_device(dev, h_out), _to_device(dev, h_node)

    def device_call(p, a, b, c):
        return rt._lib.rt1w_path_step_device(ctx._h, None if p is None else C.byref(p), a, b, c, None)
    P.step_refusals(rt, device_call, d_in, d_out, d_node, n)
    p = rt.PathParams(n, 0, 1, 0, (C.c_uint32 * 2)(0, 0))
    for a, b in ((d_in + 8, d_out), (d_in, d_out + 8), (d_in + 4, d_in + 4)):
        assert device_call(p, a, b, None) == rt.ERR_INVALID and "aligned" in rt.last_error()
    px = np.array([[0, 0, 0], [3, 2, 1], [4, 0, 0]], dtype=np.uint32)
    with pytest.raises(rt.Rt1wError) as e:
        ctx.path_begin(4, 4, px)
    assert e.value.code == rt.ERR_INVALID and "outside the frame" in str(e.value)
    d_px, d_s = _to_device(dev, px), _to_device(dev, np.zeros(3, dtype=rt.PATH_STATE))
    for args in ((1, 4, 0, d_px, 3, d_s), (4, 4, 1 << 32, d_px, 3, d_s), (4, 4, 0, d_px, 0, d_s), (4, 4, 0, None, 3, d_s), (4, 4, 0, d_px, 3, None),
                 (4, 4, 0, d_px, 3, d_s + 8), (4, 4, 0, d_px, 3, d_s)):
        rc = rt._lib.rt1w_path_begin_device(ctx._h, args[0], args[1], args[2], 50, args[3], args[4], args[5], None)
        assert rc == rt.ERR_INVALID, args
    begun = dev.download(d_s, (3,), rt.PATH_STATE)
    assert np.all(begun["status"][:2] == P.ALIVE) and np.all(begun[2:].view(np.uint8) == 0), "the entry outside the frame, and it alone, is zeros"
    assert rt._lib.rt1w_path_begin_device(ctx._h, 5, 4, 0, 50, d_px, 3, d_s, None) == rt.OK
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the tool --

def test_cli_trace_path_ends_on_the_render_sample(rt, gpu_ctx_factory):
    """rt1w --scene 5 --trace-path I J S prints one Cornell path level by level (n = 1, steps = 1 per call); %.17g round-trips a double,
    so its last radiance line is that pixel sample of rt1w_render (spp 1, sample_offset S, RT1W_OUT_SUM) as numbers, and there are as
    many levels as the events say."""
    import os
    import subprocess
    tool = os.path.join(os.path.dirname(rt.LIB_PATH), "rt1w")
    ctx = gpu_ctx_factory(rt.Scene.reference(5, build_seed=1, aspect_ratio=1.0))
    for i, j, s in ((20, 30, 2), (32, 60, 0), (5, 3, 7)):
        out = subprocess.run([tool, "--scene", "5", "--width", "64", "--height", "64", "--seed", "3", "--trace-path", str(i), str(j), str(s)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert lines[0] == f"pixel {i} {j} sample {s} stream {j * 64 + i}" and lines[1] == "level 0: camera"
        levels = [l for l in lines if l.startswith("level ")]
        assert levels[-1].endswith(", the path ends") and not any(l.endswith(", the path ends") for l in levels[:-1]) and len(levels) >= 2
        last = [float(x) for x in [l for l in lines if l.startswith("  radiance ")][-1].split()[1:]]
        img, _ = ctx.render(64, 64, 1, sample_offset=s, global_seed=3, chunk=1, out_sum=True)
        assert P.radiance_equal(np.array(last), img[j, i]), (i, j, s, last, img[j, i].tolist())
    ctx.close()
