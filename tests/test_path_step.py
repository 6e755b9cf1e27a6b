"""Path states (rt1w_path_step, rt1w_path_begin, include/rt1w.h; csrc/rt_path_state.h): ray_color one level at a time -- CPU tier.

The CPU twins (librt1w_lab.so: rt1w_lab_path_step_host, rt1w_lab_path_begin_host; rt_path_state.h and rt_core.h built for the host):
split, order and compaction of a list change no bit (A); carried to its end a state holds rt.ray_color_host's radiance and segments on
the radiance sets of tests/query_rays.py (B); begun at the camera it holds the CPU core's render (C); level by level its ray is the
literal oracle's next segment (E); refusals, unknown status bits, dead states (F).  The GPU tier (test_path_step_gpu.py) holds the
kernels to these twins, bit for bit.

Bounds.  A, B, C, F: bits, or `==` on the radiance as numbers (a NaN equals a NaN), as the issue of these entries states.  E: the
project's bound for product against literal, 1e-12 -- points through query_rays.check_hit's scaling, directions relative to |d|."""
import ctypes as C

import numpy as np
import pytest

import hit_reference as HR
import orc
import path_reference as P
import query_rays as Q
import ray_color_reference as RC

W, H = RC.W, RC.H
_SCENES = {}


def _arm(rt, arm):
    if arm not in _SCENES:
        _SCENES[arm] = rt.Scene.reference(arm, build_seed=1, aspect_ratio=1.5)
    return _SCENES[arm]


def _mixed_states(rt, sc, n, max_depth=50):
    """n fresh states on incoherent rays with drawn start words, one in sixteen of them on a ray that is not finite"""
    rays = RC.bounce_rays(rt, sc, n)
    rays[5::16, 3] = np.inf
    rays[11::32, 6] = np.nan
    words = (np.arange(n, dtype=np.uint32) * 7) % 23
    return P.fresh(rt, rays, 900, 3, words, max_depth)


# ---------------------------------------------------------------------------------------------------------------- A --

@pytest.mark.parametrize("name", ["arm5", "arm6", "graph0"])
def test_split_order_and_compaction_change_no_bit(rt, name):
    """64 levels in one call; in 64 calls; as 3 + 61; with the list shuffled and its dead states dropped between calls, matched back by
    (stream, sample); with the list cut into two calls: the same 128 bytes for every state."""
    sc = Q.scene_pair(name)[0]
    s0 = _mixed_states(rt, sc, 257)

    def step(s, k):
        return rt.path_step_host(sc, s, k, global_seed=9)
    one, node = step(s0, 64)
    assert not P.alive(one).any() and (P.event(one) == P.EV_UNTRACED).sum() >= 16
    s = s0
    for _ in range(64):
        s, last = step(s, 1)
    assert P.same_states(s, one), P.first_difference(s, one)
    a, _ = step(s0, 3)
    assert P.alive(a).any()
    b, _ = step(a, 61)
    assert P.same_states(b, one), P.first_difference(b, one)
    g = np.random.default_rng(4)
    done, live = [], s0
    for _ in range(64):
        live = live[g.permutation(len(live))]
        live, _ = step(live, 1)
        done.append(live[~P.alive(live)])
        live = live[P.alive(live)]
        if not len(live):
            break
    assert not len(live)
    done = np.concatenate(done)
    assert len(done) == len(one)
    order = np.argsort(done["stream"])  # one sample: the streams are the key
    assert np.array_equal(done["stream"][order], one["stream"]) and P.same_states(done[order], one)
    lo, n_lo = step(s0[:100], 64)
    hi, n_hi = step(s0[100:], 64)
    assert P.same_states(np.concatenate([lo, hi]), one) and np.array_equal(np.concatenate([n_lo, n_hi]), node)
    inplace = s0.copy()  # in == out through the twin itself
    p = rt.PathParams(len(inplace), 9, 64, 0, (C.c_uint32 * 2)(0, 0))
    assert rt.load_lab().rt1w_lab_path_step_host(sc._h, C.byref(p), inplace.ctypes.data, inplace.ctypes.data, None, None) == rt.OK
    assert P.same_states(inplace, one)


# ---------------------------------------------------------------------------------------------------------------- B --

@pytest.mark.parametrize("name", Q.scene_names())
def test_carried_to_its_end_a_state_is_ray_color(rt, name):
    """A fresh state of ray r, advanced until it is dead (max_depth + 1 levels suffice), holds rt.ray_color_host's raw sum of that sample
    (`==`; a NaN equals a NaN) and took as many traced levels as that ray has segments: the generic, continuation and axis-parallel sets
    (zero, denormal and huge rays among them), with the non-finite rays of the refusal table appended so that event 9 is exercised;
    samples 0 and 7; start words none and drawn; max_depth 1, 2 and 50; every variant that covers the scene.  The level counts come from
    single levels on the states still alive, the radiance from that loop and from one call of max_depth + 1 levels, which agree in
    every byte."""
    prod, _ = Q.scene_pair(name)
    bad_rays, bad = RC.nonfinite_lists()
    variants = HR.valid_variants(prod.info())
    for which in Q.RADIANCE_SETS:
        rays = np.concatenate([Q.sets(name).rays[which][:, :7], bad_rays])
        for sample in Q.SAMPLES:
            for word in (None, np.concatenate([Q.start_words(name, which, len(rays) - len(bad_rays)), np.arange(len(bad_rays), dtype=np.uint32)])):
                for depth in Q.DEPTHS:
                    want, st = rt.ray_color_host(prod, rays, word, spp=1, sample_offset=sample, first_stream=Q.FIRST_STREAM, global_seed=3,
                                                 max_depth=depth, out_sum=True, with_stats=True)
                    s0 = P.fresh(rt, rays, Q.FIRST_STREAM, sample, word, depth)
                    tag = (name, which, sample, word is not None, depth)
                    for v in variants:
                        one, _, stats = rt.path_step_host(prod, s0, depth + 1, global_seed=3, variant=v, with_stats=True)
                        assert not P.alive(one).any(), tag
                        assert P.radiance_equal(one["radiance"], want), tag + (v,)
                        assert stats["segments"] == st["segments"], tag + (v, stats["segments"], st["segments"])
                    end, levels = P.run_counted(lambda s, k: rt.path_step_host(prod, s, k, global_seed=3), s0, depth + 1)
                    assert P.same_states(end, rt.path_step_host(prod, s0, depth + 1, global_seed=3)[0]), tag
                    assert np.array_equal(levels, st["ray_segments"]), tag + (int((levels != st["ray_segments"]).sum()),)
                    untraced = P.event(end) == P.EV_UNTRACED
                    assert np.array_equal(untraced[-len(bad):], bad) and not untraced[:-len(bad)].any(), tag


# ---------------------------------------------------------------------------------------------------------------- C --

@pytest.mark.parametrize("arm", range(8))
def test_from_the_camera_it_is_the_render(rt, arm):
    """path_begin + levels to the end equals the CPU build of the core: the raw sums of spp 1, sample_offset s, chunk 1 of the same
    pixels at 24 x 16, s in {0, 7}, bit for bit as numbers, with equal segments; and the begin twin's ray and word are
    rt1w_lab_camera_rays_pos_host's bits."""
    sc = _arm(rt, arm)
    for s in (0, 7):
        px = np.array([[i, j, s] for j in range(H) for i in range(W)], dtype=np.uint32)
        st = rt.path_begin_host(sc, W, H, px, global_seed=2, max_depth=50)
        rays, word = RC.camera_list(rt, sc, W, H, s, 2)
        assert HR.same_bits(st["ray"], rays) and np.array_equal(st["word"], word)
        assert np.all(st["beta"] == 1.0) and np.all(st["radiance"] == 0.0) and np.all(st["status"] == P.ALIVE) and np.all(st["depth_left"] == 50)
        assert np.array_equal(st["stream"], px[:, 1].astype(np.uint64) * W + px[:, 0]) and np.all(st["sample"] == s)
        end, _, stats = rt.path_step_host(sc, st, 51, global_seed=2, with_stats=True)
        want, fs = orc.flat_render(sc, W, H, 1, sample_offset=s, global_seed=2, out_sum=True, chunk=1)
        assert not P.alive(end).any()
        assert P.radiance_equal(end["radiance"].reshape(H, W, 3), want), (arm, s)
        assert stats["segments"] == fs["segments"], (arm, s)
    scattered = px[::-7][:50]  # any order, any subset, a pixel twice
    sub = rt.path_begin_host(sc, W, H, np.concatenate([scattered, scattered[:3]]), global_seed=2, max_depth=50)
    assert P.same_states(sub[:50], st[scattered[:, 1] * W + scattered[:, 0]]) and P.same_states(sub[50:], sub[:3])


# ---------------------------------------------------------------------------------------------------------------- E --

_E_MAX = {"origin": 0.0, "direction": 0.0, "time": 0.0}


@pytest.mark.parametrize("name", Q.scene_names())
def test_level_by_level_against_the_literal_oracle(rt, name):
    """OracleScene.ray_color(.., trace=64) notes every segment's ray of one path.  After level k the state's ray is row k + 1's ray (the
    origin is the hit point); the events agree with the rows' hit flags; the path is as long as the trace.  The first 16 rays of the
    continuation and of the generic set of each scene, max_depth 50.  Bound 1e-12: origins through check_hit's scaling for points (the
    larger of |p|, |origin| and |t * direction| of the segment that made them; the scene's extent under a Translate / RotateY),
    directions relative to |d|, the time relative.

    Largest deviation seen over all 18 scenes (CPU twin, x86-64): 0 for origins, directions and times alike -- on these 576 paths the
    twin's next rays are the oracle's bits -- so the bound stands as it is, for directions too.  The test prints the running maxima."""
    prod, orac = Q.scene_pair(name)
    for which in ("continuation", "generic"):
        rays = Q.sets(name).rays[which][:16, :7]
        rec, _, aux = Q.sets(name).oracle[which]  # check_hit's extent: the largest |p| of the set's finite hits under a wrapper
        under = (rec[:, 0] == 1.0) & Q._wrapped(aux) & np.isfinite(rec[:, 2:5]).all(axis=1)
        extent = max(1.0, float(np.abs(rec[under, 2:5]).max())) if under.any() else 1.0
        for r in range(16):
            col, seg, rows = orac.ray_color(rays[r:r + 1], None, Q.FIRST_STREAM + r, 0, 3, 50, trace=64)
            s = P.fresh(rt, rays[r:r + 1], Q.FIRST_STREAM + r, 0, None, 50)
            taken = 0
            while P.alive(s)[0]:
                before = s.copy()
                s, node = rt.path_step_host(prod, s, 1, global_seed=3)
                ev = int(P.event(s)[0])
                if ev == P.EV_DEPTH:
                    break
                assert taken < len(rows), (name, which, r, "the path is longer than the trace")
                row = rows[taken]
                assert np.array_equal(row[8:15], before["ray"][0]) or taken > 0, (name, which, r)
                assert (ev == P.EV_MISS) == (row[0] == 0.0) and (ev >= P.EV_LIGHT) == (row[0] == 1.0), (name, which, r, taken, ev, row[0])
                assert (node[0] == P.NO_NODE) == (row[0] == 0.0)
                taken += 1
                if P.alive(s)[0] and taken < len(rows):
                    got, nxt = s["ray"][0], rows[taken][8:15]
                    wrapped = (int(row[5]) & (orc.TAG_TRANSLATE | orc.TAG_ROTATE)) != 0
                    with np.errstate(invalid="ignore", over="ignore"):
                        scale = max(float(np.abs(nxt[0:3]).max()), float(np.abs(row[8:11]).max()), float(np.abs(row[1] * row[11:14]).max()))
                    scale = max(scale, extent) if wrapped else scale
                    scale = scale if np.isfinite(scale) else 0.0
                    norm = float(np.sqrt((nxt[3:6] * nxt[3:6]).sum()))
                    with np.errstate(invalid="ignore"):
                        d_o, d_d, d_t = np.abs(got[0:3] - nxt[0:3]), np.abs(got[3:6] - nxt[3:6]), abs(got[6] - nxt[6])
                    if np.isfinite(nxt).all() and scale > 0.0 and norm > 0.0:
                        _E_MAX["origin"] = max(_E_MAX["origin"], float(d_o.max()) / scale)
                        _E_MAX["direction"] = max(_E_MAX["direction"], float(d_d.max()) / norm)
                        _E_MAX["time"] = max(_E_MAX["time"], d_t / max(abs(nxt[6]), 1e-300))
                    assert np.all(Q._agree(got[0:3], nxt[0:3], Q.RTOL * scale)), (name, which, r, taken, "origin", got[0:3], nxt[0:3])
                    assert np.all(Q._agree(got[3:6], nxt[3:6], Q.RTOL * norm)), (name, which, r, taken, "direction", got[3:6], nxt[3:6])
                    assert np.all(Q._agree(got[6], nxt[6], Q.RTOL * abs(nxt[6]))), (name, which, r, taken, "time")
            assert taken == len(rows) == seg[0], (name, which, r, taken, len(rows), int(seg[0]))
            assert np.all(Q._agree(s["radiance"][0], col[0], Q.RTOL * np.abs(col[0]))), (name, which, r)
    print(name, "largest deviations so far:", _E_MAX)


# ---------------------------------------------------------------------------------------------------------------- F --

def _call_step(rt, sc, p, s_in, s_out, node):
    return rt.load_lab().rt1w_lab_path_step_host(sc._h, None if p is None else C.byref(p), s_in, s_out, node, None)


def test_refusals_status_bits_and_dead_states(rt):
    sc = _arm(rt, 6)
    n = 8
    s0 = _mixed_states(rt, sc, n)
    buf_in, buf_out, node = np.zeros(n + 2, dtype=rt.PATH_STATE), np.zeros(n + 2, dtype=rt.PATH_STATE), np.zeros(n * 40, dtype=np.uint32)
    buf_in[:n] = s0
    P.step_refusals(rt, lambda p, a, b, c: _call_step(rt, sc, p, a, b, c), buf_in.ctypes.data, buf_out.ctypes.data, node.ctypes.data, n)
    p = rt.PathParams(n, 0, 1, 0, (C.c_uint32 * 2)(0, 0))
    assert rt.load_lab().rt1w_lab_path_step_host(None, C.byref(p), buf_in.ctypes.data, buf_out.ctypes.data, None, None) == rt.ERR_INVALID
    for fn in (rt._lib.rt1w_path_step, rt._lib.rt1w_path_step_device):
        assert fn(None, C.byref(p), buf_in.ctypes.data, buf_out.ctypes.data, None, None) == rt.ERR_INVALID and rt.last_error() == "null argument"
    for fn in (rt._lib.rt1w_path_begin, rt._lib.rt1w_path_begin_device):
        assert fn(None, 4, 4, 0, 50, node.ctypes.data, 1, buf_out.ctypes.data, None) == rt.ERR_INVALID and rt.last_error() == "null argument"
    assert rt._lib.rt1w_abi_sizeof(11) == rt.PATH_STATE.itemsize == 128 and rt._lib.rt1w_abi_sizeof(10) == C.sizeof(rt.PathParams) == 32
    assert rt._lib.rt1w_abi_sizeof(5) == 0 and rt._lib.rt1w_abi_sizeof(7) == 0 and rt._lib.rt1w_abi_sizeof(9) == 0 and rt._lib.rt1w_abi_sizeof(12) == 0
    # the host form takes any alignment
    raw = np.zeros(n * 128 + 8, dtype=np.uint8)
    odd = raw[3:3 + n * 128].view(rt.PATH_STATE)
    odd[:] = s0
    want, _ = rt.path_step_host(sc, s0, 2)
    assert _call_step(rt, sc, rt.PathParams(n, 0, 2, 0, (C.c_uint32 * 2)(0, 0)), odd.ctypes.data, odd.ctypes.data, None) == rt.OK and P.same_states(odd, want)
    # unknown status bits are ignored and come back 0; a dead state comes back unchanged, every bit of it
    noisy = s0.copy()
    noisy["status"] |= 0xABCD00FC
    got, _ = rt.path_step_host(sc, noisy, 2)
    assert P.same_states(got, want) and np.all((got["status"] & ~np.uint32(0xFF03)) == 0)
    dead = want.copy()
    dead["status"] = (dead["status"] & ~np.uint32(P.ALIVE)) | np.uint32(0x5A000000)
    dead["ray"][:, 1] = np.nan
    back, nd = rt.path_step_host(sc, dead, 5)
    assert P.same_states(back, dead) and np.all(nd == P.NO_NODE)
    # a fresh state with no depth: one level, event 2, radiance + beta * 0, no segment
    zero = P.fresh(rt, RC.bounce_rays(rt, sc, 4), 0, 0, None, 0)
    end, nd, st = rt.path_step_host(sc, zero, 1, with_stats=True)
    assert np.all(P.event(end) == P.EV_DEPTH) and not P.alive(end).any() and np.all(end["radiance"] == 0.0) and st["segments"] == 0 and np.all(nd == P.NO_NODE)
    assert np.all((end["status"] & P.TRACED) != 0)


def test_begin_refusals(rt):
    sc = _arm(rt, 5)
    px = np.array([[0, 0, 0], [3, 2, 1]], dtype=np.uint32)
    for kw, pixels in ((dict(width=1, height=4), px), (dict(width=4, height=1), px), (dict(width=4, height=4, global_seed=1 << 32), px),
                       (dict(width=4, height=4), np.array([[4, 0, 0]], dtype=np.uint32)), (dict(width=4, height=4), np.array([[0, 4, 0]], dtype=np.uint32)),
                       (dict(width=4, height=4), np.zeros((0, 3), dtype=np.uint32))):
        with pytest.raises(rt.Rt1wError) as e:
            rt.path_begin_host(sc, kw["width"], kw["height"], pixels, global_seed=kw.get("global_seed", 0))
        assert e.value.code == rt.ERR_INVALID, kw
    ok = rt.path_begin_host(sc, 4, 3, px, global_seed=(1 << 32) - 1)
    assert np.all(ok["status"] == P.ALIVE) and list(ok["stream"]) == [0, 2 * 4 + 3] and list(ok["sample"]) == [0, 1]
    with pytest.raises(ValueError):
        rt.path_begin_host(sc, 4, 4, np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(ValueError):
        rt.path_step_host(sc, np.zeros((2, 15)))
