"""Helpers of tests/test_path_step.py and tests/test_path_step_gpu.py: fresh path states from a ray list, the loop that carries states to
their end one level at a time on the states still alive (and counts the levels that traced a ray, per state), comparisons of whole
records.  Nothing of csrc/ is in the formulas.  Test infrastructure."""
import ctypes as C

import numpy as np

ALIVE, TRACED = 1, 2
EV_NONE, EV_MISS, EV_DEPTH, EV_LIGHT, EV_ABSORBED, EV_LAMBERTIAN, EV_METAL, EV_DIELECTRIC, EV_ISOTROPIC, EV_UNTRACED = range(10)
NO_NODE = 0xFFFFFFFF


def fresh(rt, rays, first_stream, sample, words, max_depth):
    """the state of ray r of a list, as the issue of rt1w_path_step states it: beta 1, radiance 0, stream first_stream + r, the sample,
    word start_word[r] (None: 0), depth_left = max_depth, status ALIVE"""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    s = np.zeros(len(r), dtype=rt.PATH_STATE)
    s["ray"] = r[:, :7]
    s["beta"] = 1.0
    s["stream"] = first_stream + np.arange(len(r), dtype=np.uint64)
    s["sample"] = sample
    s["word"] = 0 if words is None else words
    s["depth_left"] = max_depth
    s["status"] = ALIVE
    return s


def event(states):
    return (states["status"] >> 8) & 0xFF


def alive(states):
    return (states["status"] & ALIVE) != 0


def same_states(a, b):
    """all 128 bytes of every state"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def first_difference(a, b):
    bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
    return (int(bad[0]), int(len(bad)), a[bad[0]], b[bad[0]]) if len(bad) else None


def run_counted(step, states, max_levels):
    """`step(states, 1)` -> (states, nodes) over the states that are still alive, level after level, the dead ones dropped from the call
    and put back by position: (final states, uint32 [n] = levels of each state that traced a ray -- those taken with depth left on a ray
    that is traced).  max_levels bounds the loop; every state must be dead by then."""
    s = states.copy()
    levels = np.zeros(len(s), dtype=np.uint32)
    for _ in range(max_levels):
        idx = np.flatnonzero(alive(s))
        if not len(idx):
            break
        before = s[idx]
        after, _ = step(before, 1)
        levels[idx] += ((before["depth_left"] != 0) & (event(after) != EV_UNTRACED)).astype(np.uint32)
        s[idx] = after
    assert not alive(s).any(), "a state outlived max_levels"
    return s, levels


def radiance_equal(got, want):
    """as numbers: ==, a NaN equals a NaN (a -0.0 equals a +0.0)"""
    return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def step_refusals(rt, call, base_in, base_out, base_node, n):
    """every RT1W_ERR_INVALID of rt1w_path_step through call(params or None, in, out, out_node) -> code, buffers at the given addresses"""
    def params(**kw):
        d = dict(n=n, global_seed=0, steps=1, flags=0, reserved=(0, 0))
        d.update(kw)
        return rt.PathParams(d["n"], d["global_seed"], d["steps"], d["flags"], (C.c_uint32 * 2)(*d["reserved"]))
    cases = [("null params", None, base_in, base_out, base_node), ("null in", params(), None, base_out, base_node),
             ("null out", params(), base_in, None, base_node), ("n = 0", params(n=0), base_in, base_out, base_node),
             ("n = 2^32", params(n=1 << 32), base_in, base_out, base_node), ("steps = 0", params(steps=0), base_in, base_out, base_node),
             ("steps = 65537", params(steps=65537), base_in, base_out, base_node),
             ("global_seed = 2^32", params(global_seed=1 << 32), base_in, base_out, base_node),
             ("flag 1", params(flags=1), base_in, base_out, base_node), ("flag 2^20", params(flags=1 << 20), base_in, base_out, base_node),
             ("variant 9", params(flags=10 << 8), base_in, base_out, base_node),
             ("reserved[0]", params(reserved=(1, 0)), base_in, base_out, base_node), ("reserved[1]", params(reserved=(0, 1)), base_in, base_out, base_node),
             ("out 128 bytes into in", params(), base_in, base_in + 128, base_node), ("in 128 bytes into out", params(), base_out + 128, base_out, base_node),
             ("out_node in the states", params(), base_in, base_out, base_in + 64), ("states in out_node", params(), base_in, base_node, base_node)]
    for what, p, a, b, c in cases:
        assert call(p, a, b, c) == rt.ERR_INVALID, what
        assert rt.last_error() != "", what
    for what, p in (("steps = 65536", params(steps=65536)), ("global_seed = 2^32 - 1", params(global_seed=(1 << 32) - 1)), ("no out_node", params())):
        assert call(p, base_in, base_out, None if what == "no out_node" else base_node) == rt.OK, (what, rt.last_error())
    assert call(params(), base_in, base_in, base_node) == rt.OK, "in == out is allowed"
