"""A list of tiles in one launch, CPU tier (include/rt1w.h: rt1w_tile, rt1w_render_tiles, rt1w_accum_merge_tiles, RT1W_ADAPTIVE_ONE_LAUNCH): the
ABI surface, the plan's flag on rt1w_adaptive_select, and the CPU twin of the list merge (librt1w_lab.so: rt1w_lab_accum_merge_tiles_host, the
kernel's own rt_adaptive.h built for the host) against the sequence of rectangle merges it must equal bit for bit.  The GPU tier is
tests/test_render_tiles_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc

ROOT = orc.ROOT
NEW = ("rt1w_render_tiles", "rt1w_render_tiles_device", "rt1w_accum_merge_tiles", "rt1w_accum_merge_tiles_device")

# the merge case: 72 x 40 with tile 16 is a 5 x 3 grid of tiles whose right column is 8 pixels wide and whose top row is 8 high
W, H, T = 72, 40, 16
# out of row order: the corner tile, a right-edge tile, a top-edge tile, interior tiles
LIST = [(64, 32), (16, 16), (64, 0), (0, 32), (48, 16), (0, 0), (32, 32)]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _clip(x0, y0):
    return min(T, W - x0), min(T, H - y0)


def _case(seed=7):
    g = np.random.default_rng(seed)
    aov = np.empty((H, W, 8))
    aov[..., 0:3] = g.uniform(0.0, 1.0, (H, W, 3))      # albedos on both sides of the floor
    aov[..., 3:6] = (0.0, 0.6, 0.8)
    aov[..., 6] = 3.0
    aov[..., 7] = 1.0
    batches = [g.uniform(0.0, 4.0, (len(LIST), T, T, 3)) for _ in range(3)]
    batches[1][1, 5, 9, 1] = np.nan                       # tile (16, 16), pixel (25, 21): no estimate from here on
    batches[0][0, 12, 3] = 1e300                          # beyond the corner tile's 8 x 8 pixels: must never be read
    return aov, batches


def test_abi_surface(rt):
    lib = C.CDLL(rt.LIB_PATH)
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = md[md.index("## 2."):md.index("## 3.")]
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"pub fn " + name + r"\(", block), name
    assert "pub struct rt1w_tile" in block
    assert C.sizeof(rt.Tile) == 16 and [f[0] for f in rt.Tile._fields_] == ["x0", "y0", "sample_offset", "reserved"]
    assert rt.ADAPTIVE_ONE_LAUNCH == 0x100
    assert rt.adaptive_params(one_launch=True).flags == 0x100 and rt.adaptive_params(one_launch=True, keep_albedo=True).flags == 0x101
    assert lib.rt1w_abi_sizeof(5) == 0                    # the record gets no index of its own
    assert hasattr(C.CDLL(os.path.join(os.path.dirname(rt.LIB_PATH), "librt1w_lab.so")), "rt1w_lab_accum_merge_tiles_host")


def test_select_accepts_the_flag_and_ignores_it(rt):
    base = dict(tile=16, batch_spp=2, pilot_batches=2, budget_spp=64, max_spp=64)
    err = np.array([[1.0, 5.0, 3.0, 5.0], [0.5, 9.0, 0.0, 3.0], [2.0, 2.0, 7.0, 1.0]])
    m = np.full((3, 4), 2, dtype=np.uint32)
    for share in (1.0, 0.25, 0.01):
        plain = rt.adaptive_select(64, 48, err, m, round_share=share, **base)
        assert plain and rt.adaptive_select(64, 48, err, m, round_share=share, one_launch=True, **base) == plain
        assert rt.adaptive_select(64, 48, err, m, round_share=share, one_launch=True, keep_albedo=True, **base) == plain
    for flags in (2, 0x200, 0x102):
        with pytest.raises(rt.Rt1wError) as e:
            rt.adaptive_select(64, 48, err, m, flags=flags, **base)
        assert e.value.code == rt.ERR_INVALID


@pytest.mark.parametrize("keep", [False, True])
def test_merge_twin_equals_the_rectangle_merges(rt, keep):
    """rt1w_lab_accum_merge_tiles_host == rt1w_lab_accum_merge_host on each tile's clipped rectangle, one after the other, bit for bit: over
    three batches (the second with a NaN pixel, whose RT1W_ACCUM_NO_ESTIMATE carries into the third), in list order and in reverse."""
    aov, batches = _case()
    acc_l = acc_r = np.zeros((H, W, 8))
    for b, sums in enumerate(batches):
        order = range(len(LIST)) if b % 2 == 0 else reversed(range(len(LIST)))
        for k in order:
            (x0, y0), (tw, th) = LIST[k], _clip(*LIST[k])
            acc_r = rt.accum_merge_host(acc_r, np.ascontiguousarray(sums[k, :th, :tw]), aov, 2, x0=x0, y0=y0, keep_albedo=keep)
        acc_l = rt.accum_merge_tiles_host(acc_l, sums, aov, 2, T, LIST, keep_albedo=keep)
        assert _same(acc_l, acc_r), (keep, b)
    assert acc_l[21, 25, 5] == acc_l[21, 25, 7] == rt.ACCUM_NO_ESTIMATE and acc_l[21, 25, 3] == 3.0
    touched = np.zeros((H, W), dtype=bool)
    for x0, y0 in LIST:
        touched[y0:y0 + T, x0:x0 + T] = True
    assert np.all(acc_l[touched][:, 3] == 3.0) and np.all(acc_l[~touched] == 0.0) and np.all(np.isfinite(acc_l[..., 0:3][touched]) | (acc_l[..., 3][touched][:, None] == 3.0))
    assert np.isfinite(acc_l[39, 71]).all() and acc_l[..., 0].max() < 100.0                   # the 1e300 beyond the edge was not read
    # sample_offset is ignored here
    with_offsets = [(x0, y0, 5 * k) for k, (x0, y0) in enumerate(LIST)]
    assert _same(rt.accum_merge_tiles_host(np.zeros((H, W, 8)), batches[0], aov, 2, T, with_offsets, keep_albedo=keep),
                 rt.accum_merge_tiles_host(np.zeros((H, W, 8)), batches[0], aov, 2, T, LIST, keep_albedo=keep))


def test_merge_twin_refusals(rt):
    aov, batches = _case()
    zero = np.zeros((H, W, 8))

    def refused(tiles, tile=T, sums=None):
        n = len(tiles)
        s = np.zeros((n, tile, tile, 3)) if sums is None else sums
        with pytest.raises(rt.Rt1wError) as e:
            rt.accum_merge_tiles_host(zero, s, aov, 2, tile, tiles)
        assert e.value.code == rt.ERR_INVALID, (tiles, tile)

    refused([(0, 0), (16, 0), (0, 0)])            # a tile named twice
    refused([(0, 0, 0), (0, 0, 8)])               # ... whatever its sample offset
    refused([(8, 0)])                             # x0 not a multiple of the tile
    refused([(0, 24)])                            # y0 not a multiple of the tile
    refused([(80, 0)])                            # outside the frame
    refused([(0, 48)])
    refused([(0, 0, 0, 1)])                       # reserved
    refused([(0, 0)], tile=24)                    # tile not a multiple of 16
    refused([(0, 0)], tile=8)
    refused([(0, 0)], tile=272)
    refused([])                                   # an empty list
    assert _same(rt.accum_merge_tiles_host(zero, batches[0][:1], aov, 2, T, LIST[:1])[32:, 64:], rt.accum_merge_host(
        zero, np.ascontiguousarray(batches[0][0, :8, :8]), aov, 2, x0=64, y0=32)[32:, 64:])   # n_tiles = 1 works
