"""The feature buffers (rt1w_render_aov, rt1w_render_aov_deep, rt1w_render_aov_tiles) against the literal oracle's own statement of them
(oracle/oracle.cpp: orc_aov, written on the restatement's classes; nothing of csrc/ is in it), on edge scenes built call for call on
both sides (tests/aov_scenes.py), the eight reference arms and six random graphs.  CPU tier: the CPU twin (rt1w_lab_aov_host,
rt1w_lab_aov_deep_host, rt1w_lab_aov_tiles_host) in every variant valid for the scene.  GPU tier: the kernels, directly.  Bit equality of
kernels and twin stays with test_aov.py, test_aov_deep.py and test_guides.py; this is the independent check beside it.

Bounds.  Coverage and the +inf pattern of the depth: equal.  Albedo and depth: 1e-12 relative, the project's bound for product against
literal (test_gpu_parity.py, test_random_scenes.py); both are sums of non-negative terms.  Normal: 1e-12 absolute per component (means of
components of unit vectors; the sums cancel, so a relative bound has no meaning).  Rays traced: equal.  No pixel or sample is left out."""
import numpy as np
import pytest

import aov_scenes

RTOL = 1e-12
NTOL = 1e-12
W, H = 48, 32
# name -> (width, height, spp, tile, sample_offset, global_seed)
FRAMES = {"whole": (W, H, 3, None, 0, 0), "ragged": (W, H, 2, (5, 3, 37, 21), 7, 2), "column": (W, H, 8, (47, 0, 1, 32), 0, 0),
          "2x2": (2, 2, 4, None, 0, 0)}
GPU_FRAMES = ("whole", "ragged", "column")
FIRST = (0, 0.0)  # the first-hit entry: the chain with no bounce followed
DEEP = [(1, 0.0), (4, 0.0), (4, 0.5), (16, 0.5), (64, 1.0)]
GPU_DEEP = [(4, 0.5), (64, 1.0)]
TILE = 16
TILE_LIST = [(0, 0, 0), (32, 16, 5), (16, 0, 1000), (32, 16, 9)]  # one tile twice, with another offset
TILE_SPP, TILE_SEED = 3, 4

_ORACLE = {}


def oracle_frame(name, frame, path):
    """the oracle's buffers and stats of (scene, frame, (max_specular, max_fuzz)): computed once per process"""
    key = (name, frame, path)
    if key not in _ORACLE:
        w, h, spp, tile, so, gs = FRAMES[frame]
        _ORACLE[key] = aov_scenes.scene_pair(name)[1].aov(w, h, spp, tile=tile, sample_offset=so, global_seed=gs, max_specular=path[0], max_fuzz=path[1])
    return _ORACLE[key]


def oracle_tiles(name):
    """the oracle's raw sums of the rectangles of TILE_LIST, [n, 16, 16, 8]"""
    key = (name, "tiles")
    if key not in _ORACLE:
        o = aov_scenes.scene_pair(name)[1]
        _ORACLE[key] = np.stack([o.aov(W, H, TILE_SPP, tile=(x0, y0, TILE, TILE), sample_offset=so, global_seed=TILE_SEED, out_sum=True)[0]
                                 for x0, y0, so in TILE_LIST])
    return _ORACLE[key]


def _valid_variants(info):
    media, tex, ms, sd = info["has_media"], info["has_textures"], info["has_moving"], info["scope_depth"]
    v = [1, 3, 4]
    if not media and not tex and not ms and sd <= 2:
        v.append(0)
    if not media:
        v.append(2)
    if not media and sd == 0:
        v.append(5)
    return sorted(v)


class Worst:
    """the largest differences seen, per channel group"""

    def __init__(self):
        self.albedo = self.normal = self.depth = 0.0

    def __str__(self):
        return f"largest difference: albedo {self.albedo:.3g} relative, normal {self.normal:.3g} absolute, depth {self.depth:.3g} relative"


def _rel(a, o):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - o) / np.abs(o)
    return np.where(a == o, 0.0, r)  # equal (0 against 0 too) is no difference; a value against an oracle 0 is infinite


def compare(got, want, worst, what):
    """`got` (twin or kernel) against `want` (oracle), both in the layout of rt1w_render_aov; every pixel"""
    assert got.shape == want.shape, what
    assert np.array_equal(got[..., 7], want[..., 7]), (what, "coverage")
    inf = np.isinf(want[..., 6])
    assert np.array_equal(np.isinf(got[..., 6]), inf) and not np.isnan(got).any(), (what, "depth +inf pattern")
    assert np.all(got[..., 6][inf] > 0), (what, "depth +inf pattern")
    ra = _rel(got[..., 0:3], want[..., 0:3])
    rd = _rel(got[..., 6][~inf], want[..., 6][~inf])
    dn = np.abs(got[..., 3:6] - want[..., 3:6])
    worst.albedo = max(worst.albedo, float(ra.max()))
    worst.normal = max(worst.normal, float(dn.max()))
    worst.depth = max(worst.depth, float(rd.max()) if rd.size else 0.0)
    assert ra.max() <= RTOL, (what, "albedo", float(ra.max()))
    assert dn.max() <= NTOL, (what, "normal", float(dn.max()))
    assert rd.size == 0 or rd.max() <= RTOL, (what, "depth", float(rd.max()))


def finish_sums(s, spp):
    """raw sums [.., 8] finished as include/rt1w.h states for rt1w_render_aov_tiles: s / spp in 0-5 and 7, s6 / s7 or +inf in 6"""
    out = s / float(spp)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[..., 6] = np.where(s[..., 7] > 0, s[..., 6] / s[..., 7], np.inf)
    return out


def compare_sums(got, want, spp, worst, what):
    assert np.array_equal(got[..., 7], want[..., 7]) and np.all(got[..., 7] == np.round(got[..., 7])), (what, "hit count")
    assert np.all(got[..., 6][got[..., 7] == 0] == 0.0), (what, "distance sum without a hit")
    compare(finish_sums(got, spp), finish_sums(want, spp), worst, what)


# ------------------------------------------------------------------------------------------------------------------ CPU tier --

PERCENT = 0.01  # a case is populated if it holds on 1 % of the frame's pixels or samples


@pytest.mark.parametrize("name", list(aov_scenes.HAND_BUILT))
def test_oracle_frames_contain_their_case(rt, name):
    """From the oracle's frames and counts alone (48 x 32, 3 spp): every hand-built scene shows the case it was built for on at least
    1 % of the frame.  A condition on the inputs; no product code runs here apart from the scene's own build."""
    prod, _ = aov_scenes.scene_pair(name)
    assert prod.info()["n_nodes"] <= 64
    a, st = oracle_frame(name, "whole", FIRST)
    px, samples = W * H * PERCENT, st["paths"] * PERCENT
    alb, nrm, cov = a[..., 0:3], a[..., 3:6], a[..., 7]
    black = np.all(alb == 0.0, axis=-1) & (cov == 1.0)
    partial = (cov > 0.0) & (cov < 1.0)
    assert sum(st["counts"][:3]) == st["paths"] and st["segments"] == st["paths"]

    def facing(n):
        return np.all(nrm == np.array(n), axis=-1)
    if name == "back_of_a_light":
        down = facing((0.0, -1.0, 0.0))
        print("back of the light", int((black & down).sum()), "() rect", int((black & facing((0.0, 0.0, 1.0))).sum()),
              "front under FlipFace", int((down & ~black & (cov == 1.0)).sum()), "partial", int(partial.sum()))
        assert (black & down).sum() >= px, "the back of the light: covered, albedo 0, normal towards the camera"
        assert (black & facing((0.0, 0.0, 1.0))).sum() >= px, "the () rect"
        lit = down & (cov == 1.0) & ~black
        assert lit.sum() >= px and len(np.unique(alb[lit], axis=0)) >= 3, "the FlipFace'd light shows its checker from the front"
        assert partial.sum() >= px
    elif name == "inside_glass":
        assert np.all(cov == 1.0) and np.all(alb == 1.0), "the camera is inside the glass: every first hit is the Dielectric"
        d, sd = oracle_frame(name, "whole", (64, 1.0))
        print("counts at 64 bounces", sd["counts"], "rays", sd["segments"], "partial", int(((d[..., 7] > 0) & (d[..., 7] < 1)).sum()))
        assert sd["counts"][2] >= samples, "chains reflected totally never leave the sphere: still specular after 64 bounces"
        assert sd["counts"][0] >= samples and sd["counts"][1] >= samples
        one, four = oracle_frame(name, "whole", (1, 0.0))[1]["counts"][0], oracle_frame(name, "whole", (4, 0.0))[1]["counts"][0]
        print("chains that end on the wall after at most 1 bounce", one, "after at most 4", four)
        assert four - one >= samples, "more glass between the sphere and the wall: the hollow sphere is in view"
        assert ((d[..., 7] > 0) & (d[..., 7] < 1)).sum() >= px
    elif name == "media":
        fog = facing((1.0, 0.0, 0.0))  # every sample of the pixel ended in a medium
        near = fog & (a[..., 6] < aov_scenes.MEDIA_CAMERA_RADIUS)  # mean free flight below the radius: one at least inside the camera's medium
        far = fog & (a[..., 6] > 5.0)                              # mean above 5: one at least beyond it, so in the box
        print("counts", st["counts"], "(1, 0, 0)", int(fog.sum()), "around the camera", int(near.sum()), "in the box", int(far.sum()),
              "partial", int(partial.sum()))
        assert st["counts"][3] >= samples and st["counts"][0] - st["counts"][3] >= samples and st["counts"][1] >= samples
        assert near.sum() >= px and far.sum() >= px and partial.sum() >= px
        assert np.all(a[..., 0:3][cov == 0.0] == a[..., 0:3][cov == 0.0][0]) and a[..., 0:3][cov == 0.0].max() > 0, "the background is not black"
    elif name == "moving_textured":
        # the ground's albedo is a mix l * (0.9, 0.9, 0.9) + (1 - l) * (0.2, 0.3, 0.1) of the checker's colours: l from red equals l from
        # blue.  A covered pixel where the two are 0.05 apart shows the sphere's image texture
        image = (cov == 1.0) & (np.abs((alb[..., 0] - 0.2) / 0.7 - (alb[..., 2] - 0.1) / 0.8) > 0.05)
        print("partial", int(partial.sum()), "covered", int((cov == 1.0).sum()), "missed", int((cov == 0.0).sum()), "image texels", int(image.sum()))
        assert partial.sum() >= px and image.sum() >= px and (cov == 0.0).sum() >= px
        assert len(np.unique(alb[image], axis=0)) >= 16, "several texels of the image"
    elif name == "three_wrappers":
        # one bounce at most: rays - samples = the camera rays whose first hit is a Metal of fuzz <= max_fuzz
        seg = [aov_scenes.scene_pair(name)[1].aov(W, H, 3, max_specular=1, max_fuzz=mf)[1]["segments"] for mf in (0.0, 0.5, 1.0)]
        oblique = (cov == 1.0) & (np.abs(nrm[..., 0]) > 0.1) & (np.abs(nrm[..., 2]) > 0.1)
        print("rays with one bounce at max_fuzz 0, 0.5, 1:", seg, "oblique normals", int(oblique.sum()))
        assert seg[0] - st["paths"] >= samples, "the fuzz-0 box is seen"
        assert seg[1] - seg[0] >= samples, "max_fuzz = 0.5 follows the box of fuzz exactly 0.5"
        assert seg[2] - seg[1] >= samples, "and stops on the box of fuzz 1"
        assert oblique.sum() >= px, "faces of the rotated boxes"
    elif name == "mirror_hall":
        _, s4 = oracle_frame(name, "whole", (4, 0.0))
        print("counts at max_specular 4", s4["counts"])
        assert min(s4["counts"][:3]) >= samples, "ends on a wall, escapes, and is cut while still specular"


def test_reference_stream_build_refuses():
    """The product refuses RT1W_RNG_REFERENCE for the feature entries, so the reference-stream build of the oracle states nothing."""
    import orc
    with pytest.raises(RuntimeError):
        orc.OracleScene(5, build_seed=1, refstream=True).aov(8, 8, 1)


@pytest.mark.parametrize("name", aov_scenes.names())
def test_twin_against_the_literal_oracle(rt, name):
    """First-hit and deep buffers of the CPU twin, every frame of FRAMES x every path x every valid variant, and the tile-list sums."""
    prod, _ = aov_scenes.scene_pair(name)
    variants = _valid_variants(prod.info())
    worst = Worst()
    for frame, (w, h, spp, tile, so, gs) in FRAMES.items():
        for path in [FIRST] + DEEP:
            want, sw = oracle_frame(name, frame, path)
            for v in variants:
                kw = dict(tile=tile, sample_offset=so, global_seed=gs, variant=v, with_stats=True)
                if path is FIRST:
                    got, sg = rt.aov_host(prod, w, h, spp, **kw)
                else:
                    got, sg = rt.aov_host(prod, w, h, spp, max_specular=path[0], max_fuzz=path[1], **kw)
                assert sg["segments"] == sw["segments"], (name, frame, path, v, "rays traced")
                compare(got, want, worst, (name, frame, path, v))
    sums = oracle_tiles(name)
    for v in variants:
        got = rt.aov_tiles_host(prod, W, H, TILE_SPP, TILE, TILE_LIST, global_seed=TILE_SEED, variant=v)
        compare_sums(got, sums, TILE_SPP, worst, (name, "tiles", v))
    print(name, "variants", variants, worst)


# ------------------------------------------------------------------------------------------------------------------ GPU tier --

@pytest.mark.gpu
@pytest.mark.parametrize("name", aov_scenes.names())
def test_gpu_against_the_literal_oracle(rt, gpu_ctx_factory, name):
    """rt1w_render_aov, rt1w_render_aov_deep at (4, 0.5) and (64, 1.0) and rt1w_render_aov_tiles against the oracle directly, not through
    the twin: the whole frame, the ragged tile and the 1-pixel-wide tile in the scene's own variant, every valid variant on the ragged
    tile."""
    prod, _ = aov_scenes.scene_pair(name)
    ctx = gpu_ctx_factory(prod)
    worst = Worst()

    def run(frame, path, variant):
        w, h, spp, tile, so, gs = FRAMES[frame]
        want, sw = oracle_frame(name, frame, path)
        kw = dict(tile=tile, sample_offset=so, global_seed=gs, variant=variant, with_stats=True)
        if path is FIRST:
            got, sg = ctx.render_aov(w, h, spp, **kw)
        else:
            got, sg = ctx.render_aov_deep(w, h, spp, max_specular=path[0], max_fuzz=path[1], **kw)
        assert sg["segments"] == sw["segments"] and sg["paths"] == sw["paths"], (name, frame, path, variant, "rays traced")
        assert variant is None or sg["variant"] == variant
        compare(got, want, worst, (name, frame, path, variant))
    for frame in GPU_FRAMES:
        for path in [FIRST] + GPU_DEEP:
            run(frame, path, None)
    for v in _valid_variants(prod.info()):
        for path in [FIRST] + GPU_DEEP:
            run("ragged", path, v)
    got = ctx.render_aov_tiles(W, H, TILE_SPP, TILE, TILE_LIST, global_seed=TILE_SEED)
    compare_sums(got, oracle_tiles(name), TILE_SPP, worst, (name, "tiles"))
    ctx.close()
    print(name, worst)
