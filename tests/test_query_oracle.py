"""Ray and radiance queries against the literal oracle on the caller's own rays -- CPU tier.

The CPU twins of rt1w_hit and rt1w_ray_color (librt1w_lab.so: rt1w_lab_hit_host, rt1w_lab_ray_color_counts_host; csrc/rt_hit.h,
csrc/rt_ray_list.h and csrc/rt_core.h built for the host) against oracle/oracle.cpp's orc_hit and orc_ray_color, which run the literal
Hittable tree and the literal recursive ray_color on the same rays: the sets of tests/query_rays.py on the reference arms 0, 5, 6, 7, the
hand-built scenes and eight random graphs.  Every ray of every set is compared; none is left out.

Bounds: the project's for product against literal (test_hit.py, test_ray_color.py), nothing new.  hit, front_face and the material
equal; t within 1e-12 relative; p within 1e-12 of the larger of |p|, |origin| and |t * direction| (p = origin + t * direction is a sum:
it carries t's relative error at the size of its terms), under a Translate / RotateY within 1e-12 of the scene's extent, as test_hit.py
has it; normal, u, v within 1e-12 absolute; a miss is zeros and 0xFFFFFFFF.  u, v are compared where the oracle says the hit material's
texture tree holds an image texture, and are 0 elsewhere.  Radiance: 1e-12 relative with equal segment counts per ray.  A NaN equals a
NaN and an infinity an infinity of the same sign: rays in a rect's plane and zero directions make both in the literal code.  On the
exact-window set t is the oracle's bits.

The whole module takes about four seconds on the CPU."""
import json

import numpy as np
import pytest

import hit_reference as HR
import orc
import query_rays as Q

PAIRS, SAMPLES, DEPTHS = Q.PAIRS, Q.SAMPLES, Q.DEPTHS
check_hit, check_radiance = Q.check_hit, Q.check_radiance


# ------------------------------------------------------------------------------------------------------------------ the sets --

def test_graph_seeds_cover_the_features():
    seeds = Q.graph_seeds()
    assert len(seeds) == Q.N_GRAPHS == len(set(seeds)) and seeds == Q.load_census()["graph_seeds"]
    have = [Q.scene_pair(f"graph{k}")[1].census()[0] for k in range(Q.N_GRAPHS)]
    for f in Q.FEATURES:
        assert sum(h[f] > 0 for h in have) >= 2, f


def test_census_document_is_the_committed_file():
    """the whole document -- the exact-window row and the (empty) list of ties included -- as `make_golden.py query` writes it"""
    assert Q.census_document() == Q.load_census()


@pytest.mark.parametrize("name", Q.scene_names())
def test_sets_meet_their_conditions_and_the_census(name):
    """From the oracle's output alone: the conditions of every set, and the counts of tests/golden/query_oracle_census.json -- a set
    cannot quietly stop testing what it is for."""
    s = Q.sets(name)
    assert s.check_conditions() == []
    doc = Q.load_census()
    print(name, json.dumps(s.census))
    assert doc["set_seeds"][name] == s.seed and doc["scenes"][name] == s.census


# ------------------------------------------------------------------------------------------------------------------ rt.hit_host --

@pytest.mark.parametrize("name", Q.scene_names())
def test_hit_twin_against_the_oracle(rt, name):
    """rt.hit_host against OracleScene.hit: the four sets, every variant that covers the scene, two (sample, global_seed) pairs."""
    prod, orac = Q.scene_pair(name)
    s = Q.sets(name)
    for which in Q.HIT_SETS:
        rays = s.rays[which]
        for sample, gs in PAIRS:
            want, wmat, waux = orac.hit(rays, Q.FIRST_STREAM, sample, gs)
            for v in HR.valid_variants(prod.info()):
                got, node = rt.hit_host(prod, rays, first_stream=Q.FIRST_STREAM, sample=sample, global_seed=gs, variant=v)
                hits = check_hit(name, which, rays, got, node, want, wmat, waux, (sample, gs, "variant", v))
        print(name, which, len(rays), "rays", hits, "hits")


def test_hit_twin_on_the_exact_windows(rt):
    """Roots equal to t_min, equal to t_max and one ulp to either side, for every leaf kind of the dyadic scene: the oracle's verdict
    and the oracle's bits of t -- and the verdicts are the ones the reference's comparisons give (a root on a bound is inside the leaf's
    window; where the root is also the face of a BVH node's box, `t_max <= t_min` of aabb.rs:27-29 ends it before the leaf is asked)."""
    prod, orac = Q.scene_pair("exact")
    rays, labels = Q.exact_window()
    want, wmat, waux = orac.hit(rays, Q.FIRST_STREAM)
    verdict = {(what, t_min, t_max): ((w[0], w[1]) if w[0] else (0.0, None)) for (what, root, t_min, t_max), w in zip(labels, want)}
    up, down = (lambda x: float(np.nextafter(x, Q.INF))), (lambda x: float(np.nextafter(x, 0.0)))
    for what, r1, r2 in (("sphere", 4.0, 12.0), ("moving sphere", 4.0, 12.0), ("sphere under Translate", 4.0, 12.0)):  # sphere.rs:41-47
        assert verdict[(what, r1, Q.INF)] == (1.0, r1) and verdict[(what, up(r1), Q.INF)] == (1.0, r2) and verdict[(what, down(r1), Q.INF)] == (1.0, r1)
        assert verdict[(what, 0.001, r1)] == (1.0, r1) and verdict[(what, 0.001, down(r1))] == (0.0, None) and verdict[(what, 0.001, up(r1))] == (1.0, r1)
        assert verdict[(what, r2, Q.INF)] == (1.0, r2) and verdict[(what, up(r2), Q.INF)] == (0.0, None)
        assert verdict[(what, 8.0, r2)] == (1.0, r2) and verdict[(what, 8.0, down(r2))] == (0.0, None)
    for what, r in (("xy rect", 2.0), ("xz rect", 4.0), ("yz rect", 8.0), ("xz rect under FlipFace", 4.0)):  # aarect.rs:48-50
        assert verdict[(what, r, Q.INF)] == (1.0, r) and verdict[(what, up(r), Q.INF)] == (0.0, None)
        assert verdict[(what, 0.001, r)] == (1.0, r) and verdict[(what, 0.001, down(r))] == (0.0, None)
    assert verdict[("box", 3.0, Q.INF)] == (1.0, 3.0) and verdict[("box", up(3.0), Q.INF)] == (1.0, 7.0)
    assert verdict[("box", 0.001, 3.0)] == (1.0, 3.0) and verdict[("box", 0.001, down(3.0))] == (0.0, None)
    # a sphere alone in a BVH node, met through its centre: the roots 3 and 13 are the slabs of the node's box.  The sphere alone would
    # answer 3 at t_max = 3 and 13 at t_min = 13 (`root < t_min || t_max < root`); the world does not: the node's box test ends with
    # `t_max <= t_min` (aabb.rs:27-29) before the sphere is asked.  One ulp further the sphere answers.
    alone = "sphere alone in a BVH node, through its centre"
    assert verdict[(alone, 0.001, 3.0)] == (0.0, None) and verdict[(alone, 0.001, up(3.0))] == (1.0, 3.0) and verdict[(alone, 3.0, Q.INF)] == (1.0, 3.0)
    assert verdict[(alone, 13.0, Q.INF)] == (0.0, None) and verdict[(alone, down(13.0), Q.INF)] == (1.0, 13.0) and verdict[(alone, 8.0, 13.0)] == (1.0, 13.0)
    assert want[:, 0].sum() >= len(rays) // 3 and (want[:, 0] == 0.0).sum() >= len(rays) // 8
    for sample, gs in PAIRS:
        want, wmat, waux = orac.hit(rays, Q.FIRST_STREAM, sample, gs)
        for v in HR.valid_variants(prod.info()):
            got, node = rt.hit_host(prod, rays, first_stream=Q.FIRST_STREAM, sample=sample, global_seed=gs, variant=v)
            check_hit("exact", "exact_window", rays, got, node, want, wmat, waux, (sample, gs, "variant", v), exact_t=True)


# ------------------------------------------------------------------------------------------------------------------ rt.ray_color_host --

@pytest.mark.parametrize("name", Q.scene_names())
def test_radiance_twin_against_the_oracle(rt, name):
    """rt.ray_color_host against OracleScene.ray_color at 1 spp, raw sums: the generic, continuation and axis-parallel sets; samples 0
    and 7; start words none and a drawn word in 0 .. 40 per ray -- the oracle's stream draws its way there, the twin's is put there by
    rt_rng_at --; max_depth 1, 2 and 50.  1e-12 relative, equal segment counts per ray."""
    prod, orac = Q.scene_pair(name)
    s = Q.sets(name)
    for which in Q.RADIANCE_SETS:
        rays = s.rays[which]
        for sample in SAMPLES:
            for word in (None, Q.start_words(name, which, len(rays))):
                for depth in DEPTHS:
                    want, wseg = orac.ray_color(rays, word, Q.FIRST_STREAM, sample, 3, depth)
                    got, st = rt.ray_color_host(prod, rays, word, spp=1, sample_offset=sample, first_stream=Q.FIRST_STREAM, global_seed=3,
                                                max_depth=depth, out_sum=True, with_stats=True)
                    assert st["segments"] == int(st["ray_segments"].sum())
                    check_radiance((name, which, sample, "start words" if word is not None else "word 0", depth), got, st["ray_segments"], want, wseg)
        print(name, which, len(rays), "rays, mean segments at depth 50:", float(wseg.mean()))


def test_oracle_entries_refuse_the_reference_stream_and_trace_a_ray():
    """In the reference-stream build both entries return an error; and the per-segment dump of one ray adds up: as many rows as
    segments, each row's ray starting where the row before it hit."""
    prod, orac = Q.scene_pair("arm5")
    rays = Q.sets("arm5").rays["continuation"][:4]
    ref = orc.OracleScene(5, build_seed=1, refstream=True)
    with pytest.raises(RuntimeError):
        ref.hit(rays)
    with pytest.raises(RuntimeError):
        ref.ray_color(rays)
    for r in range(4):
        col, seg, rows = orac.ray_color(rays[r:r + 1], None, Q.FIRST_STREAM + r, 0, 0, 50, trace=64)
        assert len(rows) == seg[0] and np.array_equal(rows[0, 8:15], rays[r, :7])
        for a, b in zip(rows[:-1], rows[1:]):
            assert a[0] == 1.0 and np.array_equal(a[2:5], b[8:11])
        assert np.array_equal(col, orac.ray_color(rays[:4], None, Q.FIRST_STREAM, 0, 0, 50)[0][r:r + 1])
