"""The scene-specialised text (jit.cpp: TopoJit; rt_core.h: the unrolled sweep, the reuse table, the static hit record, the light and
wall shapes, the box-free sweep) on topologies nobody built by hand: 48 random and 48 lattice scene graphs (spec_graphs.py), the flat
core built for the host around the library's own generated Topos, 16 to a library.

Per graph, at max_depth 50 and 3: specialised build == generic flat core, bit for bit with equal segment counts; generic flat core
within 1e-12 (relative) of the literal recursive oracle with equal segment counts; the frame is not empty and paths did bounce.  The
lattice half again with -DRT_BOX_FREE=0, -DRT_DIV_SHARED=0 and -DRT_HIT_STATIC=15: the shipped build's bits.  16 graphs through the f32
twin.  What the corpus covers is a condition of its own (test_the_corpus_covers_what_it_is_for) and a recorded result
(golden/spec_fuzz_census.json).

On the host the box-free sweep is built with -DRT_BOX_FREE=1 (rt_core.h: what the device takes by default), so that is the shipped
build here; RT_DIV_SHARED is device text only and its switch changes nothing in a host build."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import core_builds as CB
import orc
import spec_graphs as G
from test_random_scenes import RTOL, close

assert RTOL == 1e-12
GOLDEN = os.path.join(orc.ROOT, "tests", "golden", "spec_fuzz_census.json")
CORPUS = G.RANDOM + G.LATTICE
BATCH = 16
W, HGT, SPP, CHUNK = 28, 20, 4, 3
DEPTHS = (50, 3)
SHIPPED = ("-DRT_BOX_FREE=1",)
SWITCHES = {"box_free_off": ("-DRT_BOX_FREE=0",), "div_shared_off": ("-DRT_BOX_FREE=1", "-DRT_DIV_SHARED=0"), "hit_static_every_part": ("-DRT_BOX_FREE=1", "-DRT_HIT_STATIC=15")}
N_F32 = 8   # per source


@pytest.fixture(scope="module")
def corpus(rt):
    """name -> (entry, product scene, literal-oracle scene), every graph built once"""
    assert len(G.RANDOM) == len(G.LATTICE) == 48 and len({G.name_of(e) for e in CORPUS}) == 96
    return {G.name_of(e): (e,) + G.build(e) for e in CORPUS}


@pytest.fixture(scope="module")
def censuses(corpus):
    return {name: G.census(prod) for name, (_, prod, _) in corpus.items()}


def f32_names(censuses):
    """8 graphs of each source for the f32 twin: four that sweep without boxes in f64 and four that do not, the first of the lists, none
    of the large ones"""
    out = []
    for entries in (G.RANDOM, G.LATTICE):
        names = [G.name_of(e) for e in entries if censuses[G.name_of(e)]["n_nodes"] <= 64]
        free = [n for n in names if censuses[n]["box_free"]][:N_F32 // 2]
        out += free + [n for n in names if not censuses[n]["box_free"]][:N_F32 - len(free)]
    return out


def _command(work, tag, scenes, flags, f32):
    """writes <tag>/topo_gen.h for `scenes` (variant 100 + k) and returns the library's path and the compiler's command line"""
    return CB.static_command(work / tag, "fuzz_" + tag, [(None, sc, CB.topo_text(sc, "Topo", f32)) for sc in scenes], flags, f32)


@pytest.fixture(scope="module")
def libs(corpus, censuses, tmp_path_factory):
    """(build, graph name) -> (library, variant): the shipped build of every graph, the three switched builds of the lattice half, the
    f32 twin of 16 graphs.  16 compiler runs, at most 16 at a time"""
    import time
    work = tmp_path_factory.mktemp("spec_fuzz")
    names = list(corpus)
    jobs = []   # (build, names of the batch, library path, command)
    for b in range(0, len(names), BATCH):
        batch = names[b:b + BATCH]
        jobs.append(("shipped", batch) + _command(work, f"shipped{b // BATCH}", [corpus[n][1] for n in batch], SHIPPED, False))
    lattice = [G.name_of(e) for e in G.LATTICE]
    for build, flags in SWITCHES.items():
        for b in range(0, len(lattice), BATCH):
            batch = lattice[b:b + BATCH]
            jobs.append((build, batch) + _command(work, f"{build}{b // BATCH}", [corpus[n][1] for n in batch], flags, False))
    batch = f32_names(censuses)
    jobs.append(("f32", batch) + _command(work, "f32", [corpus[n][1] for n in batch], (), True))
    t0 = time.time()
    CB.build_all([j[3] for j in jobs])
    print(f"spec_fuzz: {len(jobs)} host libraries in {time.time() - t0:.0f} s")
    out = {}
    for build, batch, so, _ in jobs:
        lib = orc.flat_f32_lib(str(so)) if build == "f32" else orc.declare_flat(C.CDLL(str(so)))
        if build != "f32":
            assert lib.orcflat_n_static() == len(batch)
        for k, n in enumerate(batch):
            out[(build, n)] = (lib, 100 + k)
    return out


@pytest.fixture(scope="module")
def frames(corpus, libs):
    """(build, graph name, max_depth) -> (frame, stats), each rendered once; build "generic": the generic flat core, "literal": the
    recursive oracle"""
    made = {}

    def get(build, name, depth):
        key = (build, name, depth)
        if key not in made:
            _, prod, oracle = corpus[name]
            if build == "literal":
                made[key] = oracle.render(W, HGT, SPP, max_depth=depth)
            elif build == "generic":
                made[key] = orc.flat_render(prod, W, HGT, SPP, max_depth=depth, chunk=CHUNK)
            else:
                lib, variant = libs[(build, name)]
                made[key] = orc.flat_render(prod, W, HGT, SPP, max_depth=depth, chunk=CHUNK, variant=variant, lib=lib)
        return made[key]

    return get


def test_the_corpus_covers_what_it_is_for(censuses):
    """conditions on the generators and the seed lists, not on the code under test; and the census as recorded"""
    cs = list(censuses.values())
    failed = [what for what, ok in G.coverage(cs).items() if not ok]
    assert not failed, failed
    sizes = [c["n_nodes"] for c in cs]
    assert sum(1 for n in sizes if n > 64) <= 6 and max(sizes) == G.JIT_MAX_NODES and {63, 64, 65, 255, 256} <= set(sizes)
    # the box-free sweep is declared up to 64 nodes and not beyond, on graphs that differ in their pad alone
    assert censuses["lattice2_n63"]["box_free"] and censuses["lattice8_n64"]["box_free"] and not censuses["lattice19_n65"]["box_free"]
    assert not any(c["has_media"] for c in (censuses["lattice2_n63"], censuses["lattice8_n64"], censuses["lattice19_n65"]))
    if os.environ.get("RT1W_WRITE_GOLDEN"):
        json.dump(censuses, open(GOLDEN, "w"), indent=0, sort_keys=True)
    recorded = json.load(open(GOLDEN))
    assert set(recorded) == set(censuses)
    for name, c in censuses.items():
        assert recorded[name] == c, name


def test_the_lattice_is_a_lattice(corpus):
    """every bound of every node of a lattice graph outside its wrappers' frames is a multiple of 0.5 up to a rect's padding, and some
    bound is written -0.0 beside a +0.0"""
    import slab_scenes as S
    signed = 0
    for name, (entry, prod, _) in corpus.items():
        if entry[0] != "lattice":
            continue
        nodes = S.nodes_of(prod)
        for i, k in enumerate(S.kinds(nodes)):
            if 4 <= k <= 6:   # a rect: its two ranges and its plane
                assert np.all(nodes['d'][i][:5] * 2 == np.round(nodes['d'][i][:5] * 2)), (name, i)
        boxes = nodes['d'][[i for i, k in enumerate(S.kinds(nodes)) if k <= S.BVH1]][:, :6]
        zeros = boxes[boxes == 0.0]
        signed += bool(np.any(np.signbit(zeros)) and not np.all(np.signbit(zeros)))
    assert signed >= 4


@pytest.mark.parametrize("name", [G.name_of(e) for e in CORPUS])
def test_specialised_equals_generic_equals_literal(frames, name):
    for depth in DEPTHS:
        s, ss = frames("shipped", name, depth)
        g, sg = frames("generic", name, depth)
        a, sa = frames("literal", name, depth)
        print(name, depth, "segments", ss["segments"], sg["segments"], sa["segments"], "max rel", float(np.nanmax(np.abs(a - g) / np.maximum(np.abs(a), 1e-300))))
        assert ss["segments"] == sg["segments"], (name, depth)
        assert np.array_equal(s, g, equal_nan=True), (name, depth, "the specialised build differs from the generic flat core")
        assert sg["segments"] == sa["segments"], (name, depth, "flat core and literal oracle trace different numbers of rays")
        assert close(a, g), (name, depth, "the generic flat core differs from the literal oracle")
        assert np.any(g > 0.0) and sg["segments"] > W * HGT * SPP, (name, depth)


@pytest.mark.parametrize("build", list(SWITCHES))
@pytest.mark.parametrize("name", [G.name_of(e) for e in G.LATTICE])
def test_switched_builds_have_the_shipped_bits(frames, name, build):
    for depth in DEPTHS:
        s, ss = frames("shipped", name, depth)
        o, so = frames(build, name, depth)
        assert ss["segments"] == so["segments"], (name, build, depth)
        assert np.array_equal(s, o, equal_nan=True), (name, build, depth)


def test_f32_specialised_twin_equals_f32_generic_twin(corpus, censuses, libs):
    names = f32_names(censuses)
    assert len(names) == 2 * N_F32 and sum(censuses[n]["box_free"] for n in names) >= N_F32 // 2
    for name in names:
        _, prod, _ = corpus[name]
        assert CB.topo_text(prod, "T", f32=True) == CB.topo_text(prod, "T"), name   # both precisions declare the same members
        lib, variant = libs[("f32", name)]
        for depth in DEPTHS:
            a, sa = orc.flat_f32_render(prod, W, HGT, SPP, max_depth=depth, chunk=CHUNK)
            b, sb = orc.flat_f32_render(prod, W, HGT, SPP, max_depth=depth, chunk=CHUNK, variant=variant, lib=lib)
            assert sa["segments"] == sb["segments"], (name, depth)
            assert np.array_equal(a, b, equal_nan=True), (name, depth)
            assert np.any(a > 0.0), (name, depth)


def test_one_node_too_many_is_refused(rt, censuses):
    """257 nodes: no unit, no key; the same graph padded to 256 is in the corpus and agrees with the generic core"""
    prod, _ = G.build(G.REFUSED)
    assert prod.info()["n_nodes"] == G.JIT_MAX_NODES + 1
    for ask in (prod.kernel_source, prod.kernel_key):
        with pytest.raises(rt.Rt1wError) as e:
            ask()
        assert e.value.code == rt.ERR_UNSUPPORTED
    assert censuses[G.name_of(G.REFUSED[:2] + (G.JIT_MAX_NODES,))]["n_nodes"] == G.JIT_MAX_NODES
