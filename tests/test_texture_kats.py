"""Texture::value, Perlin::noise / turb and sphere_uv against the reference's own text (tests/tex_reference.py: numpy and Python
integers, written from perlin.rs, texture.rs and math.rs), on the CPU: the f64 twin of the device probe (rt.texture_host,
librt1w_lab.so) and the f32 twin (orc.flat_f32_texture).  csrc/rt_core.h and oracle/oracle.cpp restate these functions by one hand and
agree by construction; here the expected side is outside the project's C++.  The scene, the points and the derivation of every bound
are in tests/texture_kats.py; tests/test_texture_kats_gpu.py runs the same points through rt1w_debug_texture.

What this found: `p.floor() as isize` saturates at 2^63 (perlin.rs:51-53), product and oracle saturated at 9.2e18.  On the points with a
coordinate in [9.2e18, 2^63) the unfixed rt_core.h missed the reference by up to 0.667 (noise, 6.0e15 e) and 0.517 (turb) where the
bounds are 44 e = 4.9e-15 and 99 e: it read perm[255] and perm[0] where the reference reads perm[0] and perm[1]."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
import tex_reference as tr
import texture_kats as tk

HERE = os.path.dirname(os.path.abspath(__file__))
_P = C.c_void_p


@pytest.fixture(scope="module")
def scene(rt):
    return tk.build_scene(rt)


def probes(rt, sc):
    return {np.float64: lambda mode, tex, q: rt.texture_host(sc, mode, tex, q),
            np.float32: lambda mode, tex, q: orc.flat_f32_texture(sc, mode, tex, q)}


def test_the_reference_loads_no_library():
    """tex_reference.py stands on numpy alone: it must not import the package, ctypes or the oracle loader."""
    text = open(os.path.join(HERE, "tex_reference.py")).read()
    imports = [line.split()[1] for line in text.splitlines() if line.startswith(("import ", "from "))]
    assert imports == ["numpy"], imports
    assert np.finfo(tr.LD).nmant >= 63


def test_the_reference_casts_as_rust_does():
    """`as isize` and `as u32`: exact below the end of the range, saturated at it, NaN -> 0"""
    two63 = 2.0**63
    below = float(np.nextafter(two63, 0.0))
    assert tr.as_isize(below) == 2**63 - 1024 and tr.as_isize(9.2e18) == 9200000000000000000
    assert tr.as_isize(two63) == tr.as_isize(1e300) == tr.as_isize(np.inf) == 2**63 - 1
    assert tr.as_isize(-two63) == tr.as_isize(-1e300) == tr.as_isize(-np.inf) == -2**63
    assert tr.as_isize(np.nan) == 0 and tr.as_isize(-0.5) == 0 and tr.as_isize(-1.0) == -1
    got = tr._as_isize_u64(np.array([below, two63, -two63, np.nan, -1.0, 3.7]))
    assert [int(x) for x in got] == [2**63 - 1024, 2**63 - 1, 2**63, 0, 2**64 - 1, 3]
    assert tr.as_u32(np.array([-1.0, -0.0, np.nan, 0.99, 4294967295.5, 2.0**32, np.inf, 1e300])).tolist() == \
        [0, 0, 0, 0, 4294967295, 4294967295, 4294967295, 4294967295]


def test_the_reference_philox_is_philox():
    """Random123's known answers, and the build stream's words as the library hands them out"""
    assert tr.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert tr.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert tr.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    out = np.empty(64)
    orc.A.orc_stream(7, 0, 0.0, 1.0, 2, out.ctypes.data_as(_P), 64)
    assert [int(x) for x in out] == tr.build_stream_words(7, 64)


def test_the_point_sets_are_what_the_fixture_says():
    """every group is present in its size, every texel column and row of every image is queried, the non-finite results are counted"""
    census = tk.census()
    assert census == tk.golden()["census"]
    assert min(census["noise_groups"].values()) > 0 and census["noise_groups"]["uniform"] == 20000
    assert census["noise_points_in_window"] >= 64 and census["noise_points_turb_carries_into_window"] >= 21
    for name, img in census["images"].items():
        assert min(img["columns"]) > 0 and min(img["rows"]) > 0, name


@pytest.mark.parametrize("name", ["random", "revealing"])
@pytest.mark.parametrize("ft", [np.float64, np.float32], ids=["f64", "f32"])
def test_noise_and_turb(rt, scene, ft, name):
    """Perlin::noise and turb(.., 7) of both twins over caller-supplied tables, every group of points, within the derived bounds;
    non-finite results in kind and place"""
    sc, ids = scene
    k = ["random", "revealing"].index(name)
    got = probes(rt, sc)[ft](1, k, tk.uvp(tk.all_noise_points()))
    assert np.array_equal(got[:, 2], np.zeros(len(got)))
    tk.check_noise(got, tk.tables()[name], name, ft)


def test_noise_in_the_saturation_window(rt, scene):
    """the points with a coordinate in [9.2e18, 2^63), and those turb's doubling carries there: floor(p) converts exactly and is a multiple
    of 1024, so the corners read perm[0] and perm[1] (perlin.rs:51-62).  The reference's values differ from what a cast saturating at
    9.2e18 gives (perm[255], perm[0]): the points tell the two apart"""
    sc, ids = scene
    pts, t = tk.noise_points(), tk.tables()["random"]
    for group in ("window", "turb_window"):
        p = pts[group]
        got = rt.texture_host(sc, 1, 0, tk.uvp(p))
        n_ref, t_ref = tr.noise(t, p), tr.turb(t, p, 7)
        e = tk.EPS[np.float64]
        dn, dt = tk.worst(got[:, 0], n_ref) / e, tk.worst(got[:, 1], t_ref) / e
        print(f"{group}: noise off by {dn:.3g} e, turb by {dt:.3g} e")
        assert dn <= tk.NOISE_EPS and dt <= tk.TURB_EPS, (group, dn * e, dt * e)
    # and the set can tell: the same points through the reference with every coordinate of the window moved to 2^63, where the cast saturates
    p = pts["window"]
    sat = np.where((p >= tk.WINDOW_LO) & (p < tk.TWO63), tk.TWO63, p)
    assert np.abs(tr.noise(t, sat) - tr.noise(t, p)).max() > 0.1


def test_noise_texture_own_tables_follow_the_reference(rt, scene):
    """the texture of rt1w_texture_noise (its tables read back) through both twins: noise, turb and value"""
    sc, ids = scene
    table = tk.perlin_record(sc, 2)
    got = rt.texture_host(sc, 1, 2, tk.uvp(tk.all_noise_points()))
    tk.check_noise(got, table, "own")
    tk.check_value(rt.texture_host(sc, 0, ids["noise_own"], tk.uvp(tk.value_points())), table, tk.SCALES[2], "own")


@pytest.mark.parametrize("name", ["random", "revealing"])
@pytest.mark.parametrize("ft", [np.float64, np.float32], ids=["f64", "f32"])
def test_noise_texture_value(rt, scene, ft, name):
    """NoiseTexture::value = 0.5 (1 + sin(scale z + 10 turb(p, 7))) within 0.5 (10 turb bound + 3 e |argument| + 1 ulp of the sine)"""
    sc, ids = scene
    k = ["random", "revealing"].index(name)
    got = probes(rt, sc)[ft](0, ids[f"noise_{name}"], tk.uvp(tk.value_points(), u=0.3, v=0.8))
    tk.check_value(got, tk.tables()[name], tk.SCALES[k], name, ft)


@pytest.mark.parametrize("seed", [1, 0x1234567887654321])
def test_rt1w_texture_noise_is_perlin_new_over_the_build_stream(rt, seed):
    """Perlin::new (perlin.rs:25-43) as the first constructor calls of a scene: the permutations equal the reference's over the Python
    Philox words of the build stream exactly, the vectors within 2 ulp a component; the second texture continues the stream"""
    sc = rt.Scene(seed)
    n0, n1 = sc.noise_texture(1.0), sc.noise_texture(2.0)
    sc.set_world(sc.bvh_node([sc.sphere((0, 0, 0), 1, sc.lambertian(n0)), sc.sphere((0, 3, 0), 1, sc.lambertian(n1))]))
    sc.set_lights([])
    sc.set_background((0.0, 0.0, 0.0))
    sc.set_camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    sc.commit()
    words = tr.build_stream_words(seed, 8192)
    pos = 0
    for k in range(2):
        want, pos = tr.perlin_new(words, pos)
        got = tk.perlin_record(sc, k)
        for a in (1, 2, 3):
            assert np.array_equal(got[a], want[a]), (k, a)
            assert sorted(got[a].tolist()) == list(range(256))
        err = np.abs(got[0].astype(tr.LD) - want[0]).astype(np.float64)
        assert (err <= 2.0 * np.spacing(np.abs(got[0]))).all(), (k, float((err / np.spacing(np.abs(got[0]))).max()))
        assert np.abs(np.linalg.norm(got[0], axis=1) - 1.0).max() < 1e-15
    assert 2 * (768 * 2 + 3 * 255) <= pos < 8192   # at least the draws without a retry


@pytest.mark.parametrize("ft", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", range(len(tk.IMAGE_SIZES)), ids=[f"{w}x{h}" for w, h in tk.IMAGE_SIZES])
def test_image_texture(rt, scene, k, ft):
    """DynamicImage::value: the clamps, 1 - v, the saturating cast, min(width - 1), the pool offset: bit for bit"""
    sc, ids = scene
    w, h = tk.IMAGE_SIZES[k]
    q = tk.image_queries(w, h)
    if ft is np.float32:   # the f32 twin rounds its inputs once: ask the reference about the rounded queries
        q32 = q.copy()
        with np.errstate(over="ignore", under="ignore"):
            q32[:, :2] = q[:, :2].astype(np.float32).astype(np.float64)
        tk.check_image(probes(rt, sc)[ft](0, ids["images"][k], q), w, h, q32, ft)
    else:
        tk.check_image(probes(rt, sc)[ft](0, ids["images"][k], q), w, h, q, ft)


def test_checkers_choose_by_the_sign_and_forward_u_v_p(rt, scene):
    """CheckerTexture::value (texture.rs:46-55): odd where the product of sines is negative; a checker over (image, noise) hands u, v to
    the image and p to the noise; a checker of checkers asks its children with the same point"""
    sc, ids = scene
    g = np.random.default_rng(80)
    n = 20000
    q = tk.uvp(g.uniform(-20.0, 20.0, size=(n, 3)))
    q[:, 0], q[:, 1] = g.uniform(-0.2, 1.2, size=n), g.uniform(-0.2, 1.2, size=n)
    q[:, 4] = g.uniform(-8.0, 8.0, size=n)
    odd, keep = tr.checker(q[:, 2:])
    assert keep.sum() > 0.99 * n and 0.4 * n < odd.sum() < 0.6 * n
    got = rt.texture_host(sc, 0, ids["checker_solids"], q)
    assert np.array_equal(got[keep], np.where(odd[keep, None], tk.SOLID_A, tk.SOLID_B))
    # (image 5x3, noise over the random tables): each child's own value at the same u, v, p
    w, h = tk.IMAGE_SIZES[3]
    img = tr.image_value(tk.image(w, h), q[:, 0], q[:, 1])
    noise = rt.texture_host(sc, 0, ids["noise_random"], q)
    tk.check_value(rt.texture_host(sc, 0, ids["noise_random"], tk.uvp(tk.value_points())), tk.tables()["random"], tk.SCALES[0], "random")
    got = rt.texture_host(sc, 0, ids["checker_image_noise"], q)
    assert np.array_equal(got[keep], np.where(odd[keep, None], img, noise)[keep])
    assert len(np.unique(img[keep & odd], axis=0)) == w * h     # every texel was asked for through the checker
    # checker of checkers: odd -> the solids' checker -> its odd child; even -> the (image, noise) checker -> its even child
    got = rt.texture_host(sc, 0, ids["checker_checkers"], q)
    assert np.array_equal(got[keep], np.where(odd[keep, None], tk.SOLID_A, noise)[keep])


def test_sphere_uv(rt, scene):
    """sphere_uv at the poles, on both sides of the seam with both signs of zero and at 2000 random unit points, within the bounds that
    the contract's 2 ulp of atan2 and acos leave after one addition and one division (tests/texture_kats.py)"""
    sc, ids = scene
    pts, n_fixed = tk.uv_points()
    got = rt.texture_host(sc, 2, 0xFFFFFFFF, tk.uvp(pts))    # mode 2 ignores `tex`
    tk.check_sphere_uv(got)
    assert got[0][1] == 1.0 and got[1][1] == 0.0             # the poles: v = acos(-1) / pi = 1, acos(1) / pi = 0
    assert got[3][0] == 0.0 and got[4][0] == 1.0             # the seam: atan2(-0, -1) = -pi -> u = 0; atan2(+0, -1) = pi -> u = 1
    assert got[9][0] < 1e-12 and got[10][0] > 1.0 - 1e-12    # and just beside it
    assert np.array_equal(got[:, 2], np.zeros(len(got)))


def test_noise_tables_refusals(rt):
    """rt1w_texture_noise_tables refuses a null table and a permutation entry beyond 255; what it returns is a texture id, and an id of
    another kind is refused where a texture is asked for"""
    t = tk.tables()["random"]
    sc = rt.Scene(3)
    lib = rt._lib
    rv = np.ascontiguousarray(t[0]).reshape(768)
    ps = [np.ascontiguousarray(p, dtype=np.uint32) for p in t[1:]]
    ptr = [rv.ctypes.data_as(_P)] + [p.ctypes.data_as(_P) for p in ps]
    for k in range(4):
        args = list(ptr)
        args[k] = None
        assert lib.rt1w_texture_noise_tables(sc._h, 1.0, *args) == rt.ERR_INVALID and "null table" in rt.last_error()
    for bad in (256, 2**32 - 1):
        for k in range(3):
            perms = [p.copy() for p in ps]
            perms[k][255 if bad == 256 else 0] = bad
            with pytest.raises(rt.Rt1wError) as why:
                sc.noise_texture_tables(1.0, t[0], *perms)
            assert why.value.code == rt.ERR_INVALID and "perm entry" in str(why.value)
    noise = sc.noise_texture_tables(1.0, *t)
    assert noise == 0                                                     # the refused calls left no texture behind
    mat = sc.lambertian(noise)
    spheres = [sc.sphere((0, 3 * i, 0), 1, mat) for i in range(3)]
    assert spheres[-1] > noise                                            # an id that is no texture of this scene
    for wrong in (spheres[-1], -1):
        with pytest.raises(rt.Rt1wError):
            sc.checker_texture(noise, wrong)
        with pytest.raises(rt.Rt1wError):
            sc.lambertian(wrong)


def test_the_probe_and_its_twin_refuse_alike(rt, scene):
    """rt1w_lab_texture_host refuses what rt1w_debug_texture refuses (one text, scene.h: debug_texture_refusal): an unknown mode, a
    texture id beyond the textures, a Perlin table index beyond the tables -- a noise TEXTURE's id is no table index"""
    sc, ids = scene
    q = tk.uvp(np.zeros((2, 3)))
    n_tex, n_perlin = sc.info()["n_textures"], sc.info()["n_perlin"]
    assert n_perlin == 3 and ids["noise_own"] >= n_perlin
    for mode, tex, text in ((3, 0, "unknown mode"), (-1, 0, "unknown mode"), (0, n_tex, "bad texture id"), (0, 0xFFFFFFFF, "bad texture id"),
                            (1, n_perlin, "bad Perlin table index"), (1, ids["noise_own"], "bad Perlin table index"), (1, 0xFFFFFFFF, "bad Perlin table index")):
        with pytest.raises(rt.Rt1wError) as why:
            rt.texture_host(sc, mode, tex, q)
        assert why.value.code == rt.ERR_INVALID and text in str(why.value), (mode, tex, str(why.value))
    assert rt.texture_host(sc, 1, n_perlin - 1, q).shape == (2, 3) and rt.texture_host(sc, 0, n_tex - 1, q).shape == (2, 3)
    assert rt.texture_host(sc, 3, 0, np.zeros((0, 5))).shape == (0, 3)   # nothing asked, nothing refused: as the probe
    plain = rt.Scene.reference(5, build_seed=1)                           # a scene without a noise texture
    with pytest.raises(rt.Rt1wError) as why:
        rt.texture_host(plain, 1, 0, q)
    assert "no Perlin table" in str(why.value)
