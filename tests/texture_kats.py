"""What tests/test_texture_kats.py (CPU) and tests/test_texture_kats_gpu.py (device) share: the scene, the tables, the points, the
bounds and the comparisons with tests/tex_reference.py.  The census of the points and the measured maxima are in
tests/golden/texture_kats.json; `python tests/texture_kats.py` rewrites the census and the CPU rows of the maxima (the device rows are
merged from the file named by --device, which the GPU module writes when TEXTURE_KATS_RECORD names a path).

THE BOUNDS, from the operation count of perlin_interp (perlin.rs:88-106) alone.  e = 2^-53 (2^-24 for the f32 twin), first order,
absolute.  The reference evaluates the same expression in longdouble (2^-64): its own error is 2^-11 of what follows.
  * u = p - floor(p) is the reference's own operation of the working type and is taken as it is: no error.
  * uu = u u (3 - 2u): 2u is exact, so 3 roundings, and uu <= 1: |d uu| <= 3e.
  * a blend factor b is uu (i = 1: 1 uu + 0 (1 - uu), exact) or 1 - uu (i = 0: one more rounding): 0 <= b <= 1, |db| <= 4e, and the two
    factors of an axis sum to 1.
  * the weight W = b_i b_j b_k takes 2 roundings: |dW| <= 4e (b_j b_k + b_i b_k + b_i b_j) + 2e W.
  * weight_v = (u - i, v - j, w - k): at most 1 rounding a component, each <= 1 in size: e a component.  dot(c, weight_v) with |c| <= 1 is
    3 products and 2 sums, 5 roundings, gamma_3 = 3e on |c| |weight_v|; with the components' own e:  |d dot| <= 3e |weight_v| + sqrt(3) e.
  * sums over the 8 corners.  S1 = sum W |weight_v| <= sqrt(sum W |weight_v|^2) = sqrt(3 max_u ((1 - uu) u^2 + uu (1 - u)^2)) = sqrt(3)/2
    (the maximum 1/4 is at u = 1/2); this also bounds |noise|.  S2 = sum (b_j b_k + b_i b_k + b_i b_j) |weight_v|: for one pair of
    axes, sum b_j b_k (|u - i| + |(v - j, w - k)|) <= (u + 1 - u) + 2 sqrt(2/4) = 1 + sqrt(2); three pairs: 3 + 3 sqrt(2) = 7.25.
  * a term W dot takes 1 rounding, the 8 terms are added with 7 (the first lands on 0.0):
        sum |dW| |dot|        <= 4e S2 + 2e S1          = 29.0e + 1.7e
        sum W |d dot|         <= 3e S1 + sqrt(3) e      = 2.6e + 1.7e
        the products' own     <= e S1                   = 0.9e
        the 7 additions       <= 7e S1                  = 6.1e
    together 42.0e.  NOISE_EPS = 44 leaves 2e for the second order and for a float32 table vector's length, 1 + 2^-24.
  * turb (perlin.rs:74-86): the weights 2^-i and the doubled points are exact; sum 2^-i 44e < 88e; 6 additions (the first lands on 0.0)
    of partial sums <= sum 2^-i sqrt(3)/2 < sqrt(3): 10.4e; abs is exact.  TURB_EPS = 2 * 44 + 11 = 99.
  * NoiseTexture::value: 0.5 (10 TURB_EPS e + 3e |argument| + 1 ulp of the sine), at |z| <= 8.  (The final 1 + sin
    rounds once more, <= e; the 2e of slack in NOISE_EPS, which enters here 20-fold, covers it.)
  * sphere_uv (math.rs:67-71), from the contract of include/rt1w_num.h (atan2, acos <= 2 ulp), one addition and one division:
        |du| <= (2 ulp(atan2) + ulp(phi) / 2) / 2pi + ulp(u) / 2        |dv| <= 2 ulp(theta) / pi + ulp(v) / 2
    At u in [1/2, 1) that is (2 * 2^-51 + 2^-51) / 2pi + 2^-54 = 2.4 ulp of u; near u = 0, where the addition cancels, it stays the
    ABSOLUTE 2 * 2^-51 / 2pi = 1.4e-16 and is no longer a count of ulps of u.  v: 2 * 2^-51 / pi + 2^-54 = 1.8 ulp at v in [1/2, 1].
    The 2pi and pi of the divisions are exact doublings of the one constant.  ulp(x) is taken at |x| (1 + 2^-40), so a value just
    under a power of two is given the spacing above it, where the computed value may lie."""
import json
import os

import numpy as np

import tex_reference as tr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "texture_kats.json")
LD = tr.LD
NOISE_EPS, TURB_EPS = 44, 99
EPS = {np.float64: 2.0**-53, np.float32: 2.0**-24}
IMAGE_SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (256, 2)]   # width, height
SCALES = (4.0, 0.1, 2.5)   # of the noise textures over the random tables, the revealing tables, and rt1w_texture_noise's own
SOLID_A, SOLID_B = (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)
WINDOW_LO, TWO63 = 9.2e18, 2.0**63


def image(width, height):
    """texel (column i, row j) = (i, j, (31 i + 17 j) & 255): every texel distinct, a transposed or offset read shows"""
    j, i = np.mgrid[0:height, 0:width]
    return np.stack([i, j, (31 * i + 17 * j) & 255], axis=-1).astype(np.uint8)


def tables():
    """{"random": unit vectors and three random permutations, "revealing": ranvec[7] = (1, 0, 0), zero otherwise, three other
    permutations: the value tells which index a corner picked}"""
    g = np.random.default_rng(20240607)
    v = g.normal(size=(256, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    random = (v, *[g.permutation(256).astype(np.uint32) for _ in range(3)])
    r = np.zeros((256, 3))
    r[7] = (1.0, 0.0, 0.0)
    revealing = (r, *[g.permutation(256).astype(np.uint32) for _ in range(3)])
    return {"random": random, "revealing": revealing}


def build_scene(rt):
    """One scene through the constructors -> (scene, ids).  The images are declared in IMAGE_SIZES' order with the other textures between
    them, so every offset of the image pool is met."""
    t = tables()
    sc = rt.Scene(11)
    ids = {"images": []}
    ids["a"], ids["b"] = sc.solid_color(SOLID_A), sc.solid_color(SOLID_B)
    ids["noise_random"] = sc.noise_texture_tables(SCALES[0], *t["random"])        # Perlin table 0
    ids["images"].append(sc.image_texture(image(*IMAGE_SIZES[0])))
    ids["noise_revealing"] = sc.noise_texture_tables(SCALES[1], *t["revealing"])  # Perlin table 1
    ids["images"].append(sc.image_texture(image(*IMAGE_SIZES[1])))
    ids["checker_solids"] = sc.checker_texture(ids["a"], ids["b"])
    ids["images"].append(sc.image_texture(image(*IMAGE_SIZES[2])))
    ids["noise_own"] = sc.noise_texture(SCALES[2])                                # Perlin table 2
    ids["images"].append(sc.image_texture(image(*IMAGE_SIZES[3])))
    ids["checker_image_noise"] = sc.checker_texture(ids["images"][3], ids["noise_random"])
    ids["checker_checkers"] = sc.checker_texture(ids["checker_solids"], ids["checker_image_noise"])
    ids["images"].append(sc.image_texture(image(*IMAGE_SIZES[4])))
    ids["sphere"] = sc.sphere((0, 2, 0), 2, sc.lambertian(ids["checker_checkers"]))
    sc.set_world(sc.bvh_node([sc.sphere((0, -1000, 0), 1000, sc.lambertian(ids["images"][4])), ids["sphere"]]))
    sc.set_lights([])
    sc.set_background((0.7, 0.8, 1.0))
    sc.set_camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    sc.commit()
    return sc, ids


def perlin_record(scene, k):
    """Perlin table k of a committed scene, read back through its flat arrays -> tables"""
    rec = scene.flat(4)[k * 9216:(k + 1) * 9216]
    return (rec[:6144].view(np.float64).reshape(256, 3).copy(), *[rec[6144 + 1024 * a:7168 + 1024 * a].view(np.uint32).copy() for a in range(3)])


def noise_points():
    """{group: points [n, 3]} of the noise and turb checks"""
    g = np.random.default_rng(77)
    base = np.array([0.3, -17.6, 120.9])
    out = {"uniform": g.uniform(-300.0, 300.0, size=(20000, 3))}

    def on_each_axis(values):
        """every value on each axis over `base`, and on all three at once"""
        rows = []
        for x in values:
            for a in range(3):
                q = base.copy()
                q[a] = x
                rows.append(q)
            rows.append(np.full(3, x))
        return np.array(rows)

    ks = np.arange(-3.0, 4.0)
    out["lattice"] = on_each_axis(np.concatenate([ks, ks + 0.5, np.nextafter(ks, -np.inf), np.nextafter(ks, np.inf)]))
    out["small_and_exact"] = on_each_axis([-0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 2.0**52 + 0.5, 2.0**53, -2.0**53])
    window = np.concatenate([[WINDOW_LO, np.nextafter(WINDOW_LO, np.inf), np.nextafter(TWO63, 0.0), TWO63 - 1024.0 * 255],
                             g.uniform(WINDOW_LO, TWO63, size=20)])
    assert ((window >= WINDOW_LO) & (window < TWO63)).all()
    rows = []
    for a in range(3):
        q = g.uniform(-300.0, 300.0, size=(len(window), 3))
        q[:, a] = window
        rows.append(q)
    out["window"] = np.concatenate(rows)                       # 72 points with one coordinate in [9.2e18, 2^63)
    out["extremes"] = on_each_axis([9.1e18, -9.1e18, TWO63, -TWO63, np.nextafter(-TWO63, 0.0), -9.2e18, 1e300, -1e300])
    # what turb's doubling carries into the window: p 2^m is in it for p in [9.2e18, 2^63) / 2^m, m <= 6, i.e. around 1.44e17 2^k
    out["turb_window"] = on_each_axis([x * 2.0**k for k in range(7) for x in (1.4376e17, 1.44e17, 1.4409e17)])
    out["non_finite"] = on_each_axis([np.inf, -np.inf, np.nan])[[i for i in range(12) if i % 4 != 3]]   # one coordinate each
    return out


def value_points():
    """points of the NoiseTexture::value check: |z| <= 8, so that the argument's own term stays small"""
    g = np.random.default_rng(78)
    p = g.uniform(-300.0, 300.0, size=(5000, 3))
    p[:, 2] = g.uniform(-8.0, 8.0, size=5000)
    return p


def axis_queries(n):
    """the u (or v) queries of an image n texels wide (high): k / n with its neighbours on both sides, the ends of [0, 1], and what the
    clamps and the saturating cast are for"""
    k = np.arange(n + 1) / n
    return np.concatenate([k, np.nextafter(k, -np.inf), np.nextafter(k, np.inf),
                           [0.0, -0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)],
                           [-1e-300, -1.0, 2.0, 1e300, np.inf, -np.inf, np.nan, 5e-324]])


def image_queries(width, height):
    """the Cartesian product of the per-axis lists -> uvp [n, 5] (p is not read by an image: a generic point)"""
    u, v = np.meshgrid(axis_queries(width), axis_queries(height), indexing="ij")
    q = np.empty((u.size, 5))
    q[:, 0], q[:, 1], q[:, 2:] = u.ravel(), v.ravel(), (0.25, -1.5, 3.0)
    return q


def uv_points():
    """the poles, both sides of the seam with both signs of zero, and 2000 random unit points"""
    g = np.random.default_rng(79)
    tiny = 1e-12
    fixed = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0.0], [-1, 0, -0.0], [0, 0, 1], [0, 0, -1], [0.6, 0.0, 0.8], [-0.6, 0.8, -0.0],
                      [-1, 0, tiny], [-1, 0, -tiny], [-1, 0, 5e-324], [-1, 0, -5e-324], [0.0, 1, 0.0], [-0.0, 1, -0.0], [-0.0, -1, 0.0]], dtype=np.float64)
    rnd = g.normal(size=(2000, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    return np.concatenate([fixed, rnd]), len(fixed)


def uvp(p, u=0.0, v=0.0):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    q = np.empty((len(p), 5))
    q[:, 0], q[:, 1], q[:, 2:] = u, v, p
    return q


# ---- the reference's values, computed once ---------------------------------------------------------------------------------------

_CACHE = {}


def reference(what, key, make):
    k = (what, key)
    if k not in _CACHE:
        _CACHE[k] = make()
    return _CACHE[k]


def all_noise_points():
    """every group of noise_points, in order: the one list the noise probes run (the device module also runs its first 1, 255, .. points)"""
    return reference("points", "noise", lambda: np.concatenate(list(noise_points().values())))


def noise_reference(name, table, ft):
    """(noise, turb) in longdouble of all_noise_points() over `table`, once per (name, precision)"""
    return reference("noise", (name, ft.__name__), lambda: (tr.noise(table, all_noise_points(), ft=ft), tr.turb(table, all_noise_points(), 7, ft=ft)))


def same_kind(got, want):
    """non-finite results match in kind and place: NaN where NaN, the same infinity where infinite"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want.astype(np.float64) if want.dtype == LD else want, dtype=np.float64)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
            and np.array_equal(np.isneginf(got), np.isneginf(want)))


def worst(got, want):
    """the largest |got - want| over the finite places, as a float"""
    fin = np.isfinite(want)
    return float(np.abs(got[fin].astype(LD) - want[fin]).max()) if fin.any() else 0.0


def check_noise(got, table, name, ft=np.float64):
    """got [n, 3] = (noise, turb, 0) of a probe over the first n of all_noise_points() against the reference -> (worst noise error,
    worst turb error) in units of e"""
    e = EPS[ft]
    n_ref, t_ref = (r[:len(got)] for r in noise_reference(name, table, ft))
    assert same_kind(got[:, 0], n_ref) and same_kind(got[:, 1], t_ref), "non-finite noise or turb differs in kind or place"
    dn, dt = worst(got[:, 0], n_ref) / e, worst(got[:, 1], t_ref) / e
    print(f"noise {name} {ft.__name__} n={len(got)}: worst {dn:.2f} e (bound {NOISE_EPS}), turb {dt:.2f} e (bound {TURB_EPS})")
    assert dn <= NOISE_EPS, (name, dn)
    assert dt <= TURB_EPS, (name, dt)
    return dn, dt


def check_value(got, table, scale, name, ft=np.float64):
    """got [n, 3] of a noise texture over value_points() against NoiseTexture::value -> the worst error in units of e"""
    e = EPS[ft]
    arg, want = reference("value", (name, ft.__name__),
                          lambda: (tr.noise_argument(table, scale, value_points(), ft=ft), tr.noise_value(table, scale, value_points(), ft=ft)))
    assert np.isfinite(want).all()
    sine_ulp = np.spacing(np.abs(np.sin(arg)).astype(ft)).astype(np.float64)
    bound = 0.5 * (10.0 * TURB_EPS * e + 3.0 * e * np.abs(arg).astype(np.float64) + sine_ulp)
    err = np.abs(got[:, 0].astype(LD) - want).astype(np.float64)
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    ratio = float((err / bound).max())
    print(f"value {name} {ft.__name__}: worst {float(err.max()) / e:.2f} e, {ratio:.4f} of its bound")
    assert (err <= bound).all(), (name, ratio)
    return float(err.max()) / e


def ulp_up(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)) * (1.0 + 2.0**-40))


def check_sphere_uv(got):
    """got [n, 3] = (u, v, 0) of uv_points() against sphere_uv -> (worst u error, worst v error), absolute"""
    u, v, phi, theta, a = reference("uv", 0, lambda: tr.sphere_uv(uv_points()[0]))
    two_pi, pi = 2.0 * np.pi, np.pi
    bu = (2.0 * ulp_up(a) + 0.5 * ulp_up(phi)) / two_pi + 0.5 * ulp_up(u)
    bv = 2.0 * ulp_up(theta) / pi + 0.5 * ulp_up(v)
    eu = np.abs(got[:, 0].astype(LD) - u).astype(np.float64)
    ev = np.abs(got[:, 1].astype(LD) - v).astype(np.float64)
    ru, rv = float((eu / bu).max()), float((ev / bv).max())
    print(f"sphere_uv: worst u {float(eu.max()):.3e} ({ru:.3f} of its bound), v {float(ev.max()):.3e} ({rv:.3f} of its bound)")
    assert (eu <= bu).all() and (ev <= bv).all(), (ru, rv)
    return float(eu.max()), float(ev.max())


def check_image(got, width, height, queries, ft=np.float64):
    """got [n, 3] of an image texture: the reference's colour, bit for bit"""
    want = tr.image_value(image(width, height), queries[:, 0], queries[:, 1], ft=ft).astype(np.float64)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        (width, height, queries[np.nonzero((got != want).any(axis=1))[0][:5]].tolist())


# ---- the census ---------------------------------------------------------------------------------------------------------------------

def census():
    """what the point sets hold: the size of every group, how many image queries fall into each texel column and row, how many noise
    points have a non-finite result.  Asserted against tests/golden/texture_kats.json, so that a set cannot quietly stop testing what it
    is for."""
    t = tables()
    pts = noise_points()
    every = all_noise_points()
    n_ref, t_ref = noise_reference("random", t["random"], np.float64)
    in_window = ((every >= WINDOW_LO) & (every < TWO63)).any(axis=1)
    carried = np.zeros(len(every), dtype=bool)
    for m in range(1, 7):
        carried |= ((every * 2.0**m >= WINDOW_LO) & (every * 2.0**m < TWO63)).any(axis=1)
    out = {"noise_groups": {k: len(v) for k, v in pts.items()},
           "noise_points_in_window": int(in_window.sum()),
           "noise_points_turb_carries_into_window": int((carried & ~in_window).sum()),
           "noise_non_finite": int((~np.isfinite(n_ref)).sum()), "turb_non_finite": int((~np.isfinite(t_ref)).sum()),
           "value_points": len(value_points()), "uv_points": len(uv_points()[0]), "images": {}}
    for w, h in IMAGE_SIZES:
        q = image_queries(w, h)
        i, j = tr.image_texel(w, h, q[:, 0], q[:, 1])
        out["images"][f"{w}x{h}"] = {"queries": len(q), "columns": np.bincount(i, minlength=w).tolist(), "rows": np.bincount(j, minlength=h).tolist()}
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def measure_cpu(rt, orc):
    """the measured maxima of the two CPU twins against the reference, in units of e (sphere_uv: absolute)"""
    sc, ids = build_scene(rt)
    t = tables()
    every, vp, pts = all_noise_points(), value_points(), uv_points()[0]
    rows = {}
    for row, ft, probe in (("twin_f64", np.float64, lambda mode, tex, q: rt.texture_host(sc, mode, tex, q)),
                           ("twin_f32", np.float32, lambda mode, tex, q: orc.flat_f32_texture(sc, mode, tex, q))):
        r = {}
        for k, name in enumerate(("random", "revealing")):
            dn, dt = check_noise(probe(1, k, uvp(every)), t[name], name, ft)
            r[f"noise_{name}_e"], r[f"turb_{name}_e"] = round(dn, 3), round(dt, 3)
            r[f"value_{name}_e"] = round(check_value(probe(0, ids[f"noise_{name}"], uvp(vp)), t[name], SCALES[k], name, ft), 3)
        if ft is np.float64:
            eu, ev = check_sphere_uv(probe(2, 0, uvp(pts)))
            r["sphere_uv_u_abs"], r["sphere_uv_v_abs"] = eu, ev
        rows[row] = r
    return rows


if __name__ == "__main__":
    import argparse
    import orc
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", help="JSON file of the device's maxima, as the GPU module writes it")
    a = ap.parse_args()
    doc = {"census": census(), "bounds": {"noise_e": NOISE_EPS, "turb_e": TURB_EPS},
           "maxima": {"note": "measured against tests/tex_reference.py; recorded, not asserted: the bounds are derived in tests/texture_kats.py",
                      **measure_cpu(orc.rt(), orc)}}
    if a.device:
        with open(a.device) as f:
            doc["maxima"]["device"] = json.load(f)
    elif os.path.exists(GOLDEN) and "device" in golden().get("maxima", {}):
        doc["maxima"]["device"] = golden()["maxima"]["device"]
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
