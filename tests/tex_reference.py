"""An independent statement of the shading-side leaf functions, written from the reference's own text and from nothing else:
    Perlin::new / noise / turb / perlin_interp   src/perlin.rs:15-43, 46-72, 74-86, 88-106
    Texture::value of CheckerTexture, NoiseTexture and DynamicImage   src/texture.rs:46-55, 57-65, 67-88
    sphere_uv   src/math.rs:67-71
No library is loaded and nothing of csrc/rt_core.h or oracle/oracle.cpp is shared: numpy and Python integers only.  The lines are
cited, none of their text is held.

How each number is taken:
  * what decides an INDEX is done in the reference's own arithmetic, so the index is decided exactly: `floor`, `p - floor(p)`,
    `u * width` and `1 - v` are single operations of the working float type (float64, or float32 for the f32 twin); `as isize` and
    `as u32` are Python integers saturated as Rust's casts saturate (NaN -> 0); `i + di` wraps modulo 2^64 (the release build);
  * what is a VALUE (perlin_interp, the turbulence sum, the sine of the noise texture, acos and atan2 of sphere_uv) is numpy
    longdouble (64 bits of mantissa or more: asserted), in the reference's order of evaluation;
  * an image colour is float(byte) * (1 / 255) in the working type: the reference's own two operations, so it is exact.

`tables` is (ranvec [256, 3], perm_x [256], perm_y [256], perm_z [256]); points are [n, 3] arrays of the working type `ft`."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy longdouble is no wider than double here: the reference would prove nothing"

POINT_COUNT = 256
ISIZE_MIN, ISIZE_MAX, U64 = -2**63, 2**63 - 1, 2**64
U32_MAX = 2**32 - 1
PI = LD(np.float64(np.pi))   # Float::PI(): the working type's constant, not a wider one (math.rs:68-70)


def as_isize(x):
    """`x as isize` of one float (perlin.rs:51-53): truncation, saturated at the ends of i64, NaN -> 0"""
    x = float(x)
    if x != x:
        return 0
    if x == float("inf"):
        return ISIZE_MAX
    if x == float("-inf"):
        return ISIZE_MIN
    return min(max(int(x), ISIZE_MIN), ISIZE_MAX)


def _as_isize_u64(f):
    """as_isize of every element of a float array, as the two's-complement uint64 that `i + di` then wraps in"""
    f = np.asarray(f)
    small = np.abs(f) < 2.0**62               # false for NaN
    out = np.zeros(f.shape, dtype=np.uint64)
    out[small] = f[small].astype(np.int64).view(np.uint64)
    for at in zip(*np.nonzero(~small)):
        out[at] = np.uint64(as_isize(f[at]) % U64)
    return out


def perlin_interp(c, u, v, w):
    """perlin.rs:88-106.  c [n, 2, 2, 2, 3] and u, v, w [n] in longdouble"""
    one, two, three = LD(1), LD(2), LD(3)
    uu = u * u * (three - two * u)
    vv = v * v * (three - two * v)
    ww = w * w * (three - two * w)
    accum = np.zeros(u.shape, dtype=LD)
    for i in range(2):
        for j in range(2):
            for k in range(2):
                wx, wy, wz = u - LD(i), v - LD(j), w - LD(k)
                cc = c[:, i, j, k]
                dot = cc[:, 0] * wx + cc[:, 1] * wy + cc[:, 2] * wz
                accum = accum + (LD(i) * uu + LD(1 - i) * (one - uu)) * (LD(j) * vv + LD(1 - j) * (one - vv)) * \
                    (LD(k) * ww + LD(1 - k) * (one - ww)) * dot
    return accum


def noise(tables, p, ft=np.float64):
    """Perlin::noise (perlin.rs:46-72) of points p [n, 3] -> longdouble [n]"""
    ranvec, perm_x, perm_y, perm_z = tables
    ranvec = np.asarray(ranvec, dtype=ft).reshape(POINT_COUNT, 3).astype(LD)
    perm = [np.asarray(q, dtype=np.int64).reshape(POINT_COUNT) for q in (perm_x, perm_y, perm_z)]
    with np.errstate(over="ignore"):
        p = np.asarray(p, dtype=ft).reshape(-1, 3)   # a float64 beyond float32's range becomes an infinity, as a cast does
    with np.errstate(invalid="ignore"):
        fl = np.floor(p)
        frac = (p - fl).astype(ft)             # :47-49, one subtraction of the working type
    ijk = _as_isize_u64(fl)                    # :51-53
    c = np.empty((len(p), 2, 2, 2, 3), dtype=LD)
    mask = np.uint64(POINT_COUNT - 1)
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                with np.errstate(over="ignore"):
                    i = ((ijk[:, 0] + np.uint64(di)) & mask).astype(np.int64)   # :60-62, wrapping
                    j = ((ijk[:, 1] + np.uint64(dj)) & mask).astype(np.int64)
                    k = ((ijk[:, 2] + np.uint64(dk)) & mask).astype(np.int64)
                c[:, di, dj, dk] = ranvec[perm[0][i] ^ perm[1][j] ^ perm[2][k]]   # :64-66
    with np.errstate(invalid="ignore"):
        return perlin_interp(c, frac[:, 0].astype(LD), frac[:, 1].astype(LD), frac[:, 2].astype(LD))


def turb(tables, p, depth=7, ft=np.float64):
    """Perlin::turb (perlin.rs:74-86) -> longdouble [n]"""
    with np.errstate(over="ignore"):
        p = np.asarray(p, dtype=ft).reshape(-1, 3)
    accum = np.zeros(len(p), dtype=LD)
    temp_p = p.copy()
    weight = LD(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(depth):
            accum = accum + weight * noise(tables, temp_p, ft)
            weight = weight * LD(0.5)
            temp_p = (temp_p * ft(2.0)).astype(ft)   # exact but for the overflow to infinity, which the reference has too
    return np.abs(accum)


def noise_argument(tables, scale, p, ft=np.float64):
    """scale * z + 10 * turb(p, 7): what NoiseTexture::value takes the sine of (texture.rs:62) -> longdouble [n]"""
    p = np.asarray(p, dtype=ft).reshape(-1, 3)
    return LD(ft(scale)) * p[:, 2].astype(LD) + LD(10) * turb(tables, p, 7, ft)


def noise_value(tables, scale, p, ft=np.float64):
    """NoiseTexture::value (texture.rs:57-65), one channel -> longdouble [n]"""
    with np.errstate(invalid="ignore"):
        return LD(0.5) * (LD(1) + np.sin(noise_argument(tables, scale, p, ft)))


def as_u32(x):
    """`x as u32` of a float array (texture.rs:73-74): truncation, saturated to 0 .. 2^32 - 1, NaN -> 0 -> int64 array"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(x.shape, dtype=np.int64)
    ok = x > 0.0                               # false for NaN
    big = ok & (x >= 2.0**32)
    out[big] = U32_MAX
    mid = ok & ~big
    out[mid] = np.trunc(x[mid]).astype(np.int64)
    return out


def _clamp01(x):
    """f64::clamp(0.0, 1.0) as texture.rs:69-70 calls it: NaN stays NaN, -0.0 stays -0.0"""
    x = np.asarray(x)
    return np.where(x < 0, x.dtype.type(0), np.where(x > 1, x.dtype.type(1), x))


def image_texel(width, height, u, v, ft=np.float64):
    """the texel (column i, row j counted from the top) that DynamicImage::value reads (texture.rs:69-77)"""
    u = _clamp01(np.asarray(u, dtype=ft))
    v = (ft(1.0) - _clamp01(np.asarray(v, dtype=ft))).astype(ft)
    with np.errstate(invalid="ignore"):
        i = as_u32((u * ft(width)).astype(ft))   # ONE multiplication of the working type
        j = as_u32((v * ft(height)).astype(ft))
    return np.minimum(i, width - 1), np.minimum(j, height - 1)


def image_value(rgb8, u, v, ft=np.float64):
    """DynamicImage::value (texture.rs:67-88) of rgb8 [height, width, 3], row 0 on top -> [n, 3] of the working type, exact"""
    rgb8 = np.asarray(rgb8, dtype=np.uint8)
    height, width = rgb8.shape[:2]
    i, j = image_texel(width, height, u, v, ft)
    colour_scale = ft(ft(1.0) / ft(255.0))     # :81
    return (rgb8[j, i].astype(ft) * colour_scale).astype(ft)


def checker(p, ft=np.float64, margin=1e-9):
    """CheckerTexture::value (texture.rs:46-55) -> (odd [n]: the point takes the `odd` child, keep [n]: |sines| > margin, so that the
    sign does not hang on the sine's last bits)"""
    p = np.asarray(p, dtype=ft).reshape(-1, 3).astype(LD)
    sines = np.sin(LD(10) * p[:, 0]) * np.sin(LD(10) * p[:, 1]) * np.sin(LD(10) * p[:, 2])
    return sines < 0, np.abs(sines) > margin


def sphere_uv(p):
    """sphere_uv (math.rs:67-71) of points [n, 3] -> (u, v, phi, theta, atan2 value) in longdouble, pi being the float64 constant"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3).astype(LD)
    theta = np.arccos(-p[:, 1])
    a = np.arctan2(-p[:, 2], p[:, 0])
    phi = a + PI
    return phi / (LD(2) * PI), theta / PI, phi, theta, a


# ---- Perlin::new over a word stream ------------------------------------------------------------------------------------------------
# The draws are rand 0.8's, in the shapes tests/test_num_contract.py pins (test_draw_shapes): a 64-bit draw is an even-aligned pair of
# 32-bit words, low word first; gen_range(-1.0..1.0) puts 52 bits under the exponent of 1.0, subtracts 1, scales by high - low, adds
# low and retries at >= high; gen_range(0..n) of the shuffle is one 32-bit word widened by n, retried outside the power-of-two zone.

def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., Random123) on Python integers: one block of four words"""
    c0, c1, c2, c3 = (int(x) for x in ctr)
    k0, k1 = (int(x) for x in key)
    m32 = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m32, (p0 >> 32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return [c0, c1, c2, c3]


def build_stream_words(build_seed, n_words):
    """the first n_words of a scene's build stream (include/rt1w_num.h, "Word stream"): block b = Philox((b, 0, 0, "BLDS"), seed)"""
    key = (build_seed & 0xFFFFFFFF, build_seed >> 32)
    out = []
    for b in range((n_words + 3) // 4):
        out += philox4x32_10((b, 0, 0, 0x424C4453), key)
    return out[:n_words]


class Words:
    def __init__(self, words, pos=0):
        self.w, self.pos = words, pos

    def u32(self):
        self.pos += 1
        return int(self.w[self.pos - 1])

    def u64(self):
        self.pos += self.pos & 1
        self.pos += 2
        return int(self.w[self.pos - 1]) << 32 | int(self.w[self.pos - 2])

    def range_f64(self, low, high):
        while True:
            v12 = float(np.array((self.u64() >> 12) | 0x3FF0000000000000, dtype=np.uint64).view(np.float64))
            res = (v12 - 1.0) * (high - low) + low
            if res < high:
                return res

    def below(self, n):
        zone = ((n << (32 - n.bit_length())) - 1) & 0xFFFFFFFF
        while True:
            m = self.u32() * n
            if (m & 0xFFFFFFFF) <= zone:
                return m >> 32


def perlin_new(words, pos=0):
    """Perlin::new (perlin.rs:25-43) over `words` from word `pos` -> (tables, the word the stream stands at afterwards).  ranvec is the
    longdouble v / |v| of the drawn vector: what a float64 normalize may differ from by its own roundings"""
    g = Words(words, pos)
    ranvec = np.empty((POINT_COUNT, 3), dtype=LD)
    for n in range(POINT_COUNT):                                  # :28-35
        v = np.array([g.range_f64(-1.0, 1.0) for _ in range(3)], dtype=np.float64).astype(LD)
        ranvec[n] = v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    perms = []
    for _ in range(3):                                            # generate_perm :15-23; shuffle: from the end, gen_range(0..i + 1)
        q = list(range(POINT_COUNT))
        for i in range(POINT_COUNT - 1, 0, -1):
            j = g.below(i + 1)
            q[i], q[j] = q[j], q[i]
        perms.append(np.array(q, dtype=np.uint32))
    return (ranvec, perms[0], perms[1], perms[2]), g.pos
