"""Helpers of tests/test_ray_color.py and tests/test_ray_color_gpu.py: the ray lists of the radiance-query tests (the camera rays of a
frame with their stream positions, incoherent bounce rays made on the CPU), a 64-bit draw of a Philox stream at a word position, the
sums the entries must make, and the call of the refusal table.  Nothing of csrc/ is in the formulas.  Test infrastructure."""
import ctypes as C
import json
import os

import numpy as np

import hit_reference as HR
import orc

W, H = 24, 16
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)  # a lone lane, partial waves, partial workgroups
RTOL = 1e-12
REFUSALS = json.load(open(os.path.join(orc.ROOT, "tests", "golden", "ray_color_refusals.json")))
same_bits = HR.same_bits


def camera_list(rt, scene, w, h, sample, global_seed, spp=1):
    """the camera rays of the full-width frame, [h * w * spp, 7] in pixel-seed order j * w + i, and the word each ray's stream stands at
    behind Camera::get_ray (rt1w_lab_camera_rays_pos_host)"""
    rays, word = rt.camera_rays_pos_host(scene, w, h, spp, sample_offset=sample, global_seed=global_seed)
    return np.ascontiguousarray(rays.reshape(-1, 8)[:, :7]), np.ascontiguousarray(word.reshape(-1))


def bounce_rays(rt, scene, n, seed=1):
    """n incoherent rays, [n, 7], made on the CPU: from the first hits of the 24 x 16 x 4 camera rays (rt1w_lab_hit_host) along the
    normal plus a vector of a fixed numpy stream -- neighbours in the list point into unrelated directions --, the list shuffled; where
    the camera rays hit too little, rays from points around the camera into directions of the same stream.  Times in [0, 1)."""
    g = np.random.default_rng(seed)
    cam = HR.camera_rays(rt, scene, W, H, 4, 0, seed)
    rec, _ = rt.hit_host(scene, cam)
    hit = rec[:, 0] == 1.0
    o = rec[hit, 2:5]
    d = rec[hit, 5:8] + g.uniform(-0.9, 0.9, size=(int(hit.sum()), 3))
    extra = max(0, n - len(o))
    o = np.concatenate([o, cam[:extra, 0:3] + g.uniform(-1.0, 1.0, size=(extra, 3))])
    d = np.concatenate([d, g.uniform(-1.0, 1.0, size=(extra, 3))])
    rays = np.concatenate([o, d, g.uniform(0.0, 1.0, size=(len(o), 1))], axis=1)
    assert len(rays) >= n and np.all(np.isfinite(rays))
    return np.ascontiguousarray(rays[g.permutation(len(rays))[:n]])


def f64_at(stream, sample, global_seed, word):
    """The f64 draw of the stream of (pixel seed, sample, global_seed) that starts at word `word` (4 * block + word in block): a 64-bit
    draw takes an even-aligned pair, low word first, of Philox4x32-10 block (block, sample, global_seed, "REND") under the key (seed low,
    seed high) (tests/test_num_contract.py: test_word_stream_is_philox_blocks_in_order, test_draw_shapes)"""
    word += word & 1
    ctr = np.array([word >> 2, sample, global_seed, 0x52454E44], dtype=np.uint32)
    key = np.array([stream & 0xFFFFFFFF, stream >> 32], dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    orc.A.orc_philox(ctr.ctypes.data_as(C.c_void_p), key.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    k = word & 3
    return float((int(out[k + 1]) << 32 | int(out[k])) >> 11) * 2.0 ** -53


def into_sampled(total, spp):
    """Color::into_sampled color.rs:14-21: NaN scrub of the sum, then * (1 / spp)"""
    t = np.where(np.isnan(total), 0.0, total)
    return t * np.float64(1.0 / spp)


def chunked_sum(singles, chunk):
    """float64 sums of single-sample results [spp, n, 3] as the entries make them: per work item of `chunk` samples in sample order from
    +0.0, then the items in order from +0.0"""
    spp = len(singles)
    total = np.zeros_like(singles[0])
    for c0 in range(0, spp, chunk):
        part = np.zeros_like(singles[0])
        for s in range(c0, min(c0 + chunk, spp)):
            part = part + singles[s]
        total = total + part
    return total


class Arena:
    """the three buffers of a call laid out as a case of the golden table asks: each on its own, or one at a byte offset into another"""

    def __init__(self, case, rays, words, alloc, upload):
        names = ("rays", "start_word", "out")
        self.mem = {k: alloc(4096) for k in names}
        self.ptr = {k: self.mem[k][0] for k in names}
        if case.get("overlap"):
            laid, base, offset = case["overlap"]
            self.ptr[laid] = self.mem[base][0] + offset
        upload(self.ptr["rays"], rays)
        upload(self.ptr["start_word"], words)
        for k in case.get("null", []):
            if k in self.ptr:
                self.ptr[k] = None


def table_params(rt, case, n):
    return rt.RayColorParams(case.get("n", n), 0, case.get("global_seed", 0), case.get("spp", 2), case.get("sample_offset", 0),
                             case.get("max_depth", 50), case.get("chunk", 0), case.get("stride", 7), case.get("flags", 0), 0, case.get("reserved", 0))


def table_rays(stride, count=4):
    """`count` times the table's plain ray, in records of `stride` doubles (the doubles behind the time: 0.001 and inf, rt1w_hit's bounds)"""
    ok = [float(x) for x in REFUSALS["ok"]] + [0.001, float("inf")]
    return np.array([ok[:max(stride, 7)]] * count, dtype=np.float64)


def run_table(rt, call, alloc, upload, download):
    """every case of the golden table through call(params or None, rays, start_word, out) -> code, with the text of every refusal"""
    words = np.array([10, 11, 12, 13], dtype=np.uint32)
    for case in REFUSALS["refusals"]:
        rays = table_rays(case.get("stride", 7))
        ar = Arena(case, rays, words, alloc, upload)
        p = None if "params" in case.get("null", []) else table_params(rt, case, len(rays))
        rc = call(p, ar.ptr["rays"], ar.ptr["start_word"], ar.ptr["out"])
        assert rc == case["code"] == rt.ERR_INVALID, (case["name"], rc)
        assert rt.last_error() == case["text"], (case["name"], rt.last_error())
    for case in REFUSALS["accepted"]:
        rays = table_rays(case.get("stride", 7))
        ar = Arena(case, rays, np.full(4, 10, dtype=np.uint32), alloc, upload)
        rc = call(table_params(rt, case, len(rays)), ar.ptr["rays"], ar.ptr["start_word"], ar.ptr["out"])
        assert rc == rt.OK, (case["name"], rc, rt.last_error())
        out = download(ar.ptr["out"], (len(rays), 3), np.float64)
        assert np.all(np.isfinite(out)) and np.all(out >= 0.0), case["name"]
        if case.get("max_depth", 50) == 0:
            assert np.all(out == 0.0), case["name"]


def nonfinite_lists():
    """(the table's plain ray and, interleaved with it, one ray per defect of the table; which of them are not traced)"""
    ok = [float(x) for x in REFUSALS["ok"]]
    rows, bad = [ok], [False]
    for m in REFUSALS["nonfinite"]:
        r = list(ok)
        r[m["slot"]] = float(m["value"])
        rows += [r, ok]
        bad += [True, False]
    return np.array(rows, dtype=np.float64), np.array(bad)


def check_nonfinite(rt, scene, query):
    """query(rays, first_stream, max_depth) -> [n, 3] means of 3 samples: the rays that are not traced return the background (0 at
    max_depth 0), the others what a call without them returns at their shifted first_stream"""
    rays, bad = nonfinite_lists()
    bg = scene.flat(6).view(np.float64)[24:27]
    got = query(rays, 40, 50)
    assert same_bits(got[bad], np.repeat(into_sampled(bg + bg + bg, 3)[None], int(bad.sum()), axis=0)), "an untraced ray is three misses"
    for k in np.flatnonzero(~bad):
        assert same_bits(got[k:k + 1], query(rays[k:k + 1], 40 + int(k), 50)), ("a bad neighbour changes nothing", int(k))
    assert np.all(query(rays, 40, 0) == 0.0), "max_depth 0 gives 0, traced or not"
    return got


class Device:
    """device memory from the HIP runtime librt1w.so itself uses (what a torch tensor's data_ptr() hands over), for the table's layouts"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.all = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        assert self.hip.hipMemset(p, 0, nbytes) == 0
        self.all.append(p.value)
        return p.value, None

    def upload(self, ptr, a):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0  # HostToDevice

    def download(self, ptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # DeviceToHost
        return out

    def free(self):
        for p in self.all:
            self.hip.hipFree(p)
        self.all = []
