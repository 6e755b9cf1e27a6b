/* hit_driver.cpp -- TEST INFRASTRUCTURE (tests/test_hit.py), not product.
 *
 * A stand-alone program around the host build of rt_hit.h, made to be compiled with -fsanitize=address,undefined: the ray query of the
 * product, one ray at a time, over a scene's flattened node array read from a file.  Nothing else of the product is linked.
 *
 * usage: hit_driver NODES.bin ROOT VARIANT RAYS.bin FIRST_STREAM SAMPLE GLOBAL_SEED OUT.bin
 *   NODES.bin  the array rt1w_scene_copy_flat(.., 0, ..) exports (96-byte records); ROOT the index of the world's record
 *   VARIANT    0 .. 5, the kernel variant whose walk runs (csrc/rt_flat.h)
 *   RAYS.bin   double[n][9]
 *   OUT.bin    receives double[n][12], then uint32[n]
 * Prints `checksum <16 hex digits>`: FNV-1a over the bytes written.  Exit 0; 2 bad usage or files; 3 a traversal stack overflowed. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_hit.h"

namespace {
struct HostStack {
    uint32_t e[RT_STACK_CAP];
    int sp = 0;
    bool overflow = false;
    void push(uint32_t v) { if (sp >= RT_STACK_CAP) { overflow = true; return; } e[sp++] = v; }
    void poke(int above, uint32_t v) { if (sp + above >= RT_STACK_CAP) { overflow = true; return; } e[sp + above] = v; }
    uint32_t pop() { return e[--sp]; }
};

template <class T>
bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    T x;
    while (std::fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return true;
}

template <class Cfg>
bool run(const RtSceneView& sc, const RtHitParams& hp, const double* rays, double* out, uint32_t* node) {
    HostStack stk;
    const RtGlobalNodes ns{sc.nodes};
    for (uint64_t r = 0; r < hp.n; ++r) {
        rt_hit_ray<Cfg>(sc, ns, rays + r * RT_HIT_RAY, r, hp, stk, out + r * RT_HIT_RECORD, node[r]);
        if (stk.overflow) return false;
    }
    return true;
}
struct Ray9 { double v[RT_HIT_RAY]; };
}

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    std::vector<RtNode> nodes;
    std::vector<Ray9> rays;
    if (!read_all(argv[1], nodes) || !read_all(argv[4], rays) || nodes.empty() || rays.empty()) return 2;
    RtSceneView sc;
    std::memset(&sc, 0, sizeof sc);
    sc.root = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    sc.n_nodes = (uint32_t)nodes.size();
    if (sc.root >= sc.n_nodes) return 2;
    nodes.push_back(RtNode{}); /* the spare record the walks may read beside the last one */
    sc.nodes = nodes.data();
    RtHitParams hp;
    hp.n = rays.size();
    hp.first_stream = std::strtoull(argv[5], nullptr, 10);
    hp.sample = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    hp.global_seed = std::strtoull(argv[7], nullptr, 10);
    hp.flags = 0u;
    std::vector<double> out(rays.size() * RT_HIT_RECORD);
    std::vector<uint32_t> node(rays.size());
    bool ok;
    switch (std::atoi(argv[3])) {
        case 0: ok = run<RtCfgV0>(sc, hp, rays[0].v, out.data(), node.data()); break;
        case 1: ok = run<RtCfgV1>(sc, hp, rays[0].v, out.data(), node.data()); break;
        case 2: ok = run<RtCfgV2>(sc, hp, rays[0].v, out.data(), node.data()); break;
        case 3: ok = run<RtCfgV3>(sc, hp, rays[0].v, out.data(), node.data()); break;
        case 4: ok = run<RtCfgV4>(sc, hp, rays[0].v, out.data(), node.data()); break;
        case 5: ok = run<RtCfgV5>(sc, hp, rays[0].v, out.data(), node.data()); break;
        default: return 2;
    }
    if (!ok) return 3;
    FILE* f = std::fopen(argv[8], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fwrite(node.data(), sizeof(uint32_t), node.size(), f);
    std::fclose(f);
    uint64_t h = 0xCBF29CE484222325ull;
    auto feed = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001B3ull; };
    feed(out.data(), out.size() * sizeof(double));
    feed(node.data(), node.size() * sizeof(uint32_t));
    std::printf("checksum %016llx\n", (unsigned long long)h);
    return 0;
}
