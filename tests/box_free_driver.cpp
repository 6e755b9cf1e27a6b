/* box_free_driver.cpp -- TEST INFRASTRUCTURE (tests/test_box_free.py), not product.
 *
 * The kernel core (rt_core.h) built for the host with -DRT_BOX_FREE=1 around the library's own generated Topos: per ray the boxed
 * sweep's answer (the parent's text: rt_sweep_static with `/`), the box-free sweep's (rt_closest_hit_free) with its verdict, and what
 * rt_closest_hit makes of the two.  BF_TOPO_H defines Topo0 ..., CfgB0 ... and BF_CASES, a list of `case k: trace<CfgBk>(...)`.
 * With -DBF_NEST_MAIN instead: a stand-alone program over the generator's host functions (rt_box_free.h), see main below. */
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#ifndef BF_NEST_MAIN
#include "rt_core.h"
#include BF_TOPO_H

namespace {
struct NoStack { int sp = 0; void push(uint32_t) {} uint32_t pop() { return 0u; } };

struct Out { uint64_t *t_boxed, *t_free, *t_final; uint32_t *p_boxed, *p_free, *p_final; uint8_t* bad; };

template <class Cfg>
void trace(const RtSceneView& sc, const double* rays, uint64_t lo, uint64_t hi, const Out& o) {
    typedef typename Cfg::Topo Topo;
    static_assert(RtBoxFreeTopo<Topo>::value && !Cfg::media, "the driver is for units that sweep without boxes");
    const RtGlobalNodes ns{sc.nodes};
    RtRng rng = rt_rng_pixel_sample(1u, 2u, 3u); /* a media-free sweep draws nothing */
    NoStack stk;
    for (uint64_t i = lo; i < hi; ++i) {
        const double* r = rays + 8u * i;
        RtRay ray; ray.o = rt_v3(r[0], r[1], r[2]); ray.d = rt_v3(r[3], r[4], r[5]); ray.time = 0.0;
        RtRayOD w; w.o = ray.o; w.d = ray.d;
        const double t_min = r[6], t_max = r[7];
        double t = t_max; uint32_t prim = RT_NONE, scope;
        const RtSlabNone none;
        rt_sweep_static<Topo, Cfg, true, Topo::root, Topo::skip[Topo::root]>(sc, ns, w, rt_inv3(w.d), 0.0, t_min, rt_isnan(t_min), rng, true, none, t, prim);
        std::memcpy(&o.t_boxed[i], &t, 8); o.p_boxed[i] = prim;
        const bool bad = rt_closest_hit_free<Cfg>(sc, ns, w, 0.0, t_min, t_max, t, prim);
        std::memcpy(&o.t_free[i], &t, 8); o.p_free[i] = prim; o.bad[i] = bad ? 1 : 0;
        rt_closest_hit<Cfg>(sc, ns, ray, t_min, t_max, rng, stk, t, prim, scope);
        std::memcpy(&o.t_final[i], &t, 8); o.p_final[i] = prim;
    }
}
}

extern "C" int bf_trace(int which, const RtNode* nodes, uint32_t n_nodes, uint32_t root, const double* rays, uint64_t n, uint64_t* t_boxed,
                        uint32_t* p_boxed, uint64_t* t_free, uint32_t* p_free, uint8_t* bad, uint64_t* t_final, uint32_t* p_final, int threads) {
    RtSceneView sc;
    std::memset(&sc, 0, sizeof sc);
    sc.nodes = nodes; sc.n_nodes = n_nodes; sc.root = root;
    const Out o{t_boxed, t_free, t_final, p_boxed, p_free, p_final, bad};
    if (threads < 1) threads = 1;
    std::vector<std::thread> pool;
    int rc = 0;
    for (int k = 0; k < threads; ++k) {
        const uint64_t lo = n * (uint64_t)k / (uint64_t)threads, hi = n * (uint64_t)(k + 1) / (uint64_t)threads;
        pool.emplace_back([&, lo, hi] {
            switch (which) {
                BF_CASES
                default: rc = -1;
            }
        });
    }
    for (std::thread& th : pool) th.join();
    return rc;
}

#else
/* usage: prog NODES.bin ROOT [INDEX PLANE ULPS]: the flat node array of a scene, optionally with bound PLANE (0-2 min, 3-5 max) of node
 * INDEX moved by ULPS units in the last place; prints `nested 0|1`, `eligible 0|1` and the members the generator would declare */
#include <cstdlib>
#include "rt_box_free.h"

int main(int argc, char** argv) {
    if (argc != 3 && argc != 6) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<RtNode> N;
    RtNode nd;
    while (std::fread(&nd, sizeof nd, 1, f) == 1) N.push_back(nd);
    std::fclose(f);
    const uint32_t root = (uint32_t)std::atoi(argv[2]);
    if (argc == 6) {
        const size_t i = (size_t)std::atoi(argv[3]);
        const int plane = std::atoi(argv[4]), ulps = std::atoi(argv[5]);
        if (i >= N.size() || plane < 0 || plane > 5) return 2;
        int64_t bits;
        std::memcpy(&bits, &N[i].d[plane], 8);
        bits += (int64_t)ulps; /* sign and magnitude: away from zero for ulps > 0, whatever the sign */
        std::memcpy(&N[i].d[plane], &bits, 8);
    }
    std::printf("nested %d\n", rt1w::box_free_boxes_nested(N.data(), (uint32_t)N.size(), root) ? 1 : 0);
    std::printf("eligible %d\n", rt1w::box_free_eligible(N.data(), (uint32_t)N.size(), root) ? 1 : 0);
    std::fputs(rt1w::box_free_members(N.data(), (uint32_t)N.size(), root).c_str(), stdout);
    return 0;
}
#endif
