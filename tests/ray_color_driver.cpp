/* ray_color_driver.cpp -- TEST INFRASTRUCTURE (tests/test_ray_color.py), not product.
 *
 * A stand-alone program around the CPU twin of rt1w_ray_color (csrc/aov_host.cpp: rt1w_lab_ray_color_host), made to be compiled together
 * with the host sources it needs (scene.cpp, scenes.cpp, output.cpp, aov_host.cpp) under -fsanitize=address,undefined: a reference arm's
 * scene is built here and a list of rays read from a file goes through the twin.  No HIP, no GPU.
 *
 * usage: ray_color_driver ARM ASPECT RAYS.bin STRIDE WORDS.bin|- FIRST_STREAM SPP SAMPLE_OFFSET GLOBAL_SEED MAX_DEPTH CHUNK FLAGS OUT.bin
 *   ARM        a scene arm of main.rs:815-937 that needs no image (not 3), built with build seed 1 at aspect ratio ASPECT
 *   RAYS.bin   double[n][STRIDE]; WORDS.bin uint32[n], or - for none
 *   OUT.bin    receives double[n][3]
 * Prints `checksum <16 hex digits>`: FNV-1a over the bytes written.  Exit 0; 2 bad usage or files; 3 the scene; 4 the twin refused. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt1w.h"
#include "walk_lab.h"

namespace {
template <class T>
bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    T x;
    while (std::fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return true;
}
}

int main(int argc, char** argv) {
    if (argc != 14) return 2;
    std::vector<double> rays;
    std::vector<uint32_t> words;
    const uint32_t stride = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const bool with_words = std::strcmp(argv[5], "-") != 0;
    if (stride < 7u || !read_all(argv[3], rays) || rays.empty() || rays.size() % stride || (with_words && !read_all(argv[5], words))) return 2;
    const uint64_t n = rays.size() / stride;
    if (with_words && words.size() != n) return 2;
    rt1w_scene* scene = nullptr;
    uint32_t defaults[3];
    if (rt1w_scene_build_reference(std::atoi(argv[1]), 1u, std::atof(argv[2]), nullptr, 0u, 0u, &scene, defaults) < 0) return 3;
    rt1w_ray_color_params p;
    std::memset(&p, 0, sizeof p);
    p.n = n; p.stride = stride;
    p.first_stream = std::strtoull(argv[6], nullptr, 10);
    p.spp = (uint32_t)std::strtoul(argv[7], nullptr, 10);
    p.sample_offset = (uint32_t)std::strtoul(argv[8], nullptr, 10);
    p.global_seed = std::strtoull(argv[9], nullptr, 10);
    p.max_depth = (uint32_t)std::strtoul(argv[10], nullptr, 10);
    p.chunk = (uint32_t)std::strtoul(argv[11], nullptr, 10);
    p.flags = (uint32_t)std::strtoul(argv[12], nullptr, 10);
    std::vector<double> out(n * 3u);
    uint64_t segments = 0;
    const int rc = rt1w_lab_ray_color_host(scene, &p, rays.data(), with_words ? words.data() : nullptr, out.data(), &segments);
    rt1w_scene_destroy(scene);
    if (rc < 0) { std::fprintf(stderr, "refused: %s\n", rt1w_last_error()); return 4; }
    FILE* f = std::fopen(argv[13], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < out.size() * sizeof(double); ++i) h = (h ^ ((const unsigned char*)out.data())[i]) * 0x100000001B3ull;
    std::printf("checksum %016llx\n", (unsigned long long)h);
    return 0;
}
