/* rt_box_free.h -- what the generator (jit.cpp) decides for the box-free sweep of a scene-specialised unit (rt_core.h: rt_sweep_free),
 * as pure host functions over the flat node array: which box a hit is verified against in every ray space (Topo::vbox), whether the
 * boxes are nested bit for bit (the verification's premise), and the members both end up as.  Host only: not one of the headers the
 * generated units include. */
#ifndef RT1W_BOX_FREE_H
#define RT1W_BOX_FREE_H

#include <string>
#include <vector>

#include "rt_flat.h"

#define RT_VBOX_SPACES 4u         /* world + below each of at most three Translate / RotateY (the flattener's depth) */
#define RT_BOX_FREE_MAX_NODES 64u /* a box-free sweep is linear in leaves: larger topologies keep their boxes (profiles/box_free_bench.json) */

namespace rt1w {

/* BVH nodes above I in I's ray space, nearest first (the way jit_slab_reuse goes up): FlipFace leaves the ray alone, a Translate,
 * RotateY or ConstantMedium ends the space.  `*wrapper`: the node that ended it, or RT_NONE at the root. */
inline std::vector<uint32_t> box_free_boxes_above(const RtNode* N, uint32_t root, uint32_t I, uint32_t* wrapper) {
    std::vector<uint32_t> out;
    *wrapper = RT_NONE;
    for (uint32_t J = I; J-- > root;) {
        if (N[J].skip <= I) continue; /* not above I */
        const uint32_t kj = N[J].kind & RT_KIND_MASK;
        if (kj == RT_FLIP) continue;
        if (kj > RT_BVH1) { *wrapper = J; break; }
        out.push_back(J);
    }
    return out;
}

/* Topo::vbox[I][s] for a leaf I: in ray space s of its wrapper chain (0 the world, then below each Translate / RotateY, outermost
 * first) the innermost BVH node above the leaf, or above the wrapper that leads to it; RT_NONE where that space has no box, in
 * spaces the leaf is not in, and in the rows of every other node.  false: a chain deeper than the table. */
inline bool box_free_vbox_row(const RtNode* N, uint32_t n, uint32_t root, uint32_t I, uint32_t row[RT_VBOX_SPACES]) {
    for (uint32_t s = 0; s < RT_VBOX_SPACES; ++s) row[s] = RT_NONE;
    const uint32_t k = N[I].kind & RT_KIND_MASK;
    if (I < root || I >= n || k < RT_SPHERE || k > RT_YZ) return true;
    std::vector<uint32_t> inner_first; /* the box of each space, from the leaf's own space outwards */
    for (uint32_t at = I;;) {
        uint32_t w = RT_NONE;
        const std::vector<uint32_t> up = box_free_boxes_above(N, root, at, &w);
        inner_first.push_back(up.empty() ? RT_NONE : up[0]);
        if (w == RT_NONE) break;
        if ((N[w].kind & RT_KIND_MASK) == RT_MEDIUM) return false; /* a boundary's leaf: not a unit this is for */
        at = w;
    }
    if (inner_first.size() > RT_VBOX_SPACES) return false;
    for (size_t s = 0; s < inner_first.size(); ++s) row[s] = inner_first[inner_first.size() - 1u - s];
    return true;
}

/* Is every BVH node's box inside the box of the nearest BVH node above it in its ray space, bound by bound, as doubles?  (A tree
 * built by surrounding_box is: fmin / fmax return one of their operands.)  A NaN bound compares false and refuses. */
inline bool box_free_boxes_nested(const RtNode* N, uint32_t n, uint32_t root) {
    for (uint32_t I = root; I < n; ++I) {
        if ((N[I].kind & RT_KIND_MASK) > RT_BVH1) continue;
        for (uint32_t k = 0; k < 3u; ++k)
            if (!(N[I].d[k] <= N[I].d[k + 3u])) return false;
        uint32_t w;
        const std::vector<uint32_t> up = box_free_boxes_above(N, root, I, &w);
        if (up.empty()) continue;
        const RtNode& P = N[up[0]];
        for (uint32_t k = 0; k < 3u; ++k)
            if (!(P.d[k] <= N[I].d[k]) || !(P.d[k + 3u] >= N[I].d[k + 3u])) return false;
    }
    return true;
}

/* the unit sweeps without box tests iff: no medium, a rect in the topology (the units of the shared divisors), at most
 * RT_BOX_FREE_MAX_NODES nodes, every chain within the table, and nested boxes */
inline bool box_free_eligible(const RtNode* N, uint32_t n, uint32_t root) {
    if (n > RT_BOX_FREE_MAX_NODES) return false;
    bool rect = false;
    for (uint32_t I = root; I < n; ++I) {
        const uint32_t k = N[I].kind & RT_KIND_MASK;
        if (k == RT_MEDIUM) return false;
        rect |= k >= RT_XY && k <= RT_YZ;
        uint32_t row[RT_VBOX_SPACES];
        if (!box_free_vbox_row(N, n, root, I, row)) return false;
    }
    return rect && box_free_boxes_nested(N, n, root);
}

/* the two members as the generated unit declares them: node indices and one flag, never a coordinate */
inline std::string box_free_members(const RtNode* N, uint32_t n, uint32_t root) {
    const bool on = box_free_eligible(N, n, root);
    std::string src = "    static constexpr uint32_t vbox[" + std::to_string(n) + "][" + std::to_string(RT_VBOX_SPACES) + "] = {";
    for (uint32_t I = 0; I < n; ++I) {
        uint32_t row[RT_VBOX_SPACES];
        if (!on || !box_free_vbox_row(N, n, root, I, row))
            for (uint32_t s = 0; s < RT_VBOX_SPACES; ++s) row[s] = RT_NONE;
        src += I ? ", {" : "{";
        for (uint32_t s = 0; s < RT_VBOX_SPACES; ++s) src += (s ? ", " : "") + std::to_string(row[s]) + "u";
        src += "}";
    }
    src += "};\n";
    src += std::string("    static constexpr bool box_free = ") + (on ? "true" : "false") + ";\n";
    return src;
}

} // namespace rt1w

#endif
