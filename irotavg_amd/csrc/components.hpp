// components.hpp -- connected components on device arrays (irotavg_components, irotavg_components_dev; docs/components.md):
// which edge is usable, the selection key, how the kernels deal their chunks, the bound on the steps of a find, the find of
// the flatten kernel, and the words of the read-back. Plain C++ with no HIP type in it, as treeinit.hpp and sweep.hpp. The
// kernels of components.hip take every piece from here, so there is one copy of each.
//
// Definition: an edge k = (a, b) is usable when rank is NULL or rank[k] >= 0, and a != b. label[v] is the least view id of
// the component of v under the usable edges. The selected component is that of view 0 (which = 0) or the one with the most
// views, ties to the smaller label (which = 1). Selected views and kept edges are renumbered in ascending order of their
// old ids.
//
// State per view: parent[v], a pointer to a view of the same component with a smaller id, or v itself (a root). Roots are
// only ever linked under smaller ids, so there are no cycles and the last root of a component is its least id.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IRH_COMP_HD __host__ __device__ __forceinline__
#else
#define IRH_COMP_HD inline
#endif

namespace irh {

constexpr int COMP_BLOCK = 256;      // threads of a workgroup: four waves
constexpr int COMP_MAX_GRID = 2048;  // a multiple of 8: adjacent chunks go to the workgroups of one XCD (tile_range)
constexpr int32_t COMP_ID_MAX = 0x7fffffff;
// the words of the read-back (uint64 each)
enum {
    COMP_ERR = 0,    // 1: an id outside [0, n_total)
    COMP_BOUND = 1,  // 1: a find or a link passed comp_step_bound
    COMP_COUNT = 2,  // components
    COMP_BEST = 3,   // the largest key (size, COMP_ID_MAX - label) over the roots
    COMP_NSEL = 4,   // n'
    COMP_MSEL = 5,   // m'
    COMP_FSEL = 6,   // f'
    COMP_HEAD_WORDS = 8
};

IRH_COMP_HD bool comp_id_ok(int32_t v, int64_t n_total) { return v >= 0 && (int64_t)v < n_total; }
// rank < 0: never used; self loops: never used
IRH_COMP_HD bool comp_usable(int32_t a, int32_t b, int32_t rank) { return rank >= 0 && a != b; }

// The selection key of a root: the larger size wins, then the smaller label. A total order: no two roots share a label.
IRH_COMP_HD uint64_t comp_key(int32_t size, int32_t label) {
    return ((uint64_t)(uint32_t)size << 32) | (uint32_t)(COMP_ID_MAX - label);
}
IRH_COMP_HD int32_t comp_key_size(uint64_t key) { return (int32_t)(key >> 32); }
IRH_COMP_HD int32_t comp_key_label(uint64_t key) { return COMP_ID_MAX - (int32_t)(uint32_t)key; }
// view 0 is the least id of its own component, so the anchor's label is 0
IRH_COMP_HD int32_t comp_selected(int which, uint64_t best) { return which ? comp_key_label(best) : 0; }

// The workgroups of a launch over `items`: one per 256 items, a multiple of 8 above 8, at most COMP_MAX_GRID.
inline unsigned comp_grid(int64_t items) {
    int64_t g = (items + COMP_BLOCK - 1) / COMP_BLOCK;
    if (g < 1) g = 1;
    if (g > 8) g = (g + 7) / 8 * 8;
    return (unsigned)(g < COMP_MAX_GRID ? g : COMP_MAX_GRID);
}
// The place of workgroup b of nb in the order of the chunks: the workgroups b, b + 8, b + 16, ... run on one XCD and take
// adjacent chunks (the order of tile_range, kernels.hpp). The compaction indexes its partial sums with this number.
IRH_COMP_HD int comp_logical_block(int b, int nb) { return (nb & 7) == 0 ? (b & 7) * (nb >> 3) + (b >> 3) : b; }
// The chunk [c0, c1) of `items` that logical block lb of nb takes: contiguous, ascending with lb, covering [0, items) once.
IRH_COMP_HD void comp_chunk(int64_t items, int lb, int nb, int64_t &c0, int64_t &c1) {
    c0 = items * lb / nb;
    c1 = items * (lb + 1) / nb;
}

// Every step of a find moves to a smaller id and so does every retried link: an edge is done after at most 2 n_total of
// them. Passing the bound is a status (IROTAVG_ERR_SOLVER), not a longer loop.
IRH_COMP_HD int64_t comp_step_bound(int64_t n_total) { return 2 * n_total + 2; }

// The root of v with path halving, for a launch in which nothing links any more (flatten): plain loads and stores. Other
// threads halve the same paths meanwhile; a parent word only ever holds an ancestor, so a store that lands late is still
// correct. `steps` counts; the caller compares it with the bound.
IRH_COMP_HD int32_t comp_find_halving(int32_t *parent, int32_t v, int64_t bound, int64_t &steps) {
    while (steps <= bound) {
        const int32_t p = parent[v];
        if (p == v) break;
        const int32_t gp = parent[p];
        if (gp != p) parent[v] = gp;
        v = gp;
        steps++;
    }
    return v;
}

}  // namespace irh
