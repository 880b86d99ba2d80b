// components.hip -- connected components of the usable edges on the device, and the selected component as a compact,
// relabelled problem (irotavg_components, irotavg_components_dev; docs/components.md). Every piece of index math is a
// function of components.hpp. On one stream, eight launches whatever the graph:
//   a fill             the eight words of `head` = 0;
//   k_comp_guard       range-checks both ends of every edge (a bad id stores 1 into the error word; every later kernel
//                      returns at once when it is set, so nothing is indexed with a bad id); parent[v] = v, size[v] = 0;
//   k_comp_link        ONE launch over the edges: a lock-free union-find. A usable edge finds both roots with path halving
//                      and links the larger root under the smaller by a compare-and-swap on the larger root's own word; a
//                      failed swap goes on from the value it returned. The lanes of a wave that found the first active
//                      lane's pair of roots leave the link to that lane;
//   k_comp_flatten     lab[v] = root(v), finds with path halving; size[lab[v]] += 1, the lanes of a wave that share a label
//                      counted by a ballot and added by one lane;
//   k_comp_select      over the roots: the largest key (size, COMP_ID_MAX - label) and the number of roots, reduced in the
//                      wave, one 64-bit atomicMax and one atomicAdd per wave;
//   k_comp_count       per workgroup the selected views of its chunk of views and the kept edges of its chunk of edges;
//   k_comp_put_views   every workgroup adds up the partial sums before its own, recomputes its ballots and writes label,
//                      view_map, views_out, n' and f';
//   k_comp_put_edges   the same over the edges: edge_map, edges_out, I_out (through view_map), m';
//   one copy of `head` into a pinned block and one host wait.
// The atomics are a compare-and-swap whose losers retry from what it returned, integer sums and an integer maximum: no
// result depends on an order. No flag between workgroups, no cooperative launch, no wait; every loop carries a bound.
// Memory: 16 bytes per view and 8 bytes per workgroup of the compaction, nothing per edge.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "graph.hpp"
#include "kernels.hpp"  // tile_range
#include "components.hpp"

namespace irh {
namespace {

constexpr int kT = COMP_BLOCK;
constexpr int kWaves = kT / 64;
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "head holds the 64-bit keys");
static_assert(COMP_HEAD_WORDS * sizeof(u64) <= PinPool::kBytes, "the read-back fits one pinned block");
static_assert(COMP_MAX_GRID % 8 == 0, "adjacent chunks go to one XCD");

__device__ __forceinline__ bool comp_stop(const u64 *__restrict__ head) { return (head[COMP_ERR] | head[COMP_BOUND]) != 0; }
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ u64 lanes_below() { return (1ull << lane_id()) - 1ull; }

// ---- link ---------------------------------------------------------------------------------------------------------------
// A parent word while other workgroups link and halve: relaxed loads and stores of device scope, so that a find follows
// what other XCDs have linked already and not a line of its own L2. A stale value would still be an ancestor.
__device__ __forceinline__ int32_t ld_parent(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_parent(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t link_find(int32_t *__restrict__ parent, int32_t v, long long bound, long long &steps) {
    while (steps <= bound) {
        const int32_t p = ld_parent(parent + v);
        if (p == v) break;
        const int32_t gp = ld_parent(parent + p);
        if (gp != p) st_parent(parent + v, gp);  // (v is no root and never becomes one again: no swap expects this word)
        v = gp;
        steps++;
    }
    return v;
}

__global__ __launch_bounds__(kT) void k_comp_guard(long long m, long long n, const int2 *__restrict__ I, int32_t *__restrict__ parent,
                                                   int32_t *__restrict__ size, u64 *__restrict__ head) {
    const int nb = gridDim.x, lb = comp_logical_block(blockIdx.x, nb);
    int64_t c0, c1;
    comp_chunk(m, lb, nb, c0, c1);
    bool bad = false;
    for (long long k = c0 + threadIdx.x; k < c1; k += kT) {
        const int2 e = I[k];
        bad |= !comp_id_ok(e.x, n) || !comp_id_ok(e.y, n);
    }
    if (bad) head[COMP_ERR] = 1;  // (every writer stores the same value)
    comp_chunk(n, lb, nb, c0, c1);
    for (long long v = c0 + threadIdx.x; v < c1; v += kT) {
        parent[v] = (int32_t)v;
        size[v] = 0;
    }
}

__global__ __launch_bounds__(kT) void k_comp_link(int m, long long n, const int2 *__restrict__ I, const int32_t *__restrict__ rank,
                                                  int32_t *__restrict__ parent, u64 *__restrict__ head) {
    if (comp_stop(head)) return;  // (uniform: a bad id; nothing is indexed with it)
    int e0, e1;
    tile_range(m, e0, e1);
    const long long bound = comp_step_bound(n);
    bool over = false;
    for (long long base = e0; base < e1; base += kT) {  // (the same trip count in every lane)
        const long long k = base + threadIdx.x;
        bool active = false;
        int32_t hi = 0, lo = 0;
        if (k < e1) {
            const int2 e = I[k];
            active = comp_usable(e.x, e.y, rank ? rank[k] : 0);
            hi = e.x;
            lo = e.y;
        }
        long long steps = 0;
        while (__ballot(active) != 0) {  // (wave-uniform; a lane leaves when its two ends share a root or it linked them)
            if (active) {
                hi = link_find(parent, hi, bound, steps);
                lo = link_find(parent, lo, bound, steps);
                if (hi < lo) {
                    const int32_t t = hi;
                    hi = lo;
                    lo = t;
                }
                if (steps > bound) over = true;
                if (over || hi == lo) active = false;
            }
            // the lanes that found the first active lane's pair of roots: that lane links for them. When it is done the two
            // roots share a root, and so do the ends of every edge below them.
            const u64 mask = __ballot(active);
            if (mask == 0) break;
            const int leader = __ffsll((long long)mask) - 1;
            const int32_t lhi = __shfl(hi, leader), llo = __shfl(lo, leader);
            if (active && lane_id() != leader && hi == lhi && lo == llo) active = false;
            if (active) {
                const int32_t old = atomicCAS(&parent[hi], hi, lo);  // the larger root's own word: hi -> lo < hi
                if (old == hi) active = false;
                else {  // another thread linked hi meanwhile, under old < hi: go on from there
                    hi = old;
                    steps++;
                }
            }
        }
    }
    if (over) head[COMP_BOUND] = 1;
}

// ---- flatten + count ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_comp_flatten(long long n, int32_t *__restrict__ parent, int32_t *__restrict__ lab,
                                                     int32_t *__restrict__ size, u64 *__restrict__ head) {
    if (comp_stop(head)) return;
    const int nb = gridDim.x, lb = comp_logical_block(blockIdx.x, nb);
    int64_t c0, c1;
    comp_chunk(n, lb, nb, c0, c1);
    const int64_t bound = comp_step_bound(n);
    bool over = false;
    for (long long base = c0; base < c1; base += kT) {
        const long long v = base + threadIdx.x;
        bool todo = v < c1;
        int32_t l = -1;
        if (todo) {
            int64_t steps = 0;
            l = comp_find_halving(parent, (int32_t)v, bound, steps);
            if (steps > bound) over = true, todo = false;
            else lab[v] = l;  // (a row of its own: other threads' halving stores land in parent, never here)
        }
        // one add per label of the wave: a giant component would otherwise put n_total atomics on one word
        u64 mask;
        while ((mask = __ballot(todo)) != 0) {  // (wave-uniform; every pass retires the first lane left: at most 64)
            const int leader = __ffsll((long long)mask) - 1;
            const int32_t ll = __shfl(l, leader);
            const bool same = todo && l == ll;
            const int cnt = __popcll(__ballot(same));
            if (lane_id() == leader) atomicAdd(&size[ll], cnt);
            if (same) todo = false;
        }
    }
    if (over) head[COMP_BOUND] = 1;
}

// ---- select ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_comp_select(long long n, const int32_t *__restrict__ lab, const int32_t *__restrict__ size,
                                                    u64 *__restrict__ head) {
    if (comp_stop(head)) return;
    const int nb = gridDim.x, lb = comp_logical_block(blockIdx.x, nb);
    int64_t c0, c1;
    comp_chunk(n, lb, nb, c0, c1);
    u64 best = 0;
    int roots = 0;
    for (long long v = c0 + threadIdx.x; v < c1; v += kT)
        if (lab[v] == (int32_t)v) {
            best = max(best, (u64)comp_key(size[v], (int32_t)v));
            roots++;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        best = max(best, (u64)__shfl_xor(best, o));
        roots += __shfl_xor(roots, o);
    }
    if (lane_id() == 0 && roots != 0) {
        atomicMax(&head[COMP_BEST], best);
        atomicAdd(&head[COMP_COUNT], (u64)roots);
    }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------
// The sum of a value over the workgroup (all threads get it). lds: kWaves ints, free again after the call.
__device__ __forceinline__ int block_sum(int x, int *lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += lds[w];
    __syncthreads();
    return s;
}
// part[0] + ... + part[lb - 1]: at most COMP_MAX_GRID words that every workgroup reads from L2
__device__ __forceinline__ int block_offset(const int32_t *__restrict__ part, int lb, int *lds) {
    int s = 0;
    for (int j = threadIdx.x; j < lb; j += kT) s += part[j];
    return block_sum(s, lds);
}
// The place of a flagged thread among the flagged threads of its 256-thread tile, and the tile's total. The place inside
// the wave is popc(ballot & lanes below), the four wave totals go through LDS. Consecutive tiles alternate between the two
// halves of lds (2 * kWaves ints), so one barrier per tile is enough.
__device__ __forceinline__ int tile_place(bool flag, int *lds, int tile, int &total) {
    const u64 b = __ballot(flag);
    int *w = lds + (tile & 1) * kWaves;
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) w[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < kWaves; j++) {
        const int t = w[j];
        if (j < wave) before += t;
        total += t;
    }
    return before + __popcll(b & lanes_below());
}

__device__ __forceinline__ bool edge_kept(const int2 e, const int32_t *__restrict__ rank, long long k, const int32_t *__restrict__ lab,
                                          int32_t sel) {
    return comp_usable(e.x, e.y, rank ? rank[k] : 0) && lab[e.x] == sel;
}

__global__ __launch_bounds__(kT) void k_comp_count(long long m, long long n, int which, const int2 *__restrict__ I,
                                                   const int32_t *__restrict__ rank, const int32_t *__restrict__ lab,
                                                   const u64 *__restrict__ head, int32_t *__restrict__ vpart,
                                                   int32_t *__restrict__ epart) {
    __shared__ int lds[kWaves];
    if (comp_stop(head)) return;
    const int nb = gridDim.x, lb = comp_logical_block(blockIdx.x, nb);
    const int32_t sel = comp_selected(which, head[COMP_BEST]);
    int64_t c0, c1;
    comp_chunk(n, lb, nb, c0, c1);
    int nv = 0, ne = 0;
    for (long long v = c0 + threadIdx.x; v < c1; v += kT) nv += lab[v] == sel;
    comp_chunk(m, lb, nb, c0, c1);
    for (long long k = c0 + threadIdx.x; k < c1; k += kT) ne += edge_kept(I[k], rank, k, lab, sel);
    nv = block_sum(nv, lds);
    ne = block_sum(ne, lds);
    if (threadIdx.x == 0) {
        vpart[lb] = nv;
        epart[lb] = ne;
    }
}

__global__ __launch_bounds__(kT) void k_comp_put_views(long long n, int f, int which, const int32_t *__restrict__ lab,
                                                       const int32_t *__restrict__ vpart, u64 *__restrict__ head,
                                                       int32_t *__restrict__ vmap, int32_t *__restrict__ label,
                                                       int32_t *__restrict__ view_map, int32_t *__restrict__ views_out) {
    __shared__ int lds[2 * kWaves];
    if (comp_stop(head)) return;
    const int nb = gridDim.x, lb = comp_logical_block(blockIdx.x, nb);
    const int32_t sel = comp_selected(which, head[COMP_BEST]);
    int64_t c0, c1;
    comp_chunk(n, lb, nb, c0, c1);
    int base_pos = block_offset(vpart, lb, lds);
    int tile = 0;
    for (long long base = c0; base < c1; base += kT, tile++) {  // (the same trip count in every thread: the barriers)
        const long long v = base + threadIdx.x;
        const bool in = v < c1;
        const int32_t l = in ? lab[v] : -1;
        const bool flag = in && l == sel;
        int total;
        const int pos = base_pos + tile_place(flag, lds, tile, total);
        if (in) {
            const int32_t nv = flag ? pos : -1;
            vmap[v] = nv;
            if (label) label[v] = l;
            if (view_map) view_map[v] = nv;
            if (flag && views_out) views_out[pos] = (int32_t)v;
            if (v == f - 1) head[COMP_FSEL] = (u64)(pos + (flag ? 1 : 0));  // the selected views below f
        }
        base_pos += total;
    }
    if (lb == nb - 1 && threadIdx.x == 0) head[COMP_NSEL] = (u64)base_pos;
}

__global__ __launch_bounds__(kT) void k_comp_put_edges(long long m, int which, const int2 *__restrict__ I, const int32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ lab, const int32_t *__restrict__ vmap,
                                                       const int32_t *__restrict__ epart, u64 *__restrict__ head,
                                                       int32_t *__restrict__ edge_map, int32_t *__restrict__ edges_out,
                                                       int2 *__restrict__ I_out) {
    __shared__ int lds[2 * kWaves];
    if (comp_stop(head)) return;
    const int nb = gridDim.x, lb = comp_logical_block(blockIdx.x, nb);
    const int32_t sel = comp_selected(which, head[COMP_BEST]);
    int64_t c0, c1;
    comp_chunk(m, lb, nb, c0, c1);
    int base_pos = block_offset(epart, lb, lds);
    int tile = 0;
    for (long long base = c0; base < c1; base += kT, tile++) {
        const long long k = base + threadIdx.x;
        const bool in = k < c1;
        int2 e = make_int2(0, 0);
        if (in) e = I[k];
        const bool flag = in && edge_kept(e, rank, k, lab, sel);
        int total;
        const int pos = base_pos + tile_place(flag, lds, tile, total);
        if (in && edge_map) edge_map[k] = flag ? pos : -1;
        if (flag) {
            if (edges_out) edges_out[pos] = (int32_t)k;
            if (I_out) I_out[pos] = make_int2(vmap[e.x], vmap[e.y]);  // both ends carry the selected label
        }
        base_pos += total;
    }
    if (lb == nb - 1 && threadIdx.x == 0) head[COMP_MSEL] = (u64)base_pos;
}

}  // namespace

int components_dev(int64_t m, int64_t n_total, int f, int which, const CompArrays &A, int64_t *info, hipStream_t stream) {
    const long long n = n_total;
    const unsigned g_edges = comp_grid(m), g_views = comp_grid(n), g_both = comp_grid(std::max<int64_t>(m, n));
    // every temporary first (the pool): nothing after the first launch can fail for want of memory
    DevBuf<int32_t> parent, size, lab, vmap, vpart, epart;
    DevBuf<u64> head;
    parent.alloc((size_t)n);
    size.alloc((size_t)n);
    lab.alloc((size_t)n);
    vmap.alloc((size_t)n);
    vpart.alloc(g_both);
    epart.alloc(g_both);
    head.alloc(COMP_HEAD_WORDS);
    u64 *h = reinterpret_cast<u64 *>(PinPool::get().take());  // pinned read-back block
    struct PinGuard {
        void *p;
        ~PinGuard() { PinPool::get().give(p); }
    } pin_guard{h};
    const int2 *I2 = reinterpret_cast<const int2 *>(A.I);

    IRH_CHECK(hipMemsetAsync(head.p, 0, COMP_HEAD_WORDS * sizeof(u64), stream));
    hipLaunchKernelGGL(k_comp_guard, dim3(g_both), dim3(kT), 0, stream, (long long)m, n, I2, parent.p, size.p, head.p);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_comp_link, dim3(g_edges), dim3(kT), 0, stream, (int)m, n, I2, A.rank, parent.p, head.p);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_comp_flatten, dim3(g_views), dim3(kT), 0, stream, n, parent.p, lab.p, size.p, head.p);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_comp_select, dim3(g_views), dim3(kT), 0, stream, n, lab.p, size.p, head.p);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_comp_count, dim3(g_both), dim3(kT), 0, stream, (long long)m, n, which, I2, A.rank, lab.p, head.p, vpart.p, epart.p);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_comp_put_views, dim3(g_both), dim3(kT), 0, stream, n, f, which, lab.p, vpart.p, head.p, vmap.p, A.label, A.view_map,
                       A.views_out);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_comp_put_edges, dim3(g_both), dim3(kT), 0, stream, (long long)m, which, I2, A.rank, lab.p, vmap.p, epart.p, head.p,
                       A.edge_map, A.edges_out, reinterpret_cast<int2 *>(A.I_out));
    IRH_CHECK(hipGetLastError());
    IRH_CHECK(hipMemcpyAsync(h, head.p, COMP_HEAD_WORDS * sizeof(u64), hipMemcpyDeviceToHost, stream));
    IRH_CHECK(hipStreamSynchronize(stream));  // the one host wait (the temporaries go back to the pool idle)
    if (h[COMP_ERR] != 0) return IROTAVG_ERR_BAD_ARG;
    if (h[COMP_BOUND] != 0) return IROTAVG_ERR_SOLVER;  // (every step goes to a smaller id: does not occur)
    if (info) {
        info[0] = (int64_t)h[COMP_COUNT];
        info[1] = (int64_t)h[COMP_NSEL];
        info[2] = (int64_t)h[COMP_MSEL];
        info[3] = (int64_t)h[COMP_FSEL];
        info[4] = comp_selected(which, h[COMP_BEST]);
        info[5] = comp_key_size(h[COMP_BEST]);
    }
    return IROTAVG_OK;
}

int components_host(int64_t m, int64_t n_total, int f, int which, const CompArrays &A, int64_t *info) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m, un = (size_t)n_total;
    DevBuf<int32_t> dI, drank, dlabel, dvmap, demap, dviews, dedges, dIout;
    dI.alloc(2 * um);
    if (A.rank) drank.alloc(um);
    if (A.label) dlabel.alloc(un);
    if (A.view_map) dvmap.alloc(un);
    if (A.edge_map) demap.alloc(um);
    if (A.views_out) dviews.alloc(un);
    if (A.edges_out) dedges.alloc(um);
    if (A.I_out) dIout.alloc(2 * um);
    IRH_CHECK(hipMemcpyAsync(dI.p, A.I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (A.rank) IRH_CHECK(hipMemcpyAsync(drank.p, A.rank, um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const CompArrays D{dI.p,
                       A.rank ? drank.p : nullptr,
                       A.label ? dlabel.p : nullptr,
                       A.view_map ? dvmap.p : nullptr,
                       A.edge_map ? demap.p : nullptr,
                       A.views_out ? dviews.p : nullptr,
                       A.edges_out ? dedges.p : nullptr,
                       A.I_out ? dIout.p : nullptr};
    int64_t inf[6] = {0, 0, 0, 0, 0, 0};
    const int rc = components_dev(m, n_total, f, which, D, inf, s);
    if (rc != IROTAVG_OK) return rc;
    // the entries past n' / m' were never written on the device and are not copied: the caller's stay as they were
    const size_t n1 = (size_t)inf[1], m1 = (size_t)inf[2];
    const struct {
        int32_t *dst;
        const int32_t *src;
        size_t count;
    } back[6] = {{A.label, dlabel.p, un}, {A.view_map, dvmap.p, un}, {A.edge_map, demap.p, um},
                 {A.views_out, dviews.p, n1}, {A.edges_out, dedges.p, m1}, {A.I_out, dIout.p, 2 * m1}};
    for (const auto &b : back)
        if (b.dst && b.count) IRH_CHECK(hipMemcpyAsync(b.dst, b.src, b.count * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    if (info) std::copy(inf, inf + 6, info);
    return IROTAVG_OK;
}

}  // namespace irh
