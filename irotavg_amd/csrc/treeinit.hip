// treeinit.hip -- the order-free spanning-tree initialiser on the device (irotavg_init_tree, irotavg_init_tree_dev;
// docs/init_tree.md): the minimum spanning tree under the keys (rank[k], k) by Boruvka rounds, rotations carried as labels
// of a union-find and composed by pointer jumping. Every step of a kernel is a function of treeinit.hpp. On one stream:
//   k_tree_init    comp[v] = v, rel[v] = identity in both copies of the state, via[v] = -1;
//   k_tree_guard   range-checks both ends of every edge (a bad id stores 1 into the error word, as k_cyc_emit does; every
//                  later kernel returns at once when it is set, so nothing is indexed with a bad id);
//   per round      best = all ones (a fill);
//     k_tree_offer   one thread per edge, contiguous chunks per workgroup: an edge between two components offers its key to
//                    both representatives by a 64-bit atomicMin, after a plain read that skips an offer that cannot win
//                    and after the lanes that share the first active lane's destination have been reduced in the wave;
//     k_tree_hook    one thread per view: a representative with an offer hooks (tree_hook). It reads copy 0 and writes
//                    copy 1; both copies are equal when it starts, so only the hooking rows are written;
//     k_tree_jump    x tree_jump_passes(components): pass j reads copy (j + 1) & 1 and writes copy j & 1; it returns at
//                    once when pass j - 1 moved no pointer. The last pass that runs moves nothing, so both copies are
//                    equal again. No host decision between the passes;
//     one read-back  error word, hooks so far, rank sums, the passes' "moved" words;
//   k_tree_finish  Q[v] = rel[v] (x) rel[0]^-1 (x) Q[0] for v >= f, in_tree[via[v]] = 1 -- launched only on success.
// The only atomics are integer minima, maxima and sums: no result depends on an order. No flag between workgroups, no
// cooperative launch, no wait; the round loop and the pass loop are bounded by 32. Memory: 88 bytes per view, nothing per
// edge.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "graph.hpp"
#include "kernels.hpp"   // tile_range
#include "winbatch.hpp"  // rows16
#include "treeinit.hpp"

namespace irh {
namespace {

constexpr int kT = 256;
constexpr int kTreeMaxGrid = 2048;  // a multiple of 8: tile_range deals adjacent chunks to the workgroups of one XCD
// the words of `head`: error, hooks so far, tree edges with rank > 0, largest rank, then per round the passes' moved words
constexpr int kErr = 0, kHooks = 1, kRankPos = 2, kRankMax = 3, kMoved = 4, kMovedPerRound = TREE_MAX_JUMPS;
constexpr int kHeadWords = kMoved + TREE_MAX_ROUNDS * kMovedPerRound;
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "best holds the 64-bit keys");
static_assert(kHeadWords * sizeof(u64) <= PinPool::kBytes, "the read-back fits one pinned block");

inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

struct TreeStridedLoad {  // QQ_k of the caller's strided matrix
    const double *qq;
    long long rs, cs;
    __host__ __device__ TreeQ operator()(uint32_t k) const {
        const double *r = qq + (long long)k * rs;
        return TreeQ{r[0], r[cs], r[2 * cs], r[3 * cs]};
    }
};

__global__ __launch_bounds__(kT) void k_tree_init(long long n, int32_t *__restrict__ comp0, int32_t *__restrict__ comp1,
                                                  TreeQ *__restrict__ rel0, TreeQ *__restrict__ rel1, int32_t *__restrict__ via) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n) return;
    comp0[v] = comp1[v] = (int32_t)v;
    rel0[v] = rel1[v] = tree_identity();
    via[v] = -1;
}

__global__ __launch_bounds__(kT) void k_tree_guard(long long m, long long n_total, const int2 *__restrict__ I, u64 *__restrict__ head) {
    const long long k = (long long)blockIdx.x * kT + threadIdx.x;
    if (k >= m) return;
    const int2 e = I[k];
    if (!tree_id_ok(e.x, n_total) || !tree_id_ok(e.y, n_total)) head[kErr] = 1;
}

// One offer of the wave: the lanes whose destination is that of the first active lane are reduced to one minimum, which
// that lane offers; every other active lane offers its own. All lanes of the wave come here together.
__device__ __forceinline__ void tree_wave_offer(u64 *__restrict__ best, bool active, int32_t dest, u64 key) {
    const u64 mask = __ballot(active);
    if (mask == 0) return;  // (wave-uniform)
    const int leader = __ffsll((long long)mask) - 1;
    const int32_t ld = __shfl(dest, leader);
    const bool same = active && dest == ld;
    u64 mn = same ? key : TREE_KEY_NONE;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, (u64)__shfl_xor(mn, o));
    const bool lead = (int)(threadIdx.x & 63) == leader;
    if (lead) key = mn;
    if (active && (lead || !same) && key < __atomic_load_n(&best[dest], __ATOMIC_RELAXED)) atomicMin(&best[dest], key);
}

__global__ __launch_bounds__(kT) void k_tree_offer(int m, const int2 *__restrict__ I, const int32_t *__restrict__ rank,
                                                   const int32_t *__restrict__ comp, u64 *__restrict__ best,
                                                   const u64 *__restrict__ head) {
    if (head[kErr] != 0) return;  // (uniform: a bad id; nothing is indexed with it)
    int e0, e1;
    tile_range(m, e0, e1);
    for (long long base = e0; base < e1; base += kT) {  // (the same trip count in every lane)
        const long long k = base + threadIdx.x;
        int32_t ca = 0, cb = 0;
        bool active = false;
        u64 key = TREE_KEY_NONE;
        if (k < e1) {
            const int2 e = I[k];
            const int32_t r = rank ? rank[k] : 0;
            active = tree_offer_ends(e.x, e.y, r, comp, ca, cb);
            key = tree_key(r, (uint32_t)k);
        }
        tree_wave_offer(best, active, ca, key);
        tree_wave_offer(best, active, cb, key);
    }
}

__global__ __launch_bounds__(kT) void k_tree_hook(long long n, const int32_t *__restrict__ comp0, const TreeQ *__restrict__ rel0,
                                                  const u64 *__restrict__ best, const int32_t *__restrict__ I, TreeStridedLoad load,
                                                  int32_t *__restrict__ comp1, TreeQ *__restrict__ rel1, int32_t *__restrict__ via,
                                                  u64 *__restrict__ head) {
    if (head[kErr] != 0) return;
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    TreeHook h;
    h.rank = 0;
    const bool hooked = v < n && tree_hook((int32_t)v, comp0, rel0, reinterpret_cast<const uint64_t *>(best), I, load, h);
    if (hooked) {
        comp1[v] = h.parent;
        rel1[v] = h.label;
        via[v] = (int32_t)h.edge;
    }
    // the sums of the wave, one atomic each from its first lane
    const bool pos = hooked && h.rank > 0;
    const u64 hooks = __popcll(__ballot(hooked)), npos = __popcll(__ballot(pos));
    int rmax = pos ? h.rank : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmax = max(rmax, __shfl_xor(rmax, o));
    if ((threadIdx.x & 63) == 0 && hooks != 0) {
        atomicAdd(&head[kHooks], hooks);
        if (npos != 0) {
            atomicAdd(&head[kRankPos], npos);
            atomicMax(&head[kRankMax], (u64)rmax);
        }
    }
}

// moved_prev: the word of the pass before (nullptr: the first pass of a round, which always runs)
__global__ __launch_bounds__(kT) void k_tree_jump(long long n, const int32_t *__restrict__ comp_src, const TreeQ *__restrict__ rel_src,
                                                  int32_t *__restrict__ comp_dst, TreeQ *__restrict__ rel_dst,
                                                  const u64 *__restrict__ head, const u64 *__restrict__ moved_prev,
                                                  u64 *__restrict__ moved) {
    if (head[kErr] != 0 || (moved_prev && *moved_prev == 0)) return;  // (uniform)
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n) return;
    int32_t c;
    TreeQ r;
    if (tree_jump((int32_t)v, comp_src, rel_src, c, r)) *moved = 1;  // (every writer stores the same value)
    comp_dst[v] = c;
    rel_dst[v] = r;
}

__global__ __launch_bounds__(kT) void k_tree_finish(long long n, int f, const int32_t *__restrict__ comp, const TreeQ *__restrict__ rel,
                                                    const int32_t *__restrict__ via, double *__restrict__ Q, long long rs, long long cs,
                                                    bool aos, int32_t *__restrict__ in_tree) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n) return;
    if (in_tree && via[v] >= 0) in_tree[via[v]] = 1;
    if (v < f) return;  // rows below f are never written
    const TreeQ q0{Q[0], Q[cs], Q[2 * cs], Q[3 * cs]};
    const TreeQ t = tree_row(rel[v], tree_base(comp[0] == 0, rel[0], q0));
    if (aos) {
        double2 *row = reinterpret_cast<double2 *>(Q) + 2 * v;
        row[0] = make_double2(t.x, t.y);
        row[1] = make_double2(t.z, t.w);
    } else {
        double *row = Q + v * rs;
        row[0] = t.x;
        row[cs] = t.y;
        row[2 * cs] = t.z;
        row[3 * cs] = t.w;
    }
}

thread_local long long t_launches = 0, t_jumps = 0;

}  // namespace

void init_tree_counters(int64_t out[2]) {
    out[0] = t_launches;
    out[1] = t_jumps;
}

int init_tree_dev(int64_t m, int64_t n_total, int f, const TreeArrays &A, int64_t *info, hipStream_t stream) {
    const long long n = n_total;
    long long nwg = std::max<long long>(1, (m + kT - 1) / kT);
    if (nwg > 8) nwg = std::min<long long>(kTreeMaxGrid, (nwg + 7) / 8 * 8);
    // every temporary first (the pool): nothing after the first launch can fail for want of memory
    DevBuf<int32_t> comp[2], via;
    DevBuf<TreeQ> rel[2];
    DevBuf<u64> best, head;
    for (int c = 0; c < 2; c++) {
        comp[c].alloc((size_t)n);
        rel[c].alloc((size_t)n);
    }
    via.alloc((size_t)n);
    best.alloc((size_t)n);
    head.alloc(kHeadWords);
    u64 *h = reinterpret_cast<u64 *>(PinPool::get().take());  // pinned read-back block
    struct PinGuard {
        void *p;
        ~PinGuard() { PinPool::get().give(p); }
    } pin_guard{h};
    const int2 *I2 = reinterpret_cast<const int2 *>(A.I);
    const TreeStridedLoad load{A.QQ, A.qq_rs, A.qq_cs};
    long long launches = 0, jumps_max = 0;
    t_launches = t_jumps = 0;

    IRH_CHECK(hipMemsetAsync(head.p, 0, kHeadWords * sizeof(u64), stream));
    hipLaunchKernelGGL(k_tree_init, dim3(grid_of(n)), dim3(kT), 0, stream, n, comp[0].p, comp[1].p, rel[0].p, rel[1].p, via.p);
    IRH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tree_guard, dim3(grid_of(m)), dim3(kT), 0, stream, (long long)m, n, I2, head.p);
    IRH_CHECK(hipGetLastError());
    launches += 2;

    long long comps = n, rounds = 0, hooks_before = 0;
    for (int round = 0;; round++) {
        if (round >= TREE_MAX_ROUNDS) return IROTAVG_ERR_SOLVER;  // (components at least halve: does not occur)
        const bool work = comps > 1;
        const int passes = tree_jump_passes(comps);
        u64 *moved = head.p + kMoved + round * kMovedPerRound;
        if (work) {
            IRH_CHECK(hipMemsetAsync(best.p, 0xff, (size_t)n * sizeof(u64), stream));
            hipLaunchKernelGGL(k_tree_offer, dim3((unsigned)nwg), dim3(kT), 0, stream, (int)m, I2, A.rank, comp[0].p, best.p, head.p);
            IRH_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_tree_hook, dim3(grid_of(n)), dim3(kT), 0, stream, n, comp[0].p, rel[0].p, best.p, A.I, load, comp[1].p,
                               rel[1].p, via.p, head.p);
            IRH_CHECK(hipGetLastError());
            for (int j = 0; j < passes; j++) {
                const int src = (j + 1) & 1, dst = j & 1;
                hipLaunchKernelGGL(k_tree_jump, dim3(grid_of(n)), dim3(kT), 0, stream, n, comp[src].p, rel[src].p, comp[dst].p, rel[dst].p,
                                   head.p, j ? moved + j - 1 : nullptr, moved + j);
                IRH_CHECK(hipGetLastError());
            }
            launches += 3 + passes;
        }
        // the one read-back of the round (a graph of one view: of the guard)
        IRH_CHECK(hipMemcpyAsync(h, head.p, kHeadWords * sizeof(u64), hipMemcpyDeviceToHost, stream));
        IRH_CHECK(hipStreamSynchronize(stream));
        if (h[kErr] != 0) return IROTAVG_ERR_BAD_ARG;
        if (!work) break;
        const u64 *mv = h + kMoved + round * kMovedPerRound;
        if (mv[passes - 1] != 0) return IROTAVG_ERR_SOLVER;  // (the bound of tree_jump_passes: does not occur)
        long long moving = 0;
        while (moving < passes && mv[moving] != 0) moving++;
        jumps_max = std::max(jumps_max, moving);
        const long long hooks = (long long)h[kHooks] - hooks_before;
        hooks_before = (long long)h[kHooks];
        if (hooks <= 0) break;  // no edge leaves any component: the forest is complete
        comps -= hooks;
        rounds++;
        if (comps <= 1) break;
    }
    t_launches = launches;
    t_jumps = jumps_max;
    const int64_t out[4] = {rounds, comps, (int64_t)h[kRankPos], (int64_t)h[kRankMax]};
    if (comps != 1) {
        if (info) std::copy(out, out + 4, info);  // the diagnosis
        return IROTAVG_ERR_NOT_SPANNING;
    }
    if (A.in_tree) IRH_CHECK(hipMemsetAsync(A.in_tree, 0, (size_t)m * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_tree_finish, dim3(grid_of(n)), dim3(kT), 0, stream, n, f, comp[0].p, rel[0].p, via.p, A.Q, A.q_rs, A.q_cs,
                       rows16(reinterpret_cast<uintptr_t>(A.Q), A.q_rs, A.q_cs), A.in_tree);
    IRH_CHECK(hipGetLastError());
    IRH_CHECK(hipStreamSynchronize(stream));  // (the temporaries go back to the pool idle)
    t_launches = launches + 2;
    if (info) std::copy(out, out + 4, info);
    return IROTAVG_OK;
}

int init_tree_host(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq, const int32_t *rank, double *Q,
                   int64_t ldq, int32_t *in_tree, int64_t *info) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m, un = (size_t)n_total;
    DevBuf<int32_t> dI, drank, dtree;
    DevBuf<double> dqq, dQ;
    dI.alloc(2 * um);
    dqq.alloc(4 * um);  // four planes of m
    dQ.alloc(4 * un);   // four planes of n_total; row 0 alone goes up, the rows from f on come back
    if (rank) drank.alloc(um);
    if (in_tree) dtree.alloc(um);
    IRH_CHECK(hipMemcpyAsync(dI.p, I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (rank) IRH_CHECK(hipMemcpyAsync(drank.p, rank, um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    for (int c = 0; c < 4; c++) {
        IRH_CHECK(hipMemcpyAsync(dqq.p + c * um, QQ + c * ldqq, um * sizeof(double), hipMemcpyHostToDevice, s));
        IRH_CHECK(hipMemcpyAsync(dQ.p + c * un, Q + c * ldq, sizeof(double), hipMemcpyHostToDevice, s));
    }
    const TreeArrays D{dI.p, dqq.p, 1, (long long)m, rank ? drank.p : nullptr, dQ.p, 1, (long long)n_total, in_tree ? dtree.p : nullptr};
    int64_t inf[4] = {0, 0, 0, 0};
    const int rc = init_tree_dev(m, n_total, f, D, inf, s);
    if (rc == IROTAVG_OK) {
        if ((size_t)f < un)
            for (int c = 0; c < 4; c++)
                IRH_CHECK(hipMemcpyAsync(Q + c * ldq + f, dQ.p + c * un + f, (un - (size_t)f) * sizeof(double), hipMemcpyDeviceToHost, s));
        if (in_tree) IRH_CHECK(hipMemcpyAsync(in_tree, dtree.p, um * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        IRH_CHECK(hipStreamSynchronize(s));
    }
    if (info && (rc == IROTAVG_OK || rc == IROTAVG_ERR_NOT_SPANNING)) std::copy(inf, inf + 4, info);
    return rc;
}

}  // namespace irh
