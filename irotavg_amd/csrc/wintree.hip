// wintree.hip -- the rank-aware tree initialisation for many window-size problems on the caller's packed device arrays,
// one workgroup per problem, ONE launch (irotavg_window_init_tree_batch_dev; docs/window_init_tree_batch.md). The
// definition is irotavg_init_tree's on the contracted graph -- the fixed views of a problem are one root --; the route is
// not irotavg_init_tree_dev's: a problem has at most 65 nodes and 640 edges, so the Boruvka rounds, the hooks and the
// pointer jumping run in LDS inside the launch, with no global temporary, no launch per step and no read-back per round.
//
// The body of k_window_tree, in order:
//   1. guard      every endpoint against [0, nv), a workgroup-wide OR before anything is indexed with one
//   2. stage      thread t keeps the nodes and the key of edges t, t + 256, t + 512 in registers (12 bytes of traffic per
//                 edge: the ids and the rank); the ends of every edge as one word of LDS; comp = self, rel = identity
//   3. rounds     at most wt_rounds(nu) of them, each: clear the best keys | offer: a 64-bit LDS atomicMin of the key to
//                 the representatives of both ends | hook: node v's thread forms its label from ONE row of QQ and, where
//                 the edge enters a fixed view, ONE row of Q, both straight from the caller's arrays | wt_passes(nu, round)
//                 passes of pointer jumping. Every step reads one copy of (comp, rel) and writes the other; one barrier
//                 per step. A round without a hook ends the rounds
//   4. spanning   a node outside the root's component: IROTAVG_ERR_NOT_SPANNING and the count
//   5. stores     the free rows (the labels themselves), in_tree, then the record, its sequence number last at system scope
// Every loop is a `for` with a bound derived from the limits (wintree.hpp): a defect ends as a wrong number or a status.
// The 64-bit minima are the only contended operations, and a minimum does not depend on the order of its operands; a
// label is the product of the same operands in the same association whatever the launch geometry: a problem gives the
// same bytes alone, first or last in a batch, and in every call. A problem that fails stores nothing but its record.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batchdev.hpp"  // the host's side of the call: block, sequence number, lock, wait
#include "graph.hpp"
#include "winbatch.hpp"  // WinDesc, the plan of a batch, rows16
#include "winio.hpp"     // ld_row / st_row
#include "wintree.hpp"   // nodes, ends, wt_hook, wt_jump, rounds and passes, the LDS layout, WinTreeResult

namespace irh {
namespace {

constexpr int WT_THREADS = 256;
constexpr int WT_EDGES = (WIN_MAX_NE + WT_THREADS - 1) / WT_THREADS;  // edges of one thread
static_assert(WT_MAX_NODES <= 2 * 64, "the final counts: lane l of the first wave takes nodes l and l + 64");
static_assert(sizeof(TreeQ) == 32 && sizeof(unsigned long long) == sizeof(uint64_t), "the layout of wintree_lds");

#pragma clang fp contract(off)  // as tree_qmul carries it in its own body

struct WinTreeUser {  // the caller's packed arrays of a batch (kernel argument)
    const int2 *I;
    const int32_t *rank;
    const double *QQ;
    long long qq_rs, qq_cs;
    double *Q;
    long long q_rs, q_cs;
    int32_t *in_tree;
    int qq_aos, q_aos;
};

struct WtRow {  // row `first + k` of a strided matrix as a TreeQ
    const double *p;
    long long rs, cs, first;
    bool aos;
    __device__ __forceinline__ TreeQ operator()(uint32_t k) const {
        const double4 r = ld_row(p, rs, cs, first + (long long)k, aos);
        return TreeQ{r.x, r.y, r.z, r.w};
    }
};

__device__ __forceinline__ void wt_finish(WinTreeResult *res, int status, int left, int rank_pos, int rank_max, int seq) {
    res->status = status;
    res->left = left;
    res->rank_pos = rank_pos;
    res->rank_max = rank_max;
    __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Workgroup b takes the problem of descriptor b: sizes and offsets from D[b], the result to R[D[b].idx].
__global__ __launch_bounds__(WT_THREADS) void k_window_tree(int seq, const WinDesc *__restrict__ D, WinTreeUser U,
                                                            WinTreeResult *__restrict__ R) {
    extern __shared__ TreeQ wt_lds[];
    __shared__ int sFlag, sOut[3];  // sOut: nodes left outside the root's component, tree edges of rank > 0, the largest rank
    const WinDesc d = D[blockIdx.x];
    WinTreeResult *res = R + d.idx;
    const int t = threadIdx.x, nv = d.nv, f = d.f, ne = d.ne;
    if (nv < 2 || nv > WIN_MAX_NV || f < 1 || f >= nv || nv - f > WIN_MAX_NU || ne < 1 || ne > WIN_MAX_NE) {  // (the host checks the same)
        if (t == 0) wt_finish(res, IROTAVG_ERR_BAD_ARG, 0, 0, 0, seq);
        return;
    }
    const int nu = nv - f, nn = nu + 1;
    const WinTreeLds L = wintree_lds(nn, ne);
    char *base = reinterpret_cast<char *>(wt_lds);
    const auto sRel = [&](int copy) { return wt_lds + copy * nn; };
    unsigned long long *sBest = reinterpret_cast<unsigned long long *>(base + L.oBest);
    uint64_t *sVia = reinterpret_cast<uint64_t *>(base + L.oVia);
    const auto sComp = [&](int copy) { return reinterpret_cast<int32_t *>(base + L.oComp) + copy * nn; };
    uint32_t *sEnds = reinterpret_cast<uint32_t *>(base + L.oEnds);
    const int2 *I = U.I + d.eoff;

    // ---- 1. guard (nothing has been indexed with an id so far)
    if (t == 0) sFlag = 0;
    __syncthreads();
    bool outside = false;
    int2 mine[WT_EDGES];
#pragma unroll
    for (int j = 0; j < WT_EDGES; j++) {
        const int k = t + j * WT_THREADS;
        mine[j] = make_int2(0, 0);
        if (k >= ne) continue;
        mine[j] = I[k];
        outside = outside || (unsigned)mine[j].x >= (unsigned)nv || (unsigned)mine[j].y >= (unsigned)nv;
    }
    if (outside) sFlag = 1;
    __syncthreads();
    if (sFlag != 0) {
        if (t == 0) wt_finish(res, IROTAVG_ERR_BAD_ARG, 0, 0, 0, seq);
        return;
    }

    // ---- 2. stage: an edge that is never used has no key (its nodes stay 0, 0)
    uint64_t key[WT_EDGES];
    int na[WT_EDGES], nb[WT_EDGES];
#pragma unroll
    for (int j = 0; j < WT_EDGES; j++) {
        const int k = t + j * WT_THREADS;
        key[j] = TREE_KEY_NONE;
        na[j] = nb[j] = 0;
        if (k >= ne) continue;
        const int32_t rk = U.rank ? U.rank[d.eoff + k] : 0;
        sEnds[k] = wt_ends(mine[j].x, mine[j].y);
        if (!wt_usable(mine[j].x, mine[j].y, f, rk)) continue;
        key[j] = tree_key(rk, (uint32_t)k);
        na[j] = wt_node(mine[j].x, f);
        nb[j] = wt_node(mine[j].y, f);
    }
    if (t < nn) {
        sComp(0)[t] = t;
        sRel(0)[t] = tree_identity();
        sVia[t] = TREE_KEY_NONE;
    }

    // ---- 3. rounds
    const WtRow qq{U.QQ, U.qq_rs, U.qq_cs, d.eoff, U.qq_aos != 0}, q{U.Q, U.q_rs, U.q_cs, d.voff, U.q_aos != 0};
    int cur = 0;
    const int rounds = min(wt_rounds(nu), WT_MAX_ROUNDS);
    for (int round = 0; round < rounds; round++) {
        if (t < nn) sBest[t] = TREE_KEY_NONE;
        if (t == 0) sFlag = 0;
        __syncthreads();  // (also: the state of `cur` is written)
#pragma unroll
        for (int j = 0; j < WT_EDGES; j++) {
            if (key[j] == TREE_KEY_NONE) continue;
            const int32_t ca = sComp(cur)[na[j]], cb = sComp(cur)[nb[j]];
            if (ca == cb) continue;
            atomicMin(&sBest[ca], (unsigned long long)key[j]);
            atomicMin(&sBest[cb], (unsigned long long)key[j]);
        }
        __syncthreads();
        if (t < nn) {
            uint64_t by;
            int32_t c;
            TreeQ r;
            if (wt_hook(t, f, sComp(cur), sRel(cur), reinterpret_cast<const uint64_t *>(sBest), sEnds, qq, q, c, r, by)) {
                sVia[t] = by;
                sFlag = 1;
            }
            sComp(cur ^ 1)[t] = c;
            sRel(cur ^ 1)[t] = r;
        }
        cur ^= 1;
        __syncthreads();
        if (sFlag == 0) break;  // uniform: read behind the barrier, written again only behind the next one
        const int passes = min(wt_passes(nu, round), WT_MAX_PASSES);
        for (int j = 0; j < passes; j++) {
            if (t < nn) {
                int32_t c;
                TreeQ r;
                wt_jump(t, sComp(cur), sRel(cur), c, r);
                sComp(cur ^ 1)[t] = c;
                sRel(cur ^ 1)[t] = r;
            }
            cur ^= 1;
            __syncthreads();
        }
    }

    // ---- 4. spanning, and the counts of the record: the first wave, lane l for nodes l and l + 64
    __syncthreads();
    if (t < 64) {
        int left = 0, rank_pos = 0, rank_max = 0;
        for (int v = t; v < WT_MAX_NODES; v += 64) {
            if (v == 0 || v >= nn) continue;
            const bool joined = sComp(cur)[v] == 0;
            left += !joined;
            if (!joined) continue;
            const int32_t rk = tree_key_rank(sVia[v]);
            rank_pos += rk > 0;
            rank_max = max(rank_max, rk);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            left += __shfl_xor(left, o, 64);
            rank_pos += __shfl_xor(rank_pos, o, 64);
            rank_max = max(rank_max, __shfl_xor(rank_max, o, 64));
        }
        if (t == 0) sOut[0] = left, sOut[1] = rank_pos, sOut[2] = rank_max;
    }
    __syncthreads();
    if (sOut[0] != 0) {
        if (t == 0) wt_finish(res, IROTAVG_ERR_NOT_SPANNING, sOut[0], 0, 0, seq);
        return;
    }

    // ---- 5. stores, last of all: every node has hooked exactly once, by a tree edge
    if (t >= 1 && t < nn) {
        const TreeQ r = sRel(cur)[t];
        st_row(U.Q, U.q_rs, U.q_cs, d.voff + wt_view(t, f), U.q_aos != 0, make_double4(r.x, r.y, r.z, r.w));
        if (U.in_tree) atomicOr(&sEnds[tree_key_edge(sVia[t])], WT_IN_TREE);
    }
    __syncthreads();
    if (U.in_tree)
        for (int k = t; k < ne; k += WT_THREADS) U.in_tree[d.eoff + k] = (sEnds[k] & WT_IN_TREE) != 0;
    __threadfence_system();
    __syncthreads();
    if (t == 0) wt_finish(res, IROTAVG_OK, 0, sOut[1], sOut[2], seq);
}

}  // namespace

// The block of records and descriptors, the sequence number and the lock: batchdev.hpp (the family's own instance).
// The arguments have been checked (devapi.hip) and `plan` made from the caller's sizes (winbatch.hpp: kernel 1, so one
// list in the caller's order)
int window_init_tree_batch_dev(const WinBatchPlan &plan, const WinTreeArrays &A, int32_t *results, hipStream_t stream) {
    auto &drv = BatchDev<WinTreeResult, WinDesc>::get();
    const size_t nb = plan.desc.size();
    size_t lds = 0;  // the largest problem of THIS batch
    for (const WinDesc &d : plan.desc) lds = std::max(lds, wintree_lds(d.nv - d.f + 1, d.ne).bytes);
    const auto s = drv.stage(plan.desc.data(), nb);
    const WinTreeUser U{reinterpret_cast<const int2 *>(A.I), A.rank, A.QQ, A.qq_rs, A.qq_cs, A.Q, A.q_rs, A.q_cs, A.in_tree,
                        rows16(reinterpret_cast<uintptr_t>(A.QQ), A.qq_rs, A.qq_cs),
                        rows16(reinterpret_cast<uintptr_t>(A.Q), A.q_rs, A.q_cs)};
    hipLaunchKernelGGL(k_window_tree, dim3((unsigned)nb), dim3(WT_THREADS), lds, stream, s.seq, s.D, U, s.Rd);
    IRH_CHECK(hipGetLastError());
    return drv.finish(s, stream, nb, [&](size_t b, const WinTreeResult &r) {  // (record b is problem b: the plan keeps the caller's order)
        if (!results) return;
        results[4 * b] = r.status;
        results[4 * b + 1] = r.left;
        results[4 * b + 2] = r.rank_pos;
        results[4 * b + 3] = r.rank_max;
    });
}

}  // namespace irh
