// winmst.hip -- irotavg_init_mst for many window-size problems on the caller's packed device arrays, one workgroup per
// problem, ONE launch (irotavg_window_init_mst_batch_dev; docs/window_init_batch.md). The host call is a sequential,
// order-dependent sweep of the edge list; winmst.hpp restates it as a least fixed point that any order of relaxations
// reaches, and the kernel relaxes with a 32-bit LDS atomicMin. The tree it finds is the sweep's, edge for edge and
// direction for direction, and the products along it are formed operand by operand as h_qmul (capi.cpp) forms them, so
// the rows it leaves are bitwise the host's.
//
// The body of k_window_mst_user, in order:
//   1. guard      every endpoint against [0, nv), a workgroup-wide OR before anything is indexed with one
//   2. endpoints into LDS; labels never, the root's 0
//   3. relaxation rounds over the edges (thread t: edges t, t + 256, ...), both directions, self-loops skipped; a
//                 workgroup-wide "changed" word ends them
//   4. spanning   a label still never: IROTAVG_ERR_NOT_SPANNING
//   5. evaluation fixed rows from the caller's array into LDS; in rounds, a free view whose parent was done in an earlier
//                 round forms its product from the parent's LDS row and its own row of QQ (only tree edges are read)
//   6. stores     the free rows, then the record, its sequence number last at system scope
// Every loop over rounds is a `for` with a bound (nv + 1 relaxation rounds, nv evaluation rounds): a defect ends as a
// wrong answer or a status, never as a workgroup that does not return. A problem that fails stores nothing but its record.
// Fixed rows are never written; free rows are never read (each is written in LDS before it is used).
#include <algorithm>
#include <cstring>

#include "batchdev.hpp"  // the host's side of the call: block, sequence number, lock, wait
#include "graph.hpp"
#include "winbatch.hpp"  // WinDesc, the plan of a batch, rows16
#include "winio.hpp"     // ld_row / st_row
#include "winmst.hpp"    // labels, mst_first_visit, mst_qmul, winmst_lds_bytes, WinMstResult

namespace irh {
namespace {

constexpr int WM_THREADS = 256;
constexpr int WM_EDGES = (WIN_MAX_NE + WM_THREADS - 1) / WM_THREADS;  // edges of one thread
constexpr int WM_PASSES = 4;            // relaxation passes between two looks at the "changed" word
constexpr int WM_PENDING = 0x7fffffff;  // the evaluation round of a free view that has no rotation yet

// hipcc would fuse products into fma chains; the x86 build of h_qmul has none (wincov.hip's note). mst_qmul carries the
// same setting in its own body; this one covers whatever else this file comes to compute.
#pragma clang fp contract(off)

struct WinMstUser {  // the caller's packed arrays of a batch (kernel argument)
    const int2 *I;
    const double *QQ;
    long long qq_rs, qq_cs;
    double *Q;
    long long q_rs, q_cs;
    int qq_aos, q_aos;
};

// A word of LDS that other threads of the workgroup write in the same round: read and written whole, never kept in a
// register across the round
template <typename T>
__device__ __forceinline__ T wm_ld(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
template <typename T>
__device__ __forceinline__ void wm_st(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ void wm_finish(WinMstResult *res, int status, int seq) {
    res->status = status;
    __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Workgroup b takes the problem of descriptor b: sizes and offsets from D[b], the result to R[D[b].idx].
__global__ __launch_bounds__(WM_THREADS) void k_window_mst_user(int seq, const WinDesc *__restrict__ D, WinMstUser U,
                                                                WinMstResult *__restrict__ R) {
    extern __shared__ double4 wm_lds[];
    __shared__ int sFlag;
    const WinDesc d = D[blockIdx.x];
    WinMstResult *res = R + d.idx;
    const int t = threadIdx.x, nv = d.nv, f = d.f, ne = d.ne;
    if (nv < 2 || nv > WIN_MAX_NV || f < 1 || f >= nv || ne < 1 || ne > WIN_MAX_NE) {  // (the host checks the same)
        if (t == 0) wm_finish(res, IROTAVG_ERR_BAD_ARG, seq);
        return;
    }
    double4 *sQ = wm_lds;                                       // nv rotations
    int2 *sI = reinterpret_cast<int2 *>(sQ + nv);               // ne endpoints
    unsigned *sL = reinterpret_cast<unsigned *>(sI + ne);       // nv labels
    int *sDone = reinterpret_cast<int *>(sL + nv);              // nv: 0 fixed, r + 1 evaluated in round r, WM_PENDING
    const int2 *I = U.I + d.eoff;

    // ---- 1. guard (nothing has been indexed with an id so far), 2. endpoints and labels
    if (t == 0) sFlag = 0;
    __syncthreads();
    bool outside = false;
    int2 mine[WM_EDGES];  // the thread's own edges tid, tid + T, ... stay in registers for the relaxation (none: a self-loop)
#pragma unroll
    for (int j = 0; j < WM_EDGES; j++) {
        const int k = t + j * WM_THREADS;
        mine[j] = make_int2(0, 0);
        if (k >= ne) continue;
        const int2 e = I[k];
        outside = outside || (unsigned)e.x >= (unsigned)nv || (unsigned)e.y >= (unsigned)nv;
        sI[k] = e;
        mine[j] = e;
    }
    for (int v = t; v < nv; v += WM_THREADS) sL[v] = v == 0 ? MST_ROOT : MST_INF;
    if (outside) sFlag = 1;
    __syncthreads();
    if (sFlag != 0) {
        if (t == 0) wm_finish(res, IROTAVG_ERR_BAD_ARG, seq);
        return;
    }

    // ---- 3. relaxation: labels only fall, towards the one fixed point; a view of tree depth r is final after round r.
    // A round is WM_PASSES passes over the thread's edges between two looks at the "changed" word: an atomicMin in LDS
    // is seen by the other waves without a barrier, so a label usually travels several edges per round and the barriers
    // (which a deep tree at the limits pays some 300 times) are shared by the passes. The bound does not rest on that:
    // the first pass of a round reads behind a barrier, so every round settles at least one more level of the tree, and
    // a round in which nothing fell has relaxed every edge against the final labels.
    for (int r = 0; r < nv + 1; r++) {
        __syncthreads();  // (everyone has read the word of the round before)
        if (t == 0) sFlag = 0;
        __syncthreads();
        bool changed = false;
        for (int pass = 0; pass < WM_PASSES; pass++) {
            // the labels of all the thread's ends first (the loads are in flight together), then the minima: a label
            // that has fallen since it was read only makes this pass offer less than it could
            unsigned lx[WM_EDGES], ly[WM_EDGES];
#pragma unroll
            for (int j = 0; j < WM_EDGES; j++) {
                lx[j] = wm_ld(&sL[mine[j].x]);
                ly[j] = wm_ld(&sL[mine[j].y]);
            }
#pragma unroll
            for (int j = 0; j < WM_EDGES; j++) {
                const int2 e = mine[j];
                if (e.x == e.y) continue;
                const unsigned k = (unsigned)(t + j * WM_THREADS);
                const unsigned la = mst_first_visit(lx[j], k), lb = mst_first_visit(ly[j], k);
                if (la < ly[j]) changed = atomicMin(&sL[e.y], la) > la || changed;
                if (lb < lx[j]) changed = atomicMin(&sL[e.x], lb) > lb || changed;
            }
        }
        if (changed) sFlag = 1;
        __syncthreads();
        if (sFlag == 0) break;  // uniform: read behind the barrier
    }

    // ---- 4. spanning
    __syncthreads();
    if (t == 0) sFlag = 0;
    __syncthreads();
    bool never = false;
    for (int v = t; v < nv; v += WM_THREADS) never = never || sL[v] == MST_INF;
    if (never) sFlag = 1;
    __syncthreads();
    if (sFlag != 0) {
        if (t == 0) wm_finish(res, IROTAVG_ERR_NOT_SPANNING, seq);
        return;
    }

    // ---- 5. evaluation
    for (int v = t; v < nv; v += WM_THREADS) {
        if (v < f) sQ[v] = ld_row(U.Q, U.q_rs, U.q_cs, d.voff + v, U.q_aos != 0);
        sDone[v] = v < f ? 0 : WM_PENDING;
    }
    for (int r = 0; r < nv; r++) {
        __syncthreads();
        if (t == 0) sFlag = 0;
        __syncthreads();
        bool pending = false;
        for (int v = f + t; v < nv; v += WM_THREADS) {
            if (sDone[v] != WM_PENDING) continue;
            const int k = (int)mst_edge_of(sL[v]);
            const int2 e = sI[k];
            const bool fwd = e.y == v;
            const int p = fwd ? e.x : e.y;
            if (wm_ld(&sDone[p]) > r) {  // not yet, or in this very round (its row may be half written)
                pending = true;
                continue;
            }
            const double4 m = ld_row(U.QQ, U.qq_rs, U.qq_cs, d.eoff + k, U.qq_aos != 0), qp = sQ[p];
            // forward Q_b = QQ_k (x) Q_a; backward Q_a = QQ_k* (x) Q_b, only w of QQ_k negated
            const double a[4] = {m.x, m.y, m.z, fwd ? m.w : -m.w}, b[4] = {qp.x, qp.y, qp.z, qp.w};
            double o[4];
            mst_qmul(a, b, o);
            sQ[v] = make_double4(o[0], o[1], o[2], o[3]);
            wm_st(&sDone[v], r + 1);
        }
        if (pending) sFlag = 1;
        __syncthreads();
        if (sFlag == 0) break;
    }
    __syncthreads();
    if (sFlag != 0) {  // (a spanning tree is evaluated in at most nv - f rounds: not reached)
        if (t == 0) wm_finish(res, IROTAVG_ERR_SOLVER, seq);
        return;
    }

    // ---- 6. stores, last of all
    for (int v = f + t; v < nv; v += WM_THREADS) st_row(U.Q, U.q_rs, U.q_cs, d.voff + v, U.q_aos != 0, sQ[v]);
    __threadfence_system();
    __syncthreads();
    if (t == 0) wm_finish(res, IROTAVG_OK, seq);
}

}  // namespace

// The block of records and descriptors, the sequence number and the lock: batchdev.hpp (the family's own instance).
// The arguments have been checked (devapi.hip) and `plan` made from the caller's sizes (winbatch.hpp: kernel 1, so one
// list in the caller's order)
int window_init_mst_batch_dev(const WinBatchPlan &plan, int device, const WinBatchArrays &A, int32_t *results, hipStream_t stream) {
    (void)device;
    auto &drv = BatchDev<WinMstResult, WinDesc>::get();
    const size_t nb = plan.desc.size();
    static_assert(winmst_lds_bytes(WIN_MAX_NV, WIN_MAX_NE) <= 20 * 1024, "many problems share a compute unit");
    static_assert(WIN_MAX_NE <= MST_STRIDE && (uint64_t)WIN_MAX_NV * MST_STRIDE < (1ull << 31), "labels: one stride per sweep, 32 bits");
    size_t lds = 0;  // the largest problem of THIS batch
    for (const WinDesc &d : plan.desc) lds = std::max(lds, winmst_lds_bytes(d.nv, d.ne));
    const auto s = drv.stage(plan.desc.data(), nb);
    const WinMstUser U{reinterpret_cast<const int2 *>(A.I), A.QQ, A.qq_rs, A.qq_cs, A.Q, A.q_rs, A.q_cs,
                       rows16(reinterpret_cast<uintptr_t>(A.QQ), A.qq_rs, A.qq_cs),
                       rows16(reinterpret_cast<uintptr_t>(A.Q), A.q_rs, A.q_cs)};
    hipLaunchKernelGGL(k_window_mst_user, dim3((unsigned)nb), dim3(WM_THREADS), lds, stream, s.seq, s.D, U, s.Rd);
    IRH_CHECK(hipGetLastError());
    return drv.finish(s, stream, nb, [&](size_t b, const WinMstResult &r) {  // (record b is problem b: the plan keeps the caller's order)
        if (results) results[b] = r.status;
    });
}

}  // namespace irh
