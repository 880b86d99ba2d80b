// wincemp.hip -- cycle-edge message passing for many window-size problems on the caller's packed device arrays, one
// workgroup per problem, ONE launch (irotavg_window_cemp_batch_dev; docs/window_cemp_batch.md). The definition is that of
// irotavg_cycle_cemp (docs/cycle_check.md, "Corruption estimates"); the route is not: everything a problem needs -- its
// measurements, its 2m half-edges as 32-bit words, a row-start table and both planes of estimates -- fits in LDS, so
// there is no global sort, no scan and no triangle table, and the start vector and all iterations run inside the launch.
// The triangles are enumerated again from LDS in every iteration.
//
// The body of k_window_cemp, in order:
//   1. guard      every endpoint against [0, nv), a workgroup-wide OR before anything is indexed with one
//   2. stage      the rows of QQ through ld_row, the ends of every edge, the two half-edge words of every edge; self loops
//                 and the padding of the network are the word of all ones
//   3. sort       a bitonic network over the next power of two, one barrier per stage; then the row-start table,
//                 nv + 1 searches of 11 rounds
//   4. start      32 groups of 8 lanes, group g takes edges g, g + 32, ...; a group walks the shorter row of its edge 8
//                 entries a round, every lane searches the longer row and walks the run of equals; the error of every
//                 hit is formed from the LDS quaternions. Per lane the sum of d in visit order and the count, then the
//                 shuffle tree (lane ^ 4, 2, 1): the plain mean into plane 0, the count into LDS
//   5. iterations the same walk; a lane keeps (e, d) of its first kHold used triangles in registers while the group
//                 forms the shift (a minimum: order-free), then adds its terms in visit order -- from the registers, and
//                 beyond them by walking its entries once more --, then the same tree. Plane t & 1 is read, the other
//                 written, one barrier per iteration
//   6. stores     s, tri_used, then the record, its sequence number last at system scope
// Every loop is bounded by a row length, the edge count, the iteration count or the network's stage count; there are no
// atomics, no flag between workgroups and no cooperative or persistent launch: a defect ends as a wrong number or a
// status. A problem that fails the guard stores nothing but its record. No sum depends on another problem or on timing:
// a problem gives the same bytes alone, first or last in a batch, and in every call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batchdev.hpp"  // the host's side of the call: block, sequence number, lock, wait
#include "cemp.hpp"      // cemp_finite, cemp_mean, cemp_e, cemp_min, cemp_term, cemp_quotient; cycles.hpp: the triangle error
#include "graph.hpp"
#include "winbatch.hpp"  // WinDesc, the plan of a batch, rows16
#include "wincemp.hpp"   // the word, the network, the rows, the walk of a lane, the LDS layout, WinCempResult
#include "winio.hpp"     // ld_row

namespace irh {
namespace {

constexpr int kEdges = (WIN_MAX_NE + WC_THREADS - 1) / WC_THREADS;  // edges of one thread in the guard and the staging
constexpr int kHold = 4;  // used triangles a lane keeps in registers between the shift and the sums: 32 per edge

struct WinCempUser {  // the caller's packed arrays of a batch (kernel argument)
    const int2 *I;
    const double *QQ;
    long long qq_rs, qq_cs;
    int qq_aos, iters;
    double *s;
    int32_t *used;
};
struct WinCempBeta {  // the schedule, by value
    double v[CEMP_MAX_ITERS];
};

__device__ __forceinline__ CycQ wc_q(const double4 *sQ, uint32_t k, bool against) {
    const double4 q = sQ[k];
    return cyc_directed(CycQ{q.x, q.y, q.z, q.w}, against);
}

// the sinks of wc_entry: (k1, against, k2, against) of one triangle of the group's edge
struct WcStart {  // the start pass: the lane's sum of d in visit order, and its count
    const double4 *sQ;
    CycQ q0;
    double sum;
    int n;
    __device__ __forceinline__ void operator()(uint32_t k1, bool g1, uint32_t k2, bool g2) {
        const double d = cyc_triangle_error(q0, wc_q(sQ, k1, g1), wc_q(sQ, k2, g2));
        if (cemp_finite(d)) {
            sum += d;
            n++;
        }
    }
};
struct WcShift {  // an iteration's first walk: the lane's smallest e; (e, d) of its first kHold used triangles stay
    const double4 *sQ;
    const double *s;
    CycQ q0;
    double mu, e[kHold], d[kHold];
    int n;
    __device__ __forceinline__ void operator()(uint32_t k1, bool g1, uint32_t k2, bool g2) {
        const double dv = cyc_triangle_error(q0, wc_q(sQ, k1, g1), wc_q(sQ, k2, g2));
        if (!cemp_finite(dv)) return;
        const double ev = cemp_e(s[k1], s[k2]);
        cemp_min(mu, ev);
#pragma unroll
        for (int j = 0; j < kHold; j++)
            if (n == j) e[j] = ev, d[j] = dv;
        n++;
    }
};
struct WcRest {  // ... and its second, for a lane with more than kHold: the terms from there on, in the same order
    const double4 *sQ;
    const double *s;
    CycQ q0;
    double beta, mu;
    CempSum a;
    int n;
    __device__ __forceinline__ void operator()(uint32_t k1, bool g1, uint32_t k2, bool g2) {
        const double dv = cyc_triangle_error(q0, wc_q(sQ, k1, g1), wc_q(sQ, k2, g2));
        if (!cemp_finite(dv)) return;
        if (n >= kHold) cemp_term(a, dv, cemp_e(s[k1], s[k2]), beta, mu);
        n++;
    }
};

__device__ __forceinline__ void wc_finish(WinCempResult *res, int status, int used, int untested, int seq) {
    res->status = status;
    res->used = used;
    res->untested = untested;
    __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Workgroup b takes the problem of descriptor b: sizes and offsets from D[b], the result to R[D[b].idx].
__global__ __launch_bounds__(WC_THREADS) void k_window_cemp(int seq, const WinDesc *__restrict__ D, WinCempUser U, WinCempBeta B,
                                                            WinCempResult *__restrict__ R) {
    extern __shared__ double4 wc_lds[];
    __shared__ int sFlag;
    __shared__ int sRed[WC_THREADS / 64][2];
    const WinDesc d = D[blockIdx.x];
    WinCempResult *res = R + d.idx;
    const int t = threadIdx.x, nv = d.nv, ne = d.ne, iters = U.iters;
    if (nv < 1 || nv > WIN_MAX_NV || ne < 1 || ne > WIN_MAX_NE || iters < 0 || iters > CEMP_MAX_ITERS) {  // (the host checks the same)
        if (t == 0) wc_finish(res, IROTAVG_ERR_BAD_ARG, 0, 0, seq);
        return;
    }
    const WinCempLds L = wincemp_lds(nv, ne);
    unsigned char *const lds = reinterpret_cast<unsigned char *>(wc_lds);
    double4 *sQ = reinterpret_cast<double4 *>(lds + L.oQQ);        // ne measurements
    double *sS = reinterpret_cast<double *>(lds + L.oS);           // two planes of ne estimates
    uint32_t *sW = reinterpret_cast<uint32_t *>(lds + L.oW);       // the network's words; the first 2 ne hold the rows
    int *sStart = reinterpret_cast<int *>(lds + L.oStart);         // nv + 1 row starts
    uint32_t *sEnds = reinterpret_cast<uint32_t *>(lds + L.oEnds);  // ne: both ends of an edge
    int *sUsed = reinterpret_cast<int *>(lds + L.oUsed);           // ne: |U(k)|
    const int2 *I = U.I + d.eoff;

    // ---- 1. guard (nothing has been indexed with an id so far)
    if (t == 0) sFlag = 0;
    __syncthreads();
    bool outside = false;
    int2 mine[kEdges];
#pragma unroll
    for (int j = 0; j < kEdges; j++) {
        const int k = t + j * WC_THREADS;
        mine[j] = make_int2(0, 0);
        if (k >= ne) continue;
        mine[j] = I[k];
        outside = outside || (unsigned)mine[j].x >= (unsigned)nv || (unsigned)mine[j].y >= (unsigned)nv;
    }
    if (outside) sFlag = 1;
    __syncthreads();
    if (sFlag != 0) {
        if (t == 0) wc_finish(res, IROTAVG_ERR_BAD_ARG, 0, 0, seq);
        return;
    }

    // ---- 2. stage
    const int n2 = 2 * ne, N = wc_sort_len(n2);
#pragma unroll
    for (int j = 0; j < kEdges; j++) {
        const int k = t + j * WC_THREADS;
        if (k >= ne) continue;
        sQ[k] = ld_row(U.QQ, U.qq_rs, U.qq_cs, d.eoff + k, U.qq_aos != 0);
        sEnds[k] = wc_ends((uint32_t)mine[j].x, (uint32_t)mine[j].y);
        uint32_t w[2];
        wc_emit((uint32_t)k, (uint32_t)mine[j].x, (uint32_t)mine[j].y, w);
        sW[2 * k] = w[0];
        sW[2 * k + 1] = w[1];
    }
    for (int i = n2 + t; i < N; i += WC_THREADS) sW[i] = WC_NONE;
    __syncthreads();

    // ---- 3. sort (the positions of one stage touch disjoint words), then the row starts
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < N; i += WC_THREADS) wc_bitonic(sW, i, j, k);
            __syncthreads();
        }
    for (int u = t; u <= nv; u += WC_THREADS) sStart[u] = wc_row_start(sW, n2, (uint32_t)u);
    __syncthreads();

    // ---- 4. start pass. A group's lanes share k, so the shuffles of a group are whole; a group without an edge in the
    // last pass walks nothing and stores nothing.
    const int lane = t % WC_GROUP, grp = t / WC_GROUP;
    for (int base = 0; base < ne; base += WC_GROUPS) {
        const int k = base + grp;
        const bool valid = k < ne;
        const uint32_t ends = valid ? sEnds[k] : 0u;
        const uint32_t a = wc_end_a(ends), b = wc_end_b(ends);
        WcStart st{sQ, CycQ{0.0, 0.0, 0.0, 1.0}, 0.0, 0};
        if (a != b) {  // (an edge and no self loop)
            st.q0 = wc_q(sQ, (uint32_t)k, false);
            wc_lane(sW, wc_rows(sStart, a, b), lane, st);
        }
#pragma unroll
        for (int o = WC_GROUP / 2; o > 0; o >>= 1) {
            st.sum += __shfl_xor(st.sum, o, WC_GROUP);
            st.n += __shfl_xor(st.n, o, WC_GROUP);
        }
        if (valid && lane == 0) {
            sS[k] = cemp_mean(st.sum, st.n);
            sUsed[k] = st.n;
        }
    }
    __syncthreads();

    // ---- 5. iterations (Jacobi: plane it & 1 is read, the other written)
    for (int it = 0; it < iters; it++) {
        const double *sin = sS + (it & 1) * ne;
        double *sout = sS + ((it + 1) & 1) * ne;
        const double beta = B.v[it];
        for (int base = 0; base < ne; base += WC_GROUPS) {
            const int k = base + grp;
            const bool valid = k < ne;
            const uint32_t ends = valid ? sEnds[k] : 0u;
            const uint32_t a = wc_end_a(ends), b = wc_end_b(ends);
            WcShift sh;
            sh.sQ = sQ, sh.s = sin, sh.q0 = CycQ{0.0, 0.0, 0.0, 1.0}, sh.mu = std::numeric_limits<double>::infinity(), sh.n = 0;
#pragma unroll
            for (int j = 0; j < kHold; j++) sh.e[j] = sh.d[j] = 0.0;
            WcRows rows{0, 0, 0, 0, 0u, false};
            if (a != b) {
                sh.q0 = wc_q(sQ, (uint32_t)k, false);
                rows = wc_rows(sStart, a, b);
                wc_lane(sW, rows, lane, sh);
            }
            double mu = sh.mu;
#pragma unroll
            for (int o = WC_GROUP / 2; o > 0; o >>= 1) cemp_min(mu, __shfl_xor(mu, o, WC_GROUP));
            CempSum acc{0.0, 0.0};
#pragma unroll
            for (int j = 0; j < kHold; j++)
                if (j < sh.n) cemp_term(acc, sh.d[j], sh.e[j], beta, mu);
            if (sh.n > kHold) {
                WcRest rest{sQ, sin, sh.q0, beta, mu, acc, 0};
                wc_lane(sW, rows, lane, rest);
                acc = rest.a;
            }
#pragma unroll
            for (int o = WC_GROUP / 2; o > 0; o >>= 1) {
                acc.num += __shfl_xor(acc.num, o, WC_GROUP);
                acc.den += __shfl_xor(acc.den, o, WC_GROUP);
            }
            if (valid && lane == 0) sout[k] = cemp_quotient(acc);
        }
        __syncthreads();
    }

    // ---- 6. stores, last of all
    const double *sfin = sS + (iters & 1) * ne;
    int used = 0, untested = 0;
    for (int k = t; k < ne; k += WC_THREADS) {
        const int c = sUsed[k];
        if (U.s) U.s[d.eoff + k] = sfin[k];
        if (U.used) U.used[d.eoff + k] = c;
        used += c;
        untested += c == 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        used += __shfl_xor(used, o, 64);
        untested += __shfl_xor(untested, o, 64);
    }
    if ((t & 63) == 0) sRed[t >> 6][0] = used, sRed[t >> 6][1] = untested;
    __threadfence_system();
    __syncthreads();
    if (t == 0) {
        used = untested = 0;
        for (int w = 0; w < WC_THREADS / 64; w++) used += sRed[w][0], untested += sRed[w][1];
        wc_finish(res, IROTAVG_OK, used, untested, seq);
    }
}

}  // namespace

// The block of records and descriptors, the sequence number and the lock: batchdev.hpp (the family's own instance).
// The arguments have been checked (devapi.hip) and `plan` made from the caller's sizes (winbatch.hpp: kernel 1, so one
// list in the caller's order)
int window_cemp_batch_dev(const WinBatchPlan &plan, const WinCempArrays &A, int iters, const double *beta, int32_t *results,
                          hipStream_t stream) {
    auto &drv = BatchDev<WinCempResult, WinDesc>::get();
    const size_t nb = plan.desc.size();
    size_t lds = 0;  // the largest problem of THIS batch
    for (const WinDesc &d : plan.desc) lds = std::max(lds, wincemp_lds(d.nv, d.ne).bytes);
    WinCempBeta B{};
    for (int t = 0; t < iters; t++) B.v[t] = beta[t];
    const auto s = drv.stage(plan.desc.data(), nb);
    const WinCempUser U{reinterpret_cast<const int2 *>(A.I), A.QQ, A.qq_rs, A.qq_cs,
                        rows16(reinterpret_cast<uintptr_t>(A.QQ), A.qq_rs, A.qq_cs), iters, A.s, A.tri_used};
    hipLaunchKernelGGL(k_window_cemp, dim3((unsigned)nb), dim3(WC_THREADS), lds, stream, s.seq, s.D, U, B, s.Rd);
    IRH_CHECK(hipGetLastError());
    return drv.finish(s, stream, nb, [&](size_t b, const WinCempResult &r) {  // (record b is problem b: the plan keeps the caller's order)
        if (results) results[3 * b] = r.status, results[3 * b + 1] = r.used, results[3 * b + 2] = r.untested;
    });
}

}  // namespace irh
