// sweep.hip -- Weiszfeld sweeps: every free view moved to the geodesic median (L1) or mean (L2) of what its neighbours
// predict for it (irotavg_weiszfeld, irotavg_weiszfeld_dev; docs/local_sweeps.md), on one stream:
//   1. emit, sort, AoS image   those of the triangle test (cycles.hip: cyc_prep_alloc / cyc_prep_run);
//   2. k_sweep_rows   one thread per free view: the bounds of its row by two searches, stored as two int32, ONCE per call
//                     (a search per sweep would put some 44 dependent loads in front of a row of about 40 entries); per
//                     workgroup the half-edges in those rows and the empty rows;
//      k_sweep_pack   the caller's strided Q into two planes of 32-byte rows that ping-pong; the fixed rows go into both;
//   3. k_sweep<L1, G> the hot path, one launch per sweep: one group of G lanes per free view, the views dealt to the
//                     workgroups in contiguous XCD-aware chunks (tile_range), so that neighbouring views of a sequence
//                     find their neighbours' rotations in one XCD's L2. A group walks its row G entries a round: key and
//                     value coalesced across the group, per lane two 16-byte loads of QQ_k and two of Q^t[u]. With
//                     inner > 1 a lane keeps the predictions of its first kStage / G rounds in the group's LDS slab and
//                     forms the later ones again from global memory in every inner iteration (slower, bounded, the same
//                     sums). A lane reads back only the slab entries it stored itself (lane l owns the terms l, l + G, ..
//                     in every inner iteration), so program order is all the ordering the slab needs: no fence and no
//                     __syncthreads in the row loop. The lanes' four partial sums go through one xor tree, after which
//                     every lane holds the same bits and forms the step redundantly: no broadcast. Lane 0 stores the row
//                     of Q^{t+1}; the workgroup's largest |x_0| goes to stepparts[t][workgroup];
//   4. k_sweep_finish writes the error word out and, with it clear, reduces stepparts per sweep (maxima: order-free),
//                     adds the row counts and scatters the free rows of the last plane into the caller's Q. The error
//                     word, info and step come back in one copy into a pinned block and one host wait.
// fp64 throughout; there is no product of any size here for the matrix cores. No atomics, no flag between workgroups, no
// persistent or cooperative launch; every loop is bounded by a row length, `inner` or 32 rounds of a search. Every kernel
// returns at once when the error word is set: nothing is indexed with a bad id and no byte of Q is written. Memory: the
// triangle test's O(m), 8 bytes per free view for the bounds and two planes of 32 n_total bytes, all from the device pool.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "graph.hpp"
#include "kernels.hpp"  // tile_range
#include "sweep.hpp"
#include "cycload.hpp"

#ifndef IRH_SWEEP_GROUP
#define IRH_SWEEP_GROUP 8  // 8 or 16; 16 is built for the measurement alone (docs/local_sweeps.md); not an interface
#endif

namespace irh {
namespace {

constexpr int kT = 256;
constexpr int kG = IRH_SWEEP_GROUP;
constexpr int kStage = 48;           // predictions of one view kept in LDS: 1.5 KB per group, 48 KB per workgroup at G = 8
constexpr int kSweepMaxGrid = 4096;  // a multiple of 8: tile_range deals adjacent chunks to the workgroups of one XCD
constexpr int kSweepPasses = 4;      // a small graph still gives every workgroup a few passes over its chunk
constexpr int kHead = 3;             // the read-back: error word, info[2], then `sweeps` doubles

inline unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, (n + kT - 1) / kT); }

// the workgroup's sum of two counts / its maximum, through the waves and one LDS round (all 256 threads call)
__device__ __forceinline__ void block_sum2(long long s[2], long long (*red)[2]) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; j++) {
        s[j] = 0;
        for (int w = 0; w < kT / 64; w++) s[j] += red[w][j];
    }
}
__device__ __forceinline__ double block_max(double mx, double *red) {
    for (int o = 32; o > 0; o >>= 1) sweep_max(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = 0.0;
    for (int w = 0; w < kT / 64; w++) sweep_max(mx, red[w]);
    return mx;
}

__global__ __launch_bounds__(kT) void k_sweep_rows(int nfree, int f, long long n2, const uint64_t *__restrict__ keys,
                                                   const long long *__restrict__ err, int2 *__restrict__ rows,
                                                   long long *__restrict__ parts) {
    __shared__ long long red[kT / 64][2];
    if (*err != 0) return;  // (uniform)
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    long long s[2] = {0, 0};
    if (v < nfree) {
        long long b0, b1;
        cyc_row(keys, n2, (uint32_t)(v + f), b0, b1);
        rows[v] = make_int2((int)b0, (int)b1);  // (n2 < 2^31)
        s[0] = b1 - b0;
        s[1] = b1 == b0;
    }
    block_sum2(s, red);
    if (threadIdx.x < 2) parts[2 * (size_t)blockIdx.x + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(kT) void k_sweep_pack(long long n_total, int f, const double *__restrict__ Q, long long rs, long long cs,
                                                   double2 *__restrict__ plane0, double2 *__restrict__ plane1) {
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (v >= n_total) return;
    const double *r = Q + v * rs;
    const double2 lo = make_double2(r[0], r[cs]), hi = make_double2(r[2 * cs], r[3 * cs]);
    plane0[2 * v] = lo;
    plane0[2 * v + 1] = hi;
    if (v < f) {
        plane1[2 * v] = lo;
        plane1[2 * v + 1] = hi;
    }
}

template <bool L1, int G>
__global__ __launch_bounds__(kT) void k_sweep(int nfree, int f, const int2 *__restrict__ rows, const uint64_t *__restrict__ keys,
                                              const uint32_t *__restrict__ vals, const double2 *__restrict__ qq,
                                              const double2 *__restrict__ qin, double2 *__restrict__ qout,
                                              const double *__restrict__ w, int inner, double floor,
                                              const long long *__restrict__ err, double *__restrict__ stepparts) {
    static_assert(G == 8 || G == 16, "a group lies within one wave");
    constexpr int kViews = kT / G;  // views of one pass
    __shared__ CycQ slab[kViews][kStage];
    __shared__ double red[kT / 64];
    if (*err != 0) return;  // (uniform: a bad id; nothing is indexed with it and nothing is written)
    int v0, v1;
    tile_range(nfree, v0, v1);
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const CycDevLoad loadqq{qq}, loadq{qin};
    const bool stage = inner > 1;
    double mx = 0.0;
    for (int base = v0; base < v1; base += kViews) {
        const int v = base + grp;
        const bool valid = v < v1;
        const int2 row = valid ? rows[v] : make_int2(0, 0);
        const long long beg = row.x;
        const int len = row.y - row.x;
        CycQ y = loadq((uint32_t)(f + (valid ? v : v0)));
        for (int j = 0; j < inner; j++) {  // (uniform: the shuffles below are whole)
            SweepSum a = sweep_zero();
            for (int idx = lane; idx < len; idx += G) {
                const bool staged = stage && idx < kStage;
                CycQ P;
                if (staged && j > 0) {
                    P = slab[grp][idx];
                } else {
                    P = sweep_form(keys, vals, beg + idx, loadqq, loadq);
                    if (staged) slab[grp][idx] = P;
                }
                sweep_term(a, y, P, sweep_weight(vals, beg + idx, w), L1, floor);
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1)
                a = sweep_add(a, SweepSum{__shfl_xor(a.x, o, G), __shfl_xor(a.y, o, G), __shfl_xor(a.z, o, G), __shfl_xor(a.c, o, G)});
            double x[3];
            const double th = sweep_mean(a, x);
            if (j == 0 && valid) sweep_max(mx, th);
            y = sweep_step(y, x, th);
        }
        if (valid && lane == 0) {
            qout[2 * (size_t)(f + v)] = make_double2(y.x, y.y);
            qout[2 * (size_t)(f + v) + 1] = make_double2(y.z, y.w);
        }
    }
    mx = block_max(mx, red);
    if (threadIdx.x == 0) stepparts[blockIdx.x] = mx;
}

// out[0]: the error word; behind it, with the word clear: out[1], out[2] the row counts (workgroup 0), out[3 + t] the
// step of sweep t as a double (workgroup t), and the free rows of `last` scattered into the caller's Q (every workgroup
// its 256 views)
__global__ __launch_bounds__(kT) void k_sweep_finish(int nfree, int f, int sweeps, int nrowparts, const long long *__restrict__ rowparts,
                                                     int nwg, const double *__restrict__ stepparts, const double2 *__restrict__ last,
                                                     double *__restrict__ Q, long long rs, long long cs,
                                                     const long long *__restrict__ err, long long *__restrict__ out) {
    __shared__ long long redi[kT / 64][2];
    __shared__ double redd[kT / 64];
    const long long e = *err;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = e;
    if (e != 0) return;  // (uniform)
    if (blockIdx.x == 0) {
        long long s[2] = {0, 0};
        for (int p = threadIdx.x; p < nrowparts; p += kT) s[0] += rowparts[2 * (size_t)p], s[1] += rowparts[2 * (size_t)p + 1];
        block_sum2(s, redi);
        if (threadIdx.x < 2) out[1 + threadIdx.x] = s[threadIdx.x];
    }
    if ((int)blockIdx.x < sweeps) {
        double mx = 0.0;
        for (int p = threadIdx.x; p < nwg; p += kT) sweep_max(mx, stepparts[(size_t)blockIdx.x * nwg + p]);
        mx = block_max(mx, redd);
        if (threadIdx.x == 0) reinterpret_cast<double *>(out + kHead)[blockIdx.x] = mx;
    }
    const long long v = (long long)blockIdx.x * kT + threadIdx.x;
    if (sweeps > 0 && v < nfree) {
        const double2 lo = last[2 * (v + f)], hi = last[2 * (v + f) + 1];
        double *r = Q + (v + f) * rs;
        r[0] = lo.x;
        r[cs] = lo.y;
        r[2 * cs] = hi.x;
        r[3 * cs] = hi.y;
    }
}

}  // namespace

int weiszfeld_dev(int64_t m, int64_t n_total, int f, const SweepArrays &A, int cost, int sweeps, int inner, double floor, double *step,
                  int64_t *info, hipStream_t stream) {
    const long long n2 = 2 * (long long)m;
    const int nfree = (int)(n_total - f);
    // without a free view, or without a sweep and without info, the call is the id check alone
    const bool rows_wanted = nfree > 0 && (sweeps > 0 || info);
    const bool run = rows_wanted && sweeps > 0;
    constexpr int kViews = kT / kG;
    long long nwg = std::max<long long>(1, ((long long)nfree + kViews * kSweepPasses - 1) / (kViews * kSweepPasses));
    if (nwg > 8) nwg = std::min<long long>(kSweepMaxGrid, (nwg + 7) / 8 * 8);
    const int nrowparts = (int)grid_of(nfree);
    const int nfinish = std::max(nrowparts, sweeps);
    // every temporary first (the pool): nothing after the first launch can fail for want of memory
    CycPrep P;
    DevBuf<int2> rows;
    DevBuf<long long> rowparts, out;
    DevBuf<double> stepparts;
    DevBuf<double2> plane[2];
    cyc_prep_alloc(P, m, n_total, A.QQ, A.qq_rs, A.qq_cs, rows_wanted, stream);
    if (rows_wanted) {
        rows.alloc((size_t)nfree);
        rowparts.alloc(2 * (size_t)nrowparts);
        out.alloc((size_t)kHead + (size_t)sweeps);
    }
    if (run) {
        stepparts.alloc((size_t)sweeps * (size_t)nwg);
        for (int p = 0; p < 2; p++) plane[p].alloc(2 * (size_t)n_total);
    }
    long long *h = nullptr;
    struct PinGuard {
        void *p;
        ~PinGuard() { PinPool::get().give(p); }
    } pin_guard{nullptr};
    if (rows_wanted) pin_guard.p = h = reinterpret_cast<long long *>(PinPool::get().take());  // pinned read-back block
    static_assert((kHead + SWEEP_MAX_SWEEPS) * sizeof(long long) <= PinPool::kBytes, "the read-back fits one pinned block");

    cyc_prep_run(P, m, n_total, A.I, A.QQ, A.qq_rs, A.qq_cs, stream);
    if (!rows_wanted) {
        const int rc = cyc_finish(P, 0, nullptr, nullptr, stream);
        if (rc != IROTAVG_OK) return rc;
        if (step) std::fill(step, step + sweeps, 0.0);
        if (info) info[0] = info[1] = 0;
        return IROTAVG_OK;
    }
    hipLaunchKernelGGL(k_sweep_rows, dim3((unsigned)nrowparts), dim3(kT), 0, stream, nfree, f, n2, P.kout.p, P.head.p, rows.p, rowparts.p);
    IRH_CHECK(hipGetLastError());
    if (run) {
        hipLaunchKernelGGL(k_sweep_pack, dim3(grid_of(n_total)), dim3(kT), 0, stream, (long long)n_total, f, A.Q, A.q_rs, A.q_cs,
                           plane[0].p, plane[1].p);
        IRH_CHECK(hipGetLastError());
        for (int t = 0; t < sweeps; t++) {
            const double2 *qin = plane[t & 1].p;
            double2 *qout = plane[(t + 1) & 1].p;
            double *parts = stepparts.p + (size_t)t * (size_t)nwg;
            if (cost == IROTAVG_L1)
                hipLaunchKernelGGL((k_sweep<true, kG>), dim3((unsigned)nwg), dim3(kT), 0, stream, nfree, f, rows.p, P.kout.p, P.vout.p,
                                   P.qq, qin, qout, A.w, inner, floor, P.head.p, parts);
            else
                hipLaunchKernelGGL((k_sweep<false, kG>), dim3((unsigned)nwg), dim3(kT), 0, stream, nfree, f, rows.p, P.kout.p, P.vout.p,
                                   P.qq, qin, qout, A.w, inner, floor, P.head.p, parts);
            IRH_CHECK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_sweep_finish, dim3((unsigned)nfinish), dim3(kT), 0, stream, nfree, f, sweeps, nrowparts, rowparts.p, (int)nwg,
                       stepparts.p, plane[sweeps & 1].p, A.Q, A.q_rs, A.q_cs, P.head.p, out.p);
    IRH_CHECK(hipGetLastError());
    IRH_CHECK(hipMemcpyAsync(h, out.p, ((size_t)kHead + (size_t)sweeps) * sizeof(long long), hipMemcpyDeviceToHost, stream));
    IRH_CHECK(hipStreamSynchronize(stream));  // the one host wait (the temporaries go back to the pool idle)
    if (h[0] != 0) return IROTAVG_ERR_BAD_ARG;
    if (info) info[0] = h[1], info[1] = h[2];
    if (step) std::copy(reinterpret_cast<const double *>(h + kHead), reinterpret_cast<const double *>(h + kHead) + sweeps, step);
    return IROTAVG_OK;
}

int weiszfeld_host(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq, double *Q, int64_t ldq,
                   const double *w, int cost, int sweeps, int inner, double floor, double *step, int64_t *info) {
    hipStream_t s = nullptr;
    const size_t um = (size_t)m, un = (size_t)n_total;
    DevBuf<int32_t> dI;
    DevBuf<double> dqq, dQ, dw;
    dI.alloc(2 * um);
    dqq.alloc(4 * um);  // four planes of m
    dQ.alloc(4 * un);   // four planes of n_total; the rows from f on come back
    if (w) dw.alloc(um);
    IRH_CHECK(hipMemcpyAsync(dI.p, I, 2 * um * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (w) IRH_CHECK(hipMemcpyAsync(dw.p, w, um * sizeof(double), hipMemcpyHostToDevice, s));
    for (int c = 0; c < 4; c++) {
        IRH_CHECK(hipMemcpyAsync(dqq.p + c * um, QQ + c * ldqq, um * sizeof(double), hipMemcpyHostToDevice, s));
        IRH_CHECK(hipMemcpyAsync(dQ.p + c * un, Q + c * ldq, un * sizeof(double), hipMemcpyHostToDevice, s));
    }
    const SweepArrays D{dI.p, dqq.p, 1, (long long)m, dQ.p, 1, (long long)n_total, w ? dw.p : nullptr};
    const int rc = weiszfeld_dev(m, n_total, f, D, cost, sweeps, inner, floor, step, info, s);
    if (rc != IROTAVG_OK) return rc;
    if (sweeps > 0 && (size_t)f < un) {
        for (int c = 0; c < 4; c++)
            IRH_CHECK(hipMemcpyAsync(Q + c * ldq + f, dQ.p + c * un + f, (un - (size_t)f) * sizeof(double), hipMemcpyDeviceToHost, s));
        IRH_CHECK(hipStreamSynchronize(s));
    }
    return IROTAVG_OK;
}

}  // namespace irh
