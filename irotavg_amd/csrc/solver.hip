// solver.hip -- kernels and drivers of the IRLS path:
//   K1 edge_residual      delta_rel + log_map            (ral/l1_irls.cpp:109-127, 498-532)
//   K2 update_weights     E = A X - w, robust weights    (ral/l1_irls.cpp:614-727)
//   K3 assemble           weighted Laplacian A'D^2A + rhs (what SPQR factorises, :596-612)
//   K4 spmv / V-cycle     PCG with an aggregation-multigrid preconditioner replacing
//                         SuiteSparseQR (:550) and UMFPACK (:147-169)
//   K6 apply_step         score, exp_map, Q update       (ral/l1_irls.cpp:729-737, 471-492)
#include <cstring>

#include "graph.hpp"
#include "kernels.hpp"
#include "asm0w.hpp"

namespace irh {

// (K1's edge_log, K2's robust_weight and K6's step_quat / step_apply: kernels.hpp, shared with window.hip)

// =============================================================================================
// K1 -- edge residual. Two edges per thread so every SoA stream moves as 16 B per lane.
// Algorithmic traffic: 8 B indices + 32 B QQ + 24 B out per edge, 32 B per view.
// =============================================================================================
__global__ __launch_bounds__(256) void k_edge_residual(long long mpad, const int *__restrict__ ei,
                                                       const int *__restrict__ ej,
                                                       const double *__restrict__ qq,
                                                       const double4 *__restrict__ Q,
                                                       double *__restrict__ er, double *__restrict__ ones) {
    const long long k = 2ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= mpad) return;
    // (irls' first pass: weights.setOnes(), ral/l1_irls.cpp:577, on the way -- a fill kernel of its own until round 4)
    if (ones) *reinterpret_cast<double2 *>(ones + k) = make_double2(1.0, 1.0);
    const int2 ii = *reinterpret_cast<const int2 *>(ei + k);
    const int2 jj = *reinterpret_cast<const int2 *>(ej + k);
    const double2 qx = *reinterpret_cast<const double2 *>(qq + k);
    const double2 qy = *reinterpret_cast<const double2 *>(qq + mpad + k);
    const double2 qz = *reinterpret_cast<const double2 *>(qq + 2 * mpad + k);
    const double2 qw = *reinterpret_cast<const double2 *>(qq + 3 * mpad + k);
    const double4 qi0 = Q[ii.x], qj0 = Q[jj.x], qi1 = Q[ii.y], qj1 = Q[jj.y];
    double2 rx, ry, rz;
    edge_log(qi0, qj0, make_double4(qx.x, qy.x, qz.x, qw.x), rx.x, ry.x, rz.x);
    edge_log(qi1, qj1, make_double4(qx.y, qy.y, qz.y, qw.y), rx.y, ry.y, rz.y);
    *reinterpret_cast<double2 *>(er + k) = rx;
    *reinterpret_cast<double2 *>(er + mpad + k) = ry;
    *reinterpret_cast<double2 *>(er + 2 * mpad + k) = rz;
}

void launch_edge_residual(Graph &g, bool weights_to_one) {
    const long long threads = g.mpad / 2;
    const int grid = (int)((threads + 255) / 256);
    hipLaunchKernelGGL(k_edge_residual, dim3(grid), dim3(256), 0, g.stream, (long long)g.mpad,
                       g.ei.p, g.ej.p, g.qq.p, g.Q.p, g.er.p, weights_to_one ? g.dw.p : (double *)nullptr);
}

// =============================================================================================
// K2 -- residual of the linearised system and robust weight update (two edges per thread).
// =============================================================================================
// Two edges per thread, as K1: index pairs, residual planes and weights move as 8 / 16 B per lane. What the kernel does
// NOT read: the per-edge flag byte (edge_flags, common.hpp, is evaluated on the endpoints and f the thread holds anyway)
// and, unless the cost keeps previous values (L2, Huber: PREV), the old weight. Algorithmic traffic: 8 B indices + 24 B
// residual + 8 B weight per edge.
__device__ __forceinline__ double step_residual2(int i, int j, int f, double r0, double r1, double r2,
                                                 const double4 *__restrict__ X) {
    double e0 = 0.0, e1 = 0.0, e2c = 0.0;
    const uint8_t fl = edge_flags(i, j, f);
    if (fl & EF_CJ) {
        const double4 xj = X[j - f];
        e0 += xj.x;
        e1 += xj.y;
        e2c += xj.z;
    }
    if (fl & EF_CI) {
        const double4 xi = X[i - f];
        e0 -= xi.x;
        e1 -= xi.y;
        e2c -= xi.z;
    }
    e0 -= r0;
    e1 -= r1;
    e2c -= r2;
    return e0 * e0 + e1 * e1 + e2c * e2c;
}

template <bool PREV, int EPT>
__global__ __launch_bounds__(256) void k_update_weights(long long m, long long mpad, int f,
                                                        const int *__restrict__ ei,
                                                        const int *__restrict__ ej,
                                                        const double *__restrict__ er,
                                                        const double4 *__restrict__ X, int cost,
                                                        double sigma, double *__restrict__ dw,
                                                        const int *__restrict__ gate,
                                                        const int *__restrict__ skip) {
    // gate: launched speculatively behind a PCG whose convergence the host has not read yet -- runs
    // only if that solve is done (run_irls reads the flag and the score in ONE round trip afterwards)
    if (gate != nullptr && gate[FL_DONE] != 1) return;
    // skip: the direct solver's single-launch upper reduction gave up on a wait and poisoned the step (bcr.hip,
    // bcr_fail_word) -- the weights stay what they are, the host repeats the solve (as k_weights_then_residual does)
    if (skip != nullptr && *skip != 0) return;
    // EPT edges per thread in EPT / 2 pairs; a wave's pairs of one load lie next to each other (16 B per lane)
    const long long base = (long long)blockIdx.x * (256 * EPT) + 2 * threadIdx.x;
    int2 ii[EPT / 2], jj[EPT / 2];
    double2 r0[EPT / 2], r1[EPT / 2], r2[EPT / 2], prev[EPT / 2];
#pragma unroll
    for (int u = 0; u < EPT / 2; u++) {
        const long long k = base + 512 * u;
        ii[u] = jj[u] = make_int2(0, 0);
        r0[u] = r1[u] = r2[u] = prev[u] = make_double2(0.0, 0.0);
        if (k < m) {
            ii[u] = *reinterpret_cast<const int2 *>(ei + k);
            jj[u] = *reinterpret_cast<const int2 *>(ej + k);
            r0[u] = *reinterpret_cast<const double2 *>(er + k);
            r1[u] = *reinterpret_cast<const double2 *>(er + mpad + k);
            r2[u] = *reinterpret_cast<const double2 *>(er + 2 * mpad + k);
            if (PREV) prev[u] = *reinterpret_cast<const double2 *>(dw + k);
        }
    }
#pragma unroll
    for (int u = 0; u < EPT / 2; u++) {
        const long long k = base + 512 * u;
        if (k >= m) continue;
        const double ea = step_residual2(ii[u].x, jj[u].x, f, r0[u].x, r1[u].x, r2[u].x, X);
        const double wa = robust_weight(cost, sigma, ea, prev[u].x);
        if (k + 1 < m) {
            const double eb = step_residual2(ii[u].y, jj[u].y, f, r0[u].y, r1[u].y, r2[u].y, X);
            *reinterpret_cast<double2 *>(dw + k) = make_double2(wa, robust_weight(cost, sigma, eb, prev[u].y));
        } else {
            dw[k] = wa;  // the pad entry behind an odd m keeps its value
        }
    }
}

void launch_update_weights(Graph &g, int cost, double sigma, bool gated) {
    // (four and eight edges per thread were measured: 17.6 -> 18.3 / 18.9 us at 2M edges; two it is)
    const int *gate = gated ? (const int *)g.flags.p : (const int *)nullptr;
    const int *skip = g.bcr_B ? bcr_fail_word(g) : nullptr;
    const int grid = (int)((g.m + 511) / 512);
    if (cost == IROTAVG_L2 || cost == IROTAVG_HUBER)
        hipLaunchKernelGGL((k_update_weights<true, 2>), dim3(grid), dim3(256), 0, g.stream, (long long)g.m, (long long)g.mpad, g.f,
                           g.ei.p, g.ej.p, g.er.p, g.X.p, cost, sigma, g.dw.p, gate, skip);
    else
        hipLaunchKernelGGL((k_update_weights<false, 2>), dim3(grid), dim3(256), 0, g.stream, (long long)g.m, (long long)g.mpad, g.f,
                           g.ei.p, g.ej.p, g.er.p, g.X.p, cost, sigma, g.dw.p, gate, skip);
}

// K1 and K2 at a ZERO step in one pass over the edges (irotavg_graph_pose_weights; the view-graph's uncertainty queries):
// the residuals of the current rotations into the planes, and the cost's weight of |0 - r_k|^2 into dw. No step vector is
// read. Two edges per thread, 16 B per lane and stream, as K1. Algorithmic traffic: 8 B indices + 32 B relative rotation
// in, 24 B residual + 8 B weight out per edge (+ 8 B old weight for the costs that keep previous values), 32 B per view.
template <bool PREV>
__global__ __launch_bounds__(256) void k_pose_weights(long long m, long long mpad, const int *__restrict__ ei,
                                                      const int *__restrict__ ej, const double *__restrict__ qq,
                                                      const double4 *__restrict__ Q, double *__restrict__ er, int cost,
                                                      double sigma, double *__restrict__ dw) {
    const long long k = 2ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= mpad) return;
    const int2 ii = *reinterpret_cast<const int2 *>(ei + k);
    const int2 jj = *reinterpret_cast<const int2 *>(ej + k);
    const double2 qx = *reinterpret_cast<const double2 *>(qq + k);
    const double2 qy = *reinterpret_cast<const double2 *>(qq + mpad + k);
    const double2 qz = *reinterpret_cast<const double2 *>(qq + 2 * mpad + k);
    const double2 qw = *reinterpret_cast<const double2 *>(qq + 3 * mpad + k);
    const double4 qi0 = Q[ii.x], qj0 = Q[jj.x], qi1 = Q[ii.y], qj1 = Q[jj.y];
    double2 prev = make_double2(0.0, 0.0);
    if (PREV && k < m) prev = *reinterpret_cast<const double2 *>(dw + k);
    double2 rx, ry, rz;
    edge_log(qi0, qj0, make_double4(qx.x, qy.x, qz.x, qw.x), rx.x, ry.x, rz.x);
    edge_log(qi1, qj1, make_double4(qx.y, qy.y, qz.y, qw.y), rx.y, ry.y, rz.y);
    *reinterpret_cast<double2 *>(er + k) = rx;
    *reinterpret_cast<double2 *>(er + mpad + k) = ry;
    *reinterpret_cast<double2 *>(er + 2 * mpad + k) = rz;
    if (k >= m) return;
    // step_residual2 with X = 0: e = -r
    const double wa = robust_weight(cost, sigma, rx.x * rx.x + ry.x * ry.x + rz.x * rz.x, prev.x);
    if (k + 1 < m)
        *reinterpret_cast<double2 *>(dw + k) =
            make_double2(wa, robust_weight(cost, sigma, rx.y * rx.y + ry.y * ry.y + rz.y * rz.y, prev.y));
    else
        dw[k] = wa;  // the pad entry behind an odd m keeps its value
}

void launch_pose_weights(Graph &g, int cost, double sigma) {
    const int grid = (int)((g.mpad / 2 + 255) / 256);
    if (cost == IROTAVG_L2 || cost == IROTAVG_HUBER)
        hipLaunchKernelGGL((k_pose_weights<true>), dim3(grid), dim3(256), 0, g.stream, (long long)g.m, (long long)g.mpad,
                           g.ei.p, g.ej.p, g.qq.p, g.Q.p, g.er.p, cost, sigma, g.dw.p);
    else
        hipLaunchKernelGGL((k_pose_weights<false>), dim3(grid), dim3(256), 0, g.stream, (long long)g.m, (long long)g.mpad,
                           g.ei.p, g.ej.p, g.qq.p, g.Q.p, g.er.p, cost, sigma, g.dw.p);
}

// |r| of measurements that are not edges of the handle (the closure gate's candidates): per measurement the quaternions
// of its first view, its second view and its relative rotation
__global__ __launch_bounds__(256) void k_candidate_angles(long long n, const double4 *__restrict__ q3,
                                                          double *__restrict__ angle) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double rx, ry, rz;
    edge_log(q3[3 * t], q3[3 * t + 1], q3[3 * t + 2], rx, ry, rz);
    angle[t] = sqrt(rx * rx + ry * ry + rz * rz);
}

void candidate_angles(Graph &g, int64_t n, const double *q12, double *angle) {
    if (n <= 0) return;
    DevBuf<double4> dq;
    DevBuf<double> da;
    dq.upload(reinterpret_cast<const double4 *>(q12), (size_t)3 * n, g.stream);
    da.alloc((size_t)n);
    hipLaunchKernelGGL(k_candidate_angles, dim3((int)((n + 255) / 256)), dim3(256), 0, g.stream, (long long)n, dq.p, da.p);
    IRH_CHECK(hipMemcpyAsync(angle, da.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
}

// K2 and the NEXT iteration's K1 in one pass over the edges (round 4; the direct solver's irls loop, run_irls): the
// weights from the old residuals and the step -- exactly k_update_weights -- and then the residuals of the rotations the
// step has just produced (k_apply_step runs in front of this kernel; it reads X, not the weights). The index pairs are
// read once instead of twice, one launch less per iteration, and the host reads the score of the step while this runs.
// Algorithmic traffic: 8 B indices + 24 B old residual + 8 B weight + 32 B relative rotation + 24 B new residual per edge.
template <bool PREV>
__global__ __launch_bounds__(256) void k_weights_then_residual(long long m, long long mpad, int f,
                                                               const int *__restrict__ ei, const int *__restrict__ ej,
                                                               double *__restrict__ er, const double4 *__restrict__ X,
                                                               int cost, double sigma, double *__restrict__ dw,
                                                               const double *__restrict__ qq,
                                                               const double4 *__restrict__ Q,
                                                               const double *__restrict__ pub_src,
                                                               double *__restrict__ pub_dst, int pub_n,
                                                               int *__restrict__ seqp, int seq, int with_residual,
                                                               const int *__restrict__ skip) {
    // the first workgroup hands the score's partial sums (left by the kernel in front of this one) to the host before it
    // turns to its edges -- what the one-workgroup k_publish did in a launch of its own (5 us per iteration)
    if (pub_n > 0 && blockIdx.x == 0) {
        for (int i = threadIdx.x; i < pub_n; i += 256) pub_dst[i] = pub_src[i];
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(seqp, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // (skip: the solve in front of this kernel gave up -- bcr_up_failed, its solution is NaN: weights and residuals
    // stay as they are, the host repeats the solve)
    if (skip && *skip != 0) return;
    const long long k = 2ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= mpad) return;
    const int2 ii = *reinterpret_cast<const int2 *>(ei + k);
    const int2 jj = *reinterpret_cast<const int2 *>(ej + k);
    const double2 r0 = *reinterpret_cast<const double2 *>(er + k);
    const double2 r1 = *reinterpret_cast<const double2 *>(er + mpad + k);
    const double2 r2 = *reinterpret_cast<const double2 *>(er + 2 * mpad + k);
    // with_residual == 0: the weights only (run_irls expects this iteration to be the last: the residual half would be
    // thrown away)
    double2 qx = make_double2(0.0, 0.0), qy = qx, qz = qx, qw = qx;
    double4 qi0 = make_double4(0, 0, 0, 1), qj0 = qi0, qi1 = qi0, qj1 = qi0;
    if (with_residual) {
        qx = *reinterpret_cast<const double2 *>(qq + k);
        qy = *reinterpret_cast<const double2 *>(qq + mpad + k);
        qz = *reinterpret_cast<const double2 *>(qq + 2 * mpad + k);
        qw = *reinterpret_cast<const double2 *>(qq + 3 * mpad + k);
        qi0 = Q[ii.x];
        qj0 = Q[jj.x];
        qi1 = Q[ii.y];
        qj1 = Q[jj.y];
    }
    double2 prev = make_double2(0.0, 0.0);
    if (PREV && k < m) prev = *reinterpret_cast<const double2 *>(dw + k);
    if (k < m) {
        const double ea = step_residual2(ii.x, jj.x, f, r0.x, r1.x, r2.x, X);
        const double wa = robust_weight(cost, sigma, ea, prev.x);
        if (k + 1 < m) {
            const double eb = step_residual2(ii.y, jj.y, f, r0.y, r1.y, r2.y, X);
            *reinterpret_cast<double2 *>(dw + k) = make_double2(wa, robust_weight(cost, sigma, eb, prev.y));
        } else {
            dw[k] = wa;  // the pad entry behind an odd m keeps its value
        }
    }
    if (!with_residual) return;
    double2 rx, ry, rz;
    edge_log(qi0, qj0, make_double4(qx.x, qy.x, qz.x, qw.x), rx.x, ry.x, rz.x);
    edge_log(qi1, qj1, make_double4(qx.y, qy.y, qz.y, qw.y), rx.y, ry.y, rz.y);
    *reinterpret_cast<double2 *>(er + k) = rx;
    *reinterpret_cast<double2 *>(er + mpad + k) = ry;
    *reinterpret_cast<double2 *>(er + 2 * mpad + k) = rz;
}

// pub (n > 0): the kernel's first workgroup publishes that part first (publish_begin has been called)
void launch_weights_then_residual(Graph &g, int cost, double sigma, const PubPart *pub, bool with_residual,
                                  const int *skip_word = nullptr) {
    const long long threads = g.mpad / 2;
    const int grid = (int)((threads + 255) / 256);
    const double *ps = pub ? pub->src : nullptr;
    double *pd = pub ? pub->dst : nullptr;
    const int pn = pub ? pub->n : 0;
    // (skip_word: the closures' gate, bcr_gate_skip_word -- such solves never go through the single-launch upper reduction)
    const int *skip = skip_word ? skip_word : (g.bcr_B ? bcr_fail_word(g) : nullptr);
    if (cost == IROTAVG_L2 || cost == IROTAVG_HUBER)
        hipLaunchKernelGGL((k_weights_then_residual<true>), dim3(grid), dim3(256), 0, g.stream, (long long)g.m,
                           (long long)g.mpad, g.f, g.ei.p, g.ej.p, g.er.p, g.X.p, cost, sigma, g.dw.p, g.qq.p, g.Q.p, ps, pd,
                           pn, g.h_seq(), g.pub_seq, with_residual ? 1 : 0, skip);
    else
        hipLaunchKernelGGL((k_weights_then_residual<false>), dim3(grid), dim3(256), 0, g.stream, (long long)g.m,
                           (long long)g.mpad, g.f, g.ei.p, g.ej.p, g.er.p, g.X.p, cost, sigma, g.dw.p, g.qq.p, g.Q.p, ps, pd,
                           pn, g.h_seq(), g.pub_seq, with_residual ? 1 : 0, skip);
}

// =============================================================================================
// K3 -- level-0 assembly. The lane that owns a free view walks the view's incident-edge entries
// (SELL layout, wave-uniform trip count): off-diagonal value -w, diagonal sum, Dirichlet excess
// and (IRLS) the right-hand side b_v = sum_k +-w_k r_k. MODE 0: w = d_k^2 from the IRLS weights,
// rhs built. MODE 1: w = s[k] (sigx of the primal-dual step), no rhs, make_AtA boundary rule.
// =============================================================================================
// Edge-parallel producer of the assembly's operands: T[e] = (w r_x, w r_y, w r_z, w), w = d_e^2, as
// ONE 32-byte record per edge, so that the view-parallel assembly issues one gather per entry
// instead of four (weights + three residual planes): PMC showed 5x the algorithmic traffic before.
__global__ __launch_bounds__(256) void k_edge_pack(long long m, long long mpad,
                                                   const double *__restrict__ d,
                                                   const double *__restrict__ er,
                                                   double4 *__restrict__ T) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const double w = d[k] * d[k];
    T[k] = make_double4(w * er[k], w * er[mpad + k], w * er[2 * mpad + k], w);
}

template <int MODE>
__global__ __launch_bounds__(kRowBlock) void k_assemble0(
    int n, int nsl, const int *__restrict__ sl_off, const uint32_t *__restrict__ slot_eid,
    const int *__restrict__ bptr, const uint32_t *__restrict__ beid,
    const uint8_t *__restrict__ bflag, const double *__restrict__ wsrc,
    const double4 *__restrict__ T, double *__restrict__ val,
    double *__restrict__ excess, double *__restrict__ diag, double *__restrict__ idg,
    double4 *__restrict__ rhs, double *__restrict__ bval) {
    const int ntiles = (nsl + 3) / 4;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    for (int t = t0; t < t1; t++) {
        const int sl = t * 4 + (threadIdx.x >> 6);
        if (sl >= nsl) break;
        const int lane = threadIdx.x & 63, row = sl * 64 + lane;
        const int o0 = sl_off[sl], w = sl_off[sl + 1] - o0;
        const uint2 *__restrict__ se_p = reinterpret_cast<const uint2 *>(slot_eid) + (size_t)(o0 / 2) * 64 + lane;
        double2 *__restrict__ v_p = reinterpret_cast<double2 *>(val) + (size_t)(o0 / 2) * 64 + lane;
        double sw = 0.0, ex = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        constexpr int U = kSellUnroll;
        for (int k0 = 0; k0 < w; k0 += U) {  // w is a multiple of U: whole batches, loads first
            uint32_t se[U];
            double4 tt[U];
#pragma unroll
            for (int u = 0; u < U / 2; u++) {
                const uint2 pr = se_p[(size_t)(k0 / 2 + u) * 64];
                se[2 * u] = pr.x;
                se[2 * u + 1] = pr.y;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const bool live = se[u] != 0xffffffffu;
                const uint32_t e = live ? (se[u] >> 1) : 0u;
                if (MODE == 0)
                    tt[u] = T[e];
                else
                    tt[u].w = wsrc[e];
                if (!live) tt[u] = make_double4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double ww = tt[u].w;
                if (MODE == 0) {
                    const double sg = (se[u] & 1u) ? 1.0 : -1.0;
                    b0 += sg * tt[u].x;
                    b1 += sg * tt[u].y;
                    b2 += sg * tt[u].z;
                }
                sw += ww;
            }
#pragma unroll
            for (int u = 0; u < U / 2; u++)
                v_p[(size_t)(k0 / 2 + u) * 64] = make_double2(-tt[2 * u].w, -tt[2 * u + 1].w);
        }
        if (row < n) {
            for (int s = bptr[row]; s < bptr[row + 1]; s++) {
                const uint8_t fl = bflag[s];
                if (!(fl & (MODE == 0 ? BF_IRLS : BF_L1H))) {
                    bval[s] = 0.0;
                    continue;
                }
                const uint32_t se = beid[s];
                const uint32_t e = se >> 1;
                double wk;
                if (MODE == 0) {
                    const double4 t = T[e];
                    wk = t.w;
                    const double sg = (se & 1u) ? 1.0 : -1.0;
                    b0 += sg * t.x;
                    b1 += sg * t.y;
                    b2 += sg * t.z;
                } else {
                    wk = wsrc[e];
                    if (fl & BF_NEG) wk = -wk;
                }
                bval[s] = wk;
                ex += wk;
            }
            const double d = sw + ex;
            excess[row] = ex;
            diag[row] = d;
            idg[row] = d > 0.0 ? 1.0 / d : 0.0;
            if (MODE == 0) rhs[row] = make_double4(b0, b1, b2, 0.0);
        }
    }
}

// K3, windowed form: ONE launch replaces k_edge_pack + k_assemble0 + (band graphs) the level-1 value and
// diagonal kernels. A workgroup owns one 64-row slice. The edges its rows touch are, on a view sequence,
// ONE contiguous run of the edge list (edges are stored by their later view: rows [r, r + 64) with
// w predecessors each touch the edges of views [r, r + 64 + w)), so the workgroup stages that run --
// w_e = d_e^2 and w_e r_e, 40 B per edge read once, coalesced -- in LDS and the row walk gathers from
// LDS instead of from a 64 MB record array written by a kernel of its own (PMC before: 3.2 x the
// algorithmic traffic over the three launches). The window start comes from the build (lowest edge id
// among the slice's near entries); an entry whose edge lies outside the window (loop closures) is
// gathered from global memory, so any graph is handled. The four waves split the slice's entry pairs;
// their partial row sums are combined in wave order (deterministic).
// L1 = true: level 0 aggregates by 8 and every level-1 row has at most 8 entries (band graphs): the
// 8 x 8 level-1 values under the slice are accumulated on the way (each (wave, row) owns its LDS
// accumulators: no atomics) and the level-1 diagonal is formed here, too.
// MODE 2 (round 4): MODE 1 -- the primal-dual Hessian from wsrc = sigx under make_AtA's boundary rule -- AND the
// right-hand side of its system in the same walk over the slice's entries: rhs_v = (A' t)_v with make_A's coefficients,
// t = the plane `er` points to (k_pd_rhs's walk of the same slots, a launch and 16 MB of slot ids per solve, until then).
template <int MODE, bool L1>
__global__ __launch_bounds__(kRowBlock) void k_assemble0w(
    int n, int nsl, long long m, long long mpad, const int *__restrict__ sl_off,
    const uint32_t *__restrict__ slot_eid, const uint8_t *__restrict__ slot_cs,
    const int *__restrict__ tile_e0, const int *__restrict__ bptr, const uint32_t *__restrict__ beid,
    const uint8_t *__restrict__ bflag, const double *__restrict__ wsrc, const double *__restrict__ er,
    double *__restrict__ val, double *__restrict__ excess, double *__restrict__ diag,
    double *__restrict__ idg, double4 *__restrict__ rhs, double *__restrict__ bval, int n1,
    const int *__restrict__ sl_off1, double *__restrict__ val1, double *__restrict__ excess1,
    double *__restrict__ diag1, double *__restrict__ idg1) {
    __shared__ double lds[Asm0wLds<MODE, L1>::doubles];
    const int nb = gridDim.x, b = blockIdx.x;  // nb is a multiple of 8: neighbouring slices share an XCD (L2)
    const int sl = (b & 7) * (nb >> 3) + (b >> 3);
    if (sl >= nsl) return;
    // (the slice's work: asm0w.hpp -- the level-0 reduction of the direct solver runs the same body for its own slices)
    asm0w_slice<MODE, L1, kRowBlock>(sl, lds, n, m, mpad, sl_off, slot_eid, slot_cs, tile_e0, bptr, beid, bflag, wsrc, er, val,
                                     excess, diag, idg, rhs, bval, n1, sl_off1, val1, excess1, diag1, idg1);
}

// value + diagonal refresh of a coarse level with SHORT rows (band graphs below level 1) in one launch:
// 8 lanes per coarse row walk its entries in CSR order (each entry = sum of the finer SELL positions
// listed for it), then form the diagonal from the aggregate's excess and the row sum.
__global__ __launch_bounds__(kRowBlock) void k_coarse_level(LevelView C, const int *__restrict__ crow,
                                                            const int *__restrict__ cptr,
                                                            const int *__restrict__ cidx,
                                                            const int *__restrict__ cpos,
                                                            const double *__restrict__ fval, double *__restrict__ cval,
                                                            int nf, int agg, const double *__restrict__ fexcess,
                                                            double *__restrict__ cexcess, double *__restrict__ cdiag,
                                                            double *__restrict__ cidg, const double *__restrict__ refv,
                                                            const double *__restrict__ refd, double spread,
                                                            unsigned long long *__restrict__ mm,
                                                            double *__restrict__ scal, int *__restrict__ flags) {
    const int I = (blockIdx.x * blockDim.x + threadIdx.x) >> 3, l = threadIdx.x & 7;
    const bool live = I < C.n;
    // refv != nullptr: this is the dense level and the caller wants the staleness verdict on its inverse (what
    // k_stale_check computes in a launch of its own): ratios new / reference of every entry and diagonal
    double lo = HUGE_VAL, hi = 0.0;
    auto visit = [&](double v, double r) {
        if (r != 0.0 && v != 0.0) {
            const double q = v / r;
            if (q > 0.0) {
                lo = fmin(lo, q);
                hi = fmax(hi, q);
            } else {
                hi = HUGE_VAL;
            }
        } else if ((r != 0.0) != (v != 0.0)) {
            hi = HUGE_VAL;  // an entry appeared or vanished
        }
    };
    double sv = 0.0;
    if (live) {
        for (int c = crow[I]; c < crow[I + 1]; c++) {
            double s = 0.0;
            for (int q = cptr[c] + l; q < cptr[c + 1]; q += 8) s += fval[cidx[q]];
            s = seg_sum(s, 8);
            if (l == 0) {
                cval[cpos[c]] = s;
                if (refv != nullptr) visit(s, refv[cpos[c]]);
            }
            sv += s;
        }
    }
    double ex = 0.0;
    if (live)
        for (int q = I * agg + l; q < min(nf, (I + 1) * agg); q += 8) ex += fexcess[q];
    ex = seg_sum(ex, 8);
    if (live && l == 0) {
        const double d = ex - sv;
        cexcess[I] = ex;
        cdiag[I] = d;
        cidg[I] = d > 0.0 ? 1.0 / d : 0.0;
        if (refv != nullptr) visit(d, refd[I]);
    }
    if (refv == nullptr) return;
    // min / max over the grid: workgroup reduction, then atomics on the bit patterns (non-negative doubles order
    // like their bits; min and max do not depend on the order of arrival); the last workgroup writes the verdict
    __shared__ double smin[kRowBlock / 64], smax[kRowBlock / 64];
    __shared__ int last;
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_down(lo, o, 64));
        hi = fmax(hi, __shfl_down(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = lo;
        smax[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRowBlock / 64; w++) {
            lo = fmin(lo, smin[w]);
            hi = fmax(hi, smax[w]);
        }
        atomicMin(mm, (unsigned long long)__double_as_longlong(lo));
        atomicMax(mm + 1, (unsigned long long)__double_as_longlong(hi));
        __threadfence();
        last = atomicAdd(mm + 2, 1ull) == (unsigned long long)gridDim.x - 1 ? 1 : 0;
        if (last) {
            __threadfence();
            const double glo = __longlong_as_double((long long)atomicAdd(mm, 0ull));
            const double ghi = __longlong_as_double((long long)atomicAdd(mm + 1, 0ull));
            // (same statements as k_stale_check) the scale follows the operator even when the verdict is 'stale'
            if (glo > 0.0 && ghi < HUGE_VAL) scal[SC_DSCALE] = 1.0 / sqrt(glo * ghi);
            flags[FL_STALE] = (glo > 0.0 && ghi < HUGE_VAL && ghi <= spread * glo) ? 0 : 1;
            mm[0] = (unsigned long long)__double_as_longlong(HUGE_VAL);  // ready for the next check
            mm[1] = 0ull;
            mm[2] = 0ull;
        }
    }
}

// coarse off-diagonal values: entry c (CSR order) = sum of the finer SELL positions listed for
// it, stored at its own SELL position. 8 lanes per entry.
__global__ __launch_bounds__(kRowBlock) void k_coarse_vals(int nent, const int *__restrict__ cptr,
                                                           const int *__restrict__ cidx,
                                                           const int *__restrict__ cpos,
                                                           const double *__restrict__ fval,
                                                           double *__restrict__ cval) {
    constexpr int G = 8, R = kRowBlock / G;
    const int grp = threadIdx.x / G, l = threadIdx.x % G;
    const int ntiles = (nent + R - 1) / R;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    for (int t = t0; t < t1; t++) {
        const int c = t * R + grp;
        double s = 0.0;
        if (c < nent) {
            const int beg = cptr[c], end = cptr[c + 1];
            for (int q = beg + l; q < end; q += G) s += fval[cidx[q]];
        }
        s = seg_sum(s, G);
        if (l == 0 && c < nent) cval[cpos[c]] = s;
    }
}

// coarse diagonal: excess_c = sum of the aggregate's excess, diag_c = excess_c - sum(row values). Eight lanes
// per coarse row (a row of a loop-closure graph's level 1 is ~30-50 entry-columns wide: one lane per row walked
// them in sequence, 12 us per level)
__global__ __launch_bounds__(kRowBlock) void k_coarse_diag(LevelView C, int nf, int agg,
                                                           const double *__restrict__ fexcess,
                                                           double *__restrict__ cexcess,
                                                           double *__restrict__ cdiag,
                                                           double *__restrict__ cidg) {
    const int I = (blockIdx.x * blockDim.x + threadIdx.x) >> 3, l = threadIdx.x & 7;
    const bool live = I < C.n;
    double sv = 0.0, ex = 0.0;
    if (live) {
        const int sl = I >> 6, lane = I & 63;
        const int o0 = C.sl_off[sl], w = C.sl_off[sl + 1] - o0;
        for (int k = l; k < w; k += 8) sv += C.val[sell_pos(o0, k, lane)];
        const int v0 = I * agg, v1 = min(nf, v0 + agg);
        for (int q = v0 + l; q < v1; q += 8) ex += fexcess[q];
    }
    sv = seg_sum(sv, 8);
    ex = seg_sum(ex, 8);
    if (live && l == 0) {
        const double d = ex - sv;
        cexcess[I] = ex;
        cdiag[I] = d;
        cidg[I] = d > 0.0 ? 1.0 / d : 0.0;
    }
}

// =============================================================================================
// K4 -- row kernels on a level (one lane per row, SELL-64)
// =============================================================================================
#define ROW_TILE_LOOP(L)                                       \
    const int ntiles_ = ((L).nsl + 3) / 4;                     \
    int t0_, t1_;                                              \
    tile_range(ntiles_, t0_, t1_);                             \
    for (int t_ = t0_; t_ < t1_; t_++)                         \
        if (const int sl_ = t_ * 4 + (threadIdx.x >> 6); sl_ < (L).nsl)

// q = L p, partial dot products p.q -- the dominant kernel of the PCG.
// The 256-row tile's window of p (rows [tile - 64, tile + 320)) is copied into LDS once (12 KB,
// coalesced); the near part of every row (all of it on a band graph) then reads p from LDS, so
// the loop is a pure 16 B/lane matrix stream without dependent global gathers. Only the far
// entries (loop closures) gather from global memory, through the pipelined loop of row_offdiag_t.
// (sharded runs: `pg` holds the halo-exchanged directions of the ghost views; boundary slots with
// a ghost endpoint contribute -w * p_ghost; pg == nullptr on a single GPU)
__global__ __launch_bounds__(kRowBlock) void k_spmv_dot(LevelView L, const double4 *__restrict__ p,
                                                        double4 *__restrict__ q,
                                                        double *__restrict__ part_pq,
                                                        const int *__restrict__ flags,
                                                        const double4 *__restrict__ pg,
                                                        const int *__restrict__ bptr,
                                                        const int *__restrict__ bghost,
                                                        const double *__restrict__ bval) {
    // every independent load of the prologue is issued before the first dependent use (the done
    // flag included): a serial chain of ~1-2 us memory round trips is what this kernel is made of
    const int done = flags[FL_DONE];
    __shared__ double wx[kWinLen], wy[kWinLen], wz[kWinLen];
    double a0 = 0, a1 = 0, a2 = 0;
    const int ntiles = (L.nsl + 3) / 4;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    const int lane = threadIdx.x & 63;
    for (int t = t0; t < t1; t++) {
        const int r0 = t * 256;
        const int wlo = max(0, r0 - kWinHalo), whi = min(L.n, r0 + 256 + kWinHalo);
        const int sl = min(t * 4 + (int)(threadIdx.x >> 6), L.nsl - 1);
        const bool live = t * 4 + (int)(threadIdx.x >> 6) < L.nsl;
        const int row = sl * 64 + lane;
        const int o0 = L.sl_off[sl], wn = L.sl_near[sl];
        const double4 pr = p[min(row, L.n - 1)];
        const double d = L.diag[row];
        NearBatch nb;
        near_prefetch(L, o0, live ? wn : 0, lane, nb);
        double4 wv0 = make_double4(0, 0, 0, 0), wv1 = wv0;
        const int i0w = threadIdx.x, i1w = threadIdx.x + kRowBlock;
        if (i0w < whi - wlo) wv0 = p[wlo + i0w];
        if (i1w < whi - wlo) wv1 = p[wlo + i1w];
        if (done) return;  // uniform across the grid
        __syncthreads();   // the previous tile's readers are done with the window
        if (i0w < kWinLen) {
            wx[i0w] = wv0.x;
            wy[i0w] = wv0.y;
            wz[i0w] = wv0.z;
        }
        if (i1w < kWinLen) {
            wx[i1w] = wv1.x;
            wy[i1w] = wv1.y;
            wz[i1w] = wv1.z;
        }
        __syncthreads();
        if (live) {
            double s0, s1, s2;
            near_window_row(L, o0, wn, lane, wlo, wx, wy, wz, nb, s0, s1, s2);
            double f0, f1, f2;
            row_offdiag_t<false>(L, row, p, nullptr, 0, 0.0, f0, f1, f2, wn);  // far entries
            s0 += f0;
            s1 += f1;
            s2 += f2;
            if (row < L.n) {
                s0 += d * pr.x;
                s1 += d * pr.y;
                s2 += d * pr.z;
                if (pg != nullptr) {
                    for (int s = bptr[row]; s < bptr[row + 1]; s++) {
                        const int gi = bghost[s];
                        if (gi >= 0) {
                            const double w = bval[s];
                            const double4 x = pg[gi];
                            s0 -= w * x.x;
                            s1 -= w * x.y;
                            s2 -= w * x.z;
                        }
                    }
                }
                q[row] = make_double4(s0, s1, s2, 0.0);
                a0 += pr.x * s0;
                a1 += pr.y * s1;
                a2 += pr.z * s2;
            }
        }
    }
    block_sum3_store(a0, a1, a2, part_pq + 4 * blockIdx.x);
}

// The p-update fused into the SpMV (single GPU, additive top level): an empty kernel costs 4.7 us
// on this machine (dispatch + completion of a dependent launch), the p-update itself 1.6 us. The
// SpMV loads the window of p its tile needs into LDS anyway; here it FORMS those entries instead,
// p_new = omega D^-1 r + kc P y1 + beta p_old (same statements as k_pcg_pupdate_add), stores its own
// 256 rows to Pnew (ping-pong with Pold: other workgroups still read p_old of these rows for their
// halos). A far entry (loop closure) needs four gathers instead of one: FAR = true handles the
// case of a FEW of them (<= 1/32 of the entry-columns); with more, the two kernels stay separate.
template <bool FIRST, bool FAR>
__global__ __launch_bounds__(kRowBlock) void k_pspmv_dot(
    LevelView L, int sh, double *__restrict__ scal, int par, const double *__restrict__ part_rz, int np0,
    const double *__restrict__ part_rz2, int np1, const double4 *__restrict__ R,
    const double4 *__restrict__ yc, double omega, double kc, const double4 *__restrict__ Pold,
    double4 *__restrict__ Pnew, double4 *__restrict__ q, double *__restrict__ part_pq,
    int *__restrict__ flags) {
    const int done = flags[FL_DONE];
    __shared__ double wx[kWinLen], wy[kWinLen], wz[kWinLen];
    double a0 = 0, a1 = 0, a2 = 0;
    const int ntiles = (L.nsl + 3) / 4;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    const int lane = threadIdx.x & 63;
    // window inputs of the first tile: requested before beta is reduced
    double4 r_pre[2], y_pre[2], p_pre[2];
    double w_pre[2];
    auto win_load = [&](int t, double4 (&r)[2], double4 (&y)[2], double4 (&po)[2], double (&w)[2]) {
        const int r0 = t * 256;
        const int wlo = max(0, r0 - kWinHalo), whi = min(L.n, r0 + 256 + kWinHalo);
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int i = wlo + (int)threadIdx.x + u * kRowBlock;
            r[u] = y[u] = po[u] = make_double4(0, 0, 0, 0);
            w[u] = 0.0;
            if (i < whi && (int)threadIdx.x + u * kRowBlock < kWinLen) {
                r[u] = R[i];
                y[u] = yc[i >> sh];
                w[u] = L.idg[i];
                if (!FIRST) po[u] = Pold[i];
            }
        }
    };
    if (t0 < t1) win_load(t0, r_pre, y_pre, p_pre, w_pre);
    if (done) return;
    double be[3];
    {
        double ra[3], rb[3], rzn[3];
        load_reduced3(part_rz, np0, ra);
        load_reduced3(part_rz2, np1, rb);
        bool finite = true;
        for (int c = 0; c < 3; c++) {
            rzn[c] = ra[c] + kc * rb[c];
            const double rzo = scal[(par ? SC_RZ1 : SC_RZ0) + c];
            be[c] = (FIRST || !(rzo > 0.0)) ? 0.0 : rzn[c] / rzo;
            finite = finite && isfinite(rzn[c]);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            for (int c = 0; c < 3; c++) scal[(par ? SC_RZ0 : SC_RZ1) + c] = rzn[c];
            if (!finite) flags[FL_DONE] = 2;
        }
    }
    auto pnew = [&](const double4 &r, const double4 &y, const double4 &po, double wi) {
        const double w = omega * wi;
        double4 p = make_double4(w * r.x + kc * y.x, w * r.y + kc * y.y, w * r.z + kc * y.z, 0.0);
        if (!FIRST) {
            p.x += be[0] * po.x;
            p.y += be[1] * po.y;
            p.z += be[2] * po.z;
        }
        return p;
    };
    for (int t = t0; t < t1; t++) {
        const int r0 = t * 256;
        const int wlo = max(0, r0 - kWinHalo), whi = min(L.n, r0 + 256 + kWinHalo);
        const int sl = min(t * 4 + (int)(threadIdx.x >> 6), L.nsl - 1);
        const bool live = t * 4 + (int)(threadIdx.x >> 6) < L.nsl;
        const int row = sl * 64 + lane;
        const int o0 = L.sl_off[sl], wn = L.sl_near[sl];
        const double d = L.diag[row];
        NearBatch nb;
        near_prefetch(L, o0, live ? wn : 0, lane, nb);
        double4 rr[2], yy[2], pp[2];
        double ww[2];
        if (t == t0) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                rr[u] = r_pre[u];
                yy[u] = y_pre[u];
                pp[u] = p_pre[u];
                ww[u] = w_pre[u];
            }
        } else {
            win_load(t, rr, yy, pp, ww);
        }
        __syncthreads();  // the previous tile's readers are done with the window
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int iw = (int)threadIdx.x + u * kRowBlock;
            if (iw < kWinLen) {
                const int i = wlo + iw;
                double4 pv = make_double4(0, 0, 0, 0);
                if (i < whi) {
                    pv = pnew(rr[u], yy[u], pp[u], ww[u]);
                    if (i >= r0 && i < r0 + 256) Pnew[i] = pv;  // own rows of this tile
                }
                wx[iw] = pv.x;
                wy[iw] = pv.y;
                wz[iw] = pv.z;
            }
        }
        __syncthreads();
        if (live) {
            double s0, s1, s2;
            near_window_row(L, o0, wn, lane, wlo, wx, wy, wz, nb, s0, s1, s2);
            if (FAR) {
                // the few far entries (a handful of loop closures): p_new of the far column is formed
                // from its four inputs, one entry pair at a time. Only used when far entry-columns
                // are rare (pcg_solve); with many of them the separate p-update is cheaper.
                const int wtot = L.sl_off[sl + 1] - o0;
                const int2 *__restrict__ fc = reinterpret_cast<const int2 *>(L.col) + (size_t)(o0 / 2) * 64 + lane;
                const double2 *__restrict__ fv = reinterpret_cast<const double2 *>(L.val) + (size_t)(o0 / 2) * 64 + lane;
                for (int k0 = wn; k0 < wtot; k0 += 2) {
                    const int2 cp = fc[(size_t)(k0 / 2) * 64];
                    const double2 vp = fv[(size_t)(k0 / 2) * 64];
                    const double4 pa = pnew(R[cp.x], yc[cp.x >> sh], FIRST ? R[cp.x] : Pold[cp.x], L.idg[cp.x]);
                    const double4 pb = pnew(R[cp.y], yc[cp.y >> sh], FIRST ? R[cp.y] : Pold[cp.y], L.idg[cp.y]);
                    s0 += vp.x * pa.x + vp.y * pb.x;
                    s1 += vp.x * pa.y + vp.y * pb.y;
                    s2 += vp.x * pa.z + vp.y * pb.z;
                }
            }
            if (row < L.n) {
                const int ir = row - wlo;
                const double px = wx[ir], py = wy[ir], pz = wz[ir];
                s0 += d * px;
                s1 += d * py;
                s2 += d * pz;
                q[row] = make_double4(s0, s1, s2, 0.0);
                a0 += px * s0;
                a1 += py * s1;
                a2 += pz * s2;
            }
        }
    }
    block_sum3_store(a0, a1, a2, part_pq + 4 * blockIdx.x);
}

// r = b - L x for the lane's row, summed over each aggregate of `agg` consecutive lanes:
// bc = P' r, and the coarse pre-smoothed iterate xc = omega Dc^-1 bc
__device__ __forceinline__ void down_row(const LevelView &L, int row, const double4 *b,
                                         const double4 *x, double4 *bc, double4 *xc,
                                         const double *cidg, double omega) {
    double s0, s1, s2;
    row_offdiag(L, row, x, s0, s1, s2);
    double r0 = 0, r1 = 0, r2 = 0;
    if (row < L.n) {
        const double4 xr = x[row], br = b[row];
        const double d = L.diag[row];
        r0 = br.x - (s0 + d * xr.x);
        r1 = br.y - (s1 + d * xr.y);
        r2 = br.z - (s2 + d * xr.z);
    }
    r0 = seg_sum(r0, L.agg);
    r1 = seg_sum(r1, L.agg);
    r2 = seg_sum(r2, L.agg);
    if ((row & (L.agg - 1)) == 0 && row < L.n) {
        const int I = row / L.agg;
        bc[I] = make_double4(r0, r1, r2, 0.0);
        const double w = omega * cidg[I];
        xc[I] = make_double4(w * r0, w * r1, w * r2, 0.0);
    }
}

// x' = x + kc * P xc; y = x' + omega D^-1 (b - L x') for the lane's row; returns y
__device__ __forceinline__ double4 up_row(const LevelView &L, int row, const double4 *b,
                                          const double4 *x, const double4 *xc, double omega,
                                          double kc, int sh) {
    double s0, s1, s2;
    row_offdiag_prolong(L, row, x, xc, sh, kc, s0, s1, s2);
    double4 y = make_double4(0, 0, 0, 0);
    if (row < L.n) {
        const double4 xf = x[row], xk = xc[row >> sh], br = b[row];
        const double d = L.diag[row], w = omega * L.idg[row];
        const double p0 = xf.x + kc * xk.x, p1 = xf.y + kc * xk.y, p2 = xf.z + kc * xk.z;
        y.x = p0 + w * (br.x - (s0 + d * p0));
        y.y = p1 + w * (br.y - (s1 + d * p1));
        y.z = p2 + w * (br.z - (s2 + d * p2));
    }
    return y;
}

template <bool CHECK>
__global__ __launch_bounds__(kRowBlock) void k_residual_restrict(
    LevelView L, const double4 *__restrict__ b, const double4 *__restrict__ x,
    double4 *__restrict__ bc, double4 *__restrict__ xc, const double *__restrict__ cidg,
    double omega, const double *__restrict__ part_rr, int nparts, int first, double rtol2,
    double *__restrict__ scal, int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    if (CHECK && pcg_check(part_rr, nparts, first, rtol2, scal, flags)) return;
    ROW_TILE_LOOP(L) {
        const int row = sl_ * 64 + (threadIdx.x & 63);
        down_row(L, row, b, x, bc, xc, cidg, omega);
    }
}

template <bool DOT>
__global__ __launch_bounds__(kRowBlock) void k_prolong_smooth(
    LevelView L, const double4 *__restrict__ b, const double4 *__restrict__ x,
    const double4 *__restrict__ xc, double4 *__restrict__ y, double omega, double kc,
    double *__restrict__ part_rz, const int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    const int sh = __ffs(L.agg) - 1;  // agg is a power of two
    double a0 = 0, a1 = 0, a2 = 0;
    ROW_TILE_LOOP(L) {
        const int row = sl_ * 64 + (threadIdx.x & 63);
        const double4 yy = up_row(L, row, b, x, xc, omega, kc, sh);
        if (row < L.n) {
            y[row] = yy;
            if (DOT) {
                const double4 br = b[row];
                a0 += br.x * yy.x;
                a1 += br.y * yy.y;
                a2 += br.z * yy.z;
            }
        }
    }
    if (DOT) block_sum3_store(a0, a1, a2, part_rz + 4 * blockIdx.x);
}

// single-level preconditioner (plain Jacobi): z = D^-1 r, with the convergence prologue
__global__ __launch_bounds__(kRowBlock) void k_jacobi_z(int n, const double *__restrict__ idg,
                                                        const double4 *__restrict__ r,
                                                        double4 *__restrict__ z,
                                                        double *__restrict__ part_rz,
                                                        const double *__restrict__ part_rr,
                                                        int nparts, int first, double rtol2,
                                                        double *__restrict__ scal,
                                                        int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    if (pcg_check(part_rr, nparts, first, rtol2, scal, flags)) return;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double w = idg[i];
        const double4 ri = r[i];
        const double4 zi = make_double4(w * ri.x, w * ri.y, w * ri.z, 0.0);
        z[i] = zi;
        a0 += ri.x * zi.x;
        a1 += ri.y * zi.y;
        a2 += ri.z * zi.z;
    }
    block_sum3_store(a0, a1, a2, part_rz + 4 * blockIdx.x);
}

// the last level of a hierarchy that the level cap ended without a dense inverse, where no other kernel of the cycle
// can carry them (cycle_from): its correction is the Jacobi sweep already in x. y = x, with the convergence prologue
// (CHECK) and the b.y partials (part_dot != nullptr) that the first and the last kernel of a deeper cycle carry
template <bool CHECK>
__global__ __launch_bounds__(kRowBlock) void k_jacobi_bottom(int n, const double4 *__restrict__ b,
                                                             const double4 *__restrict__ x, double4 *__restrict__ y,
                                                             double *__restrict__ part_dot,
                                                             const double *__restrict__ part_rr, int nparts,
                                                             int first, double rtol2, double *__restrict__ scal,
                                                             int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    if (CHECK && pcg_check(part_rr, nparts, first, rtol2, scal, flags)) return;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double4 bi = b[i], xi = x[i];
        y[i] = xi;
        a0 += bi.x * xi.x;
        a1 += bi.y * xi.y;
        a2 += bi.z * xi.z;
    }
    if (part_dot != nullptr) block_sum3_store(a0, a1, a2, part_dot + 4 * blockIdx.x);
}

// The guard of the banded direct solver's closure path (Graph::bcr_guard): the preconditioner IS a direct solve
// (regularised: bcr.hip), so the convergence prologue and the r.z partials are kernels of their own around it.
__global__ void k_pcg_check_only(const double *__restrict__ part_rr, int nparts, int first, double rtol2,
                                 double *__restrict__ scal, int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    (void)pcg_check(part_rr, nparts, first, rtol2, scal, flags);
}
__global__ __launch_bounds__(kRowBlock) void k_rz_parts(int n, const double4 *__restrict__ r,
                                                        const double4 *__restrict__ z, double *__restrict__ part_rz,
                                                        const int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double4 ri = r[i], zi = z[i];
        a0 += ri.x * zi.x;
        a1 += ri.y * zi.y;
        a2 += ri.z * zi.z;
    }
    block_sum3_store(a0, a1, a2, part_rz + 4 * blockIdx.x);
}

// =============================================================================================
// K5 -- PCG vector kernels (three independent columns share the matrix and the preconditioner)
// =============================================================================================
// INIT: x = 0, r = b (already in R), x0 = omega D^-1 r, partials of ||r||^2.
// else: alpha = rz/pq; x += alpha p; r -= alpha q; x0 = omega D^-1 r; partials of ||r||^2.
template <bool INIT>
__global__ __launch_bounds__(kRowBlock) void k_pcg_update(
    int n, const double *__restrict__ scal, int par, const double *__restrict__ part_pq, int nparts,
    double4 *__restrict__ X, double4 *__restrict__ R, const double4 *__restrict__ P,
    const double4 *__restrict__ AP, const double *__restrict__ idg, double4 *__restrict__ x0,
    double omega, double *__restrict__ part_rr, int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    double al[3] = {0, 0, 0};
    if (!INIT) {
        double pq[3];
        load_reduced3(part_pq, nparts, pq);
        for (int c = 0; c < 3; c++) {
            const double rz = scal[(par ? SC_RZ1 : SC_RZ0) + c];
            al[c] = pq[c] > 0.0 ? rz / pq[c] : 0.0;  // pq = 0: column already solved exactly
        }
    }
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double4 r = R[i];
        if (INIT) {
            X[i] = make_double4(0, 0, 0, 0);
        } else {
            const double4 p = P[i], q = AP[i];
            double4 x = X[i];
            x.x += al[0] * p.x;
            x.y += al[1] * p.y;
            x.z += al[2] * p.z;
            X[i] = x;
            r.x -= al[0] * q.x;
            r.y -= al[1] * q.y;
            r.z -= al[2] * q.z;
            R[i] = r;
        }
        const double w = omega * idg[i];
        x0[i] = make_double4(w * r.x, w * r.y, w * r.z, 0.0);
        a0 += r.x * r.x;
        a1 += r.y * r.y;
        a2 += r.z * r.z;
    }
    block_sum3_store(a0, a1, a2, part_rr + 4 * blockIdx.x);
    if (!INIT && blockIdx.x == 0 && threadIdx.x == 0) flags[FL_ITERS] += 1;
}

// beta = rz_new / rz_old (0 on the first pass); p = z + beta p; rz_new stored under the other parity
__global__ __launch_bounds__(kRowBlock) void k_pcg_pupdate(int n, double *__restrict__ scal, int par,
                                                           int first,
                                                           const double *__restrict__ part_rz,
                                                           int nparts, const double4 *__restrict__ Z,
                                                           double4 *__restrict__ P,
                                                           int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    double rzn[3], be[3];
    load_reduced3(part_rz, nparts, rzn);
    bool finite = true;
    for (int c = 0; c < 3; c++) {
        const double rzo = scal[(par ? SC_RZ1 : SC_RZ0) + c];
        be[c] = (first || !(rzo > 0.0)) ? 0.0 : rzn[c] / rzo;
        finite = finite && isfinite(rzn[c]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) scal[(par ? SC_RZ0 : SC_RZ1) + c] = rzn[c];
        if (!finite) flags[FL_DONE] = 2;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double4 z = Z[i];
        if (first) {
            P[i] = z;
        } else {
            double4 p = P[i];
            p.x = z.x + be[0] * p.x;
            p.y = z.y + be[1] * p.y;
            p.z = z.z + be[2] * p.z;
            P[i] = p;
        }
    }
}

// =============================================================================================
// K5' -- additive top level. Level 0 enters the preconditioner additively:
//   z = omega D0^-1 r + kc * P0 M1^-1 P0' r      (M1 = multiplicative cycle on levels >= 1)
// so the preconditioner needs NO pass over the fine matrix (the multiplicative variant needs
// two). The PCG update restricts r on the fly, r.z is assembled from two partial sets
// (r.z0 here, b1.y1 on level 1) and the p-update prolongs on the fly.
// =============================================================================================
template <bool INIT>
__global__ __launch_bounds__(kRowBlock) void k_pcg_update_restrict(
    int n, int nsl, int agg, const double *__restrict__ scal, int par,
    const double *__restrict__ part_pq, int nparts, double4 *__restrict__ X, double4 *__restrict__ R,
    const double4 *__restrict__ P, const double4 *__restrict__ AP, const double *__restrict__ idg,
    double4 *__restrict__ bc, double4 *__restrict__ xc, const double *__restrict__ cidg,
    double omega, double *__restrict__ part_rr, double *__restrict__ part_rz,
    int *__restrict__ flags) {
    const int done = flags[FL_DONE];
    const int ntiles = (nsl + 3) / 4;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    // The vectors of the first tile are requested BEFORE alpha is reduced from the partials: the
    // reduction (dependent loads + two barriers) then overlaps the ~2 us the streams take to land.
    double4 r_pre = make_double4(0, 0, 0, 0), p_pre = r_pre, q_pre = r_pre, x_pre = r_pre;
    double w_pre = 0.0;
    {
        const int sl = t0 * 4 + (threadIdx.x >> 6);
        const int i = sl * 64 + (threadIdx.x & 63);
        if (t0 < t1 && sl < nsl && i < n) {
            r_pre = R[i];
            w_pre = idg[i];
            if (!INIT) {
                p_pre = P[i];
                q_pre = AP[i];
                x_pre = X[i];
            }
        }
    }
    if (done) return;
    double al[3] = {0, 0, 0};
    if (!INIT) {
        double pq[3];
        load_reduced3(part_pq, nparts, pq);
        for (int c = 0; c < 3; c++) {
            const double rz = scal[(par ? SC_RZ1 : SC_RZ0) + c];
            al[c] = pq[c] > 0.0 ? rz / pq[c] : 0.0;
        }
    }
    double a0 = 0, a1 = 0, a2 = 0, z0 = 0, z1 = 0, z2 = 0;
    for (int t = t0; t < t1; t++) {
        const int sl = t * 4 + (threadIdx.x >> 6);
        if (sl < nsl) {
            const int i = sl * 64 + (threadIdx.x & 63);
            double4 r = make_double4(0, 0, 0, 0);
            if (i < n) {
                double4 p, q, x;
                double wi;
                if (t == t0) {
                    r = r_pre;
                    p = p_pre;
                    q = q_pre;
                    x = x_pre;
                    wi = w_pre;
                } else {
                    r = R[i];
                    wi = idg[i];
                    if (!INIT) {
                        p = P[i];
                        q = AP[i];
                        x = X[i];
                    }
                }
                if (INIT) {
                    X[i] = make_double4(0, 0, 0, 0);
                } else {
                    x.x += al[0] * p.x;
                    x.y += al[1] * p.y;
                    x.z += al[2] * p.z;
                    X[i] = x;
                    r.x -= al[0] * q.x;
                    r.y -= al[1] * q.y;
                    r.z -= al[2] * q.z;
                    R[i] = r;
                }
                const double w = omega * wi;
                a0 += r.x * r.x;
                a1 += r.y * r.y;
                a2 += r.z * r.z;
                z0 += w * r.x * r.x;
                z1 += w * r.y * r.y;
                z2 += w * r.z * r.z;
            }
            const double c0 = seg_sum(r.x, agg), c1 = seg_sum(r.y, agg), c2 = seg_sum(r.z, agg);
            if ((i & (agg - 1)) == 0 && i < n) {
                const int I = i / agg;
                bc[I] = make_double4(c0, c1, c2, 0.0);
                const double w = omega * cidg[I];
                xc[I] = make_double4(w * c0, w * c1, w * c2, 0.0);
            }
        }
    }
    block_sum3_store(a0, a1, a2, part_rr + 4 * blockIdx.x);
    block_sum3_store(z0, z1, z2, part_rz + 4 * blockIdx.x);
    if (!INIT && blockIdx.x == 0 && threadIdx.x == 0) flags[FL_ITERS] += 1;
}

// The PCG update AND the down-sweep of level 1 in one launch (one dependent launch = 4.7 us): the
// workgroup forms r_new not only for its 256 rows but for the window [tile - 64, tile + 320) (two
// more loads of r and q per halo row), restricts it to b1 / x1 = omega D1^-1 b1 for the 48 level-1
// rows of the window (LDS), and lanes 0..31 then evaluate the level-1 residual b1 - L1 x1 of the
// tile's own 32 level-1 rows from that window and restrict it to level 2 -- what
// k_residual_restrict did in a launch of its own. Requires agg = 8 on levels 0 and 1 and every
// level-1 neighbour within 8 rows of the tile's level-1 range (Graph::l1_fused, checked at build
// time: band graphs). Thread tid holds window slots tid and tid + 256; exactly one of them is an
// own row of the tile. The residual ping-pongs between two buffers (Rin -> Rout).
template <bool INIT>
__global__ __launch_bounds__(kRowBlock) void k_pcg_update_restrict2(
    int n, int nsl, const double *__restrict__ scal, int par, const double *__restrict__ part_pq,
    int nparts, double4 *__restrict__ X, const double4 *__restrict__ Rin, double4 *__restrict__ Rout,
    const double4 *__restrict__ P, const double4 *__restrict__ AP, const double *__restrict__ idg,
    LevelView L1, double4 *__restrict__ b1, double4 *__restrict__ x1, double4 *__restrict__ b2,
    double4 *__restrict__ x2, const double *__restrict__ idg2, double omega,
    double *__restrict__ part_rr, double *__restrict__ part_rz, int *__restrict__ flags) {
    const int done = flags[FL_DONE];
    __shared__ double wb[3][kL1Win], wxv[3][kL1Win];
    const int ntiles = (nsl + 3) / 4;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    const int tid = threadIdx.x;
    struct Win {
        double4 r[2], q[2], p, x;  // r, q of both slots; p, x and idg of the own row
        double w;
    };
    auto win_load = [&](int t, Win &W) {
        const int r0 = t * 256;
        const int wlo = max(0, r0 - kWinHalo);
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int iw = tid + u * kRowBlock, i = wlo + iw;
            W.r[u] = W.q[u] = make_double4(0, 0, 0, 0);
            if (iw < kWinLen && i < n) {
                W.r[u] = Rin[i];
                if (!INIT) W.q[u] = AP[i];
            }
        }
        const int io = wlo + tid + (tid >= r0 - wlo ? 0 : kRowBlock);  // the own row among the two slots
        W.p = W.x = make_double4(0, 0, 0, 0);
        W.w = 0.0;
        if (io < n) {
            W.w = idg[io];
            if (!INIT) {
                W.p = P[io];
                W.x = X[io];
            }
        }
    };
    // the first tile's vectors are requested BEFORE alpha is reduced from the partials
    Win W0;
    if (t0 < t1) win_load(t0, W0);
    if (done) return;
    double al[3] = {0, 0, 0};
    if (!INIT) {
        double pq[3];
        load_reduced3(part_pq, nparts, pq);
        for (int c = 0; c < 3; c++) {
            const double rz = scal[(par ? SC_RZ1 : SC_RZ0) + c];
            al[c] = pq[c] > 0.0 ? rz / pq[c] : 0.0;
        }
    }
    double a0 = 0, a1 = 0, a2 = 0, z0 = 0, z1 = 0, z2 = 0;
    for (int t = t0; t < t1; t++) {
        const int r0 = t * 256;
        const int wlo = max(0, r0 - kWinHalo);
        Win W;
        if (t == t0)
            W = W0;
        else
            win_load(t, W);
        const int uo = tid >= r0 - wlo ? 0 : 1;  // which slot is the own row
        __syncthreads();  // the previous tile's level-1 rows are done with the window
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int iw = tid + u * kRowBlock, i = wlo + iw;
            double4 r = W.r[u];
            if (!INIT) {
                r.x -= al[0] * W.q[u].x;
                r.y -= al[1] * W.q[u].y;
                r.z -= al[2] * W.q[u].z;
            }
            if (u == uo && i < n) {  // own row: x, r, ||r||^2 and the Jacobi part of r.z
                if (INIT) {
                    X[i] = make_double4(0, 0, 0, 0);
                } else {
                    double4 x = W.x;
                    x.x += al[0] * W.p.x;
                    x.y += al[1] * W.p.y;
                    x.z += al[2] * W.p.z;
                    X[i] = x;
                }
                Rout[i] = r;  // never in place: neighbouring workgroups read Rin of these rows as halo
                const double w = omega * W.w;
                a0 += r.x * r.x;
                a1 += r.y * r.y;
                a2 += r.z * r.z;
                z0 += w * r.x * r.x;
                z1 += w * r.y * r.y;
                z2 += w * r.z * r.z;
            }
            // restriction to level 1 (aggregates of 8 consecutive rows = 8 consecutive lanes)
            const double c0 = seg_sum(r.x, 8), c1 = seg_sum(r.y, 8), c2 = seg_sum(r.z, 8);
            if ((i & 7) == 0 && iw < kWinLen) {
                const int I = i >> 3, Iw = iw >> 3;
                const bool live = i < n;
                const double w = live ? omega * L1.idg[I] : 0.0;
                wb[0][Iw] = c0;
                wb[1][Iw] = c1;
                wb[2][Iw] = c2;
                wxv[0][Iw] = w * c0;
                wxv[1][Iw] = w * c1;
                wxv[2][Iw] = w * c2;
                if (live && i >= r0 && i < r0 + 256) {
                    b1[I] = make_double4(c0, c1, c2, 0.0);
                    x1[I] = make_double4(w * c0, w * c1, w * c2, 0.0);
                }
            }
        }
        __syncthreads();
        // level-1 residual of the tile's own 32 level-1 rows, restricted to level 2
        if (tid < 32) {
            const int W1lo = wlo >> 3;
            const int row = (r0 >> 3) + tid;
            double s0 = 0, s1 = 0, s2 = 0, e0 = 0, e1 = 0, e2 = 0;
            if (row < L1.n) {
                const int sl = row >> 6, ln = row & 63;
                const int o0 = L1.sl_off[sl], w = L1.sl_off[sl + 1] - o0;
                for (int k = 0; k < w; k++) {
                    const size_t pos = sell_pos(o0, k, ln);
                    const double v = L1.val[pos];
                    const int ci = min(max(L1.col[pos] - W1lo, 0), kL1Win - 1);  // padding: v = 0
                    s0 += v * wxv[0][ci];
                    s1 += v * wxv[1][ci];
                    s2 += v * wxv[2][ci];
                }
                const int me = row - W1lo;
                const double d = L1.diag[row];
                e0 = wb[0][me] - (s0 + d * wxv[0][me]);
                e1 = wb[1][me] - (s1 + d * wxv[1][me]);
                e2 = wb[2][me] - (s2 + d * wxv[2][me]);
            }
            e0 = seg_sum(e0, 8);
            e1 = seg_sum(e1, 8);
            e2 = seg_sum(e2, 8);
            if ((row & 7) == 0 && row < L1.n) {
                const int J = row >> 3;
                b2[J] = make_double4(e0, e1, e2, 0.0);
                const double w = omega * idg2[J];
                x2[J] = make_double4(w * e0, w * e1, w * e2, 0.0);
            }
        }
    }
    block_sum3_store(a0, a1, a2, part_rr + 4 * blockIdx.x);
    block_sum3_store(z0, z1, z2, part_rz + 4 * blockIdx.x);
    if (!INIT && blockIdx.x == 0 && threadIdx.x == 0) flags[FL_ITERS] += 1;
}

// ---------------------------------------------------------------------------------------------
// Chronopoulos-Gear recurrences for the SHARDED PCG (dist.hip): one all-reduce ({||r||^2, r.u, u.w})
// and one halo exchange (of u) per iteration instead of two all-reduces. Generic row kernels (any
// aggregate size, far entries allowed); the single-GPU tile-fused form lives in cgcg.hip.
// ---------------------------------------------------------------------------------------------
// u = omega D^-1 r + kc P0 y1 (the additive-top preconditioner applied), partial sums of r.u
__global__ __launch_bounds__(kRowBlock) void k_form_u(int n, int sh, const double4 *__restrict__ R,
                                                      const double *__restrict__ idg,
                                                      const double4 *__restrict__ yc, double omega, double kc,
                                                      double4 *__restrict__ U, double *__restrict__ part_g,
                                                      const int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double4 r = R[i], y = yc[i >> sh];
        const double w = omega * idg[i];
        const double4 u = make_double4(w * r.x + kc * y.x, w * r.y + kc * y.y, w * r.z + kc * y.z, 0.0);
        U[i] = u;
        a0 += r.x * u.x;
        a1 += r.y * u.y;
        a2 += r.z * u.z;
    }
    block_sum3_store(a0, a1, a2, part_g + 4 * blockIdx.x);
}

// INIT: x = 0, r = b: restriction + ||r||^2. Else: convergence test on the (all-reduced) ||r||^2 of the
// current residual; alpha, beta from the all-reduced gamma = r.u, delta = u.w (row 0 of part_g / part_d);
// p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s; restriction of r to level 1; ||r||^2
// partials of the new residual into rr_out (not the array being tested: other workgroups still read it).
template <bool INIT>
__global__ __launch_bounds__(kRowBlock) void k_cgd_update(
    int n, int nsl, int agg, double *__restrict__ scal, int par, const double *__restrict__ part_g,
    const double *__restrict__ part_d, const double *__restrict__ rr_in, int first, double rtol2,
    double4 *__restrict__ X, double4 *__restrict__ R, double4 *__restrict__ P, double4 *__restrict__ S,
    const double4 *__restrict__ U, const double4 *__restrict__ W, double4 *__restrict__ bc,
    double4 *__restrict__ xc, const double *__restrict__ cidg, double omega, double *__restrict__ rr_out,
    int *__restrict__ flags) {
    if (flags[FL_DONE]) return;
    double al[3] = {0, 0, 0}, be[3] = {0, 0, 0};
    if (!INIT) {
        if (pcg_check(rr_in, 1, first, rtol2, scal, flags)) return;  // every workgroup takes the same decision
        bool finite = true;
        for (int c = 0; c < 3; c++) {
            const double g = part_g[c], d = part_d[c];
            const double go = scal[(par ? SC_GAM1 : SC_GAM0) + c], ao = scal[(par ? SC_ALF1 : SC_ALF0) + c];
            const bool chain = !first && go > 0.0 && ao > 0.0;
            be[c] = chain ? g / go : 0.0;
            double den = d - (chain ? be[c] * g / ao : 0.0);
            if (chain && !(den > 0.0)) {  // see k_cg_update: restart the direction
                be[c] = 0.0;
                den = d;
            }
            al[c] = den > 0.0 ? g / den : 0.0;
            finite = finite && isfinite(g) && isfinite(d);
        }
        __syncthreads();  // all reads of scal done before workgroup 0 publishes the new values
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            for (int c = 0; c < 3; c++) {
                scal[(par ? SC_GAM0 : SC_GAM1) + c] = part_g[c];
                scal[(par ? SC_ALF0 : SC_ALF1) + c] = al[c];
            }
            if (!finite) flags[FL_DONE] = 2;
        }
    }
    const int ntiles = (nsl + 3) / 4;
    int t0, t1;
    tile_range(ntiles, t0, t1);
    double a0 = 0, a1 = 0, a2 = 0;
    for (int t = t0; t < t1; t++) {
        const int sl = t * 4 + (threadIdx.x >> 6);
        if (sl < nsl) {
            const int i = sl * 64 + (threadIdx.x & 63);
            double4 r = make_double4(0, 0, 0, 0);
            if (i < n) {
                r = R[i];
                if (INIT) {
                    X[i] = make_double4(0, 0, 0, 0);
                } else {
                    const double4 u = U[i], w = W[i];
                    double4 p = u, s = w;
                    if (!first) {
                        const double4 po = P[i], so = S[i];
                        p.x += be[0] * po.x;
                        p.y += be[1] * po.y;
                        p.z += be[2] * po.z;
                        s.x += be[0] * so.x;
                        s.y += be[1] * so.y;
                        s.z += be[2] * so.z;
                    }
                    P[i] = p;
                    S[i] = s;
                    double4 x = X[i];
                    x.x += al[0] * p.x;
                    x.y += al[1] * p.y;
                    x.z += al[2] * p.z;
                    X[i] = x;
                    r.x -= al[0] * s.x;
                    r.y -= al[1] * s.y;
                    r.z -= al[2] * s.z;
                    R[i] = r;
                }
                a0 += r.x * r.x;
                a1 += r.y * r.y;
                a2 += r.z * r.z;
            }
            const double c0 = seg_sum(r.x, agg), c1 = seg_sum(r.y, agg), c2 = seg_sum(r.z, agg);
            if ((i & (agg - 1)) == 0 && i < n) {
                const int I = i / agg;
                bc[I] = make_double4(c0, c1, c2, 0.0);
                const double w = omega * cidg[I];
                xc[I] = make_double4(w * c0, w * c1, w * c2, 0.0);
            }
        }
    }
    block_sum3_store(a0, a1, a2, rr_out + 4 * blockIdx.x);
    if (!INIT && blockIdx.x == 0 && threadIdx.x == 0) flags[FL_ITERS] += 1;
}

void launch_form_u(Graph &g, double *part_g) {
    Level &L0 = g.levels[0];
    hipLaunchKernelGGL(k_form_u, dim3(grid_for_elems(L0.n)), dim3(kRowBlock), 0, g.stream, L0.n,
                       __builtin_ctz((unsigned)L0.agg), L0.b.p, L0.idg.p, g.levels[1].y.p, g.opt.mg_omega,
                       g.opt.mg_kc, g.P.p, part_g, g.flags.p);
}

// buffers: u = P, w = AP, p = P2, s = levels[0].e, r = levels[0].b
void launch_cgd_update(Graph &g, bool init, int par, int first, double rtol2, const double *part_g,
                       const double *part_d, const double *rr_in, double *rr_out) {
    Level &L0 = g.levels[0];
    Level &L1 = g.levels[1];
    const int grid = grid_for_rows(L0);
    if (init)
        hipLaunchKernelGGL((k_cgd_update<true>), dim3(grid), dim3(kRowBlock), 0, g.stream, L0.n, L0.nsl, L0.agg,
                           g.scal.p, par, part_g, part_d, rr_in, first, rtol2, g.X.p + g.ng, L0.b.p, g.P2.p, L0.e.p,
                           g.P.p, g.AP.p, L1.b.p, L1.x.p, L1.idg.p, g.opt.mg_omega, rr_out, g.flags.p);
    else
        hipLaunchKernelGGL((k_cgd_update<false>), dim3(grid), dim3(kRowBlock), 0, g.stream, L0.n, L0.nsl, L0.agg,
                           g.scal.p, par, part_g, part_d, rr_in, first, rtol2, g.X.p + g.ng, L0.b.p, g.P2.p, L0.e.p,
                           g.P.p, g.AP.p, L1.b.p, L1.x.p, L1.idg.p, g.opt.mg_omega, rr_out, g.flags.p);
}

// beta from r.z = (r.z0 partials) + kc * (b1.y1 partials); p = omega D^-1 r + kc * P y1 + beta p
template <bool CHECK>
__global__ __launch_bounds__(kRowBlock) void k_pcg_pupdate_add(
    int n, int sh, double *__restrict__ scal, int par, int first, const double *__restrict__ part_rz,
    int np0, const double *__restrict__ part_rz2, int np1, const double4 *__restrict__ R,
    const double *__restrict__ idg, const double4 *__restrict__ yc, double omega, double kc,
    double4 *__restrict__ P, int *__restrict__ flags, const double *__restrict__ part_rr, int np_rr,
    double rtol2) {
    const int done = flags[FL_DONE];
    const int i_pre = blockIdx.x * blockDim.x + threadIdx.x;
    double4 r_pre = make_double4(0, 0, 0, 0), y_pre = r_pre, p_pre = r_pre;
    double w_pre = 0.0;
    if (i_pre < n) {  // first grid-stride element: requested before beta is reduced (see update)
        r_pre = R[i_pre];
        y_pre = yc[i_pre >> sh];
        w_pre = idg[i_pre];
        if (!first) p_pre = P[i_pre];
    }
    if (done) return;
    // sharded runs test convergence here (||r||^2 arrives with r.z in ONE all-reduce after the
    // preconditioner) instead of in the preconditioner's first kernel
    if (CHECK && pcg_check(part_rr, np_rr, first, rtol2, scal, flags)) return;
    double ra[3], rb[3], rzn[3], be[3];
    load_reduced3(part_rz, np0, ra);
    load_reduced3(part_rz2, np1, rb);
    bool finite = true;
    for (int c = 0; c < 3; c++) {
        rzn[c] = ra[c] + kc * rb[c];
        const double rzo = scal[(par ? SC_RZ1 : SC_RZ0) + c];
        be[c] = (first || !(rzo > 0.0)) ? 0.0 : rzn[c] / rzo;
        finite = finite && isfinite(rzn[c]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) scal[(par ? SC_RZ0 : SC_RZ1) + c] = rzn[c];
        if (!finite) flags[FL_DONE] = 2;
    }
    for (int i = i_pre; i < n; i += gridDim.x * blockDim.x) {
        const bool pre = i == i_pre;
        const double4 r = pre ? r_pre : R[i], y = pre ? y_pre : yc[i >> sh];
        const double w = omega * (pre ? w_pre : idg[i]);
        double4 p = make_double4(w * r.x + kc * y.x, w * r.y + kc * y.y, w * r.z + kc * y.z, 0.0);
        if (!first) {
            const double4 po = pre ? p_pre : P[i];
            p.x += be[0] * po.x;
            p.y += be[1] * po.y;
            p.z += be[2] * po.z;
        }
        P[i] = p;
    }
}

// =============================================================================================
// K6 -- score, exp map and rotation update (one free view per thread)
// =============================================================================================
__global__ __launch_bounds__(kRowBlock) void k_apply_step(int n, int f, int nghost,
                                                       const double4 *__restrict__ X,
                                                       double4 *__restrict__ Q,
                                                       double *__restrict__ part_score,
                                                       int write, const int *__restrict__ gate) {
    if (gate != nullptr && gate[FL_DONE] != 1) return;  // see k_update_weights
    double acc = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double4 x = X[i];
        // A step that is not finite (a solve that broke down on non-finite inputs or weights) leaves its rotation alone:
        // the score turns non-finite, the caller gets IROTAVG_ERR_SOLVER, and the handle still holds the rotations it had
        // (the reference would store zero quaternions there, :491 -- and exit)
        const double th = step_apply(x.x, x.y, x.z, Q, i + f, write != 0);
        if (i >= nghost) acc += th;  // score = mean ||W3 row|| BEFORE the exp map (ral/l1_irls.cpp:729); ghosts are scored by their owner
    }
    block_sum3_store(acc, 0.0, 0.0, part_score + 4 * blockIdx.x);
}

__global__ __launch_bounds__(256) void k_normalise(int n_total, int f, double4 *__restrict__ Q) {
    const int i = f + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    double4 q = Q[i];
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 > 0.0) {  // Eigen normalized() (ral/l1_irls.cpp:982-991)
        const double nn = sqrt(n2);
        q.x /= nn;
        q.y /= nn;
        q.z /= nn;
        q.w /= nn;
    }
    Q[i] = q;
}

__global__ __launch_bounds__(256) void k_fill(long long n, double v, double *__restrict__ p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
// scal (SC_COUNT doubles) and flags (FL_COUNT ints) share one allocation so that a poll of the solver
// state is ONE device -> host copy, into the handle's pinned block
void alloc_state(Graph &g) {
    static_assert(sizeof(int) * FL_COUNT <= 2 * sizeof(double), "flags tail");
    g.scal.alloc(SC_COUNT + 2);
    g.scal.zero(g.stream);
    const double one = 1.0;
    IRH_CHECK(hipMemcpyAsync(g.scal.p + SC_DSCALE, &one, sizeof(double), hipMemcpyHostToDevice, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
    g.flags.release();
    g.flags.p = reinterpret_cast<int *>(g.scal.p + SC_COUNT);
    g.flags.n = FL_COUNT;
    g.flags.own = false;
    if (!g.hpin) g.hpin = static_cast<double *>(PinPool::get().take());
}
void read_back_state(Graph &g) {
    IRH_CHECK(hipMemcpyAsync(g.h_scal(), g.scal.p, sizeof(double) * (SC_COUNT + 2), hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
}

void fill(Graph &g, double *p, long long n, double v) {
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g.stream, n, v, p);
}

void normalise_rotations(Graph &g) {
    const int cnt = (int)(g.n_total - g.f);
    if (cnt <= 0) return;
    hipLaunchKernelGGL(k_normalise, dim3((cnt + 255) / 256), dim3(256), 0, g.stream,
                       (int)g.n_total, g.f, g.Q.p);
}

// one-shot variant for host-resident rows (irotavg_quat_normalised): staged through HBM so the
// arithmetic is the same kernel as the resident path
int normalise_host_rows(int64_t n, double *Q, int64_t ldq, int f) {
    if (n - f <= 0) return IROTAVG_OK;
    DevBuf<double4> d;
    std::vector<double4> h((size_t)n);
    for (int64_t i = 0; i < n; i++) h[i] = make_double4(Q[i], Q[ldq + i], Q[2 * ldq + i], Q[3 * ldq + i]);
    d.alloc((size_t)n);
    IRH_CHECK(hipMemcpy(d.p, h.data(), sizeof(double4) * (size_t)n, hipMemcpyHostToDevice));
    const int cnt = (int)(n - f);
    hipLaunchKernelGGL(k_normalise, dim3((cnt + 255) / 256), dim3(256), 0, 0, (int)n, f, d.p);
    IRH_CHECK(hipMemcpy(h.data(), d.p, sizeof(double4) * (size_t)n, hipMemcpyDeviceToHost));
    for (int64_t i = f; i < n; i++) {
        Q[i] = h[i].x;
        Q[ldq + i] = h[i].y;
        Q[2 * ldq + i] = h[i].z;
        Q[3 * ldq + i] = h[i].w;
    }
    return IROTAVG_OK;
}

// =============================================================================================
// host drivers
// =============================================================================================
int round_grid(long long gsz) {
    // a multiple of 8 (tile_range deals adjacent chunks to the workgroups of one XCD), rounded UP: with
    // fewer workgroups than tiles some workgroup gets two tiles and the whole launch waits for it
    // (391 tiles on 384 workgroups: every row kernel took two tile times)
    if (gsz >= 8) gsz = (gsz + 7) & ~7ll;
    gsz = std::min<long long>(gsz, kMaxParts);
    return (int)std::max<long long>(gsz, 1);
}
int grid_for_rows(const Level &L) { return round_grid((L.nsl + 3) / 4); }
int grid_for_elems(long long n) { return round_grid((n + kRowBlock - 1) / kRowBlock); }

// refresh all matrix values from per-edge weights: mode 0 = IRLS (d^2, rhs), mode 1 = L1 Hessian
void assemble(Graph &g, int mode, const double *wsrc, bool refresh_dense) {
    assemble_values(g, mode, wsrc);
    if (g.bcr_B) return;  // banded operator, solved directly (bcr.hip): no coarse levels, no dense inverse
    // IRLS on a graph with loop closures re-inverts in every iteration: after two 'stale'
    // verdicts in a row the test (three small launches + a host round trip, ~40 us) is skipped three times out
    // of four and the inverse refreshed straight away
    bool assume_stale = false;
    if (!refresh_dense && mode == 0 && g.ndense > 0 && g.dense_valid && g.stale_streak >= 2) {
        assume_stale = (g.stale_skips++ & 3) != 3;
    }
    bool stale = refresh_dense || assume_stale;
    // The robust weights follow the residuals, and the residuals moved by the last step: once that step is tiny
    // (run_irls sets irls_settle when the score fell below 20 x change_th) the coarse operator has settled except
    // for entries that no longer matter (down-weighted outliers, whose ratios still swing by decades and keep the
    // entry-wise test at 'stale'). Re-using the inverse there costs ~3 PCG iterations instead of a 1 ms sweep
    // (100k/2M with 2 % loop edges: 14.1 -> 13.5 ms per irls call; IROTAVG_NO_SETTLE=1 switches it off).
    if (!refresh_dense && mode == 0 && g.irls_settle > 0.0 && g.ndense > 0 && g.dense_valid && dense_rescale_only(g)) {
        g.dense_fresh = false;
        return;
    }
    if (!stale) {
        stale = dense_is_stale(g, mode == 0);
        if (mode == 0) g.stale_streak = stale ? g.stale_streak + 1 : 0;
    }
    if (stale) {
        dense_refresh(g);
        g.dense_valid = true;
        g.dense_fresh = true;
    } else {
        g.dense_fresh = false;
    }
}

void assemble_values(Graph &g, int mode, const double *wsrc) {
    Level &L0 = g.levels[0];
    g.bcr_wsrc = wsrc;
    g.bcr_wsquare = mode == 0;
    const int grid = grid_for_rows(L0);
    size_t first_coarse = 1;
    if (g.asm_windowed) {
        // one workgroup per slice, the grid padded to a multiple of 8 (XCD-chunked slice order)
        const int gw = (L0.nsl + 7) / 8 * 8;
        const bool l1 = g.asm_l1_fused != 0 && !g.bcr_B;
        Level *C1 = g.levels.size() > 1 ? &g.levels[1] : nullptr;
#define IRH_ASM_ARGS                                                                                         \
    L0.n, L0.nsl, (long long)g.m, (long long)g.mpad, L0.sl_off.p, g.slot_eid.p, g.slot_cs.p, g.tile_e0.p,    \
        g.bptr.p, g.beid.p, g.bflag.p, wsrc, g.er.p, L0.val.p, L0.excess.p, L0.diag.p, L0.idg.p, L0.b.p,     \
        g.bval.p, l1 ? C1->n : 0, l1 ? C1->sl_off.p : nullptr, l1 ? C1->val.p : nullptr,                    \
        l1 ? C1->excess.p : nullptr, l1 ? C1->diag.p : nullptr, l1 ? C1->idg.p : nullptr
        if (mode == 0 && l1)
            hipLaunchKernelGGL((k_assemble0w<0, true>), dim3(gw), dim3(kRowBlock), 0, g.stream, IRH_ASM_ARGS);
        else if (mode == 0)
            hipLaunchKernelGGL((k_assemble0w<0, false>), dim3(gw), dim3(kRowBlock), 0, g.stream, IRH_ASM_ARGS);
        else if (l1)
            hipLaunchKernelGGL((k_assemble0w<1, true>), dim3(gw), dim3(kRowBlock), 0, g.stream, IRH_ASM_ARGS);
        else if (g.pd_rhs_src) {
            // the primal-dual Hessian and the right-hand side of its system in one walk (MODE 2): t instead of the residuals
            const double *er_keep = g.er.p;
            g.er.p = const_cast<double *>(g.pd_rhs_src);
            hipLaunchKernelGGL((k_assemble0w<2, false>), dim3(gw), dim3(kRowBlock), 0, g.stream, IRH_ASM_ARGS);
            g.er.p = const_cast<double *>(er_keep);
            g.pd_rhs_done = true;
        } else
            hipLaunchKernelGGL((k_assemble0w<1, false>), dim3(gw), dim3(kRowBlock), 0, g.stream, IRH_ASM_ARGS);
#undef IRH_ASM_ARGS
        if (l1) first_coarse = 2;
    } else if (mode == 0) {
        if (g.T.n < (size_t)g.mpad) g.T.alloc((size_t)g.mpad);
        hipLaunchKernelGGL(k_edge_pack, dim3((unsigned)((g.m + 255) / 256)), dim3(256), 0, g.stream,
                           (long long)g.m, (long long)g.mpad, wsrc, g.er.p, g.T.p);
        hipLaunchKernelGGL((k_assemble0<0>), dim3(grid), dim3(kRowBlock), 0, g.stream, L0.n, L0.nsl,
                           L0.sl_off.p, g.slot_eid.p, g.bptr.p, g.beid.p, g.bflag.p, wsrc, g.T.p,
                           L0.val.p, L0.excess.p, L0.diag.p, L0.idg.p, L0.b.p, g.bval.p);
    } else {
        hipLaunchKernelGGL((k_assemble0<1>), dim3(grid), dim3(kRowBlock), 0, g.stream, L0.n, L0.nsl,
                           L0.sl_off.p, g.slot_eid.p, g.bptr.p, g.beid.p, g.bflag.p, wsrc,
                           (const double4 *)nullptr, L0.val.p, L0.excess.p, L0.diag.p, L0.idg.p, L0.b.p,
                           g.bval.p);
    }
    if (g.bcr_B) return;  // the direct solver reads level 0 only
    for (size_t l = first_coarse; l < g.levels.size(); l++) {
        Level &F = g.levels[l - 1];
        Level &C = g.levels[l];
        if (g.asm_windowed && C.max_row <= 16 && C.crow.n > 0) {
            // the last level of a graph whose inverse is about to be re-used: the staleness verdict rides along
            const bool chk = g.asm_check_stale && l + 1 == g.levels.size() && g.ndense > 0 &&
                             g.dense_ref_val.n >= (size_t)C.sell_len && C.sell_len > 0;
            if (chk && g.dense_mm.n < 3) {
                g.dense_mm.alloc(3);
                const unsigned long long init[3] = {0x7ff0000000000000ull, 0ull, 0ull};  // +inf, 0, 0
                IRH_CHECK(hipMemcpyAsync(g.dense_mm.p, init, sizeof(init), hipMemcpyHostToDevice, g.stream));
                IRH_CHECK(hipStreamSynchronize(g.stream));
            }
            hipLaunchKernelGGL(k_coarse_level, dim3((C.n * 8 + kRowBlock - 1) / kRowBlock), dim3(kRowBlock), 0,
                               g.stream, view_of(C), C.crow.p, C.cptr.p, C.cidx.p, C.cpos.p, F.val.p, C.val.p,
                               F.n, F.agg, F.excess.p, C.excess.p, C.diag.p, C.idg.p,
                               chk ? g.dense_ref_val.p : (const double *)nullptr, g.dense_ref_diag.p, g.stale_spread,
                               chk ? g.dense_mm.p : (unsigned long long *)nullptr, g.scal.p, g.flags.p);
            if (chk) g.asm_check_done = true;
            continue;
        }
        if (C.nnz > 0) {
            const int grid2 = round_grid((C.nnz + 31) / 32);
            hipLaunchKernelGGL(k_coarse_vals, dim3(grid2), dim3(kRowBlock), 0, g.stream, C.nnz,
                               C.cptr.p, C.cidx.p, C.cpos.p, F.val.p, C.val.p);
        }
        hipLaunchKernelGGL(k_coarse_diag, dim3((C.n * 8 + kRowBlock - 1) / kRowBlock),
                           dim3(kRowBlock), 0, g.stream, view_of(C), F.n, F.agg, F.excess.p,
                           C.excess.p, C.diag.p, C.idg.p);
    }
}

// Multiplicative part of the cycle on levels [from, nl): down-sweeps, exact dense solve (or one
// Jacobi sweep when no dense inverse exists), up-sweeps. Input: levels[from].b and .x (pre-
// smoothed iterate omega D^-1 b); output: levels[from].y. `check_first`: the first kernel
// launched carries the PCG convergence prologue. `dot_from`: the kernel producing
// levels[from].y also emits partial sums of b.y into `part_dot`.
static void cycle_from(Graph &g, int from, bool check_first, bool dot_from, double *part_dot,
                       int np_rr, int first, double rtol2, int *np_dot, bool first_down_done = false) {
    const int nl = (int)g.levels.size();
    const double omega = g.opt.mg_omega, kc = g.opt.mg_kc;
    bool check = check_first;
    // first_down_done: levels[from + 1].b / .x were already produced (k_pcg_update_restrict2)
    for (int l = first_down_done ? from + 1 : from; l < nl - 1; l++) {
        Level &F = g.levels[l];
        Level &C = g.levels[l + 1];
        const int grid = grid_for_rows(F);
        if (check)
            hipLaunchKernelGGL((k_residual_restrict<true>), dim3(grid), dim3(kRowBlock), 0, g.stream,
                               view_of(F), F.b.p, F.x.p, C.b.p, C.x.p, C.idg.p, omega, g.part_rr.p,
                               np_rr, first, rtol2, g.scal.p, g.flags.p);
        else
            hipLaunchKernelGGL((k_residual_restrict<false>), dim3(grid), dim3(kRowBlock), 0,
                               g.stream, view_of(F), F.b.p, F.x.p, C.b.p, C.x.p, C.idg.p, omega,
                               g.part_rr.p, np_rr, first, rtol2, g.scal.p, g.flags.p);
        check = false;
    }
    Level &CL = g.levels[nl - 1];
    const bool last_is_from = (from == nl - 1);
    if (g.ndense > 0) {
        dense_apply(g, CL.b.p, CL.y.p, check, dot_from && last_is_from, part_dot, np_rr, first, rtol2);
        if (dot_from && last_is_from && np_dot) *np_dot = dense_apply_grid(g);
    } else if (last_is_from || check) {
        // level cap reached without a dense level, and no kernel before this one in the cycle (additive top level over
        // a capped level 1; or over levels 1 and 2 with the level-1 down-sweep done by the update): the copy carries the
        // convergence prologue itself, and the b.y partials when no up-sweep follows (nl == 1 never comes here: the
        // caller's k_jacobi_z path)
        const int ge = grid_for_elems(CL.n);
        double *pd = (dot_from && last_is_from) ? part_dot : nullptr;
        if (check)
            hipLaunchKernelGGL((k_jacobi_bottom<true>), dim3(ge), dim3(kRowBlock), 0, g.stream, CL.n, CL.b.p, CL.x.p,
                               CL.y.p, pd, g.part_rr.p, np_rr, first, rtol2, g.scal.p, g.flags.p);
        else
            hipLaunchKernelGGL((k_jacobi_bottom<false>), dim3(ge), dim3(kRowBlock), 0, g.stream, CL.n, CL.b.p, CL.x.p,
                               CL.y.p, pd, g.part_rr.p, np_rr, first, rtol2, g.scal.p, g.flags.p);
        if (pd && np_dot) *np_dot = ge;
    } else {
        // level cap reached without a dense level: its correction is the Jacobi sweep already in x.
        IRH_CHECK(hipMemcpyAsync(CL.y.p, CL.x.p, sizeof(double4) * (size_t)CL.n,
                                 hipMemcpyDeviceToDevice, g.stream));
    }
    for (int l = nl - 2; l >= from; l--) {
        Level &F = g.levels[l];
        Level &C = g.levels[l + 1];
        const int grid = grid_for_rows(F);
        if (l == from && dot_from) {
            hipLaunchKernelGGL((k_prolong_smooth<true>), dim3(grid), dim3(kRowBlock), 0, g.stream,
                               view_of(F), F.b.p, F.x.p, C.y.p, F.y.p, omega, kc, part_dot, g.flags.p);
            if (np_dot) *np_dot = grid;
        } else {
            hipLaunchKernelGGL((k_prolong_smooth<false>), dim3(grid), dim3(kRowBlock), 0, g.stream,
                               view_of(F), F.b.p, F.x.p, C.y.p, F.y.p, omega, kc, part_dot, g.flags.p);
        }
    }
}

void cycle_levels(Graph &g, int from) {
    cycle_from(g, from, false, false, nullptr, 0, 0, 0.0, nullptr, false);
}

// Preconditioner application. Multiplicative mode: z = levels[0].y, r.z partials in part_rz
// (np_rz of them). Additive-top mode: levels[1].y = M1^-1 P0' r and b1.y1 partials in part_rz2
// (np_rz2); z itself is formed inside the p-update.
PrecInfo precondition(Graph &g, int first, double rtol2, bool check) {
    PrecInfo pi;
    const int nl = (int)g.levels.size();
    Level &L0 = g.levels[0];
    int np_rr = g.additive_top && nl > 1 ? grid_for_rows(L0) : grid_for_elems(L0.n);
    if (g.force_np) np_rr = g.force_np;  // sharded run: partials were reduced across shards into row 0
    if (nl == 1 && g.bcr_B && g.bcr_guard) {
        // z = (A_b + E + V C V')^-1 r: the regularised direct solve (every dead pivot of the band part replaced by the
        // row's own diagonal entry: E); the operator of the iteration is the true one, so the iteration ends after about
        // as many steps as there are dead pivots
        hipLaunchKernelGGL(k_pcg_check_only, dim3(1), dim3(kRowBlock), 0, g.stream, g.part_rr.p, np_rr, first, rtol2,
                           g.scal.p, g.flags.p);
        BcrRequest rq;
        rq.out = L0.y.p;
        (void)bcr_solve(g, rq);
        pi.np_rz = grid_for_elems(L0.n);
        hipLaunchKernelGGL(k_rz_parts, dim3(pi.np_rz), dim3(kRowBlock), 0, g.stream, L0.n, L0.b.p, L0.y.p, g.part_rz.p,
                           g.flags.p);
        return pi;
    }
    if (nl == 1) {
        if (g.ndense > 0) {  // the whole system is the dense level: z = L^-1 r exactly
            dense_apply(g, L0.b.p, L0.y.p, true, true, g.part_rz.p, np_rr, first, rtol2);
            pi.np_rz = dense_apply_grid(g);
        } else {
            pi.np_rz = grid_for_elems(L0.n);
            hipLaunchKernelGGL(k_jacobi_z, dim3(pi.np_rz), dim3(kRowBlock), 0, g.stream, L0.n,
                               L0.idg.p, L0.b.p, L0.y.p, g.part_rz.p, g.part_rr.p, np_rr, first,
                               rtol2, g.scal.p, g.flags.p);
        }
        return pi;
    }
    if (g.additive_top) {
        pi.np_rz = g.additive_top && nl > 1 ? grid_for_rows(L0) : np_rr;  // r.z0 partials of the update kernel
        cycle_from(g, 1, check, true, g.part_rz2.p, np_rr, first, rtol2, &pi.np_rz2, g.l1_fused && nl > 2);
    } else {
        cycle_from(g, 0, true, true, g.part_rz.p, np_rr, first, rtol2, &pi.np_rz);
    }
    return pi;
}

void launch_spmv(Graph &g, const double4 *p, const double4 *pg, const int *flags) {
    Level &L0 = g.levels[0];
    hipLaunchKernelGGL(k_spmv_dot, dim3(grid_for_rows(L0)), dim3(kRowBlock), 0, g.stream, view_of(L0),
                       p ? p : (const double4 *)g.P.p, g.AP.p, g.part_pq.p, flags ? flags : (const int *)g.flags.p,
                       g.ng > 0 ? (pg ? pg : (const double4 *)g.PG.p) : (const double4 *)nullptr, g.bptr.p,
                       g.bghost.p, g.bval.p);
}

void launch_update(Graph &g, bool init, int par, int np_pq, const double4 *pvec, const double4 *rin,
                   double4 *rout) {
    Level &L0 = g.levels[0];
    const double4 *P = pvec ? pvec : g.P.p;
    const int nl = (int)g.levels.size();
    if (g.additive_top && nl > 2 && g.l1_fused && rin && rout) {
        Level &L1 = g.levels[1];
        Level &L2 = g.levels[2];
        const int grid = grid_for_rows(L0);
        if (init)
            hipLaunchKernelGGL((k_pcg_update_restrict2<true>), dim3(grid), dim3(kRowBlock), 0, g.stream, L0.n,
                               L0.nsl, g.scal.p, par, g.part_pq.p, np_pq, g.X.p + g.ng, rin, rout, P, g.AP.p,
                               L0.idg.p, view_of(L1), L1.b.p, L1.x.p, L2.b.p, L2.x.p, L2.idg.p, g.opt.mg_omega,
                               g.part_rr.p, g.part_rz.p, g.flags.p);
        else
            hipLaunchKernelGGL((k_pcg_update_restrict2<false>), dim3(grid), dim3(kRowBlock), 0, g.stream, L0.n,
                               L0.nsl, g.scal.p, par, g.part_pq.p, np_pq, g.X.p + g.ng, rin, rout, P, g.AP.p,
                               L0.idg.p, view_of(L1), L1.b.p, L1.x.p, L2.b.p, L2.x.p, L2.idg.p, g.opt.mg_omega,
                               g.part_rr.p, g.part_rz.p, g.flags.p);
    } else if (g.additive_top && nl > 1) {
        Level &L1 = g.levels[1];
        const int grid = grid_for_rows(L0);
        if (init)
            hipLaunchKernelGGL((k_pcg_update_restrict<true>), dim3(grid), dim3(kRowBlock), 0, g.stream,
                               L0.n, L0.nsl, L0.agg, g.scal.p, par, g.part_pq.p, np_pq, g.X.p + g.ng, L0.b.p,
                               P, g.AP.p, L0.idg.p, L1.b.p, L1.x.p, L1.idg.p, g.opt.mg_omega,
                               g.part_rr.p, g.part_rz.p, g.flags.p);
        else
            hipLaunchKernelGGL((k_pcg_update_restrict<false>), dim3(grid), dim3(kRowBlock), 0,
                               g.stream, L0.n, L0.nsl, L0.agg, g.scal.p, par, g.part_pq.p, np_pq,
                               g.X.p + g.ng, L0.b.p, P, g.AP.p, L0.idg.p, L1.b.p, L1.x.p, L1.idg.p,
                               g.opt.mg_omega, g.part_rr.p, g.part_rz.p, g.flags.p);
    } else {
        const int ge = grid_for_elems(L0.n);
        if (init)
            hipLaunchKernelGGL((k_pcg_update<true>), dim3(ge), dim3(kRowBlock), 0, g.stream, L0.n,
                               g.scal.p, par, g.part_pq.p, np_pq, g.X.p + g.ng, L0.b.p, P, g.AP.p,
                               L0.idg.p, L0.x.p, g.opt.mg_omega, g.part_rr.p, g.flags.p);
        else
            hipLaunchKernelGGL((k_pcg_update<false>), dim3(ge), dim3(kRowBlock), 0, g.stream, L0.n,
                               g.scal.p, par, g.part_pq.p, np_pq, g.X.p + g.ng, L0.b.p, P, g.AP.p,
                               L0.idg.p, L0.x.p, g.opt.mg_omega, g.part_rr.p, g.flags.p);
    }
}

void launch_pupdate(Graph &g, int par, int first, const PrecInfo &pi, bool check, int np_rr, double rtol2) {
    Level &L0 = g.levels[0];
    const int nl = (int)g.levels.size();
    const int ge = grid_for_elems(L0.n);
    if (g.additive_top && nl > 1) {
        const int sh = __builtin_ctz((unsigned)L0.agg);
        if (check)
            hipLaunchKernelGGL((k_pcg_pupdate_add<true>), dim3(ge), dim3(kRowBlock), 0, g.stream, L0.n, sh,
                               g.scal.p, par, first, g.part_rz.p, pi.np_rz, g.part_rz2.p, pi.np_rz2,
                               L0.b.p, L0.idg.p, g.levels[1].y.p, g.opt.mg_omega, g.opt.mg_kc, g.P.p,
                               g.flags.p, g.part_rr.p, np_rr, rtol2);
        else
            hipLaunchKernelGGL((k_pcg_pupdate_add<false>), dim3(ge), dim3(kRowBlock), 0, g.stream, L0.n, sh,
                               g.scal.p, par, first, g.part_rz.p, pi.np_rz, g.part_rz2.p, pi.np_rz2,
                               L0.b.p, L0.idg.p, g.levels[1].y.p, g.opt.mg_omega, g.opt.mg_kc, g.P.p,
                               g.flags.p, g.part_rr.p, np_rr, rtol2);
    } else {
        hipLaunchKernelGGL(k_pcg_pupdate, dim3(ge), dim3(kRowBlock), 0, g.stream, L0.n, g.scal.p, par,
                           first, g.part_rz.p, pi.np_rz, L0.y.p, g.P.p, g.flags.p);
    }
}

// PCG on L X = levels[0].b (three columns). Matrix values must be assembled. Result in g.X.
// Iteration k: [precondition (its first kernel tests convergence of the previous update)] ->
// p-update -> q = L p -> x/r update. The host polls the done flag every pcg_check_every
// iterations; kernels enqueued past convergence return immediately.
int pcg_solve(Graph &g, const std::function<void()> *tail, bool *tail_ran) {
    if (g.cg2) return pcg_solve_cg2(g, tail, tail_ran, false);
    return pcg_solve_classic(g, tail, tail_ran);
}

// `tail`: work to run once the solve has converged, enqueued behind the first convergence test and gated on the
// done flag by its own kernels (run_irls: weight update + rotation update); *tail_ran tells whether it took effect.
int pcg_solve_classic(Graph &g, const std::function<void()> *tail, bool *tail_ran) {
    if (tail_ran) *tail_ran = false;
    Level &L0 = g.levels[0];
    // A graph that is ONE dense level (<= mg_dense_max views) has the explicit inverse of its whole operator as the
    // preconditioner: an iteration is a step of iterative refinement. Stopping at pcg_rtol = 1e-10 leaves an error of up
    // to cond * 1e-10 in the step -- on a barely connected graph (cond 1e6) whose IRLS iteration does not contract that
    // is amplified from outer iteration to outer iteration until the strict `score > change_th` test
    // (ral/l1_irls.cpp:590) ends the run after a different number of iterations than any exact factorisation would:
    // fuzz seed 603 case 163, 15 iterations and 0.11 rad where four exact CPU solves agree on 13 (tools/referee.py,
    // tests/test_gpu_referee.py). Such a level is therefore solved to the residual it can ATTAIN, as the reference's
    // factorisations are (:536-556): the device tests against kRefineTol, and the host takes the iterate once the
    // residual is within pcg_rtol and has stopped halving (or after kRefineExtra more iterations).
    constexpr double kRefineTol = 1e-15;
    constexpr int kRefineExtra = 6;
    const bool refine = g.levels.size() == 1 && g.ndense > 0 && !g.bcr_B && g.ng == 0 && !g.sw.no_dense_refine &&
                        g.opt.pcg_rtol > kRefineTol;
    const double rtol_dev = refine ? kRefineTol : g.opt.pcg_rtol;
    const double rtol2 = rtol_dev * rtol_dev;
    const int gr = grid_for_rows(L0);
    IRH_CHECK(hipMemsetAsync(g.flags.p, 0, sizeof(int) * FL_COUNT, g.stream));
    // with the level-1 down-sweep fused into the update (l1_fused) the residual ping-pongs between
    // levels[0].b and R2: rcur is the buffer holding the current r
    double4 *RR[2] = {L0.b.p, g.R2.p};
    int rcur = 0;
    auto update = [&](bool init, int par, const double4 *pvec) {
        if (g.l1_fused) {
            launch_update(g, init, par, gr, pvec, RR[rcur], RR[rcur ^ 1]);
            rcur ^= 1;
        } else {
            launch_update(g, init, par, gr, pvec);
        }
    };
    update(true, 0, nullptr);
    int *h_flags = g.h_flags();
    for (int c = 0; c < FL_COUNT; c++) h_flags[c] = 0;
    int it = 0;
    const int check = std::max(1, g.opt.pcg_check_every);
    const int maxit = std::max(1, g.opt.pcg_max_iters);
    // single GPU + additive top level: p-update and SpMV are one launch (k_pspmv_dot), the search
    // direction ping-pongs between P and P2
    const bool fused = g.additive_top && g.levels.size() > 1 && g.ng == 0 &&
                       g.l0_far_entries * 32 <= g.levels[0].sell_len / 64 && g.opt.no_fused_pspmv != 1;
    const bool far = g.l0_far_entries > 0;
    double4 *PP[2] = {g.P.p, g.P2.p};
    auto iteration_tail = [&](const PrecInfo &pi) {
        const int first = (it == 0);
        const int par = it & 1;
        if (fused) {
            const int sh = __builtin_ctz((unsigned)L0.agg);
#define PSPMV_LAUNCH(F1, FR)                                                                           \
    hipLaunchKernelGGL((k_pspmv_dot<F1, FR>), dim3(gr), dim3(kRowBlock), 0, g.stream, view_of(L0), sh,   \
                       g.scal.p, par, g.part_rz.p, pi.np_rz, g.part_rz2.p, pi.np_rz2, RR[rcur],            \
                       g.levels[1].y.p, g.opt.mg_omega, g.opt.mg_kc, PP[par], PP[par ^ 1], g.AP.p,        \
                       g.part_pq.p, g.flags.p)
            if (first && far)
                PSPMV_LAUNCH(true, true);
            else if (first)
                PSPMV_LAUNCH(true, false);
            else if (far)
                PSPMV_LAUNCH(false, true);
            else
                PSPMV_LAUNCH(false, false);
#undef PSPMV_LAUNCH
            update(false, par ^ 1, PP[par ^ 1]);
        } else {
            launch_pupdate(g, par, first, pi);
            launch_spmv(g);
            update(false, par ^ 1, nullptr);
        }
        it++;
    };
    // Poll schedule: consecutive solves of an IRLS run need almost the same number of iterations,
    // so the first poll is placed where the previous solve converged and later ones every few
    // iterations (each poll drains the stream; iterations enqueued past convergence are no-ops).
    int chunk = g.stats.pcg_iters_last > 2 ? (int)std::min<int64_t>(g.stats.pcg_iters_last, maxit) : check;
    if (g.bcr_guard) chunk = 2;  // (every iteration is a direct solve: poll often)
    // Stagnation: an ill-conditioned system (weights spread over many decades, e.g. a sub-tree held
    // by one down-weighted edge) can have an attainable residual above pcg_rtol. If the residual
    // has not halved over kStallIters iterations and is at most `accept`, the iterate is taken as
    // the solution (counted in stats.pcg_stagnated) instead of running into the iteration cap --
    // the reference's direct factorisations return whatever accuracy they reach, too.
    constexpr int kStallIters = 64;
    const int ax = g.opt.pcg_stall_accept;
    const double accept = ax < 0 ? -1.0 : (ax == 0 ? 1e-6 : std::pow(10.0, -(double)ax));
    double best = HUGE_VAL;
    int best_it = 0;
    bool stagnated = false;
    bool first_poll = true;
    bool attained = false;      // refine: the residual is within pcg_rtol and no longer falls
    int met_it = -1;            // refine: the iteration at which pcg_rtol was first seen met
    double met_prev = HUGE_VAL;
    double *h_scal = g.h_scal();
    if (refine) chunk = std::min(chunk, 2);
    while (true) {
        for (int c = 0; c < chunk; c++) {
            PrecInfo pi = precondition(g, it == 0, rtol2);
            iteration_tail(pi);
        }
        chunk = (g.bcr_guard || refine) ? 1 : std::max(2, check / 2);
        // the convergence test of the last update runs in the next preconditioner prologue
        PrecInfo pi = precondition(g, it == 0, rtol2);
        const bool with_tail = tail != nullptr && first_poll;
        if (with_tail) (*tail)();  // gated on the flag that test just wrote
        read_back_state(g);
        if (with_tail && tail_ran) *tail_ran = h_flags[FL_DONE] == 1;
        first_poll = false;
        if (h_flags[FL_DONE] != 0) break;
        const double cur = std::max(h_scal[SC_RELRES], std::max(h_scal[SC_RELRES + 1], h_scal[SC_RELRES + 2]));
        if (refine && cur <= g.opt.pcg_rtol) {
            if (met_it < 0) met_it = it;
            if (!(cur < 0.5 * met_prev) || it - met_it >= kRefineExtra) {
                attained = true;
                break;
            }
            met_prev = cur;
        }
        if (cur < 0.5 * best) {
            best = cur;
            best_it = it;
        } else if (it - best_it >= kStallIters && cur <= accept) {
            stagnated = true;
            break;
        }
        if (it >= maxit) break;
        iteration_tail(pi);  // not converged: that preconditioner pass is the next iteration's
    }
    g.stats.pcg_solves += 1;
    g.stats.pcg_iters += (stagnated || attained) ? it : h_flags[FL_ITERS];
    g.stats.pcg_iters_last = (stagnated || attained) ? it : h_flags[FL_ITERS];
    for (int c = 0; c < 3; c++) g.stats.last_relres[c] = h_scal[SC_RELRES + c];
    if (h_flags[FL_DONE] == 2) return IROTAVG_ERR_SOLVER;
    if (attained) return IROTAVG_OK;
    if (stagnated) {
        g.stats.pcg_stagnated += 1;
        return IROTAVG_OK;
    }
    if (h_flags[FL_DONE] == 0) return IROTAVG_ERR_NOT_CONVERGED;
    return IROTAVG_OK;
}

// Dense-inverse refresh policy: the inverse of the coarse operator is only a preconditioner
// component, so a stale one costs PCG iterations, never accuracy, while a refresh costs about as
// much as ~25 PCG iterations. After the coarse values are refreshed, dense_is_stale() compares the
// coarse diagonal with the one the inverse was computed from; the inverse is re-used (rescaled)
// when the change is a nearly uniform factor. Depends on data only (deterministic).
int ls_solve(Graph &g, const std::function<void()> *tail, bool *tail_ran, bool direct_apply, int direct_unit) {
    if (tail_ran) *tail_ran = false;
    // no launch of K3 where the workgroups of the level-0 reduction assemble their own slices first (bcr_can_assemble): the
    // answer goes to the solve with the request, which refuses a route that disagrees with it
    BcrRequest direct;
    direct.apply = direct_apply;
    direct.unit = direct_unit;
    direct.assemble = bcr_can_assemble(bcr_shape(g));
    if (direct.assemble) {
        g.bcr_wsrc = g.dw.p;
        g.bcr_wsquare = 1;
    } else {
        assemble(g, 0, g.dw.p, g.opt.dense_always_refresh == 1);
    }
    if (g.bcr_B) {
        g.bcr_last_guarded = false;
        g.bcr_asm_fused_last = direct.assemble;
        return bcr_solve(g, direct);  // asynchronous; a non-finite result shows in the score of the step
    }
    int rc = pcg_solve(g, tail, tail_ran);
    auto failed = [&]() { return rc == IROTAVG_ERR_NOT_CONVERGED || rc == IROTAVG_ERR_SOLVER; };
    // The reference's direct solvers always return an answer. Two more attempts before an error code:
    // (1) the solve ran on a re-used or repaired coarse inverse: re-invert and solve again (a repaired inverse
    //     is exact only up to the `stale_spread` band on the entries it did not touch -- enough to stall an
    //     ill-conditioned solve: fuzz seed 31 case 511);
    // (2) a single small level: the backward-stable Cholesky solve (dense.hip, k_chol_solve).
    if (failed() && g.ndense > 0 && !g.dense_fresh) {
        assemble(g, 0, g.dw.p, true);
        rc = pcg_solve(g);
    }
    if (failed()) {
        assemble_values(g, 0, g.dw.p);  // the right-hand side again (the PCG consumed it)
        if (dense_direct_solve(g)) {
            g.stats.pcg_stagnated += 1;  // a solve accepted outside the PCG's own criterion
            rc = IROTAVG_OK;
        }
    }
    return rc;
}

__global__ __launch_bounds__(256) void k_publish(const double *__restrict__ s0, double *__restrict__ d0, int n0,
                                                 const double *__restrict__ s1, double *__restrict__ d1, int n1,
                                                 const double *__restrict__ s2, double *__restrict__ d2, int n2,
                                                 int *__restrict__ seqp, int seq) {
    for (int i = threadIdx.x; i < n0; i += 256) d0[i] = s0[i];
    for (int i = threadIdx.x; i < n1; i += 256) d1[i] = s1[i];
    for (int i = threadIdx.x; i < n2; i += 256) d2[i] = s2[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(seqp, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the host's half of a publication: a new sequence number (g.pub_seq), the pinned copy of it cleared; the kernel that
// stores it last is launched by the caller (k_publish below, or a kernel that publishes on its way)
void publish_begin(Graph &g) {
    next_seq(g.pub_seq);
    __atomic_store_n(g.h_seq(), 0, __ATOMIC_RELEASE);
}
void publish_parts(Graph &g, const PubPart *parts, int nparts) {
    PubPart p[3] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
    for (int i = 0; i < nparts && i < 3; i++) p[i] = parts[i];
    publish_begin(g);
    // (the pinned block is mapped: under unified addressing the device uses the host's pointer)
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, g.stream, p[0].src, p[0].dst, p[0].n, p[1].src, p[1].dst,
                       p[1].n, p[2].src, p[2].dst, p[2].n, g.h_seq(), g.pub_seq);
    IRH_CHECK(hipGetLastError());
}

void wait_published(Graph &g) {
    // (a pinned block that is not coherent -- the IROTAVG_PIN_DEFAULT experiment -- cannot be polled: every wait would run
    // into the 2 ms limit; env_no_poll covers both switches. Process-wide, like the pinned pool.)
    static const bool no_poll = env_no_poll();
    // (yielding after 100 us: l1ra's three polling threads on a host with few cores)
    if (no_poll || !wait_seq(g.h_seq(), 0, 1, g.pub_seq, 2e-3, 100e-6)) IRH_CHECK(hipStreamSynchronize(g.stream));
}

// score, exp map, rotation update: kernel + copy of the score partials into the pinned block (no
// synchronisation); finish_apply_step sums them once the stream has been synchronised
void launch_apply_step(Graph &g, bool gated) {
    const int n = g.nu;
    const int grid = grid_for_elems(n);
    hipLaunchKernelGGL(k_apply_step, dim3(grid), dim3(kRowBlock), 0, g.stream, n, g.f, g.ng, g.X.p,
                       g.Q.p, g.part_score.p, 1, gated ? (const int *)g.flags.p : (const int *)nullptr);
    IRH_CHECK(hipMemcpyAsync(g.h_part(), g.part_score.p, sizeof(double) * 4 * (size_t)grid,
                             hipMemcpyDeviceToHost, g.stream));
}
double finish_apply_step(Graph &g) {
    const int grid = grid_for_elems(g.nu);
    double s = 0.0;
    for (int b = 0; b < grid; b++) s += g.h_part()[4 * (size_t)b];
    g.last_score_sum = s;
    return s / (double)g.no;
}
// gated: the step is applied only if flags[FL_DONE] == 1, and the flags come back with the score (h_flags())
// behind: launches enqueued behind the publishing kernel, before the host waits for the score (they run while it does)
double apply_step(Graph &g, bool gated, const std::function<void()> *behind) {
    const int n = g.nu;
    const int grid = grid_for_elems(n);
    hipLaunchKernelGGL(k_apply_step, dim3(grid), dim3(kRowBlock), 0, g.stream, n, g.f, g.ng, g.X.p, g.Q.p,
                       g.part_score.p, 1, gated ? (const int *)g.flags.p : (const int *)nullptr);
    PubPart part[2] = {{g.part_score.p, g.h_part(), 4 * grid},
                       {reinterpret_cast<const double *>(g.flags.p), reinterpret_cast<double *>(g.h_flags()), FL_COUNT / 2}};
    publish_parts(g, part, gated ? 2 : 1);
    if (behind) (*behind)();
    wait_published(g);
    return finish_apply_step(g);
}

// ral/l1_irls.cpp:559-752
int run_irls(Graph &g, int cost, double sigma, int max_iters, double change_th, int *iters,
             double *runtime, double *trace) {
    if (cost < IROTAVG_L2 || cost > IROTAVG_WELSCH) return IROTAVG_ERR_UNKNOWN_COST;
    const double tic = now_seconds();
    double score = HUGE_VAL;
    int it = 0, rc = IROTAVG_OK;
    // weights.setOnes() (:577): by the first pass of K1 (an irls call that makes no iteration fills them here)
    if (!(score > change_th && 0 < max_iters)) fill(g, g.dw.p, (long long)g.mpad, 1.0);
    // the direct solver's plain loop (no closures, one GPU) runs the weight update and the NEXT iteration's residuals as
    // one kernel behind the step (k_weights_then_residual): er_fresh = the residual planes already belong to Q
    const bool fuse_wr = g.bcr_B && g.ng == 0 && !g.bcr_shard;
    bool er_fresh = false;
    // An iteration that is expected to be the last one skips the residual half (18 us at 2M edges that nobody would read):
    // expected = the previous step was within 50 x change_th (the iteration converges quadratically at the end: the
    // last steps of the bench's graphs are 3.5e-2 -> 1.3e-4, 1.6e-2 -> 1.3e-4, 2.5e-2 -> 3.1e-4 for change_th = 1e-3) or
    // the iteration count ends here. A wrong guess costs one separate K1 launch.
    bool with_res = true;
    const std::function<void()> wr_tail = [&]() { launch_weights_then_residual(g, cost, sigma, nullptr, with_res); };
    // ... and the ways back of its solve make the step themselves (K6 inside k_bcr_back / k_bcr_back_top, bcr.hip): the
    // score comes back as one partial sum per workgroup of those two launches
    const int ap_slots = fuse_wr ? bcr_apply_slots(g) : 0;
    while (score > change_th && it < max_iters) {  // :590, strict >
        if (!er_fresh) launch_edge_residual(g, it == 0);
        er_fresh = false;
        // Inexact outer iterations (round 5; the iterative solver only -- a direct solve has no tolerance). While the
        // outer iteration is far from its fixed point its linear system does not need pcg_rtol = 1e-10: the step of an
        // iteration is wanted to ~1 % of change_th, the quantity every decision of the loop is made on. With X of the
        // size of the LAST step (the steps shrink), a relative residual of 0.01 change_th / last step does that:
        // 7e-6 after a step of 1.4 rad, 5e-5 after 0.2 rad, capped at 1e-4; as soon as the last step is within 50 x
        // change_th -- the iteration converges quadratically there, the next step is expected below change_th, it decides
        // the stop and leaves the weights the caller gets -- and in the last iteration allowed the solve is exact again.
        // 100k views / 2M edges with 2 % loop edges: 27.8 -> 15-17 PCG iterations per solve, 13.4 -> ~10 ms per irls,
        // the same 5 outer iterations, final rotations within 5e-8 rad (mean; 5e-7 max) of the all-exact run -- the
        // reference's QR is exact in every iteration (ral/l1_irls.cpp:536-556); the north star's bar is 1e-4 rad.
        // Opt-in (options.inexact_outer = 1 or IROTAVG_INEXACT=1): by default every system is solved to pcg_rtol, like
        // the reference.
        const double rtol_keep = g.opt.pcg_rtol;
        if (!g.bcr_B && (it == 0 || score > 50.0 * change_th) && it + 1 < max_iters) {
            const bool on = g.sw.inexact >= 0 ? g.sw.inexact != 0 : g.opt.inexact_outer == 1;
            if (on) {
                const double last = it == 0 ? 1.0 : score;
                g.opt.pcg_rtol = std::max(rtol_keep, std::min(1e-4, 0.01 * change_th / last));
            }
        }
        struct Restore {
            double &r, v;
            ~Restore() { r = v; }
        } restore_rtol{g.opt.pcg_rtol, rtol_keep};
        if (g.bcr_B) {
            // banded operator: assembly of level 0, direct solve, weight and rotation update -- ~14 launches and
            // ONE host round trip (the score) per iteration
            const double score_before = score;
            with_res = !(it + 1 >= max_iters || (it > 0 && score <= 50.0 * change_th));
            // (the first system of a call is the unit-weight one, whatever the rotations: the direct solver may keep its factor)
            rc = ls_solve(g, nullptr, nullptr, ap_slots > 0, it == 0 && fuse_wr ? 1 : 0);
            if (rc != IROTAVG_OK) break;
            if (bcr_closures(g) > 0) {
                // The Woodbury correction of the closures needs the BAND part alone to be positive definite. A cost whose
                // weights reach exactly 0 (Talwar, bisquare, Andrews) can cut a view off all its band neighbours while a
                // closure still holds it: the band factor then has a dead pivot and the step would be wrong. The
                // reduction counts dead pivots; weight and rotation update are gated on "none", and the verdict comes
                // back with the score. One or more: the system is solved again by conjugate gradients on the true operator
                // (closures included), preconditioned by the regularised direct solve -- about one iteration per dead
                // pivot -- and the tail runs ungated. (ral/l1_irls.cpp:536-556 always solves the full system.)
                // (round 6) behind the gate: the step (K6, gated), then K2 and the NEXT iteration's K1 as one pass over
                // the edges (k_weights_then_residual, skipping behind the gate's verdict) whose first workgroup hands
                // score AND verdict to the host -- three launches and a copy kernel were four (K2, K6, k_publish, K1)
                const int sgrid = grid_for_elems(g.nu);
                const bool fuse_cl = fuse_wr && 4 * sgrid + 2 <= 4 * kMaxParts && !g.sw.no_fused_cl;
                if (fuse_cl) {
                    bcr_gate(g, g.part_score.p + 4 * (size_t)sgrid);
                    hipLaunchKernelGGL(k_apply_step, dim3(sgrid), dim3(kRowBlock), 0, g.stream, g.nu, g.f, g.ng, g.X.p, g.Q.p,
                                       g.part_score.p, 1, (const int *)g.flags.p);
                    const PubPart part = {g.part_score.p, g.h_part(), 4 * sgrid + 2};
                    publish_begin(g);
                    launch_weights_then_residual(g, cost, sigma, &part, with_res, bcr_gate_skip_word(g));
                    wait_published(g);
                    std::memcpy(g.h_flags(), g.h_part() + 4 * (size_t)sgrid, sizeof(int) * FL_COUNT);
                    score = finish_apply_step(g);
                    er_fresh = with_res && g.h_flags()[FL_DONE] == 1;
                } else {
                    bcr_gate(g);
                    launch_update_weights(g, cost, sigma, true);
                    score = apply_step(g, true);
                }
                if (g.h_flags()[FL_DONE] != 1) {
                    // flags[FL_ITERS] = 1: no pivot died, but the residual of the full system is above the gate (the
                    // Woodbury correction cancelled digits, bcr.hip k_bcr_gate) -- the same repair: CG on the true operator
                    // with this very solve as the preconditioner, a few iterations; what it reaches is taken
                    const bool inexact_only = g.h_flags()[FL_ITERS] == 1 && g.h_flags()[3] == 0;
                    g.stats.direct_guarded += 1;
                    g.stats.direct_dead_pivots = g.h_flags()[3];
                    {
                        // (restored on every way out, a HipError thrown inside the solve included: the handle must not
                        // keep guard mode and a 12-iteration cap for its later calls -- advisor, round 5)
                        struct GuardScope {
                            Graph &g;
                            const int64_t ds_keep;
                            const int maxit_keep;
                            ~GuardScope() {
                                g.opt.pcg_max_iters = maxit_keep;
                                g.bcr_guard = false;
                                // (the preconditioner applications of that solve are not linear systems of the caller's)
                                g.stats.direct_solves = ds_keep;
                            }
                        } guard_scope{g, g.stats.direct_solves, g.opt.pcg_max_iters};
                        g.bcr_guard = true;
                        if (inexact_only) g.opt.pcg_max_iters = 12;
                        rc = pcg_solve_classic(g);
                    }
                    g.bcr_last_guarded = true;
                    if (inexact_only && rc == IROTAVG_ERR_NOT_CONVERGED) {
                        g.stats.pcg_stagnated += 1;
                        rc = IROTAVG_OK;
                    }
                    // What those iterations reached must still be a solution (relative residual 1e-8; a first bar of 1e-6 let a
                    // run through that ended 1e-5 rad off the oracle: fuzz seed 36 case 93). Where the band part is next to singular
                    // (a thin chain whose robust weights are at their floor over whole stretches, held together by
                    // hundreds of closures: fuzz seed 22 case 69) the Woodbury solve is no approximate inverse at all and
                    // the repair stalls at 1e-3: an ERROR, rotations untouched -- such a graph belongs to the iterative
                    // solver (band_direct = -1), which the one-shot calls and ViewGraph::rotAvg then take by themselves.
                    if (rc == IROTAVG_OK && inexact_only) {
                        const double worst = std::max(g.stats.last_relres[0], std::max(g.stats.last_relres[1], g.stats.last_relres[2]));
                        if (!(worst <= kClosureRepairAccept)) rc = IROTAVG_ERR_SOLVER;
                    }
                    // (tests: the give-up path on a graph the iterative solver can take)
                    if (g.sw.bcr_fake_give_up) rc = IROTAVG_ERR_SOLVER;
                    if (rc != IROTAVG_OK) break;
                    launch_update_weights(g, cost, sigma);
                    score = apply_step(g);
                }
            } else if (fuse_wr && bcr_last_route(g).apply) {
                const PubPart part = {g.part_score.p, g.h_part(), ap_slots};
                publish_begin(g);
                launch_weights_then_residual(g, cost, sigma, &part, with_res);  // (its first workgroup publishes)
                wait_published(g);
                double ssum = 0.0;
                for (int b = 0; b < ap_slots; b++) ssum += g.h_part()[b];
                g.last_score_sum = ssum;
                score = ssum / (double)g.no;
                er_fresh = with_res;
            } else if (fuse_wr) {
                score = apply_step(g, false, &wr_tail);
                er_fresh = with_res;
            } else {
                launch_update_weights(g, cost, sigma);
                score = apply_step(g);
            }
            bcr_unit_commit(g, std::isfinite(score));
            if (!std::isfinite(score)) {
                // the single-launch upper reduction gave up on a wait (another process held its workgroups back: the
                // reservation only knows this process): its solution is NaN, no view took a step, the kernel behind it left
                // weights and residuals alone -- the iteration once more, level by level from now on
                // (whichever kernel stood behind the solve: the plain weight update skips its work behind the same word
                // as the fused weights-and-residual kernel does -- advisor round 5)
                if (bcr_up_failed(g)) {
                    er_fresh = true;  // (no view took a step: the residual planes still belong to Q)
                    score = score_before;
                    continue;
                }
                rc = IROTAVG_ERR_SOLVER;
                break;
            }
        } else if (g.cg2) {
            // The weight update and the rotation update are enqueued BEHIND the PCG before the host has
            // read its done flag, gated on that flag: convergence and score come back in one round trip
            // instead of two (each costs the GPU ~15-30 us of idling). If the solve needs more
            // iterations than predicted the gated kernels did nothing and run again, ungated.
            // ... and the staleness verdict on the dense inverse rides on the same round trip: the check runs
            // on the device (dense_check_async) and a re-inversion it asks for happens before the NEXT
            // solve (a stale inverse costs PCG iterations, never accuracy)
            // will the inverse be re-used? then the assembly's last launch also delivers the verdict on it
            g.asm_check_stale = g.ndense > 0 && g.dense_valid && !g.dense_stale_pending && g.opt.dense_always_refresh != 1;
            g.asm_check_done = false;
            assemble_values(g, 0, g.dw.p);
            g.asm_check_stale = false;
            bool spec = false;
            if (g.ndense > 0) {
                if (!g.dense_valid || g.dense_stale_pending || g.opt.dense_always_refresh == 1) {
                    dense_refresh(g);
                    g.dense_valid = true;
                    g.dense_fresh = true;
                    g.dense_stale_pending = false;
                } else {
                    if (!g.asm_check_done) dense_check_async(g);
                    g.dense_fresh = false;
                    spec = true;
                }
            }
            bool tail_ran = false;
            const std::function<void()> tail = [&]() {
                launch_update_weights(g, cost, sigma, true);
                launch_apply_step(g, true);
            };
            rc = pcg_solve_cg2(g, &tail, &tail_ran, spec);
            if (spec) {
                // 'stale' only says that the coarse operator moved away from the inverted one by more than
                // `stale_spread`; what that costs is known, too: this solve just ran with it. Re-invert for
                // the next solve only if it needed clearly more iterations than the last solve on a fresh
                // inverse did -- an inversion is worth ~10 (banded) / ~20 (dense sweep) PCG iterations and
                // IRLS typically has one or two solves left when the weights have settled this far.
                if (g.h_flags()[FL_STALE]) {
                    const int64_t slack = (g.dense_bw >= 1 && g.dense_bw <= kBandMax) ? 4 : 8;
                    g.dense_stale_pending = rc != IROTAVG_OK || g.its_fresh <= 0 ||
                                            g.stats.pcg_iters_last > g.its_fresh + slack;
                } else {
                    g.dense_scale = g.h_scal()[SC_DSCALE];
                }
            } else if (rc == IROTAVG_OK && g.ndense > 0) {
                g.its_fresh = g.stats.pcg_iters_last;
            }
            if (rc == IROTAVG_RETRY_STALE) {
                // the verdict was 'stale' AND the solve did not converge in the predicted number of
                // iterations: re-invert now and solve again from the saved right-hand side
                dense_refresh(g);
                g.dense_valid = true;
                g.dense_fresh = true;
                g.dense_stale_pending = false;
                IRH_CHECK(hipMemcpyAsync(g.levels[0].b.p, g.levels[0].x.p, sizeof(double4) * (size_t)g.levels[0].n,
                                         hipMemcpyDeviceToDevice, g.stream));
                rc = pcg_solve_cg2(g, &tail, &tail_ran, false);
                if (rc == IROTAVG_OK) g.its_fresh = g.stats.pcg_iters_last;
            }
            if ((rc == IROTAVG_ERR_NOT_CONVERGED || rc == IROTAVG_ERR_SOLVER) && g.ndense > 0 && !g.dense_fresh) {
                // ls_solve's safety net on this path, too (irotavg_hip.h: NOT_CONVERGED only after these attempts):
                // the solve ran on a re-used coarse inverse -- re-invert, restore the right-hand side and solve
                // again with the classic recurrences
                dense_refresh(g);
                g.dense_valid = true;
                g.dense_fresh = true;
                g.dense_stale_pending = false;
                IRH_CHECK(hipMemcpyAsync(g.levels[0].b.p, g.levels[0].x.p, sizeof(double4) * (size_t)g.levels[0].n,
                                         hipMemcpyDeviceToDevice, g.stream));
                tail_ran = false;
                rc = pcg_solve_classic(g);
                if (rc == IROTAVG_OK) g.its_fresh = 0;  // not comparable with a two-launch count
            }
            if (rc != IROTAVG_OK) break;
            if (tail_ran) {
                score = finish_apply_step(g);
            } else {
                launch_update_weights(g, cost, sigma);
                score = apply_step(g);
            }
        } else {
            // the same one-round-trip scheme on the classic launches: weight and rotation update ride behind the
            // first convergence test, gated on its verdict
            g.irls_settle = (!g.sw.no_settle && it > 0 && score <= 20.0 * change_th) ? score : -1.0;
            bool tail_ran = false;
            const std::function<void()> tail = [&]() {
                launch_update_weights(g, cost, sigma, true);
                launch_apply_step(g, true);
            };
            rc = ls_solve(g, &tail, &tail_ran);
            if (rc != IROTAVG_OK) break;
            if (tail_ran) {
                score = finish_apply_step(g);
            } else {
                launch_update_weights(g, cost, sigma);
                score = apply_step(g);
            }
        }
        if (trace) trace[it] = score;
        it++;
    }
    g.irls_settle = -1.0;
    IRH_CHECK(hipStreamSynchronize(g.stream));
    bcr_up_release(g);
    const double toc = now_seconds();
    *iters = it;
    *runtime = toc - tic;
    g.stats.outer_iters += it;
    g.stats.edge_updates += (int64_t)it * g.m;
    g.stats.seconds_irls += toc - tic;
    return rc;
}

// ---------------------------------------------------------------------------------------------
// kernel timing for the roofline leg of bench.py (HIP events on the handle's stream)
// ---------------------------------------------------------------------------------------------
int time_kernel(Graph &g, int which, int reps, double *ms) {
    if (which >= 100 && which < 116) {  // development aid: phase stamp (us) of k_cg_apply, see cgcg.hip
        if (!g.cg2) return IROTAVG_ERR_BAD_ARG;
        double st[16];
        const int rc = cg2_phase_stamps(g, st, 16);
        *ms = st[which - 100];
        return rc;
    }
    if (which >= 600 && which < 600 + 32 * 8) {  // development aid: stamps inside k_bcr_reduce_up (bcr_stamps_up)
        double st[32 * 8];
        const int rc = bcr_stamps_up(g, st);
        *ms = st[which - 600];
        return rc;
    }
    if (which >= 200 && which < 200 + 16 * 16) {  // development aid: phase stamps (shader clocks) of k_bcr_reduce, level
        double st[16];                             // (which - 200) / 16, chunk IROTAVG_BCR_STAMP_CHUNK, see bcr.hip
        const int rc = bcr_stamps(g, (which - 200) / 16, g.sw.bcr_stamp_chunk, st);
        *ms = st[(which - 200) % 16];
        return rc;
    }
    hipEvent_t e0, e1;
    IRH_CHECK(hipEventCreate(&e0));
    IRH_CHECK(hipEventCreate(&e1));
    bool unit_served = true;  // (17 / 18: every repetition took the right-hand-side-only route)
    auto once = [&]() {
        switch (which) {
        case 1: launch_edge_residual(g); break;
        case 2: launch_update_weights(g, IROTAVG_GEMAN_MCCLURE, 5 * IRH_PI / 180.0); break;
        case 3: assemble_values(g, 0, g.dw.p); break;  // K3 proper (no staleness test of the dense inverse)
        case 7: dense_refresh(g); break;
        case 4:
            launch_spmv(g);
            break;
        case 5: (void)precondition(g, 0, -1.0); break;
        case 8: {  // the fused p-update + SpMV of the single-GPU PCG (k_pspmv_dot)
            Level &L0 = g.levels[0];
            hipLaunchKernelGGL((k_pspmv_dot<false, false>), dim3(grid_for_rows(L0)), dim3(kRowBlock), 0, g.stream,
                               view_of(L0), __builtin_ctz((unsigned)L0.agg), g.scal.p, 0, g.part_rz.p, 1,
                               g.part_rz2.p, 1, L0.b.p, g.levels[1].y.p, g.opt.mg_omega, g.opt.mg_kc, g.P.p,
                               g.P2.p, g.AP.p, g.part_pq.p, g.flags.p);
            break;
        }
        case 9: cg2_time_once(g, 0); break;   // k_cg_apply (u = M^-1 r, w = L u) of the two-launch iteration
        case 10: cg2_time_once(g, 1); break;  // k_cg_update
        case 11: launch_weights_then_residual(g, IROTAVG_GEMAN_MCCLURE, 5 * IRH_PI / 180.0, nullptr, true); break;  // K2 + the next K1
        case 12: launch_pose_weights(g, IROTAVG_GEMAN_MCCLURE, 5 * IRH_PI / 180.0); break;  // K1 + the weights of a zero step
        case 6:
            hipLaunchKernelGGL(k_apply_step, dim3(grid_for_elems(g.nu)), dim3(kRowBlock), 0, g.stream,
                               g.nu, g.f, g.ng, g.X.p, g.Q.p, g.part_score.p, 0, (const int *)nullptr);
            break;
        default: {
            // 20 + l: reduction of level l of the banded direct solver, 40 + l: its way back, 19: a whole solve
            BcrRequest rq;
            if (which == 19) (void)bcr_solve(g);
            else if (which == 17 || which == 18) {
                // the right-hand-side-only solve over the kept unit-weight factor: all four launches / its upper launch alone
                rq.unit = which == 17 ? 2 : 3;
                rq.assemble = which == 17;
                g.bcr_wsrc = g.dw.p;
                g.bcr_wsquare = 1;
                (void)bcr_solve(g, rq);
                unit_served = unit_served && bcr_unit_last(g) == 2;
                bcr_unit_commit(g, false);
            }
            else if (which >= 20 && which < 60) {
                rq.only = which < 40 ? which - 20 : 100 + which - 40;
                (void)bcr_solve(g, rq);
            }
            break;
        }
        }
    };
    if (which == 17 || which == 18) {
        if (!g.bcr_B || !bcr_unit_valid(g)) return IROTAVG_ERR_BAD_ARG;
    } else if (which >= 19 && which < 60) {
        if (!g.bcr_B) return IROTAVG_ERR_BAD_ARG;
        const int nl = bcr_levels(g);
        if ((which >= 20 && which < 40 && which - 20 >= nl) || (which >= 40 && which - 40 >= nl)) return IROTAVG_ERR_BAD_ARG;
    } else if (which < 1 || which > 12) return IROTAVG_ERR_BAD_ARG;
    if ((which == 9 || which == 10) && !g.cg2) return IROTAVG_ERR_BAD_ARG;  // not this graph's PCG
    if (which == 8 && !(g.additive_top && g.levels.size() > 1 && g.ng == 0 && g.l0_far_entries == 0 &&
                        g.opt.no_fused_pspmv != 1))
        return IROTAVG_ERR_BAD_ARG;  // this graph's PCG does not use the fused kernel
    IRH_CHECK(hipMemsetAsync(g.flags.p, 0, sizeof(int) * FL_COUNT, g.stream));
    // kernels 11 (weights, then the next residuals) and 12 (residuals and the weights of a zero step) write the handle's
    // weights and residual planes: they are put back
    // afterwards, so that a solve or a read-back behind the timing sees what it would have seen without it
    DevBuf<double> keep_dw, keep_er;
    if (which == 11 || which == 12) {
        keep_dw.alloc((size_t)g.mpad);
        keep_er.alloc((size_t)3 * g.mpad);
        IRH_CHECK(hipMemcpyAsync(keep_dw.p, g.dw.p, sizeof(double) * (size_t)g.mpad, hipMemcpyDeviceToDevice, g.stream));
        IRH_CHECK(hipMemcpyAsync(keep_er.p, g.er.p, sizeof(double) * 3 * (size_t)g.mpad, hipMemcpyDeviceToDevice, g.stream));
    }
    once();  // warm-up
    IRH_CHECK(hipEventRecord(e0, g.stream));
    for (int r = 0; r < reps; r++) once();
    IRH_CHECK(hipEventRecord(e1, g.stream));
    if (which == 11 || which == 12) {
        IRH_CHECK(hipMemcpyAsync(g.dw.p, keep_dw.p, sizeof(double) * (size_t)g.mpad, hipMemcpyDeviceToDevice, g.stream));
        IRH_CHECK(hipMemcpyAsync(g.er.p, keep_er.p, sizeof(double) * 3 * (size_t)g.mpad, hipMemcpyDeviceToDevice, g.stream));
        IRH_CHECK(hipStreamSynchronize(g.stream));
    }
    IRH_CHECK(hipEventSynchronize(e1));
    bcr_up_release(g);
    float t = 0.f;
    IRH_CHECK(hipEventElapsedTime(&t, e0, e1));
    *ms = (double)t / std::max(reps, 1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if ((which == 17 || which == 18) && !unit_served) return IROTAVG_ERR_BAD_ARG;
    return IROTAVG_OK;
}

}  // namespace irh
