// edgediag.hip -- diagnostics of every measurement (irotavg_graph_edge_diagnostics, docs/edge_diagnostics.md).
//
// With M = A' diag(d^2) A and Sigma = M^-1 as in marginals.hip, for every edge k (u_k = row k of A):
//   edge_var[k] = u_k' Sigma u_k,  leverage[k] = d_k^2 edge_var[k] (the diagonal of the hat matrix),
//   chi2[k] = d_k^2 |r_k|^2 / (s^2 max(0, 1 - leverage[k])).
// Routes (single GPU):
//  * nu <= 2048: marginals.hip's scaled dense inverse, one gather per edge.
//  * the banded direct solver's handles: every band edge lies inside one block or two neighbouring ones, so its variance
//    is a gather from the selected inverse's blocks SD[k] = Sigma_kk, SU[k] = Sigma_k,k+1. With closures the Woodbury
//    correction G = Z S^-1 Z' is formed on the same block pattern first (k_ed_wband: SD -= G_kk, SU -= G_k,k+1), the
//    closure edges themselves (<= 2048 pairs of far-apart views) go through the multi right-hand-side pair solve.
//  * any other handle: IROTAVG_ERR_UNSUPPORTED.
// Buffers are the query's own, every sum has a fixed order, no atomics: read-only and deterministic like the variance query.
#include <algorithm>
#include <cmath>
#include <vector>

#include "graph.hpp"
#include "kernels.hpp"
#include "marginals.hpp"

namespace irh {
namespace {

int grid1(long long n) { return (int)((n + 255) / 256); }

// ---- Woodbury correction on the block pattern ------------------------------------------------------------------------
// One workgroup per window of W = 64 / B blocks (R = W B <= 64 rows from r0): T = Z_win S^-1 by 64 x 64 tiles (the
// tiling of k_mv_wcorr: thread (ty, tx) of 16 x 16 owns rows ty + 16 u, columns tx + 16 v), each tile multiplied at once
// by the matching columns of Z_c', c the R + B <= 96 rows from r0 that the window's blocks and their upper neighbours
// span: G_win (64 x 96) stays in registers, 24 entries per thread. 2 nu k^2 flops x 64 / R, + 96 / k of that for G.
__global__ __launch_bounds__(256) void k_ed_wband(int nb, int B, int W, int nrowsZ, int ld, const double *__restrict__ Z,
                                                  const double *__restrict__ Sinv, double *__restrict__ SD,
                                                  double *__restrict__ SU) {
    __shared__ double sZ[64][17], sS[16][65], sT[64][65], sC[96][17];
    const int kb0 = blockIdx.x * W, r0 = kb0 * B, R = min(W, nb - kb0) * B;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double gw[4][6] = {};
    for (int j0 = 0; j0 < ld; j0 += 64) {
        double acc[4][4] = {};
        for (int k0 = 0; k0 < ld; k0 += 16) {
            __syncthreads();
            for (int e = threadIdx.x; e < 64 * 16; e += 256) {
                const int zr = r0 + (e >> 4);
                sZ[e >> 4][e & 15] = zr < nrowsZ ? Z[(size_t)zr * ld + k0 + (e & 15)] : 0.0;
                sS[e >> 6][e & 63] = Sinv[(size_t)(k0 + (e >> 6)) * ld + j0 + (e & 63)];
            }
            __syncthreads();
            for (int kk = 0; kk < 16; kk++) {
                double zr[4], sc[4];
                for (int u = 0; u < 4; u++) zr[u] = sZ[ty + 16 * u][kk];
                for (int u = 0; u < 4; u++) sc[u] = sS[kk][tx + 16 * u];
                for (int u = 0; u < 4; u++)
                    for (int v = 0; v < 4; v++) acc[u][v] += zr[u] * sc[v];
            }
        }
        // (every thread is past the previous tile's reads of sT: the loop above has barriers)
        for (int u = 0; u < 4; u++)
            for (int v = 0; v < 4; v++) sT[ty + 16 * u][tx + 16 * v] = acc[u][v];
        for (int k0 = 0; k0 < 64; k0 += 16) {
            __syncthreads();
            for (int e = threadIdx.x; e < 96 * 16; e += 256) {
                const int zr = r0 + (e >> 4);
                sC[e >> 4][e & 15] = zr < nrowsZ ? Z[(size_t)zr * ld + j0 + k0 + (e & 15)] : 0.0;
            }
            __syncthreads();
            for (int kk = 0; kk < 16; kk++) {
                double tr[4], zc[6];
                for (int u = 0; u < 4; u++) tr[u] = sT[ty + 16 * u][k0 + kk];
                for (int v = 0; v < 6; v++) zc[v] = sC[tx + 16 * v][kk];
                for (int u = 0; u < 4; u++)
                    for (int v = 0; v < 6; v++) gw[u][v] += tr[u] * zc[v];
            }
        }
    }
    const size_t BB = (size_t)B * B;
    for (int u = 0; u < 4; u++) {
        const int row = ty + 16 * u;
        if (row >= R) continue;
        const int gr = r0 + row, kb = gr / B, rr = gr - kb * B;
        for (int v = 0; v < 6; v++) {
            const int gc = r0 + tx + 16 * v, kc = gc / B, cc = gc - kc * B;
            if (kc >= nb) continue;
            if (kc == kb) SD[kb * BB + (size_t)rr * B + cc] -= gw[u][v];
            else if (kc == kb + 1) SU[kb * BB + (size_t)rr * B + cc] -= gw[u][v];
        }
    }
}

// ---- the pass over the edges -------------------------------------------------------------------------------------------
// u' Sigma u of an edge from the blocks of the (corrected) selected inverse; a, b: the rows of the +1 / -1 coefficient
// (-1: none). far: the rows lie two or more blocks apart (a closure; its value comes from the pair solve).
__device__ __forceinline__ double band_usu(int a, int b, int B, const double *__restrict__ SD,
                                           const double *__restrict__ SU, bool *far) {
    const size_t BB = (size_t)B * B;
    const int ka = a >= 0 ? a / B : 0, ra = a - ka * B, kb = b >= 0 ? b / B : 0, rb = b - kb * B;
    double v = 0.0;
    if (a >= 0) v += SD[ka * BB + (size_t)ra * B + ra];
    if (b >= 0) v += SD[kb * BB + (size_t)rb * B + rb];
    if (a >= 0 && b >= 0) {
        if (ka == kb) v -= 2.0 * SD[ka * BB + (size_t)ra * B + rb];
        else if (kb == ka + 1) v -= 2.0 * SU[ka * BB + (size_t)ra * B + rb];
        else if (ka == kb + 1) v -= 2.0 * SU[kb * BB + (size_t)rb * B + ra];
        else *far = true;
    }
    return v;
}

// k_mv_dense_pairs' formula: S the inverse of the Jacobi-scaled operator, sc the scaling
__device__ __forceinline__ double dense_usu(int a, int b, int npad, const double *__restrict__ S,
                                            const double *__restrict__ sc) {
    double v = 0.0;
    if (a >= 0) v += S[(size_t)a * npad + a] * sc[a] * sc[a];
    if (b >= 0) v += S[(size_t)b * npad + b] * sc[b] * sc[b];
    if (a >= 0 && b >= 0) v -= (S[(size_t)a * npad + b] + S[(size_t)b * npad + a]) * sc[a] * sc[b];
    return v;
}

__device__ __forceinline__ double chi_of(double w, double x, double y, double z, double s2, double lev) {
    return w * (x * x + y * y + z * z) / (s2 * fmax(0.0, 1.0 - lev));
}

// Two consecutive edges per thread, every stream read and written as one 16-byte (the flags: 2-byte) access; the streams
// are padded to mpad (a multiple of 64), the outputs likewise. BP = B (band) or npad (dense), S2 = SU or sc.
// An output that was not asked for is a null pointer. er: the query's own residual planes (chi2 only).
template <bool kDense>
__global__ __launch_bounds__(256) void k_ed_edges(long long mpad, int f, int BP, const int2 *__restrict__ ei,
                                                  const int2 *__restrict__ ej, const uchar2 *__restrict__ eflag,
                                                  const double2 *__restrict__ dw, const double *__restrict__ er,
                                                  const double *__restrict__ S1, const double *__restrict__ S2, double s2,
                                                  double2 *__restrict__ ev, double2 *__restrict__ lev,
                                                  double2 *__restrict__ chi, int *__restrict__ dead) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (2 * t >= mpad) return;
    const int2 i2 = ei[t], j2 = ej[t];
    const uchar2 fl = eflag[t];
    const double2 d = dw[t];
    const int a0 = (fl.x & EF_CJ) ? j2.x - f : -1, b0 = (fl.x & EF_CI) ? i2.x - f : -1;
    const int a1 = (fl.y & EF_CJ) ? j2.y - f : -1, b1 = (fl.y & EF_CI) ? i2.y - f : -1;
    bool far0 = false, far1 = false;
    double v0, v1;
    if (kDense) {
        v0 = dense_usu(a0, b0, BP, S1, S2);
        v1 = dense_usu(a1, b1, BP, S1, S2);
    } else {
        v0 = band_usu(a0, b0, BP, S1, S2, &far0);
        v1 = band_usu(a1, b1, BP, S1, S2, &far1);
    }
    if (far0) v0 = 0.0;  // k_ed_closures writes these
    if (far1) v1 = 0.0;
    if (!(fabs(v0) < INFINITY) || !(fabs(v1) < INFINITY)) dead[0] = 1;
    const double w0 = d.x * d.x, w1 = d.y * d.y, l0 = w0 * v0, l1 = w1 * v1;
    if (ev) ev[t] = make_double2(v0, v1);
    if (lev) lev[t] = make_double2(l0, l1);
    if (chi) {
        const double2 x = reinterpret_cast<const double2 *>(er)[t];
        const double2 y = reinterpret_cast<const double2 *>(er + mpad)[t];
        const double2 z = reinterpret_cast<const double2 *>(er + 2 * mpad)[t];
        chi[t] = make_double2(chi_of(w0, x.x, y.x, z.x, s2, l0), chi_of(w1, x.y, y.y, z.y, s2, l1));
    }
}

// the closure edges: pv from the pair solve (one thread each)
__global__ __launch_bounds__(256) void k_ed_closures(int nf, long long mpad, const int *__restrict__ fe,
                                                     const double *__restrict__ pv, const double *__restrict__ dw,
                                                     const double *__restrict__ er, double s2, double *__restrict__ ev,
                                                     double *__restrict__ lev, double *__restrict__ chi,
                                                     int *__restrict__ dead) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nf) return;
    const int k = fe[t];
    const double v = pv[t], w = dw[k] * dw[k], l = w * v;
    if (!(fabs(v) < INFINITY)) dead[0] = 1;
    if (ev) ev[k] = v;
    if (lev) lev[k] = l;
    if (chi) chi[k] = chi_of(w, er[k], er[mpad + k], er[2 * mpad + k], s2, l);
}

}  // namespace

int edge_diagnostics(Graph &g, double *edge_var, double *leverage, double *chi2, double *scale, bool dev_out) {
    if (g.ng != 0 || g.is_clone || g.levels.empty()) return IROTAVG_ERR_UNSUPPORTED;
    const bool dense = g.no <= 2048, band = !dense && g.bcr_B > 0;
    if (!dense && !band) return IROTAVG_ERR_UNSUPPORTED;  // no factorisation to read all edges off
    const bool arrays = edge_var || leverage || chi2;
    BandFactor F;
    BandClosures C;
    DenseInverse Dn;
    DevBuf<int> dead;
    const int rc = dense ? dense_inverse(g, Dn, dead) : band_setup(g, F, C, dead);
    if (rc != IROTAVG_OK) return rc;
    if (band && arrays) {
        F.select(g);
        if (C.k > 0) {
            const int W = std::max(1, 64 / F.B);
            hipLaunchKernelGGL(k_ed_wband, dim3((F.nb + W - 1) / W), dim3(256), 0, g.stream, F.nb, F.B, W, C.nrowsZ, C.ldZ,
                               C.Z.p, C.S.p, F.D.p, F.U.p);
        }
    }
    DevBuf<double> er;  // the residual planes s^2 was formed from, kept for chi2
    double num = 0.0, cnt = 0.0;
    const double s2 = (chi2 || scale) ? residual_scale(g, &num, &cnt, chi2 ? &er : nullptr) : 0.0;
    if (arrays) {
        DevBuf<double> dev, dlev, dchi;
        if (edge_var) dev.alloc((size_t)g.mpad);
        if (leverage) dlev.alloc((size_t)g.mpad);
        if (chi2) dchi.alloc((size_t)g.mpad);
        const int grid = grid1(g.mpad / 2);
        auto launch = [&](auto kern, int BP, const double *S1, const double *S2) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, g.stream, (long long)g.mpad, g.f, BP,
                               reinterpret_cast<const int2 *>(g.ei.p), reinterpret_cast<const int2 *>(g.ej.p),
                               reinterpret_cast<const uchar2 *>(g.eflag.p), reinterpret_cast<const double2 *>(g.dw.p),
                               er.p, S1, S2, s2, reinterpret_cast<double2 *>(dev.p), reinterpret_cast<double2 *>(dlev.p),
                               reinterpret_cast<double2 *>(dchi.p), dead.p);
        };
        if (dense) launch(k_ed_edges<true>, Dn.npad, Dn.M.p, Dn.sc.p);
        else launch(k_ed_edges<false>, F.B, F.D.p, F.U.p);
        if (band && !g.bcr_far_e.empty()) {
            const int nf = (int)g.bcr_far_e.size();
            std::vector<double> pv;
            band_pairs(g, F, C, g.bcr_far_j, g.bcr_far_i, pv);
            DevBuf<int> fe;
            DevBuf<double> dpv;
            fe.upload(g.bcr_far_e, g.stream);
            dpv.upload(pv, g.stream);
            hipLaunchKernelGGL(k_ed_closures, dim3(grid1(nf)), dim3(256), 0, g.stream, nf, (long long)g.mpad, fe.p, dpv.p,
                               g.dw.p, er.p, s2, dev.p, dlev.p, dchi.p, dead.p);
            if (read_dead(g, dead)) return IROTAVG_ERR_SOLVER;  // (also keeps fe / dpv alive until the kernel has run)
        } else if (read_dead(g, dead)) {
            return IROTAVG_ERR_SOLVER;
        }
        // Both edge kernels raise the dead-pivot word in the very pass that writes the arrays, on every route: the
        // caller's arrays -- host or device -- are filled from the query's own buffers once that word has been read.
        const size_t bytes = sizeof(double) * (size_t)g.m;
        const hipMemcpyKind kind = dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (edge_var) IRH_CHECK(hipMemcpyAsync(edge_var, dev.p, bytes, kind, g.stream));
        if (leverage) IRH_CHECK(hipMemcpyAsync(leverage, dlev.p, bytes, kind, g.stream));
        if (chi2) IRH_CHECK(hipMemcpyAsync(chi2, dchi.p, bytes, kind, g.stream));
        IRH_CHECK(hipStreamSynchronize(g.stream));
    }
    if (scale) *scale = s2;
    return IROTAVG_OK;
}

}  // namespace irh
