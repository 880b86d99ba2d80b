// marginals.hip -- uncertainty of the IRLS solution (irotavg_graph_rotation_variance, docs/rotation_variance.md).
//
// M = A' diag(d^2) A (the operator of the IRLS linear system, make_A's rows incl. the edge-drop quirk of
// ral/l1_irls.cpp:770-771), Sigma = M^-1. The query returns diag(Sigma) (marginal variances), u' Sigma u for pairs
// u = e_i - e_j (relative variances) and the residual variance s^2 of the reference's least-squares problem.
//
// Routes (single GPU):
//  * nu <= 2048: M assembled densely from the level-0 adjacency and the current weights, inverted by dense_invert_spd.
//  * the banded direct solver's handles (bcr_B > 0): M = A_b + V C V', A_b block tridiagonal (blocks of bcr_B rows),
//    V = [e_p - e_q] over the loop closures bcr_far_*, C = diag(d^2) of those edges. A_b is reduced by odd-even block
//    cyclic reduction that KEEPS D_i^-1 and G = D_i^-1 A_i{a,c}; a downward sweep (selected inversion, Takahashi) gives
//    the diagonal and adjacent blocks of A_b^-1; Woodbury: Z = A_b^-1 V (multi right-hand side solve through the same
//    factor), S = C^-1 + V'Z, diag(Sigma) = diag(A_b^-1) - rowsum((Z S^-1) o Z).
//  * any other (multigrid-PCG) handle: pairs only, each u solved by the handle's own PCG on a solver clone; marginals
//    IROTAVG_ERR_UNSUPPORTED.
// Everything runs on buffers of the query's own: the handle's matrix values, right-hand side, X, dense inverse, its
// reuse bookkeeping and the residual planes are as before the call. Every sum has a fixed order (no atomics).
#include <algorithm>
#include <cmath>
#include <vector>

#include "graph.hpp"
#include "kernels.hpp"
#include "marginals.hpp"

namespace irh {
namespace {

constexpr int kT = 33;           // LDS row stride of a block (B <= 32)
constexpr double kPivTol = 1e-13;  // dead pivot: not above this x the row's diagonal in A_b (the direct solver's rule)

// ---- assembly ----------------------------------------------------------------------------------------------------
// One thread per row walks the row's level-0 entries (SELL, fixed order) and boundary slots. Dense form: row r of M.
__global__ __launch_bounds__(256) void k_mv_dense_assemble(int n, int npad, const int *__restrict__ sl_off,
                                                           const int *__restrict__ col, const uint32_t *__restrict__ slot_eid,
                                                           const int *__restrict__ bptr, const uint32_t *__restrict__ beid,
                                                           const uint8_t *__restrict__ bflag, const double *__restrict__ d,
                                                           double *__restrict__ M) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= npad) return;
    double *row = M + (size_t)r * npad;
    if (r >= n) {
        row[r] = 1.0;
        return;
    }
    const int sl = r >> 6, lane = r & 63, o0 = sl_off[sl], w = sl_off[sl + 1] - o0;
    double dg = 0.0;
    for (int k = 0; k < w; k++) {
        const size_t pos = sell_pos(o0, k, lane);
        const uint32_t se = slot_eid[pos];
        if (se == 0xffffffffu) continue;
        const double de = d[se >> 1], wk = de * de;
        row[col[pos]] -= wk;
        dg += wk;
    }
    for (int s = bptr[r]; s < bptr[r + 1]; s++) {
        if (!(bflag[s] & BF_IRLS)) continue;
        const double de = d[beid[s] >> 1];
        dg += de * de;
    }
    row[r] += dg;
}

// Band form: diagonal block D[r/B] and upper coupling U[r/B] (to block r/B + 1), row-major B x B each; entries of a
// block distance >= 2 are the closures (Woodbury part) and are left out, their weight included.
__global__ __launch_bounds__(256) void k_mv_band_assemble(int n, int B, int nrows, const int *__restrict__ sl_off,
                                                          const int *__restrict__ col, const uint32_t *__restrict__ slot_eid,
                                                          const int *__restrict__ bptr, const uint32_t *__restrict__ beid,
                                                          const uint8_t *__restrict__ bflag, const double *__restrict__ d,
                                                          double *__restrict__ D, double *__restrict__ U,
                                                          double *__restrict__ orig) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    const int kb = r / B, rr = r - kb * B;
    double *Dr = D + (size_t)kb * B * B + (size_t)rr * B;
    if (r >= n) {
        Dr[rr] = 1.0;
        orig[r] = 1.0;
        return;
    }
    double *Ur = U + (size_t)kb * B * B + (size_t)rr * B;
    const int sl = r >> 6, lane = r & 63, o0 = sl_off[sl], w = sl_off[sl + 1] - o0;
    double dg = 0.0;
    for (int k = 0; k < w; k++) {
        const size_t pos = sell_pos(o0, k, lane);
        const uint32_t se = slot_eid[pos];
        if (se == 0xffffffffu) continue;
        const int c = col[pos], kc = c / B;
        if (kc > kb + 1 || kc < kb - 1) continue;  // a closure
        const double de = d[se >> 1], wk = de * de;
        if (kc == kb) Dr[c - kc * B] -= wk;
        else if (kc == kb + 1) Ur[c - kc * B] -= wk;
        dg += wk;
    }
    for (int s = bptr[r]; s < bptr[r + 1]; s++) {
        if (!(bflag[s] & BF_IRLS)) continue;
        const double de = d[beid[s] >> 1];
        dg += de * de;
    }
    Dr[rr] += dg;
    orig[r] = dg;
}

// ---- LDS block helpers (256 threads; entry e = tid + 256 q of a B x B block, q < 4) ----------------------------------
__device__ __forceinline__ void blk_load(double (*s)[kT], const double *__restrict__ g, int B) {
    for (int e = threadIdx.x; e < B * B; e += 256) s[e / B][e % B] = g ? g[e] : 0.0;
}

// ---- odd-even block cyclic reduction that keeps D_i^-1 ---------------------------------------------------------------
// Level with stride s: block i = s + 2 s x (eliminated) between a = i - s and c = i + s (when < nb). Couplings: A_ai =
// U[a], A_ic = U[i]. Stores Dinv_i, Ga_i = Dinv_i A_ia = Dinv_i U[a]', Gc_i = Dinv_i U[i]. top: block 0 alone.
__global__ __launch_bounds__(256) void k_mv_elim(int nb, int B, int s, int top, const double *__restrict__ D,
                                                 const double *__restrict__ U, double *__restrict__ Dinv,
                                                 double *__restrict__ Ga, double *__restrict__ Gc,
                                                 const double *__restrict__ orig, int *__restrict__ dead) {
    __shared__ double sD[32][kT], sA[32][kT], sC[32][kT];
    const int i = top ? 0 : s + blockIdx.x * 2 * s;
    const int a = top ? -1 : i - s;
    const bool hasc = !top && i + s < nb;
    const size_t BB = (size_t)B * B;
    blk_load(sD, D + i * BB, B);
    blk_load(sA, a >= 0 ? U + a * BB : nullptr, B);
    blk_load(sC, hasc ? U + i * BB : nullptr, B);
    __syncthreads();
    // in-place Gauss-Jordan (SPD: no pivoting); every thread reads the pivot row / column before anyone writes
    for (int p = 0; p < B; p++) {
        const double piv = sD[p][p];
        const double thr = kPivTol * orig[(size_t)i * B + p];
        if (!(piv > thr) && threadIdx.x == 0) dead[0] = 1;
        const double ip = 1.0 / piv;
        double nv[4];
        int q = 0;
        for (int e = threadIdx.x; e < B * B; e += 256, q++) {
            const int r = e / B, c = e % B;
            if (r == p && c == p) nv[q] = ip;
            else if (r == p) nv[q] = sD[p][c] * ip;
            else if (c == p) nv[q] = -sD[r][p] * ip;
            else nv[q] = sD[r][c] - sD[r][p] * sD[p][c] * ip;
        }
        __syncthreads();
        q = 0;
        for (int e = threadIdx.x; e < B * B; e += 256, q++) sD[e / B][e % B] = nv[q];
        __syncthreads();
    }
    for (int e = threadIdx.x; e < B * B; e += 256) {
        const int r = e / B, c = e % B;
        double ga = 0.0, gc = 0.0;
        for (int t = 0; t < B; t++) {
            ga += sD[r][t] * sA[c][t];
            gc += sD[r][t] * sC[t][c];
        }
        Dinv[i * BB + e] = sD[r][c];
        Ga[i * BB + e] = ga;
        Gc[i * BB + e] = gc;
    }
}

// survivors a = 2 s x: D_a -= U[a] Ga[a+s] + U[a-s]' Gc[a-s]; U[a] <- -U[a] Gc[a+s] (the coupling to a + 2 s)
__global__ __launch_bounds__(256) void k_mv_update(int nb, int B, int s, double *__restrict__ D, double *__restrict__ U,
                                                   const double *__restrict__ Ga, const double *__restrict__ Gc) {
    __shared__ double sU[32][kT], sGa[32][kT], sGc[32][kT], sUl[32][kT], sGl[32][kT];
    const int a = blockIdx.x * 2 * s;
    const bool hr = a + s < nb, hl = a >= s;
    const size_t BB = (size_t)B * B;
    blk_load(sU, U + a * BB, B);
    blk_load(sGa, hr ? Ga + (a + s) * BB : nullptr, B);
    blk_load(sGc, hr ? Gc + (a + s) * BB : nullptr, B);
    blk_load(sUl, hl ? U + (a - s) * BB : nullptr, B);
    blk_load(sGl, hl ? Gc + (a - s) * BB : nullptr, B);
    __syncthreads();
    for (int e = threadIdx.x; e < B * B; e += 256) {
        const int r = e / B, c = e % B;
        double t = 0.0, u = 0.0;
        for (int k = 0; k < B; k++) {
            t += sU[r][k] * sGa[k][c];
            u += sU[r][k] * sGc[k][c];
        }
        double l = 0.0;
        for (int k = 0; k < B; k++) l += sUl[k][r] * sGl[k][c];
        D[a * BB + e] -= t + l;
        U[a * BB + e] = -u;
    }
}

// ---- downward sweep: selected inversion --------------------------------------------------------------------------
// SD[k] = Sigma_kk, SU[k] = Sigma_{k, next active block} of the level. For eliminated i between a and c:
//   Sigma_ia = -(Ga Sigma_aa + Gc Sigma_ca), Sigma_ic = -(Ga Sigma_ac + Gc Sigma_cc),
//   Sigma_ii = Dinv_i - Ga Sigma_ai - Gc Sigma_ci.
__global__ __launch_bounds__(256) void k_mv_down(int nb, int B, int s, const double *__restrict__ Dinv,
                                                 const double *__restrict__ Ga, const double *__restrict__ Gc,
                                                 double *__restrict__ SD, double *__restrict__ SU) {
    __shared__ double sGa[32][kT], sGc[32][kT], sA[32][kT], sC[32][kT], sX[32][kT];
    const int i = s + blockIdx.x * 2 * s, a = i - s, c = i + s;
    const bool hasc = c < nb;
    const size_t BB = (size_t)B * B;
    blk_load(sGa, Ga + i * BB, B);
    blk_load(sGc, hasc ? Gc + i * BB : nullptr, B);
    blk_load(sA, SD + a * BB, B);
    blk_load(sC, hasc ? SD + c * BB : nullptr, B);
    blk_load(sX, hasc ? SU + a * BB : nullptr, B);  // Sigma_ac
    __syncthreads();
    double P[4], Q[4];
    int q = 0;
    for (int e = threadIdx.x; e < B * B; e += 256, q++) {
        const int r = e / B, cc = e % B;
        double p = 0.0, x = 0.0;
        for (int t = 0; t < B; t++) {
            p += sGa[r][t] * sA[t][cc] + sGc[r][t] * sX[cc][t];
            x += sGa[r][t] * sX[t][cc] + sGc[r][t] * sC[t][cc];
        }
        P[q] = -p;
        Q[q] = -x;
    }
    __syncthreads();
    q = 0;
    for (int e = threadIdx.x; e < B * B; e += 256, q++) {
        sA[e / B][e % B] = P[q];
        sC[e / B][e % B] = Q[q];
    }
    __syncthreads();
    q = 0;
    for (int e = threadIdx.x; e < B * B; e += 256, q++) {
        const int r = e / B, cc = e % B;
        double v = Dinv[i * BB + e];
        for (int t = 0; t < B; t++) v -= sGa[r][t] * sA[cc][t] + sGc[r][t] * sC[cc][t];
        SD[i * BB + e] = v;
        if (hasc) SU[i * BB + e] = Q[q];
        SU[a * BB + (size_t)cc * B + r] = P[q];  // Sigma_ai = Sigma_ia'
    }
}

// ---- multi right-hand-side solve through the factor (Y: nb B rows x ld columns, row-major) --------------------------
// survivors a: b_a -= Ga[a+s]' b_{a+s} + Gc[a-s]' b_{a-s}; 64 columns per workgroup (blockIdx.y)
__global__ __launch_bounds__(256) void k_mv_fwd(int nb, int B, int s, int ld, const double *__restrict__ Ga,
                                                const double *__restrict__ Gc, double *__restrict__ Y) {
    __shared__ double sG[32][kT], sY[32][65];
    const int a = blockIdx.x * 2 * s, c0 = blockIdx.y * 64, cc = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const size_t BB = (size_t)B * B;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int side = 0; side < 2; side++) {
        const int nbk = side == 0 ? a + s : a - s;
        if (side == 0 ? nbk >= nb : a < s) continue;
        __syncthreads();
        blk_load(sG, (side == 0 ? Ga : Gc) + nbk * BB, B);
        for (int r = r0; r < B; r += 4) sY[r][cc] = Y[((size_t)nbk * B + r) * ld + c0 + cc];
        __syncthreads();
        for (int q = 0; q < B / 4; q++) {
            const int r = r0 + 4 * q;
            double t = 0.0;
            for (int k = 0; k < B; k++) t += sG[k][r] * sY[k][cc];
            acc[q] += t;
        }
    }
    for (int q = 0; q < B / 4; q++) Y[((size_t)a * B + r0 + 4 * q) * ld + c0 + cc] -= acc[q];
}

// eliminated i (top: block 0): x_i = Dinv_i b_i - Ga_i x_a - Gc_i x_c
__global__ __launch_bounds__(256) void k_mv_bwd(int nb, int B, int s, int top, int ld, const double *__restrict__ Dinv,
                                                const double *__restrict__ Ga, const double *__restrict__ Gc,
                                                double *__restrict__ Y) {
    __shared__ double sG[32][kT], sY[32][65];
    const int i = top ? 0 : s + blockIdx.x * 2 * s;
    const int c0 = blockIdx.y * 64, cc = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const size_t BB = (size_t)B * B;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int part = 0; part < 3; part++) {
        const int blk = part == 0 ? i : (part == 1 ? i - s : i + s);
        if (part > 0 && (top || blk >= nb)) continue;
        const double *G = part == 0 ? Dinv : (part == 1 ? Ga : Gc);
        __syncthreads();
        blk_load(sG, G + i * BB, B);
        for (int r = r0; r < B; r += 4) sY[r][cc] = Y[((size_t)blk * B + r) * ld + c0 + cc];
        __syncthreads();
        const double sg = part == 0 ? 1.0 : -1.0;
        for (int q = 0; q < B / 4; q++) {
            const int r = r0 + 4 * q;
            double t = 0.0;
            for (int k = 0; k < B; k++) t += sG[r][k] * sY[k][cc];
            acc[q] += sg * t;
        }
    }
    __syncthreads();  // every read of b_i is done
    for (int q = 0; q < B / 4; q++) Y[((size_t)i * B + r0 + 4 * q) * ld + c0 + cc] = acc[q];
}

// column c of Y = e_p - e_q (rows; -1: no entry)
__global__ __launch_bounds__(256) void k_mv_rhs(int ncol, int ld, const int *__restrict__ p, const int *__restrict__ q,
                                                double *__restrict__ Y) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncol) return;
    if (p[c] >= 0) Y[(size_t)p[c] * ld + c] = 1.0;
    if (q[c] >= 0) Y[(size_t)q[c] * ld + c] = -1.0;
}

// ---- Woodbury -----------------------------------------------------------------------------------------------------
// S = C^-1 + V'Z (symmetrised), npad x npad, padding = identity
__global__ __launch_bounds__(256) void k_mv_wsys(int k, int npad, int ld, const int *__restrict__ p,
                                                 const int *__restrict__ q, const double *__restrict__ cinv,
                                                 const double *__restrict__ Z, double *__restrict__ S) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)npad * npad) return;
    const int r = (int)(t / npad), c = (int)(t % npad);
    double v;
    if (r >= k || c >= k) {
        v = r == c ? 1.0 : 0.0;
    } else {
        const double a = Z[(size_t)p[r] * ld + c] - Z[(size_t)q[r] * ld + c];
        const double b = Z[(size_t)p[c] * ld + r] - Z[(size_t)q[c] * ld + r];
        v = 0.5 * (a + b) + (r == c ? cinv[r] : 0.0);
    }
    S[t] = v;
}

// corr[r] = sum_{c1,c2} Z[r][c1] Sinv[c1][c2] Z[r][c2] (= rowsum((Z Sinv) o Z)); 64 rows per workgroup, 2 n k^2 flops.
// Thread (ty, tx) of 16 x 16 owns rows ty + 16 i and columns tx + 16 j of each 64 x 64 tile of Z Sinv.
__global__ __launch_bounds__(256) void k_mv_wcorr(int ld, const double *__restrict__ Z, const double *__restrict__ Sinv,
                                                  int ldS, double *__restrict__ corr) {
    __shared__ double sZ[64][17], sS[16][65], red[64][17];
    const int r0 = blockIdx.x * 64, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double part[4] = {0, 0, 0, 0};
    for (int j0 = 0; j0 < ld; j0 += 64) {
        double acc[4][4] = {};
        for (int k0 = 0; k0 < ld; k0 += 16) {
            __syncthreads();
            for (int e = threadIdx.x; e < 64 * 16; e += 256) {
                sZ[e >> 4][e & 15] = Z[(size_t)(r0 + (e >> 4)) * ld + k0 + (e & 15)];
                sS[e >> 6][e & 63] = Sinv[(size_t)(k0 + (e >> 6)) * ldS + j0 + (e & 63)];
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
        for (int u = 0; u < 4; u++)
            for (int v = 0; v < 4; v++) part[u] += acc[u][v] * Z[(size_t)(r0 + ty + 16 * u) * ld + j0 + tx + 16 * v];
    }
    __syncthreads();
    for (int u = 0; u < 4; u++) red[ty + 16 * u][tx] = part[u];
    __syncthreads();
    if (threadIdx.x < 64) {
        double t = 0.0;
        for (int x = 0; x < 16; x++) t += red[threadIdx.x][x];
        corr[r0 + threadIdx.x] = t;
    }
}

// var[r] = SD diag - corr (corr may be null); negative / non-finite -> dead
__global__ __launch_bounds__(256) void k_mv_band_var(int n, int B, const double *__restrict__ SD,
                                                     const double *__restrict__ corr, double *__restrict__ var,
                                                     int *__restrict__ dead) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int kb = r / B, rr = r - kb * B;
    double v = SD[(size_t)kb * B * B + (size_t)rr * B + rr];
    if (corr) v -= corr[r];
    if (!(v > 0.0) || !(v < INFINITY)) dead[0] = 1;
    var[r] = v;
}

// sc: the symmetric scaling the matrix was inverted under (Sigma = diag(sc) S diag(sc)), or null
__global__ __launch_bounds__(256) void k_mv_dense_var(int n, int npad, const double *__restrict__ S,
                                                      const double *__restrict__ sc, double *__restrict__ var,
                                                      int *__restrict__ dead) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double v = S[(size_t)r * npad + r] * (sc ? sc[r] * sc[r] : 1.0);
    if (!(v > 0.0) || !(v < INFINITY)) dead[0] = 1;
    var[r] = v;
}

// pairs on the dense inverse: Sigma_ii + Sigma_jj - 2 Sigma_ij, rows of fixed views dropped (-1)
__global__ __launch_bounds__(256) void k_mv_dense_pairs(int np, int npad, const int *__restrict__ pi,
                                                        const int *__restrict__ pj, const double *__restrict__ S,
                                                        const double *__restrict__ sc, double *__restrict__ pv) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= np) return;
    const int i = pi[t], j = pj[t];
    double v = 0.0;
    if (i >= 0) v += S[(size_t)i * npad + i] * sc[i] * sc[i];
    if (j >= 0) v += S[(size_t)j * npad + j] * sc[j] * sc[j];
    if (i >= 0 && j >= 0) v -= (S[(size_t)i * npad + j] + S[(size_t)j * npad + i]) * sc[i] * sc[j];
    pv[t] = v;
}

// Jacobi scaling of the dense operator: sc = diag^-1/2, M <- diag(sc) M diag(sc). Unit diagonal makes
// dense_invert_spd's dead-pivot rule (1e-13 x the largest diagonal entry) the row's own: a pivot of the scaled
// elimination is the original one over the row's diagonal. A zero diagonal (a view without a weighted edge) is dead.
__global__ __launch_bounds__(256) void k_mv_dense_diag(int npad, const double *__restrict__ M, double *__restrict__ sc,
                                                       int *__restrict__ dead) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= npad) return;
    const double d = M[(size_t)r * npad + r];
    if (!(d > 0.0)) dead[0] = 1;
    sc[r] = d > 0.0 ? 1.0 / sqrt(d) : 1.0;
}
__global__ __launch_bounds__(256) void k_mv_dense_scale(int npad, double *__restrict__ M, const double *__restrict__ sc) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)npad * npad) return;
    const int r = (int)(t / npad), c = (int)(t % npad);
    M[t] = r == c ? 1.0 : M[t] * sc[r] * sc[c];  // (called once every diagonal entry is positive)
}

// pairs on the band path, one workgroup per pair (column t of Y = A_b^-1 u):
// u' A_b^-1 u - (V'y)' S^-1 (V'y)
__global__ __launch_bounds__(256) void k_mv_band_pairs(int ldY, const int *__restrict__ pi, const int *__restrict__ pj,
                                                       const double *__restrict__ Y, int k, const int *__restrict__ cp,
                                                       const int *__restrict__ cq, const double *__restrict__ Sinv,
                                                       int ldS, double *__restrict__ pv) {
    __shared__ double vy[2048];
    __shared__ double red[256];
    const int t = blockIdx.x, i = pi[t], j = pj[t];
    for (int c = threadIdx.x; c < k; c += 256)
        vy[c] = Y[(size_t)cp[c] * ldY + t] - Y[(size_t)cq[c] * ldY + t];
    __syncthreads();
    double part = 0.0;
    for (int c = threadIdx.x; c < k; c += 256) {
        double x = 0.0;
        for (int c2 = 0; c2 < k; c2++) x += Sinv[(size_t)c * ldS + c2] * vy[c2];
        part += vy[c] * x;
    }
    red[threadIdx.x] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double v = 0.0;
        if (i >= 0) v += Y[(size_t)i * ldY + t];
        if (j >= 0) v -= Y[(size_t)j * ldY + t];
        pv[t] = v - red[0];
    }
}

__global__ __launch_bounds__(256) void k_mv_gather(int n, const int *__restrict__ e, const double *__restrict__ d,
                                                   double *__restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[t] = d[e[t]];
}

// ---- residual variance ----------------------------------------------------------------------------------------------
// partials over a fixed grid: [0] sum d^2 |r|^2 over edges with a nonzero row of A, [1] their number
constexpr int kScaleGrid = 256;
__global__ __launch_bounds__(256) void k_mv_scale(long long m, long long mpad, const uint8_t *__restrict__ eflag,
                                                  const double *__restrict__ d, const double *__restrict__ er,
                                                  double *__restrict__ part) {
    __shared__ double s0[256], s1[256];
    double a = 0.0, b = 0.0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < m; k += (long long)gridDim.x * 256) {
        if (!eflag[k]) continue;
        const double x = er[k], y = er[mpad + k], z = er[2 * mpad + k];
        a += d[k] * d[k] * (x * x + y * y + z * z);
        b += 1.0;
    }
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            s0[threadIdx.x] += s0[threadIdx.x + o];
            s1[threadIdx.x] += s1[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s0[0];
        part[kScaleGrid + blockIdx.x] = s1[0];
    }
}

int grid1(long long n) { return (int)((n + 255) / 256); }

// the marginals of the nu free views -> the caller's device array of n_total entries (0 for the f fixed views)
__global__ __launch_bounds__(256) void k_mv_var_out(long long n_total, int f, const double *__restrict__ dvar,
                                                    double *__restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n_total) out[v] = v < f ? 0.0 : dvar[v - f];
}

constexpr int kPairChunk = 1024;  // pair columns per multi right-hand-side solve

}  // namespace

// ---- shared with the edge diagnostics (marginals.hpp) ----------------------------------------------------------------
double residual_scale(Graph &g, double *num_out, double *cnt_out, DevBuf<double> *er_keep) {
    DevBuf<double> er, part;
    er.alloc((size_t)3 * g.mpad);
    part.alloc(2 * kScaleGrid);
    std::swap(er, g.er);  // the handle's residual planes stay as they are
    launch_edge_residual(g);
    hipLaunchKernelGGL(k_mv_scale, dim3(kScaleGrid), dim3(256), 0, g.stream, (long long)g.m, (long long)g.mpad,
                       g.eflag.p, g.dw.p, g.er.p, part.p);
    std::swap(er, g.er);
    std::vector<double> h(2 * kScaleGrid);
    IRH_CHECK(hipMemcpyAsync(h.data(), part.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
    double num = 0.0, cnt = 0.0;
    for (int b = 0; b < kScaleGrid; b++) {
        num += h[b];
        cnt += h[kScaleGrid + b];
    }
    *num_out = num;
    *cnt_out = cnt;
    if (er_keep) *er_keep = std::move(er);
    return cnt > g.nu ? num / (3.0 * (cnt - g.nu)) : NAN;
}

int read_dead(Graph &g, const DevBuf<int> &dead) {
    int h = 0;
    IRH_CHECK(hipMemcpyAsync(&h, dead.p, sizeof(int), hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
    return h;
}

void invert_own(Graph &g, double *A, int npad) {
    DevBuf<double> keep;
    const bool had = g.dense_maxdiag.n >= 1;
    if (had) {
        keep.alloc(1);
        IRH_CHECK(hipMemcpyAsync(keep.p, g.dense_maxdiag.p, sizeof(double), hipMemcpyDeviceToDevice, g.stream));
    }
    dense_invert_spd(g, A, npad);
    if (had) IRH_CHECK(hipMemcpyAsync(g.dense_maxdiag.p, keep.p, sizeof(double), hipMemcpyDeviceToDevice, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
}

void BandFactor::factor(Graph &g, int *dead) {
    const Level &L0 = g.levels[0];
    const size_t BB = (size_t)B * B, tot = (size_t)nb * BB;
    D.alloc(tot);
    U.alloc(tot);
    Dinv.alloc(tot);
    Ga.alloc(tot);
    Gc.alloc(tot);
    orig.alloc((size_t)nb * B);
    D.zero(g.stream);
    U.zero(g.stream);
    hipLaunchKernelGGL(k_mv_band_assemble, dim3(grid1((long long)nb * B)), dim3(256), 0, g.stream, n, B, nb * B,
                       L0.sl_off.p, L0.col.p, g.slot_eid.p, g.bptr.p, g.beid.p, g.bflag.p, g.dw.p, D.p, U.p, orig.p);
    int s = 1;
    for (; s < nb; s *= 2) {
        const int ne = (nb - s + 2 * s - 1) / (2 * s), ns = (nb + 2 * s - 1) / (2 * s);
        hipLaunchKernelGGL(k_mv_elim, dim3(ne), dim3(256), 0, g.stream, nb, B, s, 0, D.p, U.p, Dinv.p, Ga.p, Gc.p,
                           orig.p, dead);
        hipLaunchKernelGGL(k_mv_update, dim3(ns), dim3(256), 0, g.stream, nb, B, s, D.p, U.p, Ga.p, Gc.p);
    }
    hipLaunchKernelGGL(k_mv_elim, dim3(1), dim3(256), 0, g.stream, nb, B, s, 1, D.p, U.p, Dinv.p, Ga.p, Gc.p, orig.p,
                       dead);
}
void BandFactor::select(Graph &g) {
    IRH_CHECK(hipMemcpyAsync(D.p, Dinv.p, sizeof(double) * B * B, hipMemcpyDeviceToDevice, g.stream));
    int top = 1;
    while (top < nb) top *= 2;
    for (int s = top / 2; s >= 1; s /= 2) {
        const int ne = (nb - s + 2 * s - 1) / (2 * s);
        if (ne > 0)
            hipLaunchKernelGGL(k_mv_down, dim3(ne), dim3(256), 0, g.stream, nb, B, s, Dinv.p, Ga.p, Gc.p, D.p, U.p);
    }
}
void BandFactor::solve(Graph &g, double *Y, int ld) {
    const int ct = ld / 64;
    int s = 1;
    for (; s < nb; s *= 2)
        hipLaunchKernelGGL(k_mv_fwd, dim3((nb + 2 * s - 1) / (2 * s), ct), dim3(256), 0, g.stream, nb, B, s, ld, Ga.p,
                           Gc.p, Y);
    hipLaunchKernelGGL(k_mv_bwd, dim3(1, ct), dim3(256), 0, g.stream, nb, B, s, 1, ld, Dinv.p, Ga.p, Gc.p, Y);
    for (s /= 2; s >= 1; s /= 2)
        hipLaunchKernelGGL(k_mv_bwd, dim3((nb - s + 2 * s - 1) / (2 * s), ct), dim3(256), 0, g.stream, nb, B, s, 0,
                           ld, Dinv.p, Ga.p, Gc.p, Y);
}

int band_setup(Graph &g, BandFactor &F, BandClosures &C, DevBuf<int> &dead) {
    F.B = g.bcr_B;
    F.n = g.no;
    F.nb = (g.no + F.B - 1) / F.B;
    const int nrows = F.nb * F.B, nrowsZ = (nrows + 63) / 64 * 64;
    C.nrows = nrows;
    C.nrowsZ = nrowsZ;
    dead.alloc(1);
    dead.zero(g.stream);
    F.factor(g, dead.p);
    // closures of non-zero weight (C^-1 does not exist for the others: they contribute nothing)
    std::vector<int> cp, cq;
    std::vector<double> cinv;
    if (!g.bcr_far_e.empty()) {
        const int nf = (int)g.bcr_far_e.size();
        DevBuf<int> fe;
        DevBuf<double> fw;
        fe.upload(g.bcr_far_e, g.stream);
        fw.alloc((size_t)nf);
        hipLaunchKernelGGL(k_mv_gather, dim3(grid1(nf)), dim3(256), 0, g.stream, nf, fe.p, g.dw.p, fw.p);
        std::vector<double> dfar((size_t)nf);
        IRH_CHECK(hipMemcpyAsync(dfar.data(), fw.p, sizeof(double) * nf, hipMemcpyDeviceToHost, g.stream));
        IRH_CHECK(hipStreamSynchronize(g.stream));
        for (int t = 0; t < nf; t++) {
            const double de = dfar[(size_t)t], w = de * de;
            if (w == 0.0) continue;
            cp.push_back(g.bcr_far_j[t]);
            cq.push_back(g.bcr_far_i[t]);
            cinv.push_back(1.0 / w);
        }
    }
    const int k = C.k = (int)cp.size();
    if (read_dead(g, dead)) return IROTAVG_ERR_SOLVER;
    const int ldZ = C.ldZ = std::max(64, (k + 63) / 64 * 64);
    if (k > 0) {
        C.dcp.upload(cp, g.stream);
        C.dcq.upload(cq, g.stream);
        DevBuf<double> dcinv;
        dcinv.upload(cinv, g.stream);
        C.Z.alloc((size_t)nrowsZ * ldZ);  // k_mv_wcorr reads whole 64-row tiles: the rows past nrows stay zero
        C.Z.zero(g.stream);
        hipLaunchKernelGGL(k_mv_rhs, dim3(grid1(k)), dim3(256), 0, g.stream, k, ldZ, C.dcp.p, C.dcq.p, C.Z.p);
        F.solve(g, C.Z.p, ldZ);
        C.S.alloc((size_t)ldZ * ldZ);
        hipLaunchKernelGGL(k_mv_wsys, dim3(grid1((long long)ldZ * ldZ)), dim3(256), 0, g.stream, k, ldZ, ldZ, C.dcp.p,
                           C.dcq.p, dcinv.p, C.Z.p, C.S.p);
        invert_own(g, C.S.p, ldZ);
        DevBuf<double> sd;
        sd.alloc((size_t)k);
        dead.zero(g.stream);
        hipLaunchKernelGGL(k_mv_dense_var, dim3(grid1(k)), dim3(256), 0, g.stream, k, ldZ, C.S.p, nullptr, sd.p,
                           dead.p);
        if (read_dead(g, dead)) return IROTAVG_ERR_SOLVER;
    }
    return IROTAVG_OK;
}

void band_pairs(Graph &g, BandFactor &F, const BandClosures &C, const std::vector<int> &pi, const std::vector<int> &pj,
                std::vector<double> &pv) {
    const int np = (int)pi.size();
    pv.assign((size_t)np, 0.0);
    for (int p0 = 0; p0 < np; p0 += kPairChunk) {
        const int nc = std::min(kPairChunk, np - p0), ld = (nc + 63) / 64 * 64;
        std::vector<int> a(pi.begin() + p0, pi.begin() + p0 + nc), b(pj.begin() + p0, pj.begin() + p0 + nc);
        for (int t = 0; t < nc; t++)
            if (a[t] == b[t]) a[t] = b[t] = -1;  // u = 0
        DevBuf<int> da, db;
        da.upload(a, g.stream);
        db.upload(b, g.stream);
        DevBuf<double> Y, dpv;
        Y.alloc((size_t)C.nrows * ld);
        Y.zero(g.stream);
        dpv.alloc((size_t)nc);
        hipLaunchKernelGGL(k_mv_rhs, dim3(grid1(nc)), dim3(256), 0, g.stream, nc, ld, da.p, db.p, Y.p);
        F.solve(g, Y.p, ld);
        hipLaunchKernelGGL(k_mv_band_pairs, dim3(nc), dim3(256), 0, g.stream, ld, da.p, db.p, Y.p, C.k, C.dcp.p, C.dcq.p,
                           C.S.p, C.ldZ, dpv.p);
        IRH_CHECK(hipMemcpyAsync(pv.data() + p0, dpv.p, sizeof(double) * nc, hipMemcpyDeviceToHost, g.stream));
        IRH_CHECK(hipStreamSynchronize(g.stream));  // the chunk's buffers go back to the pool
    }
}

int dense_inverse(Graph &g, DenseInverse &Dn, DevBuf<int> &dead) {
    const Level &L0 = g.levels[0];
    const int n = Dn.n = g.no, npad = Dn.npad = std::max(64, (n + 63) / 64 * 64);
    DevBuf<double> &M = Dn.M, &sc = Dn.sc;
    dead.alloc(1);
    dead.zero(g.stream);
    M.alloc((size_t)npad * npad);
    M.zero(g.stream);
    hipLaunchKernelGGL(k_mv_dense_assemble, dim3(grid1(npad)), dim3(256), 0, g.stream, n, npad, L0.sl_off.p, L0.col.p,
                       g.slot_eid.p, g.bptr.p, g.beid.p, g.bflag.p, g.dw.p, M.p);
    sc.alloc((size_t)npad);
    hipLaunchKernelGGL(k_mv_dense_diag, dim3(grid1(npad)), dim3(256), 0, g.stream, npad, M.p, sc.p, dead.p);
    if (read_dead(g, dead)) return IROTAVG_ERR_SOLVER;
    hipLaunchKernelGGL(k_mv_dense_scale, dim3(grid1((long long)npad * npad)), dim3(256), 0, g.stream, npad, M.p, sc.p);
    invert_own(g, M.p, npad);
    // every diagonal entry of the inverse is positive unless a pivot was dead (its row and column come back zero)
    Dn.dvar.alloc((size_t)n);
    hipLaunchKernelGGL(k_mv_dense_var, dim3(grid1(n)), dim3(256), 0, g.stream, n, npad, M.p, sc.p, Dn.dvar.p, dead.p);
    if (read_dead(g, dead)) return IROTAVG_ERR_SOLVER;
    return IROTAVG_OK;
}

namespace {

// var_dev: the marginals go to the caller's device array (behind the dead-pivot test: written only on success)
void var_to_device(Graph &g, const double *dvar, double *var_dev) {
    hipLaunchKernelGGL(k_mv_var_out, dim3(grid1(g.n_total)), dim3(256), 0, g.stream, (long long)g.n_total, g.f, dvar,
                       var_dev);
}

int band_path(Graph &g, bool want_var, std::vector<double> &var, const std::vector<int> &pi,
              const std::vector<int> &pj, std::vector<double> &pv, double *var_dev) {
    BandFactor F;
    BandClosures C;
    DevBuf<int> dead;
    const int rc = band_setup(g, F, C, dead);
    if (rc != IROTAVG_OK) return rc;
    if (want_var) {
        DevBuf<double> corr, dvar;
        F.select(g);
        if (C.k > 0) {
            corr.alloc((size_t)C.nrowsZ);
            hipLaunchKernelGGL(k_mv_wcorr, dim3(C.nrowsZ / 64), dim3(256), 0, g.stream, C.ldZ, C.Z.p, C.S.p, C.ldZ,
                               corr.p);
        }
        dvar.alloc((size_t)F.n);
        hipLaunchKernelGGL(k_mv_band_var, dim3(grid1(F.n)), dim3(256), 0, g.stream, F.n, F.B, F.D.p,
                           C.k > 0 ? corr.p : nullptr, dvar.p, dead.p);
        if (!var_dev) {
            var.resize((size_t)F.n);
            IRH_CHECK(hipMemcpyAsync(var.data(), dvar.p, sizeof(double) * F.n, hipMemcpyDeviceToHost, g.stream));
        }
        if (read_dead(g, dead)) return IROTAVG_ERR_SOLVER;
        if (var_dev) {
            var_to_device(g, dvar.p, var_dev);
            IRH_CHECK(hipStreamSynchronize(g.stream));  // dvar goes back to the pool
        }
    }
    band_pairs(g, F, C, pi, pj, pv);
    IRH_CHECK(hipStreamSynchronize(g.stream));
    return IROTAVG_OK;
}

int dense_path(Graph &g, bool want_var, std::vector<double> &var, const std::vector<int> &pi,
               const std::vector<int> &pj, std::vector<double> &pv, double *var_dev) {
    DenseInverse Dn;
    DevBuf<int> dead;
    const int rc = dense_inverse(g, Dn, dead);
    if (rc != IROTAVG_OK) return rc;
    const int n = Dn.n, npad = Dn.npad;
    if (want_var && var_dev) {
        var_to_device(g, Dn.dvar.p, var_dev);
    } else if (want_var) {
        var.resize((size_t)n);
        IRH_CHECK(hipMemcpyAsync(var.data(), Dn.dvar.p, sizeof(double) * n, hipMemcpyDeviceToHost, g.stream));
    }
    const int np = (int)pi.size();
    pv.assign((size_t)np, 0.0);
    if (np > 0) {
        std::vector<int> a(pi), b(pj);
        for (int t = 0; t < np; t++)
            if (a[t] == b[t]) a[t] = b[t] = -1;
        DevBuf<int> da, db;
        DevBuf<double> dpv;
        da.upload(a, g.stream);
        db.upload(b, g.stream);
        dpv.alloc((size_t)np);
        hipLaunchKernelGGL(k_mv_dense_pairs, dim3(grid1(np)), dim3(256), 0, g.stream, np, npad, da.p, db.p, Dn.M.p,
                           Dn.sc.p, dpv.p);
        IRH_CHECK(hipMemcpyAsync(pv.data(), dpv.p, sizeof(double) * np, hipMemcpyDeviceToHost, g.stream));
    }
    IRH_CHECK(hipStreamSynchronize(g.stream));
    return IROTAVG_OK;
}

// right-hand sides of up to three pairs as the three coordinates of one PCG solve: b_r = (u_0, u_1, u_2)_r
__global__ __launch_bounds__(256) void k_mv_pcg_rhs(int n, int4 a, int4 b, double4 *__restrict__ rhs) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    auto u = [&](int i, int j) { return (r == i ? 1.0 : 0.0) - (r == j ? 1.0 : 0.0); };
    rhs[r] = make_double4(u(a.x, b.x), u(a.y, b.y), u(a.z, b.z), 0.0);
}
// u_c' x_c for the three coordinates of the solution
__global__ void k_mv_pcg_dot(int4 a, int4 b, const double4 *__restrict__ X, double *__restrict__ out) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    const int i = c == 0 ? a.x : (c == 1 ? a.y : a.z), j = c == 0 ? b.x : (c == 1 ? b.y : b.z);
    auto comp = [&](int r) { const double4 v = X[r]; return c == 0 ? v.x : (c == 1 ? v.y : v.z); };
    out[c] = (i >= 0 ? comp(i) : 0.0) - (j >= 0 ? comp(j) : 0.0);
}

// Pairs on a multigrid-PCG handle: u' M^-1 u by the handle's own solver, three pairs per solve, to pcg_rtol. The solve
// runs on a solver clone (the static structure aliased, its own matrix values, dense coarse inverse, vectors and
// counters), so the handle's adaptive coarse-inverse state is exactly as before.
int pcg_pairs(Graph &g, const std::vector<int> &pi, const std::vector<int> &pj, std::vector<double> &pv) {
    const int np = (int)pi.size();
    pv.assign((size_t)np, 0.0);
    std::vector<int> live;  // pairs with u != 0
    for (int t = 0; t < np; t++)
        if (pi[t] != pj[t]) live.push_back(t);
    if (live.empty()) return IROTAVG_OK;
    std::unique_ptr<Graph> q = make_solver_clone(g, g.stream);
    assemble(*q, 0, g.dw.p, true);  // M with the current weights (the right-hand side it forms is replaced below)
    const int n = q->levels[0].n;
    DevBuf<double> dout;
    dout.alloc(3);
    for (size_t t0 = 0; t0 < live.size(); t0 += 3) {
        int ia[3], jb[3];
        for (int c = 0; c < 3; c++) {  // a short last group repeats its first pair (no zero column)
            const int t = live[t0 + c < live.size() ? t0 + c : t0];
            ia[c] = pi[t];
            jb[c] = pj[t];
        }
        const int4 a = make_int4(ia[0], ia[1], ia[2], -1), b = make_int4(jb[0], jb[1], jb[2], -1);
        hipLaunchKernelGGL(k_mv_pcg_rhs, dim3(grid1(n)), dim3(256), 0, g.stream, n, a, b, q->levels[0].b.p);
        IRH_CHECK(hipMemsetAsync(q->X.p, 0, sizeof(double4) * q->X.n, g.stream));
        const int rc = pcg_solve(*q);
        if (rc != IROTAVG_OK) return rc;
        hipLaunchKernelGGL(k_mv_pcg_dot, dim3(1), dim3(64), 0, g.stream, a, b, q->X.p + q->ng, dout.p);
        double h[3];
        IRH_CHECK(hipMemcpyAsync(h, dout.p, sizeof(h), hipMemcpyDeviceToHost, g.stream));
        IRH_CHECK(hipStreamSynchronize(g.stream));
        for (int c = 0; c < 3 && t0 + c < live.size(); c++) pv[(size_t)live[t0 + c]] = h[c];
    }
    return IROTAVG_OK;
}

}  // namespace

int rotation_variance(Graph &g, double *var, int64_t npairs, const int32_t *pairs, double *pair_var, double *scale,
                      double *var_dev) {
    if (g.ng != 0 || g.is_clone || g.levels.empty()) return IROTAVG_ERR_UNSUPPORTED;
    const int f = g.f;
    const bool dense = g.no <= 2048, band = !dense && g.bcr_B > 0;
    const bool want_var = var || var_dev;
    if (!dense && !band && want_var) return IROTAVG_ERR_UNSUPPORTED;  // marginals of a PCG handle: not offered
    // pair ends as operator rows (-1: a fixed view, dropped from u)
    std::vector<int> pi((size_t)npairs), pj((size_t)npairs);
    for (int64_t t = 0; t < npairs; t++) {
        pi[(size_t)t] = pairs[2 * t] >= f ? pairs[2 * t] - f : -1;
        pj[(size_t)t] = pairs[2 * t + 1] >= f ? pairs[2 * t + 1] - f : -1;
    }
    std::vector<double> v, pv;
    const int rc = dense  ? dense_path(g, want_var, v, pi, pj, pv, var_dev)
                   : band ? band_path(g, want_var, v, pi, pj, pv, var_dev)
                          : pcg_pairs(g, pi, pj, pv);
    if (rc != IROTAVG_OK) return rc;
    double num = 0.0, cnt = 0.0;
    const double s2 = scale ? residual_scale(g, &num, &cnt) : 0.0;
    if (var) {
        for (int v0 = 0; v0 < f; v0++) var[v0] = 0.0;
        std::copy(v.begin(), v.end(), var + f);
    }
    if (npairs > 0) std::copy(pv.begin(), pv.end(), pair_var);
    if (scale) *scale = s2;
    return IROTAVG_OK;
}

}  // namespace irh
