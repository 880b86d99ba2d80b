// window.hip -- the sliding-window solve of ViewGraph::rotAvg(10) (src/ViewGraph.cpp:1263-1435,
// called once per admitted frame, src/IRotAvg.cpp:371-378) as ONE kernel launch.
//
// A window problem has <= 64 free views and a few hundred edges: far too small for the
// multi-kernel path (one l1ra + irls there is ~150 launches and ~40 host round trips, ~6 ms),
// so the complete pipeline -- l1ra (primal-dual LP per coordinate, ral/l1_irls.cpp:228-468,
// 851-912) followed by irls (:559-752) -- runs inside a single workgroup with every vector and
// the dense normal matrix in LDS: one H2D, one launch, one D2H. The per-edge math is the code the
// multi-kernel path runs (kernels.hpp: edge_log, robust_weight, step_quat; common.hpp: edge_flags);
// the primal-dual LP follows the same reference statements as l1pd.hip; the linear solves are exact
// (dense Gauss-Jordan in LDS, dead pivots -> 0 like the oracle).
#include "batchdev.hpp"  // the host's side of irotavg_window_solve_batch_dev: block, sequence number, lock, wait
#include "graph.hpp"
#include "kernels.hpp"
#include "winbatch.hpp"  // the size limits (WIN_MAX_*, SM_MAX_*), win_lds_bytes, WinParams / WinResult, the staging layout, the plan of a batch
#include "winio.hpp"     // ld_row / st_row

namespace irh {

constexpr int WIN_THREADS = 256;
static_assert(sizeof(double4) == 32 && sizeof(int2) == 8, "win_lds_bytes (winbatch.hpp) counts with these");

struct WinShared {
    double4 *Q;       // nv
    double *r;        // 3 * ne (planes)
    double *d;        // ne   IRLS weights
    double *W;        // 3 * nu (planes): the step X
    double *H;        // nu * (nu + 1)
    double *B;        // nu * 3
    double *pd;       // 12 * ne  primal-dual edge vectors
    double *pn;       // 5 * nu   primal-dual view vectors
    double *red;      // 16 reduction scratch
    int2 *I;          // ne
    unsigned char *fl;  // ne
};

// ---- where a problem's arrays live --------------------------------------------------------------
// The two kernel bodies below are written once; what differs between the single-problem entry points and the batched
// form on caller arrays (irotavg_window_solve_batch_dev) is how a row is fetched and stored, and whether the edge
// endpoints have been checked by the host (kGuard = false) or must be checked by the workgroup (kGuard = true).
struct WinIoOwn {  // the library's own staging block: one double4 per row, every row stored
    static constexpr bool kGuard = false;  // capi checked the endpoints
    static constexpr bool kSeq = false;    // the general kernel's result goes home by a copy command, no sequence number
    static constexpr bool kStage = false;  // the general kernel reads the measurements where they are
    const int2 *I;
    const double4 *QQ;
    double4 *Q;
    double *w;
    __device__ __forceinline__ int2 edge(int k) const { return I[k]; }
    __device__ __forceinline__ double4 qq(int k) const { return QQ[k]; }
    __device__ __forceinline__ const double4 *measurements(double4 *, int) const { return QQ; }
    __device__ __forceinline__ double4 q(int i) const { return Q[i]; }
    __device__ __forceinline__ int store_from(int) const { return 0; }
    __device__ __forceinline__ void put_q(int i, const double4 &v) const { Q[i] = v; }
    __device__ __forceinline__ void put_w(int k, double v) const { w[k] = v; }
};
// (a row of the caller's strided arrays: ld_row / st_row, winio.hpp)
struct WinUser {  // the caller's packed arrays of a batch (kernel argument)
    const int2 *I;
    const double *QQ;
    long long qq_rs, qq_cs;
    double *Q;
    long long q_rs, q_cs;
    double *w;  // or nullptr
    int qq_aos, q_aos;
};
struct WinIoUser {  // one problem of them: rows eoff.. of I / QQ / w, rows voff.. of Q; fixed rows of Q are not stored
    static constexpr bool kGuard = true;
    static constexpr bool kSeq = true;
    static constexpr bool kStage = true;  // the general kernel keeps the measurements in LDS (measurements() below)
    WinUser U;
    long long eoff, voff;
    __device__ __forceinline__ int2 edge(int k) const { return U.I[eoff + k]; }
    __device__ __forceinline__ double4 qq(int k) const { return ld_row(U.QQ, U.qq_rs, U.qq_cs, eoff + k, U.qq_aos != 0); }
    __device__ __forceinline__ double4 q(int i) const { return ld_row(U.Q, U.q_rs, U.q_cs, voff + i, U.q_aos != 0); }
    // The general kernel reads every measurement once per outer iteration. The compiler contracts edge_log's quaternion
    // products into fma chains, and which product of a sum stays a plain multiplication depends on the form the
    // measurement arrives in: after four 8-byte loads it chose another one than after the double4 load of the staging
    // block, and the batched results differed from the single-problem ones in the last bits. So the rows are brought
    // into LDS once (ne double4 behind the poses: win_lds_bytes_user) and the iterations load them as double4, as
    // k_window_solve does: the same expression, the same rounding. (Visible to the workgroup after its next barrier.)
    __device__ __forceinline__ const double4 *measurements(double4 *lds, int ne) const {
        for (int k = threadIdx.x; k < ne; k += blockDim.x) lds[k] = qq(k);
        return lds;
    }
    __device__ __forceinline__ int store_from(int f) const { return f; }
    __device__ __forceinline__ void put_q(int i, const double4 &v) const { st_row(U.Q, U.q_rs, U.q_cs, voff + i, U.q_aos != 0, v); }
    __device__ __forceinline__ void put_w(int k, double v) const {
        if (U.w) U.w[eoff + k] = v;
    }
};
// what a workgroup of the batched form leaves when an endpoint of its problem is outside [0, nv): nothing else is written
__device__ __forceinline__ void win_refuse(WinResult *out, int seq) {
    out->l1_iters = 0;
    out->irls_iters = 0;
    out->status = IROTAVG_ERR_BAD_ARG;
    out->l1_score = 0.0;
    out->irls_score = 0.0;
    __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- workgroup reductions (result to every thread) -------------------------------------------
__device__ __forceinline__ double wg_sum(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double wg_min(double v, double *red) {
    v = wave_min(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    __syncthreads();
    return s;
}
__device__ __forceinline__ double wg_max(double v, double *red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return s;
}

// ---- dense SPD solve in LDS: H (n x n, leading dim n+1) X = B (n x nrhs, row-major) ----------
// Gauss-Jordan without pivoting; a non-positive pivot marks a dead variable (row/column dropped,
// solution 0), like the oracle's sparse Cholesky. Returns false if a non-finite value appears.
__device__ bool dense_solve(double *H, int n, double *B, int nrhs, double *red) {
    const int ld = n + 1;
    // dead-pivot threshold: kDeadTol (common.hpp) x the largest original diagonal entry
    __syncthreads();
    double dm = 0.0;
    for (int k = threadIdx.x; k < n; k += blockDim.x) dm = fmax(dm, H[k * ld + k]);
    const double thr0 = kDeadTol * wg_max(dm, red);
    for (int k = 0; k < n; k++) {
        const double piv = H[k * ld + k];
        const bool dead = !(piv > thr0) || !(piv > 0.0);
        const double ip = dead ? 0.0 : 1.0 / piv;
        __syncthreads();
        // scale row k (entries j > k and the right-hand sides)
        for (int j = threadIdx.x; j < n + nrhs; j += blockDim.x) {
            if (j < n) {
                if (j > k) H[k * ld + j] *= ip;
            } else {
                B[k * nrhs + (j - n)] *= ip;
            }
        }
        __syncthreads();
        // eliminate column k from every other row
        const int cols = n - k - 1 + nrhs;
        for (int e = threadIdx.x; e < n * cols; e += blockDim.x) {
            const int i = e / cols, c = e - i * cols;
            if (i == k) continue;
            const double fk = H[i * ld + k];
            if (fk == 0.0) continue;
            if (c < n - k - 1)
                H[i * ld + k + 1 + c] -= fk * H[k * ld + k + 1 + c];
            else
                B[i * nrhs + (c - (n - k - 1))] -= fk * B[k * nrhs + (c - (n - k - 1))];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            if (i != k) H[i * ld + k] = 0.0;
    }
    __syncthreads();
    double bad = 0.0;
    for (int e = threadIdx.x; e < n * nrhs; e += blockDim.x)
        if (!isfinite(B[e])) bad = 1.0;
    return wg_sum(bad, red) == 0.0;
}

// ---- K1 on the window: r_k = log(Qinv_j (x) QQ_k (x) Q_i) -------------------------------------
__device__ __forceinline__ void win_residual(const WinParams &P, const WinShared &S, const double4 *QQ) {
    for (int k = threadIdx.x; k < P.ne; k += blockDim.x) {
        double ox, oy, oz;
        edge_log(S.Q[S.I[k].x], S.Q[S.I[k].y], QQ[k], ox, oy, oz);
        S.r[k] = ox;
        S.r[P.ne + k] = oy;
        S.r[2 * P.ne + k] = oz;
    }
    __syncthreads();
}

// (A' t)_v with make_A's coefficients, v a free-view index
__device__ __forceinline__ double at_dot(const WinParams &P, const WinShared &S, const double *t, int v) {
    double s = 0.0;
    for (int k = 0; k < P.ne; k++) {
        const unsigned char fl = S.fl[k];
        if ((fl & EF_CJ) && S.I[k].y - P.f == v) s += t[k];
        if ((fl & EF_CI) && S.I[k].x - P.f == v) s -= t[k];
    }
    return s;
}

// score = mean ||W row|| (before the exp map), exp map, Q_{f+i} <- Q_{f+i} (x) W_i
// (ral/l1_irls.cpp:729-737 / :894-902)
__device__ double win_apply_step(const WinParams &P, const WinShared &S) {
    const int nu = P.nv - P.f;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nu; i += blockDim.x) {
        double th;
        const double4 w = step_quat(S.W[i], S.W[nu + i], S.W[2 * nu + i], th);
        acc += th;
        S.Q[i + P.f] = qmul(S.Q[i + P.f], w);
    }
    const double s = wg_sum(acc, S.red);
    return s / (double)nu;
}

// ---- one coordinate of the primal-dual LP, x0 = 0 (ral/l1_irls.cpp:228-468) -------------------
// y: LDS vector of ne entries; result written to xout (nu entries). Returns 0 ok, 1 solver error.
__device__ int win_l1decode(const WinParams &P, const WinShared &S, const double *y, int pdmaxiter,
                            double *xout) {
    const double PDTOL = 1e-3, alpha = 0.01, beta = 0.5, mu = 10;
    const int m = P.ne, nu = P.nv - P.f, f = P.f;
    double *u = S.pd, *Ax = u + m, *f1 = Ax + m, *f2 = f1 + m, *l1 = f2 + m, *l2 = l1 + m;
    double *sigx = l2 + m, *t1 = sigx + m, *t2 = t1 + m, *Adx = t2 + m, *du = Adx + m, *dl1 = du + m;
    double *dl2 = S.r + 3 * m;  // one spare plane behind the residuals (allocated 4 * ne)
    double *x = S.pn, *Atv = x + nu, *Atdv = Atv + nu, *dx = Atdv + nu;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < nu; i += nt) x[i] = 0.0;
    double loc = -HUGE_VAL;
    for (int k = tid; k < m; k += nt) {
        Ax[k] = 0.0;
        loc = fmax(loc, fabs(y[k]));
    }
    const double maxabs = wg_max(loc, S.red);
    double a0 = 0, a1 = 0, a2 = 0;
    for (int k = tid; k < m; k += nt) {  // :252-276
        const double uu = fabs(y[k] - Ax[k]) * 0.95 + maxabs * 0.10;
        const double g1 = Ax[k] - y[k] - uu, g2 = -Ax[k] + y[k] - uu;
        const double m1 = -(1.0 / g1), m2 = -(1.0 / g2);
        u[k] = uu;
        f1[k] = g1;
        f2[k] = g2;
        l1[k] = m1;
        l2[k] = m2;
        t1[k] = m1 - m2;
        a0 += g1 * m1;
        a1 += g2 * m2;
        const double rd = 1.0 - m1 - m2;
        a2 += rd * rd;
    }
    const double sa = wg_sum(a0, S.red), sb = wg_sum(a1, S.red), rd_tail2 = wg_sum(a2, S.red);
    double sdg = -(sa + sb);
    double tau = mu * 2 * (double)m / sdg;
    double acc = 0.0;
    for (int v = tid; v < nu; v += nt) {
        const double s = at_dot(P, S, t1, v);
        Atv[v] = s;
        acc += s * s;
    }
    const double atv2 = wg_sum(acc, S.red);
    acc = 0.0;
    for (int k = tid; k < m; k += nt) {
        const double c1 = -l1[k] * f1[k] - 1.0 / tau, c2 = -l2[k] * f2[k] - 1.0 / tau;
        acc += c1 * c1 + c2 * c2;
    }
    double resnorm = sqrt(atv2 + rd_tail2 + wg_sum(acc, S.red));
    int pditer = 0;
    bool done = (sdg < PDTOL) || (pditer >= pdmaxiter);
    while (!done) {
        pditer++;
        const double itau = 1.0 / tau;
        for (int k = tid; k < m; k += nt) {  // :292-305
            const double if1 = 1.0 / f1[k], if2 = 1.0 / f2[k];
            const double w2 = -1 - itau * (if1 + if2);
            const double a = l1[k] / f1[k], b = l2[k] / f2[k];
            const double s1 = -a - b, s2 = a - b;
            sigx[k] = s1 - (s2 * s2) / s1;
            t1[k] = -if1 + if2;
            t2[k] = (s2 / s1) * w2;
        }
        __syncthreads();
        // H11p = reshape(AtA * sigx) (make_AtA: endpoints skipped independently, :825-843),
        // right-hand side w1p = -(1/tau) A't1 - A't2
        const int ld = nu + 1;
        for (int e = tid; e < nu * ld; e += nt) S.H[e] = 0.0;
        __syncthreads();
        for (int v = tid; v < nu; v += nt) {
            double *row = S.H + v * ld;
            for (int k = 0; k < m; k++) {
                const int i = S.I[k].x - f, j = S.I[k].y - f;
                const double s = sigx[k];
                if (i >= 0 && i == j) {
                    if (i == v) row[v] -= s;
                    continue;
                }
                if (i == v) {
                    row[v] += s;
                    if (j >= 0) row[j] -= s;
                }
                if (j == v) {
                    row[v] += s;
                    if (i >= 0) row[i] -= s;
                }
            }
            const double w1 = -itau * at_dot(P, S, t1, v);
            dx[v] = w1 - at_dot(P, S, t2, v);
        }
        __syncthreads();
        if (!dense_solve(S.H, nu, dx, 1, S.red)) return 1;
        double smin = HUGE_VAL;
        for (int k = tid; k < m; k += nt) {  // :324-381
            const unsigned char fl = S.fl[k];
            double adx = 0.0;
            if (fl & EF_CJ) adx += dx[S.I[k].y - f];
            if (fl & EF_CI) adx -= dx[S.I[k].x - f];
            const double g1 = f1[k], g2 = f2[k], m1 = l1[k], m2 = l2[k];
            const double if1 = 1.0 / g1, if2 = 1.0 / g2;
            const double w2 = -1 - itau * (if1 + if2);
            const double a = m1 / g1, b = m2 / g2;
            const double s1 = -a - b, s2 = a - b;
            const double d_u = (w2 - s2 * adx) / s1;
            double d1 = -m1 / g1;
            d1 *= (adx - d_u);
            d1 -= m1;
            d1 -= itau * if1;
            double d2 = m2 / g2;
            d2 *= (adx + d_u);
            d2 -= m2;
            d2 -= itau * if2;
            Adx[k] = adx;
            du[k] = d_u;
            dl1[k] = d1;
            dl2[k] = d2;
            t1[k] = d1 - d2;
            if (d1 < 0) smin = fmin(smin, -m1 / d1);
            if (d2 < 0) smin = fmin(smin, -m2 / d2);
            const double p = adx - d_u;
            if (p > 0) smin = fmin(smin, -g1 / p);
            const double q = -adx - d_u;
            if (q > 0) smin = fmin(smin, -g2 / q);
        }
        double s = fmin(1.0, wg_min(smin, S.red));
        if (!(s == s)) return 1;
        s *= 0.99;
        for (int v = tid; v < nu; v += nt) Atdv[v] = at_dot(P, S, t1, v);
        __syncthreads();
        bool suffdec = false;
        int backiter = 0;
        double s_acc = s, rdp2 = 0.0;
        while (!suffdec) {  // :384-429
            double b0 = 0, b1 = 0;
            for (int v = tid; v < nu; v += nt) {
                const double q = Atv[v] + s * Atdv[v];
                b0 += q * q;
            }
            for (int k = tid; k < m; k += nt) {
                const double up = u[k] + s * du[k];
                const double axp = Ax[k] + s * Adx[k];
                const double m1 = l1[k] + s * dl1[k], m2 = l2[k] + s * dl2[k];
                const double g1 = axp - y[k] - up, g2 = -axp + y[k] - up;
                const double r = 1.0 + (-m1 - m2);
                b0 += r * r;
                const double c1 = -m1 * g1 - itau, c2 = -m2 * g2 - itau;
                b1 += c1 * c1 + c2 * c2;
            }
            rdp2 = wg_sum(b0, S.red);
            const double rcp2 = wg_sum(b1, S.red);
            suffdec = sqrt(rdp2 + rcp2) <= (1 - alpha * s) * resnorm;
            s_acc = s;
            s *= beta;
            backiter++;
            if (backiter > 32) {  // "Stuck backtracking": the previous iterate is returned
                for (int v = tid; v < nu; v += nt) xout[v] = x[v];
                __syncthreads();
                return 0;
            }
        }
        for (int v = tid; v < nu; v += nt) {
            x[v] += s_acc * dx[v];
            Atv[v] += s_acc * Atdv[v];
        }
        a0 = a1 = 0;
        for (int k = tid; k < m; k += nt) {
            const double up = u[k] + s_acc * du[k];
            const double axp = Ax[k] + s_acc * Adx[k];
            const double m1 = l1[k] + s_acc * dl1[k], m2 = l2[k] + s_acc * dl2[k];
            const double g1 = axp - y[k] - up, g2 = -axp + y[k] - up;
            u[k] = up;
            Ax[k] = axp;
            l1[k] = m1;
            l2[k] = m2;
            f1[k] = g1;
            f2[k] = g2;
            a0 += g1 * m1;
            a1 += g2 * m2;
        }
        sdg = -(wg_sum(a0, S.red) + wg_sum(a1, S.red));
        tau = mu * 2 * (double)m / sdg;
        acc = 0.0;
        for (int k = tid; k < m; k += nt) {
            const double c1 = -l1[k] * f1[k] - 1.0 / tau, c2 = -l2[k] * f2[k] - 1.0 / tau;
            acc += c1 * c1 + c2 * c2;
        }
        resnorm = sqrt(rdp2 + wg_sum(acc, S.red));
        done = (sdg < PDTOL) || (pditer >= pdmaxiter);
    }
    for (int v = tid; v < nu; v += nt) xout[v] = x[v];
    __syncthreads();
    return 0;
}

// The general kernel's body: one workgroup, one problem (every entry kernel below runs exactly this).
template <class IO>
__device__ __forceinline__ void win_solve_body(const WinParams &P, const IO &io, WinResult *__restrict__ out) {
    extern __shared__ double4 smem4[];
    const int nv = P.nv, ne = P.ne, f = P.f, nu = nv - f;
    WinShared S;
    S.Q = smem4;
    double4 *const stage = S.Q + nv;  // ne rows where IO::kStage
    double *p = reinterpret_cast<double *>(stage + (IO::kStage ? ne : 0));
    S.r = p;          p += 4 * ne;
    S.d = p;          p += ne;
    S.W = p;          p += 3 * nu;
    S.H = p;          p += nu * (nu + 1);
    S.B = p;          p += 3 * nu;
    S.pd = p;         p += 12 * ne;
    S.pn = p;         p += 5 * nu;
    S.red = p;        p += 16;
    S.I = reinterpret_cast<int2 *>(p);
    S.fl = reinterpret_cast<unsigned char *>(S.I + ne);
    const int tid = threadIdx.x, nt = blockDim.x;
    if (IO::kGuard && tid == 0) *reinterpret_cast<int *>(S.red) = 0;
    if (IO::kGuard) __syncthreads();
    for (int i = tid; i < nv; i += nt) S.Q[i] = io.q(i);
    const double4 *QQ = io.measurements(stage, ne);
    bool outside = false;
    for (int k = tid; k < ne; k += nt) {
        const int2 e = io.edge(k);
        S.I[k] = e;
        S.fl[k] = edge_flags(e.x, e.y, f);
        outside = outside || (unsigned)e.x >= (unsigned)nv || (unsigned)e.y >= (unsigned)nv;
    }
    if (IO::kGuard) {
        // The endpoints come from the device here and no host has seen them: a workgroup-wide OR before anything is
        // indexed with one (so far LDS and the arrays were indexed with i < nv and k < ne alone).
        if (outside) *reinterpret_cast<volatile int *>(S.red) = 1;
        __syncthreads();
        const bool refuse = *reinterpret_cast<volatile int *>(S.red) != 0;
        if (refuse) {
            if (tid == 0) win_refuse(out, P.seq);
            return;
        }
    }
    __syncthreads();
    int status = 0;
    // ---------------- l1ra (ral/l1_irls.cpp:851-912) ----------------
    double score = HUGE_VAL, change_th = P.change_th;
    int iter = 0, l1_step = 2;
    while (((score >= change_th) || (l1_step < 2)) && (iter < P.l1_max) && status == 0) {
        if (score < change_th) {  // unreachable under the guard above; kept literal (:879-883)
            l1_step *= 4;
            change_th /= 100.0;
        }
        win_residual(P, S, QQ);
        for (int c = 0; c < 3 && status == 0; c++)
            status = win_l1decode(P, S, S.r + c * ne, l1_step, S.W + c * nu);
        if (status) break;
        score = win_apply_step(P, S);
        iter++;
    }
    const int l1_iters = iter;
    const double l1_score = score;
    // ---------------- irls (ral/l1_irls.cpp:559-752) ----------------
    for (int k = tid; k < ne; k += nt) S.d[k] = 1.0;
    __syncthreads();
    score = HUGE_VAL;
    iter = 0;
    while (score > P.change_th && iter < P.irls_max && status == 0) {
        win_residual(P, S, QQ);
        const int ld = nu + 1;
        for (int e = tid; e < nu * ld; e += nt) S.H[e] = 0.0;
        __syncthreads();
        for (int v = tid; v < nu; v += nt) {  // A'D^2A and A'D^2 r with make_A's A
            double *row = S.H + v * ld;
            double b0 = 0, b1 = 0, b2 = 0;
            for (int k = 0; k < ne; k++) {
                const unsigned char fl = S.fl[k];
                if (!fl) continue;
                const int i = S.I[k].x - f, j = S.I[k].y - f;
                const double s = S.d[k] * S.d[k];
                if ((fl & EF_CJ) && j == v) {
                    row[v] += s;
                    if (fl & EF_CI) row[i] -= s;
                    b0 += s * S.r[k];
                    b1 += s * S.r[ne + k];
                    b2 += s * S.r[2 * ne + k];
                }
                if ((fl & EF_CI) && i == v) {
                    row[v] += s;
                    if (fl & EF_CJ) row[j] -= s;
                    b0 -= s * S.r[k];
                    b1 -= s * S.r[ne + k];
                    b2 -= s * S.r[2 * ne + k];
                }
            }
            S.B[3 * v] = b0;
            S.B[3 * v + 1] = b1;
            S.B[3 * v + 2] = b2;
        }
        __syncthreads();
        if (!dense_solve(S.H, nu, S.B, 3, S.red)) {
            status = IROTAVG_ERR_SOLVER;
            break;
        }
        for (int v = tid; v < nu; v += nt) {
            S.W[v] = S.B[3 * v];
            S.W[nu + v] = S.B[3 * v + 1];
            S.W[2 * nu + v] = S.B[3 * v + 2];
        }
        __syncthreads();
        for (int k = tid; k < ne; k += nt) {  // E = A W3 - w, weights (:614-727)
            const unsigned char fl = S.fl[k];
            double e0 = 0, e1 = 0, e2c = 0;
            if (fl & EF_CJ) {
                const int j = S.I[k].y - f;
                e0 += S.W[j];
                e1 += S.W[nu + j];
                e2c += S.W[2 * nu + j];
            }
            if (fl & EF_CI) {
                const int i = S.I[k].x - f;
                e0 -= S.W[i];
                e1 -= S.W[nu + i];
                e2c -= S.W[2 * nu + i];
            }
            e0 -= S.r[k];
            e1 -= S.r[ne + k];
            e2c -= S.r[2 * ne + k];
            S.d[k] = robust_weight(P.cost, P.sigma, e0 * e0 + e1 * e1 + e2c * e2c, S.d[k]);
        }
        __syncthreads();
        score = win_apply_step(P, S);
        iter++;
    }
    if (status == 1) status = IROTAVG_ERR_SOLVER;
    __syncthreads();
    for (int i = io.store_from(f) + tid; i < nv; i += nt) io.put_q(i, S.Q[i]);
    for (int k = tid; k < ne; k += nt) io.put_w(k, S.d[k]);
    if (IO::kSeq) {  // the record is polled by the host: the sequence number goes out last (see k_window_wave)
        __threadfence_system();
        __syncthreads();
    }
    if (tid == 0) {
        out->l1_iters = l1_iters;
        out->irls_iters = iter;
        out->status = status;
        out->l1_score = l1_score;
        out->irls_score = score;
        if (IO::kSeq) __hip_atomic_store(&out->seq, P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(WIN_THREADS) void k_window_solve(WinParams P, const int2 *__restrict__ Ig,
                                                              const double4 *__restrict__ QQ,
                                                              double4 *__restrict__ Qg,
                                                              double *__restrict__ weights,
                                                              WinResult *__restrict__ out) {
    win_solve_body(P, WinIoOwn{Ig, QQ, Qg, weights}, out);
}

// Workgroup b solves the problem of descriptor b on the caller's packed arrays (irotavg_window_solve_batch_dev): sizes
// and offsets from D[b], iteration limits and cost from Pk, the result to R[D[b].idx].
__global__ __launch_bounds__(WIN_THREADS) void k_window_solve_user(WinParams Pk, const WinDesc *__restrict__ D, WinUser U,
                                                                   WinResult *__restrict__ R) {
    const WinDesc d = D[blockIdx.x];
    WinParams P = Pk;
    P.nv = d.nv;
    P.f = d.f;
    P.ne = d.ne;
    win_solve_body(P, WinIoUser{U, d.eoff, d.voff}, R + d.idx);
}

// =================================================================================================
// The wave-resident variant for the usual rotAvg(10) sub-problem (<= 64 edges, <= 16 free views,
// src/IRotAvg.cpp:158-161,371-378: each view is linked to its 4 predecessors). The general kernel
// above spends its time in LDS round trips and workgroup barriers; here every edge vector of the
// primal-dual LP lives in the registers of ONE lane of a wave (lane k = edge k, lane v = free view
// v), the dense normal matrix is a 16-register row per lane (Gauss-Jordan by v_readlane
// broadcasts), reductions are wave butterflies, and the three coordinate LPs of l1ra / the three
// right-hand sides of irls run on three waves at once. Two workgroup barriers per outer iteration.
// Statement order inside the sums follows the general kernel (k ascending), so both give the same
// normal matrices bit for bit; only the order of the wave reductions differs.
// =================================================================================================
constexpr int SM_THREADS = 192;
constexpr unsigned ADJ_NEG = 1u << 16;   // the edge enters the view's row with coefficient -1
constexpr unsigned ADJ_SELF = 1u << 17;  // make_AtA self-loop entry

__device__ __forceinline__ int rl_i(int x, int k) { return __builtin_amdgcn_readlane(x, k); }

// wave64 reductions on the DPP network (no LDS traffic): four steps inside each row of 16 lanes,
// two row broadcasts, the total is read from lane 63 -> identical bits in every lane
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_d(double ident, double x) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(ident), __double2loint(x), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(ident), __double2hiint(x), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
struct OpSum {
    static __device__ __forceinline__ double id() { return 0.0; }
    static __device__ __forceinline__ double f(double a, double b) { return a + b; }
};
struct OpMin {
    static __device__ __forceinline__ double id() { return HUGE_VAL; }
    static __device__ __forceinline__ double f(double a, double b) { return fmin(a, b); }
};
struct OpMax {
    static __device__ __forceinline__ double id() { return -HUGE_VAL; }
    static __device__ __forceinline__ double f(double a, double b) { return fmax(a, b); }
};
template <class Op>
__device__ __forceinline__ double wv_reduce(double v) {
    v = Op::f(v, dpp_d<0xb1, 0xf>(Op::id(), v));   // quad_perm [1,0,3,2]
    v = Op::f(v, dpp_d<0x4e, 0xf>(Op::id(), v));   // quad_perm [2,3,0,1]
    v = Op::f(v, dpp_d<0x124, 0xf>(Op::id(), v));  // row_ror 4
    v = Op::f(v, dpp_d<0x128, 0xf>(Op::id(), v));  // row_ror 8
    v = Op::f(v, dpp_d<0x142, 0xa>(Op::id(), v));  // row_bcast 15 -> rows 1, 3
    v = Op::f(v, dpp_d<0x143, 0xc>(Op::id(), v));  // row_bcast 31 -> rows 2, 3
    return readlane_d(v, 63);
}
__device__ __forceinline__ double wv_sum(double v) { return wv_reduce<OpSum>(v); }
__device__ __forceinline__ double wv_min(double v) { return wv_reduce<OpMin>(v); }
__device__ __forceinline__ double wv_max(double v) { return wv_reduce<OpMax>(v); }

// what a lane knows about "its" edge (lane k < m) -- and, as lane v < nu, about its free view
struct SmLane {
    int m, nu, lane;
    int cj, ci;  // make_A columns of the edge (+1 at cj, -1 at ci), -1 = absent (ral/l1_irls.cpp:764-777)
    // incidence lists of view `lane`, ascending edge id; entry = k | (other column + 1) << 8 | flags
    const unsigned *adjA;  // make_A's A: rows that touch the view (A' products, the IRLS normal matrix)
    const unsigned *adjH;  // make_AtA's endpoint rule (:825-843): the primal-dual normal matrix
    int degA, degH, maxA, maxH;  // own list lengths, wave-wide maxima
    double *Hrow;                // this wave's LDS row of the view (16 entries)
};

// (A' t)_v on lane v: k ascending, +t_k through cj then -t_k through ci (same order as at_dot)
__device__ __forceinline__ double sm_at(const SmLane &E, double t) {
    double s = 0.0;
    // four entries per step: the list loads and the lane exchanges of a step are independent of each other (one by one
    // each entry was an LDS load -> ds_bpermute -> add chain); the sum keeps its order
    for (int d0 = 0; d0 < E.maxA; d0 += 4) {
        unsigned e[4];
        double tk[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = d0 + u < E.degA ? E.adjA[d0 + u] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++) tk[u] = __shfl(t, (int)(e[u] & 63u), 64);
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (d0 + u < E.degA) s += (e[u] & ADJ_NEG) ? -tk[u] : tk[u];
    }
    return s;
}
// (A x)_k on lane k
__device__ __forceinline__ double sm_ax(const SmLane &E, double x) {
    const double xj = __shfl(x, E.cj < 0 ? 0 : E.cj, 64), xi = __shfl(x, E.ci < 0 ? 0 : E.ci, 64);
    double s = 0.0;
    if (E.cj >= 0) s += xj;
    if (E.ci >= 0) s -= xi;
    return s;
}

// Gauss-Jordan on rows held in registers: lane i owns row i (h[c], c < 16) and its right-hand
// side. Pivot rows stay unscaled (row i -= (h_ik / h_kk) * row k, x_i = b_i / h_ii at the end): one
// broadcast + one fma per column. A non-positive pivot marks a dead variable (never eliminates,
// solution 0), like dense_solve above / the oracle's Cholesky. False if a non-finite value appears.
// NUP: nu rounded up to a multiple of four -- the loops unroll to straight-line code (with nu as a run-time bound every
// column update sat behind a scalar branch: ~12 clocks per instruction, the solve 30 % of the kernel). Rows and
// columns nu .. NUP - 1 are zero: their pivots are dead, their multipliers 0.
template <int NUP>
__device__ __forceinline__ void sm_solve_t(double (&h)[SM_MAX_NU], double &b, double thr, int lane, double &myip) {
#pragma unroll
    for (int k = 0; k < NUP; k++) {
        // the reciprocal -- the only chain from pivot to pivot -- by v_rcp_f64 + two Newton steps (a third of the IEEE
        // division's dependent instructions)
        const double piv = readlane_d(h[k], k);
        double ip = __builtin_amdgcn_rcp(piv);
        ip = fma(fma(-piv, ip, 1.0), ip, ip);
        ip = fma(fma(-piv, ip, 1.0), ip, ip);
        ip = (piv > thr && piv > 0.0) ? ip : 0.0;
        const bool me = lane == k;
        if (me) myip = ip;
        const double mult = me ? 0.0 : -(h[k] * ip);
#pragma unroll
        for (int c = k + 1; c < NUP; c++) h[c] = fma(mult, readlane_d(h[c], k), h[c]);
        b = fma(mult, readlane_d(b, k), b);
    }
}
__device__ __forceinline__ bool sm_solve(double (&h)[SM_MAX_NU], double &b, int nu, int lane) {
    double myip = 0.0;
    double dg = 0.0;  // own original diagonal entry
#pragma unroll
    for (int c = 0; c < SM_MAX_NU; c++)
        if (c == lane) dg = h[c];
    const double thr = kDeadTol * wv_max(lane < nu ? dg : 0.0);  // relative to the largest one
    if (lane >= nu) b = 0.0;
    if (nu <= 4)
        sm_solve_t<4>(h, b, thr, lane, myip);
    else if (nu <= 8)
        sm_solve_t<8>(h, b, thr, lane, myip);
    else if (nu <= 12)
        sm_solve_t<12>(h, b, thr, lane, myip);
    else
        sm_solve_t<16>(h, b, thr, lane, myip);
    b *= myip;
    return __ballot(lane < nu && !isfinite(b)) == 0ull;
}

// one coordinate of the primal-dual LP on one wave, x0 = 0 (ral/l1_irls.cpp:228-468); y on edge
// lanes, result on view lanes. Returns 0 ok, 1 solver error.
__device__ int sm_l1decode(const SmLane &E, const double y, const int pdmaxiter, double &xout) {
    const double PDTOL = 1e-3, alpha = 0.01, beta = 0.5, mu = 10;
    const int m = E.m, lane = E.lane;
    const bool ek = lane < m, vk = lane < E.nu;
    double x = 0.0, Ax = 0.0;
    const double maxabs = wv_max(ek ? fabs(y) : -HUGE_VAL);
    double u = 0, f1 = 0, f2 = 0, l1 = 0, l2 = 0, t1 = 0;
    double a0 = 0, a1 = 0, a2 = 0;
    if (ek) {  // :252-276
        u = fabs(y - Ax) * 0.95 + maxabs * 0.10;
        f1 = Ax - y - u;
        f2 = -Ax + y - u;
        l1 = -(1.0 / f1);
        l2 = -(1.0 / f2);
        t1 = l1 - l2;
        a0 = f1 * l1;
        a1 = f2 * l2;
        const double rd = 1.0 - l1 - l2;
        a2 = rd * rd;
    }
    const double sa = wv_sum(a0), sb = wv_sum(a1), rd_tail2 = wv_sum(a2);
    double sdg = -(sa + sb);
    double tau = mu * 2 * (double)m / sdg;
    double Atv = sm_at(E, t1);
    const double atv2 = wv_sum(Atv * Atv);
    double acc = 0.0;
    if (ek) {
        const double c1 = -l1 * f1 - 1.0 / tau, c2 = -l2 * f2 - 1.0 / tau;
        acc = c1 * c1 + c2 * c2;
    }
    double resnorm = sqrt(atv2 + rd_tail2 + wv_sum(acc));
    int pditer = 0;
    bool done = (sdg < PDTOL) || (pditer >= pdmaxiter);
    while (!done) {
        pditer++;
        const double itau = 1.0 / tau;
        double sigx = 0.0, t2 = 0.0, if1 = 0, if2 = 0, w2 = 0, s1 = 1, s2 = 0, qa = 0, qb = 0;
        t1 = 0.0;
        if (ek) {  // :292-305
            if1 = 1.0 / f1;
            if2 = 1.0 / f2;
            w2 = -1 - itau * (if1 + if2);
            qa = l1 / f1;
            qb = l2 / f2;
            s1 = -qa - qb;
            s2 = qa - qb;
            sigx = s1 - (s2 * s2) / s1;
            t1 = -if1 + if2;
            t2 = (s2 / s1) * w2;
        }
        // H11p = A' diag(sigx) A with make_AtA's endpoint rule: lane v accumulates row v in LDS
        // (k ascending), then holds it in registers for the elimination
        double h[SM_MAX_NU];
        {
            double hd = 0.0;
            if (vk) {
#pragma unroll
                for (int c = 0; c < SM_MAX_NU; c++) E.Hrow[c] = 0.0;
            }
            for (int d0 = 0; d0 < E.maxH; d0 += 4) {  // (four entries per step, as sm_at)
                unsigned e[4];
                double sk[4];
#pragma unroll
                for (int u = 0; u < 4; u++) e[u] = d0 + u < E.degH ? E.adjH[d0 + u] : 0u;
#pragma unroll
                for (int u = 0; u < 4; u++) sk[u] = __shfl(sigx, (int)(e[u] & 63u), 64);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (d0 + u < E.degH) {
                        const double s = sk[u];
                        if (e[u] & ADJ_SELF) {
                            hd -= s;
                        } else {
                            hd += s;
                            const int o = (int)((e[u] >> 8) & 255u);
                            if (o) atomicAdd(&E.Hrow[o - 1], -s);  // ds_add_f64 without return: no read-modify-write round trip per entry; same bits as -= s
                        }
                    }
                }
            }
            if (vk) E.Hrow[lane] = hd;
#pragma unroll
            for (int c = 0; c < SM_MAX_NU; c++) h[c] = vk ? E.Hrow[c] : 0.0;
        }
        const double w1 = -itau * sm_at(E, t1);
        double dx = w1 - sm_at(E, t2);
        if (!sm_solve(h, dx, E.nu, lane)) return 1;
        if (!vk) dx = 0.0;
        const double adx = sm_ax(E, dx);
        double du = 0, dl1 = 0, dl2 = 0, Adx = 0, smin = HUGE_VAL;
        t1 = 0.0;
        if (ek) {  // :324-381
            const double d_u = (w2 - s2 * adx) / s1;
            double d1 = -qa;
            d1 *= (adx - d_u);
            d1 -= l1;
            d1 -= itau * if1;
            double d2 = qb;
            d2 *= (adx + d_u);
            d2 -= l2;
            d2 -= itau * if2;
            Adx = adx;
            du = d_u;
            dl1 = d1;
            dl2 = d2;
            t1 = d1 - d2;
            if (d1 < 0) smin = fmin(smin, -l1 / d1);
            if (d2 < 0) smin = fmin(smin, -l2 / d2);
            const double p = adx - d_u;
            if (p > 0) smin = fmin(smin, -f1 / p);
            const double q = -adx - d_u;
            if (q > 0) smin = fmin(smin, -f2 / q);
        }
        double s = fmin(1.0, wv_min(smin));
        if (!(s == s)) return 1;
        s *= 0.99;
        const double Atdv = sm_at(E, t1);
        bool suffdec = false;
        int backiter = 0;
        double s_acc = s, rdp2 = 0.0;
        while (!suffdec) {  // :384-429
            double b0 = 0, b1 = 0;
            if (vk) {
                const double q = Atv + s * Atdv;
                b0 = q * q;
            }
            if (ek) {
                const double up = u + s * du;
                const double axp = Ax + s * Adx;
                const double m1 = l1 + s * dl1, m2 = l2 + s * dl2;
                const double g1 = axp - y - up, g2 = -axp + y - up;
                const double r = 1.0 + (-m1 - m2);
                b0 += r * r;
                const double c1 = -m1 * g1 - itau, c2 = -m2 * g2 - itau;
                b1 = c1 * c1 + c2 * c2;
            }
            rdp2 = wv_sum(b0);
            const double rcp2 = wv_sum(b1);
            suffdec = sqrt(rdp2 + rcp2) <= (1 - alpha * s) * resnorm;
            s_acc = s;
            s *= beta;
            backiter++;
            if (backiter > 32) {  // "Stuck backtracking": the previous iterate is returned
                xout = x;
                return 0;
            }
        }
        x += s_acc * dx;
        Atv += s_acc * Atdv;
        a0 = a1 = 0;
        if (ek) {
            u = u + s_acc * du;
            Ax = Ax + s_acc * Adx;
            l1 = l1 + s_acc * dl1;
            l2 = l2 + s_acc * dl2;
            f1 = Ax - y - u;
            f2 = -Ax + y - u;
            a0 = f1 * l1;
            a1 = f2 * l2;
        }
        sdg = -(wv_sum(a0) + wv_sum(a1));
        tau = mu * 2 * (double)m / sdg;
        acc = 0.0;
        if (ek) {
            const double c1 = -l1 * f1 - 1.0 / tau, c2 = -l2 * f2 - 1.0 / tau;
            acc = c1 * c1 + c2 * c2;
        }
        resnorm = sqrt(rdp2 + wv_sum(acc));
        done = (sdg < PDTOL) || (pditer >= pdmaxiter);
    }
    xout = x;
    return 0;
}

// The wave kernel's body: one workgroup of three waves, one problem (every entry kernel below runs exactly this).
template <class IO>
__device__ __forceinline__ void win_wave_body(const WinParams &P, const IO &io, WinResult *__restrict__ out) {
    __shared__ double4 sQ[WIN_MAX_NV];
    __shared__ double sW[3][SM_MAX_NU];
    __shared__ double sH[3][SM_MAX_NU][SM_MAX_NU + 1];
    __shared__ unsigned sAdjA[SM_MAX_NU][SM_MAX_NE], sAdjH[SM_MAX_NU][SM_MAX_NE];
    __shared__ int sDeg[2][SM_MAX_NU];
    __shared__ int sStatus[3];
    const int nv = P.nv, ne = P.ne, f = P.f, nu = nv - f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long stamp[6];
    stamp[0] = (long long)__builtin_amdgcn_s_memtime();
    for (int i = tid; i < nv; i += SM_THREADS) sQ[i] = io.q(i);
    SmLane E;
    E.m = ne;
    E.nu = nu;
    E.lane = lane;
    E.cj = E.ci = -1;
    int ai = -1, aj = -2;  // make_AtA endpoints i - f, j - f (negative = fixed)
    int ex = 0, ey = 0;
    bool outside = false;
    double4 qq = make_double4(0, 0, 0, 1);
    if (lane < ne) {
        const int2 e = io.edge(lane);
        if (IO::kGuard) {
            // The endpoints come from the device here and no host has seen them. Every wave loads every edge, so the
            // ballot below is the same in all three: the workgroup leaves as one, before anything is indexed with an
            // endpoint (so far LDS and the arrays were indexed with i < nv and lane < ne alone).
            outside = (unsigned)e.x >= (unsigned)nv || (unsigned)e.y >= (unsigned)nv;
        }
        qq = io.qq(lane);
        ex = e.x;
        ey = e.y;
        ai = e.x - f;
        aj = e.y - f;
        const uint8_t fl = edge_flags(e.x, e.y, f);
        if (fl & EF_CJ) E.cj = e.y - f;
        if (fl & EF_CI) E.ci = e.x - f;
    }
    if (IO::kGuard && __ballot(outside) != 0ull) {
        if (tid == 0) win_refuse(out, P.seq);
        return;
    }
    const bool ek = lane < ne, vk = lane < nu;
    if (wave == 0) {
        // Incidence lists of the free views, ascending edge id. The edges that touch view v are the set bits of wave
        // ballots (lane k = edge k), taken for all views in turn and kept by lane v; lane v then walks ITS bits in
        // ascending order -- a handful of steps -- and fetches the other endpoint of each edge from the edge's lane.
        // (Until round 4 every lane walked all ne edges through readlanes: 40 serial steps, a fifth of the kernel.)
        const bool self = ek && ai >= 0 && ai == aj;
        unsigned long long mAj = 0, mAi = 0, mHs = 0, mHi = 0, mHj = 0;
        for (int v = 0; v < nu; v++) {
            const unsigned long long bj = __ballot(ek && E.cj == v), bi = __ballot(ek && E.ci == v);
            const unsigned long long hs = __ballot(self && ai == v), hi = __ballot(ek && !self && ai == v),
                                     hj = __ballot(ek && !self && aj == v);
            if (lane == v) {
                mAj = bj;
                mAi = bi;
                mHs = hs;
                mHi = hi;
                mHj = hj;
            }
        }
        const int row = vk ? lane : 0;
        int da = 0, dh = 0;
        unsigned long long ma = mAj | mAi, mh = mHs | mHi | mHj;
        while (__ballot(ma != 0ull || mh != 0ull) != 0ull) {  // wave-uniform trip count: the shuffles need every lane
            const int ka = ma ? (int)__builtin_ctzll(ma) : 0, kh = mh ? (int)__builtin_ctzll(mh) : 0;
            const int kj = __shfl(E.cj, ka, 64), ki = __shfl(E.ci, ka, 64);
            const int hi_ = __shfl(ai, kh, 64), hj_ = __shfl(aj, kh, 64);
            if (ma) {  // (an edge is in at most one of the two make_A lists of a view: cj == ci only for a self loop, whose cj is -1)
                const unsigned long long bit = 1ull << ka;
                if (mAj & bit)
                    sAdjA[row][da++] = (unsigned)ka | ((unsigned)(ki + 1) << 8);
                else
                    sAdjA[row][da++] = (unsigned)ka | ((unsigned)(kj + 1) << 8) | ADJ_NEG;
                ma &= ma - 1;
            }
            if (mh) {
                const unsigned long long bit = 1ull << kh;
                if (mHs & bit)
                    sAdjH[row][dh++] = (unsigned)kh | ADJ_SELF;
                else if (mHi & bit)
                    sAdjH[row][dh++] = (unsigned)kh | ((unsigned)(hj_ >= 0 ? hj_ + 1 : 0) << 8);
                else
                    sAdjH[row][dh++] = (unsigned)kh | ((unsigned)(hi_ >= 0 ? hi_ + 1 : 0) << 8);
                mh &= mh - 1;
            }
        }
        if (vk) {
            sDeg[0][lane] = da;
            sDeg[1][lane] = dh;
        }
    }
    if (tid < 3) sStatus[tid] = 0;
    __syncthreads();
    stamp[1] = (long long)__builtin_amdgcn_s_memtime();
    E.adjA = sAdjA[vk ? lane : 0];
    E.adjH = sAdjH[vk ? lane : 0];
    E.degA = vk ? sDeg[0][lane] : 0;
    E.degH = vk ? sDeg[1][lane] : 0;
    E.maxA = (int)wv_max((double)E.degA);
    E.maxH = (int)wv_max((double)E.degH);
    E.Hrow = sH[wave][vk ? lane : 0];
    double r[3] = {0, 0, 0};
    auto residual = [&]() {  // K1 on lane k
        if (ek) edge_log(sQ[ex], sQ[ey], qq, r[0], r[1], r[2]);
    };
    // score = mean ||W row|| before the exp map; wave 0 updates Q (:729-737 / :894-902)
    auto apply_step = [&]() -> double {
        double acc = 0.0;
        if (vk) {
            const double4 w = step_quat(sW[0][lane], sW[1][lane], sW[2][lane], acc);
            if (wave == 0) sQ[lane + f] = qmul(sQ[lane + f], w);
        }
        const double s = wv_sum(acc) / (double)nu;
        __syncthreads();
        return s;
    };
    int status = 0;
    // ---------------- l1ra (ral/l1_irls.cpp:851-912): wave c solves coordinate c ----------------
    double score = HUGE_VAL, change_th = P.change_th;
    int iter = 0, l1_step = 2;
    while (((score >= change_th) || (l1_step < 2)) && (iter < P.l1_max) && status == 0) {
        if (score < change_th) {  // unreachable under the guard above; kept literal (:879-883)
            l1_step *= 4;
            change_th /= 100.0;
        }
        residual();
        double xo = 0.0;
        const int st = sm_l1decode(E, wave == 0 ? r[0] : (wave == 1 ? r[1] : r[2]), l1_step, xo);
        if (lane == 0) sStatus[wave] = st;
        if (vk) sW[wave][lane] = xo;
        __syncthreads();
        status = sStatus[0] | sStatus[1] | sStatus[2];
        if (status) break;
        score = apply_step();
        iter++;
    }
    const int l1_iters = iter;
    const double l1_score = score;
    stamp[2] = (long long)__builtin_amdgcn_s_memtime();
    // ---------------- irls (ral/l1_irls.cpp:559-752): wave c solves right-hand side c ------------
    double d = 1.0;
    score = HUGE_VAL;
    iter = 0;
    while (score > P.change_th && iter < P.irls_max && status == 0) {
        residual();
        const double rc = wave == 0 ? r[0] : (wave == 1 ? r[1] : r[2]);
        // A'D^2A and A'D^2 r with make_A's A: row v on lane v (k ascending)
        double h[SM_MAX_NU];
        double hd = 0.0, b = 0.0;
        if (vk) {
#pragma unroll
            for (int c = 0; c < SM_MAX_NU; c++) E.Hrow[c] = 0.0;
        }
        for (int q0 = 0; q0 < E.maxA; q0 += 4) {  // (four entries per step, as sm_at)
            unsigned e[4];
            double dk[4], rk[4];
#pragma unroll
            for (int u = 0; u < 4; u++) e[u] = q0 + u < E.degA ? E.adjA[q0 + u] : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                dk[u] = __shfl(d, (int)(e[u] & 63u), 64);
                rk[u] = __shfl(rc, (int)(e[u] & 63u), 64);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (q0 + u < E.degA) {
                    const double s = dk[u] * dk[u];
                    hd += s;
                    const int o = (int)((e[u] >> 8) & 255u);
                    if (o) atomicAdd(&E.Hrow[o - 1], -s);  // ds_add_f64 without return: no read-modify-write round trip per entry; same bits as -= s
                    if (e[u] & ADJ_NEG)
                        b -= s * rk[u];
                    else
                        b += s * rk[u];
                }
            }
        }
        if (vk) E.Hrow[lane] = hd;
#pragma unroll
        for (int c = 0; c < SM_MAX_NU; c++) h[c] = vk ? E.Hrow[c] : 0.0;
        const bool ok = sm_solve(h, b, nu, lane);
        if (lane == 0) sStatus[wave] = ok ? 0 : 1;
        if (vk) sW[wave][lane] = b;
        __syncthreads();
        status = sStatus[0] | sStatus[1] | sStatus[2];
        if (status) break;
        if (ek) {  // E = A W3 - w, weights (:614-727)
            double e0 = 0, e1 = 0, e2c = 0;
            if (E.cj >= 0) {
                e0 += sW[0][E.cj];
                e1 += sW[1][E.cj];
                e2c += sW[2][E.cj];
            }
            if (E.ci >= 0) {
                e0 -= sW[0][E.ci];
                e1 -= sW[1][E.ci];
                e2c -= sW[2][E.ci];
            }
            e0 -= r[0];
            e1 -= r[1];
            e2c -= r[2];
            d = robust_weight(P.cost, P.sigma, e0 * e0 + e1 * e1 + e2c * e2c, d);
        }
        score = apply_step();
        iter++;
    }
    if (status) status = IROTAVG_ERR_SOLVER;
    __syncthreads();
    stamp[3] = (long long)__builtin_amdgcn_s_memtime();
    for (int i = io.store_from(f) + tid; i < nv; i += SM_THREADS) io.put_q(i, sQ[i]);
    if (wave == 0 && ek) io.put_w(lane, d);
    // The outputs live in pinned host memory; the sequence number goes out last, after a system-scope fence
    // of every thread: a host that sees it sees everything (window_solve polls it instead of waiting for
    // the runtime's completion signal)
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        stamp[4] = (long long)__builtin_amdgcn_s_memtime();
        for (int q = 0; q < 5; q++) out->stamp[q] = stamp[q];
        out->l1_iters = l1_iters;
        out->irls_iters = iter;
        out->status = status;
        out->l1_score = l1_score;
        out->irls_score = score;
        __hip_atomic_store(&out->seq, P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// BATCH: workgroup b solves the b-th of several INDEPENDENT windows (one per view-graph of a multi-session
// server: irotavg_viewgraph_rot_avg_batch) -- its parameters come from Pb[b] and its arrays lie b * stride bytes
// behind the first problem's. A single window is the kernel-argument form (no extra round trip for P).
template <bool BATCH>
__global__ __launch_bounds__(SM_THREADS) void k_window_wave(WinParams Pk, const WinParams *__restrict__ Pb,
                                                           size_t stride, const int2 *__restrict__ Ig,
                                                           const double4 *__restrict__ QQ,
                                                           double4 *__restrict__ Qg,
                                                           double *__restrict__ weights,
                                                           WinResult *__restrict__ out) {
    const WinParams P = BATCH ? *reinterpret_cast<const WinParams *>(reinterpret_cast<const unsigned char *>(Pb) + stride * blockIdx.x) : Pk;
    if (BATCH) {
        const size_t off = stride * blockIdx.x;
        Ig = reinterpret_cast<const int2 *>(reinterpret_cast<const unsigned char *>(Ig) + off);
        QQ = reinterpret_cast<const double4 *>(reinterpret_cast<const unsigned char *>(QQ) + off);
        Qg = reinterpret_cast<double4 *>(reinterpret_cast<unsigned char *>(Qg) + off);
        weights = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(weights) + off);
        out = reinterpret_cast<WinResult *>(reinterpret_cast<unsigned char *>(out) + off);
    }
    win_wave_body(P, WinIoOwn{Ig, QQ, Qg, weights}, out);
}

// The batched form on the caller's packed arrays, as k_window_solve_user
__global__ __launch_bounds__(SM_THREADS) void k_window_wave_user(WinParams Pk, const WinDesc *__restrict__ D, WinUser U,
                                                                 WinResult *__restrict__ R) {
    const WinDesc d = D[blockIdx.x];
    WinParams P = Pk;
    P.nv = d.nv;
    P.f = d.f;
    P.ne = d.ne;
    win_wave_body(P, WinIoUser{U, d.eoff, d.voff}, R + d.idx);
}

// ---- host side: persistent staging, one H2D / launch / D2H per solve ---------------------------
// Completion of the kernels that store a sequence number last (k_window_wave, the _user kernels): hostwait.hpp.
struct WindowSolver {
    hipStream_t stream = nullptr;
    DevBuf<unsigned char> dev;   // the general kernel's device copy of `own`
    MappedBlock own;             // window_solve: one problem (kStageOwn)
    MappedBlock batch;           // window_solve_batch: slots of kStageBatch
    int seq = 0;       // sequence number of the last wave-kernel launch
    bool attr_set = false;
    bool stamps = false;  // Switches::window_stamps of whoever made the solver: print the wave kernel's phase stamps
    ~WindowSolver() {
        if (stream) StreamPool::get().give(stream);
    }
};

bool window_fits_wave(int nv, int f, int ne) { return win_fits_wave(nv, f, ne); }

bool window_fits(int nv, int f, int ne) { return win_fits(nv, f, ne); }

// a problem into its slot `h` of a staging block; the record's sequence number is 0 until the kernel stores the launch's
static void stage_problem(unsigned char *h, const WinStage &L, int nv, int ne, const int32_t *I, const double *QQ_aos,
                          const double *Q_aos) {
    std::memcpy(h + L.oI, I, sizeof(int32_t) * 2 * (size_t)ne);
    std::memcpy(h + L.oQQ, QQ_aos, sizeof(double) * 4 * (size_t)ne);
    std::memcpy(h + L.oQ, Q_aos, sizeof(double) * 4 * (size_t)nv);
    reinterpret_cast<WinResult *>(h + L.oR)->seq = 0;
}
// the record a workgroup left; rc becomes the first status that is not OK
static const WinResult &take_result(const void *rec, int &rc) {
    const WinResult &R = *static_cast<const WinResult *>(rec);  // (every oR and the slot stride are multiples of 8)
    if (R.status != IROTAVG_OK && rc == IROTAVG_OK) rc = R.status;
    return R;
}

int window_solve(WindowSolver &ws, int nv, int f, int ne, const int32_t *I, const double *QQ_aos,
                 double *Q_aos, double *weights, int l1_max, int irls_max, int cost, double sigma,
                 double change_th, int *l1_iters, int *irls_iters, int kernel) {
    if (!window_fits(nv, f, ne)) return IROTAVG_ERR_BAD_ARG;
    if (kernel == 2 && !window_fits_wave(nv, f, ne)) return IROTAVG_ERR_BAD_ARG;
    const bool wave = kernel == 2 || (kernel == 0 && window_fits_wave(nv, f, ne));
    if (!ws.stream) ws.stream = StreamPool::get().take();
    constexpr WinStage L = kStageOwn;
    constexpr size_t total = L.oP;  // sized exactly: every problem takes the same block
    if (ws.own.cap < total) ws.dev.alloc(total);
    ws.own.reserve(total);
    unsigned char *const host = ws.own.host, *const hdev = ws.own.hdev;
    stage_problem(host, L, nv, ne, I, QQ_aos, Q_aos);
    WinParams P{nv, f, ne, l1_max, irls_max, cost, change_th, sigma, 0};
    if (wave) {
        P.seq = next_seq(ws.seq);
        // the wave kernel touches its inputs once and its outputs once: it works directly on the
        // pinned (device-visible) staging block -- launch + wait, no copy commands
        hipLaunchKernelGGL((k_window_wave<false>), dim3(1), dim3(SM_THREADS), 0, ws.stream, P,
                           (const WinParams *)nullptr, (size_t)0,
                           (const int2 *)(hdev + L.oI), (const double4 *)(hdev + L.oQQ),
                           (double4 *)(hdev + L.oQ), (double *)(hdev + L.oW),
                           (WinResult *)(hdev + L.oR));
        IRH_CHECK(hipGetLastError());
        if (!wait_seq(&reinterpret_cast<const WinResult *>(host + L.oR)->seq, 0, 1, P.seq, 2e-3))
            IRH_CHECK(hipStreamSynchronize(ws.stream));
    } else {
        IRH_CHECK(hipMemcpyAsync(ws.dev.p, host, L.oW, hipMemcpyHostToDevice, ws.stream));
        const size_t shm = win_lds_bytes(nv, ne, nv - f);
        if (!ws.attr_set) {
            IRH_CHECK(hipFuncSetAttribute((const void *)k_window_solve,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ws.attr_set = true;
        }
        hipLaunchKernelGGL(k_window_solve, dim3(1), dim3(WIN_THREADS), shm, ws.stream, P,
                           (const int2 *)(ws.dev.p + L.oI), (const double4 *)(ws.dev.p + L.oQQ),
                           (double4 *)(ws.dev.p + L.oQ), (double *)(ws.dev.p + L.oW),
                           (WinResult *)(ws.dev.p + L.oR));
        IRH_CHECK(hipMemcpyAsync(host + L.oQ, ws.dev.p + L.oQ, total - L.oQ, hipMemcpyDeviceToHost, ws.stream));
        IRH_CHECK(hipStreamSynchronize(ws.stream));
    }
    int rc = IROTAVG_OK;
    const WinResult &R = take_result(host + L.oR, rc);
    if (ws.stamps && wave)  // s_memtime counts at 100 MHz
        std::fprintf(stderr, "[window] nv %d f %d ne %d l1 %d irls %d: load+lists %.2f us, l1ra %.2f us, irls %.2f us, store %.2f us\n", nv,
                     f, ne, R.l1_iters, R.irls_iters, (R.stamp[1] - R.stamp[0]) * 1e-2, (R.stamp[2] - R.stamp[1]) * 1e-2,
                     (R.stamp[3] - R.stamp[2]) * 1e-2, (R.stamp[4] - R.stamp[3]) * 1e-2);
    std::memcpy(Q_aos, host + L.oQ, sizeof(double) * 4 * (size_t)nv);
    if (weights) std::memcpy(weights, host + L.oW, sizeof(double) * (size_t)ne);
    if (l1_iters) *l1_iters = R.l1_iters;
    if (irls_iters) *irls_iters = R.irls_iters;
    return rc;
}

// Several independent window problems in ONE launch (one workgroup each): every problem must fit the
// wave-resident kernel. The pinned block holds nb slots of kStageBatch, parameters included.
int window_solve_batch(WindowSolver &ws, int nb, WinBatchItem *items, int l1_max, int irls_max, int cost, double sigma,
                       double change_th) {
    if (nb <= 0) return IROTAVG_OK;
    for (int b = 0; b < nb; b++)
        if (!window_fits_wave(items[b].nv, items[b].f, items[b].ne)) return IROTAVG_ERR_BAD_ARG;
    if (!ws.stream) ws.stream = StreamPool::get().take();
    constexpr WinStage L = kStageBatch;
    const size_t total = L.stride * (size_t)nb;
    ws.batch.reserve(total, total / 2);
    unsigned char *const host = ws.batch.host, *const hdev = ws.batch.hdev;
    const int seq = next_seq(ws.seq);
    for (int b = 0; b < nb; b++) {
        unsigned char *h = host + L.stride * (size_t)b;
        const WinBatchItem &it = items[b];
        stage_problem(h, L, it.nv, it.ne, it.I, it.QQ_aos, it.Q_aos);
        WinParams P{it.nv, it.f, it.ne, l1_max, irls_max, cost, change_th, sigma, seq};
        std::memcpy(h + L.oP, &P, sizeof(P));
    }
    hipLaunchKernelGGL((k_window_wave<true>), dim3(nb), dim3(SM_THREADS), 0, ws.stream, WinParams{},
                       (const WinParams *)(hdev + L.oP), L.stride, (const int2 *)(hdev + L.oI),
                       (const double4 *)(hdev + L.oQQ), (double4 *)(hdev + L.oQ), (double *)(hdev + L.oW),
                       (WinResult *)(hdev + L.oR));
    IRH_CHECK(hipGetLastError());
    if (!wait_seq(&reinterpret_cast<const WinResult *>(host + L.oR)->seq, L.stride, (size_t)nb, seq, 5e-3))
        IRH_CHECK(hipStreamSynchronize(ws.stream));
    int rc = IROTAVG_OK;
    for (int b = 0; b < nb; b++) {
        const unsigned char *h = host + L.stride * (size_t)b;
        WinBatchItem &it = items[b];
        const WinResult &R = take_result(h + L.oR, rc);
        std::memcpy(it.Q_aos, h + L.oQ, sizeof(double) * 4 * (size_t)it.nv);
        it.l1_iters = R.l1_iters;
        it.irls_iters = R.irls_iters;
        it.status = R.status;
    }
    return rc;
}

// ---- irotavg_window_solve_batch_dev: many problems on the caller's device arrays ------------------------------------
// The block of records and descriptors, the sequence number and the lock: batchdev.hpp (the family's own instance).
static int win_attr_device = -1;  // k_window_solve_user may use 160 KB of dynamic LDS on this device (under the driver's lock)

// the arguments have been checked (devapi.hip) and `plan` made from the caller's sizes (winbatch.hpp)
int window_solve_batch_dev(const WinBatchPlan &plan, int device, const WinBatchArrays &A, int cost, double sigma,
                           int l1_max, int irls_max, double change_th, int32_t *results, hipStream_t stream) {
    auto &drv = BatchDev<WinResult, WinDesc>::get();
    const size_t nb = plan.desc.size(), nw = (size_t)plan.nwave, ng = nb - nw;
    const auto s = drv.stage(plan.desc.data(), nb);
    const WinParams P{0, 0, 0, l1_max, irls_max, cost, change_th, sigma, s.seq};
    const WinUser U{reinterpret_cast<const int2 *>(A.I), A.QQ, A.qq_rs, A.qq_cs, A.Q, A.q_rs, A.q_cs, A.weights,
                    rows16(reinterpret_cast<uintptr_t>(A.QQ), A.qq_rs, A.qq_cs),
                    rows16(reinterpret_cast<uintptr_t>(A.Q), A.q_rs, A.q_cs)};
    if (nw) {
        hipLaunchKernelGGL(k_window_wave_user, dim3((unsigned)nw), dim3(SM_THREADS), 0, stream, P, s.D, U, s.Rd);
        IRH_CHECK(hipGetLastError());
    }
    if (ng) {
        if (win_attr_device != device) {
            IRH_CHECK(hipFuncSetAttribute((const void *)k_window_solve_user, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)WIN_MAX_LDS));
            win_attr_device = device;
        }
        hipLaunchKernelGGL(k_window_solve_user, dim3((unsigned)ng), dim3(WIN_THREADS), plan.lds, stream, P, s.D + nw, U, s.Rd);
        IRH_CHECK(hipGetLastError());
    }
    const int rc = drv.finish(s, stream, nb, [&](size_t b, const WinResult &r) {
        if (!results) return;
        results[4 * b] = r.status;
        results[4 * b + 1] = r.l1_iters;
        results[4 * b + 2] = r.irls_iters;
    });
    if (results)
        for (size_t i = 0; i < nb; i++) results[4 * (size_t)plan.desc[i].idx + 3] = i < nw ? 2 : 1;
    return rc;
}

WindowSolver *window_solver_new(const Switches &sw) {
    WindowSolver *w = new WindowSolver();
    w->stamps = sw.window_stamps;
    return w;
}
void window_solver_delete(WindowSolver *w) { delete w; }

}  // namespace irh
