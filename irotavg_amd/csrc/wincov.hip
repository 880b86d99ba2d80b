// wincov.hip -- uncertainty of a window-size problem in ONE kernel launch (docs/viewgraph_uncertainty.md): what
// irotavg_viewgraph_rotation_variance / _edge_diagnostics / _gate_connections run for every problem window_fits accepts
// (<= 64 free views, <= 640 edges, <= 320 views: every rotAvg(10)). No handle is involved.
//
// One workgroup per problem; everything stays in LDS: the quaternions (10 KB), per edge the endpoints, the residual and
// the weight (25 KB), the operator M = A' diag(d^2) A (33 KB), inverted in place. The body is written once (wincov_body)
// over an I/O policy, as window.hip's solve:
//   k_window_cov       blockIdx.x selects the slot of the library's staging block (the view-graph route and
//                      irotavg_window_uncertainty, one problem on host arrays)
//   k_window_cov_user  blockIdx.x selects a descriptor; the problem lies in the caller's packed device arrays
//                      (irotavg_window_uncertainty_batch_dev, docs/window_uncertainty_batch.md): ids checked by the
//                      workgroup, outputs stored only once the problem is known to have succeeded
//   k_window_gate_user the same on caller arrays with the candidates of the closure gate, which the instance above
//                      compiles out (irotavg_window_gate_batch_dev, docs/window_gate_batch.md)
//   1. residuals r_k (K1's formula) and weights: d_k = 1 / (|r_k|^2 + sigma^2), Geman-McClure at a zero step, or the
//      caller's own (a per-call switch)
//   2. M: one owner thread per row walks the edges in index order (no atomics: bitwise deterministic)
//   3. Jacobi scaling, Gauss-Jordan in place under the dead-pivot rule (a pivot not above 1e-13 x the row's diagonal,
//      which the scaling has made 1 -> IROTAVG_ERR_SOLVER), scaling back: Sigma
//   4. from the resident Sigma: the diagonal, s^2 (fixed-order tree), edge_var / leverage / chi2 of every edge, the
//      pairs, the candidates of the closure gate
// Staging follows window_solve's wave kernel: one pinned, device-visible block that the kernel reads and writes
// directly; one launch, one wait (the sequence number the kernel stores last: hostwait.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "batchdev.hpp"  // the host's side of the two batched calls: block, sequence number, lock, wait
#include "graph.hpp"
#include "kernels.hpp"
#include "winbatch.hpp"  // the limits, wincov_lds, WinCovResult, the plan of a batch, rows16
#include "winio.hpp"     // ld_row

namespace irh {
namespace {

constexpr int WC_MAX_NU = WIN_MAX_NU, WC_MAX_NV = WIN_MAX_NV, WC_MAX_NE = WIN_MAX_NE;  // window_fits' limits
constexpr int WC_MAX_P = 1024;                                   // pairs staged per launch
constexpr int WC_MAX_C = WINCOV_CAND_CHUNK;                      // candidates staged per launch, and per LDS chunk of the batched gate
constexpr int WC_LD = WINCOV_LD;                                 // row stride of M in LDS (bank spread)
constexpr int WC_THREADS = WINCOV_THREADS;

struct WinCovParams {
    int nv, f, ne, np, nc, seq;
    int first;  // 0: a further launch of the same problem for more pairs / candidates -- var and the edge outputs stay
    int use_w;  // 0: d_k = 1 / (|r_k|^2 + sigma^2); 1: d_k as the caller supplies it (sigma unused)
    double sigma;
};
struct WinCovCand {  // a candidate connection (lo, hi, R): rows of its ends (-1 held, -2 not in the problem)
    double4 qi, qj, qq;
};

// the slot of one problem in the staging block
constexpr size_t oP = 0;
constexpr size_t oI = 64;
constexpr size_t oQQ = oI + sizeof(int2) * WC_MAX_NE;
constexpr size_t oQ = oQQ + sizeof(double4) * WC_MAX_NE;
constexpr size_t oWt = oQ + sizeof(double4) * WC_MAX_NV;       // supplied weights (use_w)
constexpr size_t oPR = oWt + sizeof(double) * WC_MAX_NE;       // pair rows
constexpr size_t oCR = oPR + sizeof(int2) * WC_MAX_P;          // candidate rows
constexpr size_t oCQ = oCR + sizeof(int2) * WC_MAX_C;          // candidate quaternions
constexpr size_t oVar = oCQ + sizeof(WinCovCand) * WC_MAX_C;   // ---- outputs from here
constexpr size_t oEv = oVar + sizeof(double) * WC_MAX_NU;
constexpr size_t oLev = oEv + sizeof(double) * WC_MAX_NE;
constexpr size_t oChi = oLev + sizeof(double) * WC_MAX_NE;
constexpr size_t oPv = oChi + sizeof(double) * WC_MAX_NE;
constexpr size_t oCa = oPv + sizeof(double) * WC_MAX_P;        // candidates: angle | pair_var | chi2
constexpr size_t oRes = oCa + sizeof(double) * 3 * WC_MAX_C;
constexpr size_t kSlot = (oRes + sizeof(WinCovResult) + 255) & ~(size_t)255;

// LDS layout (dynamic: above the 64 KB a static allocation may take): winbatch.hpp. The staged form is laid out for
// the limits, the batched form for its own problem (the launch asks for the largest of the batch).
constexpr WinCovLds kLdsOwn = wincov_lds(WC_MAX_NV, WC_MAX_NE, WC_MAX_NU, false);
constexpr size_t kLds = kLdsOwn.bytes;
static_assert(sizeof(double4) == 32 && sizeof(int2) == 8, "wincov_lds (winbatch.hpp) counts with these");

// The staged kernel and the batched one must give the same bits, and which product of a sum the compiler fuses into an
// fma depends on the code around it (the note at WinIoUser::measurements, window.hip): the same source line came out as
// fma(-w, v, 1) in one kernel and as 1 - round(w v) in the other. So nothing below is left to that choice: contraction is
// off for the functions of this file and every fused product is written as fma(), in the form the staged kernel has
// always been compiled to. (edge_log, kernels.hpp, keeps its own setting; its measurement arrives as a double4 in both.)
#pragma clang fp contract(off)

// x^2 + y^2 + z^2 as the kernels have always summed it
__device__ __forceinline__ double wc_norm2(double x, double y, double z) { return fma(z, z, fma(x, x, y * y)); }

// u' Sigma u from the resident Sigma; a, b: the rows of the +1 / -1 coefficient (-1: none)
__device__ __forceinline__ double wc_usu(const double *M, int a, int b) {
    double v = 0.0;
    if (a >= 0) v += M[a * WC_LD + a];
    if (b >= 0) v += M[b * WC_LD + b];
    if (a >= 0 && b >= 0) v -= M[a * WC_LD + b] + M[b * WC_LD + a];
    return v;
}
// edge_var of edge e from the resident Sigma
__device__ __forceinline__ double wc_edge_var(const double *M, int2 e, int f) {
    const uint8_t fl = edge_flags(e.x, e.y, f);
    const int a = (fl & EF_CJ) ? e.y - f : -1, b = (fl & EF_CI) ? e.x - f : -1;
    return wc_usu(M, a, b);
}

// ---- where a problem's arrays live (as window.hip's WinIoOwn / WinIoUser) ---------------------------------------------
// The body below is written once; the staged form of the view-graph route and the batched form on caller arrays differ
// in how a row is fetched and stored, in who has seen the ids (kUser: nobody, the workgroup checks them before it
// indexes with one) and in when the outputs may be stored (kUser: only once the problem is known to have succeeded).
struct WcIoSlot {  // the library's own staging slot: every output has its place in it, the host copies on success
    static constexpr bool kUser = false;
    unsigned char *slot;
    __device__ __forceinline__ int2 edge(int k) const { return reinterpret_cast<const int2 *>(slot + oI)[k]; }
    __device__ __forceinline__ double4 q(int v) const { return reinterpret_cast<const double4 *>(slot + oQ)[v]; }
    __device__ __forceinline__ const double4 *measurements(double4 *, int) const { return reinterpret_cast<const double4 *>(slot + oQQ); }
    __device__ __forceinline__ double weight(int k) const { return reinterpret_cast<const double *>(slot + oWt)[k]; }
    __device__ __forceinline__ int2 pair_rows(int q, int) const { return reinterpret_cast<const int2 *>(slot + oPR)[q]; }
    __device__ __forceinline__ void put_edge(int k, double v, double l, double c) const {
        reinterpret_cast<double *>(slot + oEv)[k] = v;
        reinterpret_cast<double *>(slot + oLev)[k] = l;
        reinterpret_cast<double *>(slot + oChi)[k] = c;
    }
    __device__ __forceinline__ void put_pair(int q, double v) const { reinterpret_cast<double *>(slot + oPv)[q] = v; }
    // candidates: the host has formed the rows and fetched the poses (one launch stages at most WC_MAX_C of them)
    static constexpr bool kCand = true;
    // (q is counted in 64 bits: the batched form has no cap, and q + 256 must not wrap next to INT32_MAX)
    __device__ __forceinline__ int2 cand_rows(long long q, int) const { return reinterpret_cast<const int2 *>(slot + oCR)[q]; }
    __device__ __forceinline__ const double4 *cand_stage(double4 *, long long, int) const { return nullptr; }
    __device__ __forceinline__ WinCovCand cand(long long q, int, const double4 *, const double4 *) const {
        return reinterpret_cast<const WinCovCand *>(slot + oCQ)[q];
    }
    __device__ __forceinline__ void put_cand(long long q, double a, double v, double c) const {
        double *ca = reinterpret_cast<double *>(slot + oCa);
        ca[q] = a;
        ca[WC_MAX_C + q] = v;
        ca[2 * WC_MAX_C + q] = c;
    }
};
struct WinCovUser {  // the caller's packed arrays of a batch (kernel argument); any output may be nullptr
    const int2 *I;
    const double *QQ;
    long long qq_rs, qq_cs;
    const double *Q;
    long long q_rs, q_cs;
    const double *w;  // or nullptr (then WinCovParams::use_w is 0)
    double *var;
    const int2 *pairs;
    double *pair_var, *edge_var, *leverage, *chi2;
    int qq_aos, q_aos;
    // the candidates of the closure gate (k_window_gate_user alone reads these)
    const int2 *cand;
    const double *CQ;
    long long cq_rs, cq_cs;
    double *angle, *cand_var, *cand_chi2;
    int cq_aos;
};
// one problem of them: rows eoff.. of I / QQ / w and the edge outputs, voff.. of Q / var, poff.. of the pairs, coff.. of
// the candidates (kGate: the instance that has them)
template <bool kGate>
struct WcIoUser {
    static constexpr bool kUser = true, kCand = kGate;
    WinCovUser U;
    long long eoff, voff, poff, coff;
    __device__ __forceinline__ int2 edge(int k) const { return U.I[eoff + k]; }
    __device__ __forceinline__ double4 q(int v) const { return ld_row(U.Q, U.q_rs, U.q_cs, voff + v, U.q_aos != 0); }
    // The rows go through LDS and are read back as double4, so that edge_log sees its measurement in the form the staged
    // kernel's load gives it and the compiler contracts the same products (the note at WinIoUser::measurements, window.hip)
    __device__ __forceinline__ const double4 *measurements(double4 *lds, int ne) const {
        for (int k = threadIdx.x; k < ne; k += blockDim.x) lds[k] = ld_row(U.QQ, U.qq_rs, U.qq_cs, eoff + k, U.qq_aos != 0);
        return lds;
    }
    __device__ __forceinline__ double weight(int k) const { return U.w[eoff + k]; }
    __device__ __forceinline__ int2 pair_ids(int q) const { return U.pairs[poff + q]; }
    // view ids (checked) -> operator rows as the host forms them for the staged kernel: i == j is u = 0
    __device__ __forceinline__ int2 pair_rows(int q, int f) const {
        const int2 p = pair_ids(q);
        if (p.x == p.y) return make_int2(-1, -1);
        return make_int2(p.x < f ? -1 : p.x - f, p.y < f ? -1 : p.y - f);
    }
    __device__ __forceinline__ void put_edge(int k, double v, double l, double c) const {
        if (U.edge_var) U.edge_var[eoff + k] = v;
        if (U.leverage) U.leverage[eoff + k] = l;
        if (U.chi2) U.chi2[eoff + k] = c;
    }
    __device__ __forceinline__ void put_pair(int q, double v) const { U.pair_var[poff + q] = v; }
    __device__ __forceinline__ int2 cand_ids(long long q) const { return U.cand[coff + q]; }
    // view ids (checked: inside, i != j) -> operator rows by the pair rule: a fixed end has no coefficient
    __device__ __forceinline__ int2 cand_rows(long long q, int f) const {
        const int2 p = cand_ids(q);
        return make_int2(p.x < f ? -1 : p.x - f, p.y < f ? -1 : p.y - f);
    }
    // n measurements from row c0 into LDS (the caller brackets this with barriers): read back as double4 there, as the
    // edges' are, so that edge_log is handed what the staged kernel's load hands it
    __device__ __forceinline__ const double4 *cand_stage(double4 *lds, long long c0, int n) const {
        for (int k = threadIdx.x; k < n; k += blockDim.x) lds[k] = ld_row(U.CQ, U.cq_rs, U.cq_cs, coff + c0 + k, U.cq_aos != 0);
        return lds;
    }
    // candidate q, the k-th of its chunk: the poses of its ends from LDS, its measurement from the chunk
    __device__ __forceinline__ WinCovCand cand(long long q, int k, const double4 *sQ, const double4 *chunk) const {
        const int2 p = cand_ids(q);
        return WinCovCand{sQ[p.x], sQ[p.y], chunk[k]};
    }
    __device__ __forceinline__ void put_cand(long long q, double a, double v, double c) const {
        if (U.angle) U.angle[coff + q] = a;
        if (U.cand_var) U.cand_var[coff + q] = v;
        if (U.cand_chi2) U.cand_chi2[coff + q] = c;
    }
};

// The gate's arithmetic, one copy for the staged and the batched kernel (they must agree bit for bit): the candidate's
// residual at its ends' poses, its norm, and chi2 = |r|^2 / (s^2 (pair_var + sigma^4)) with sigma^4 = 1 / d0^2, d0 the
// weight of a zero residual.
__device__ __forceinline__ void wc_gate(const WinCovCand &cd, double v, double s2, double sg2, double &angle, double &chi2) {
    double rx, ry, rz;
    edge_log(cd.qi, cd.qj, cd.qq, rx, ry, rz);
    const double e2 = wc_norm2(rx, ry, rz);
    angle = sqrt(e2);
    chi2 = e2 / (s2 * (v + sg2 * sg2));
}

__device__ __forceinline__ void wc_finish(WinCovResult *res, int status, double s2, int seq) {
    res->status = status;
    res->s2 = s2;
    __threadfence_system();
    __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One workgroup, one problem (both entry kernels below run exactly this). L: where its arrays lie in the dynamic LDS.
template <class IO>
__device__ __forceinline__ void wincov_body(const WinCovParams &P, const IO &io, const WinCovLds &L, WinCovResult *res) {
    extern __shared__ double4 wc_lds[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(wc_lds);
    double4 *sQ = reinterpret_cast<double4 *>(lds + L.oQ);
    double4 *sR = reinterpret_cast<double4 *>(lds + L.oR);  // (r_x, r_y, r_z, d)
    double *M = reinterpret_cast<double *>(lds + L.oM);
    int2 *sI = reinterpret_cast<int2 *>(lds + L.oI);
    double *sc = reinterpret_cast<double *>(lds + L.oSc);
    double *colk = reinterpret_cast<double *>(lds + L.oCol);
    double *rowk = reinterpret_cast<double *>(lds + L.oRow);
    double *red = reinterpret_cast<double *>(lds + L.oRed);
    __shared__ int sDead;

    const int t = threadIdx.x, nv = P.nv, f = P.f, ne = P.ne, nu = nv - f;
    const bool ok = nv >= 1 && nv <= WC_MAX_NV && f >= 0 && nu >= 1 && nu <= WC_MAX_NU && ne >= 1 && ne <= WC_MAX_NE &&
                    P.np >= 0 && (IO::kUser || P.np <= WC_MAX_P) && P.nc >= 0 && (IO::kUser || P.nc <= WC_MAX_C);
    if (!ok) {  // (the host checks the same before the launch)
        if (t == 0) wc_finish(res, IROTAVG_ERR_BAD_ARG, NAN, P.seq);
        return;
    }
    if (t == 0) sDead = 0;
    for (int v = t; v < nv; v += WC_THREADS) sQ[v] = io.q(v);
    const double4 *QQ = io.measurements(reinterpret_cast<double4 *>(lds + L.oQQ), ne);
    for (int x = t; x < (IO::kUser ? nu : WC_MAX_NU) * WC_LD; x += WC_THREADS) M[x] = 0.0;
    __syncthreads();
    if constexpr (IO::kUser) {
        // The ids come from the device here and no host has seen them: a workgroup-wide OR before anything is indexed
        // with one (so far LDS and the arrays were indexed with v < nv, k < ne and q < np alone). An id outside refuses
        // the problem: nothing of it is written but its record.
        bool outside = false;
        for (int k = t; k < ne; k += WC_THREADS) {
            const int2 e = io.edge(k);
            outside = outside || (unsigned)e.x >= (unsigned)nv || (unsigned)e.y >= (unsigned)nv;
        }
        for (int q = t; q < P.np; q += WC_THREADS) {
            const int2 p = io.pair_ids(q);
            outside = outside || (unsigned)p.x >= (unsigned)nv || (unsigned)p.y >= (unsigned)nv;
        }
        if constexpr (IO::kCand)
            for (long long q = t; q < P.nc; q += WC_THREADS) {  // i == j is no measurement between two views
                const int2 p = io.cand_ids(q);
                outside = outside || (unsigned)p.x >= (unsigned)nv || (unsigned)p.y >= (unsigned)nv || p.x == p.y;
            }
        if (outside) sDead = 2;
        __syncthreads();
        if (sDead != 0) {
            if (t == 0) wc_finish(res, IROTAVG_ERR_BAD_ARG, NAN, P.seq);
            return;
        }
    }
    // ---- residuals and weights
    const double sg2 = P.sigma * P.sigma;
    for (int k = t; k < ne; k += WC_THREADS) {
        int2 e = io.edge(k);
        if (!IO::kUser && ((unsigned)e.x >= (unsigned)nv || (unsigned)e.y >= (unsigned)nv)) {  // never with the view-graph's own lists
            sDead = 2;
            e = make_int2(0, 0);
        }
        double rx, ry, rz;
        edge_log(sQ[e.x], sQ[e.y], QQ[k], rx, ry, rz);
        sI[k] = e;
        sR[k] = make_double4(rx, ry, rz, P.use_w ? io.weight(k) : 1.0 / (wc_norm2(rx, ry, rz) + sg2));
    }
    __syncthreads();
    // ---- M: row r belongs to thread r. Row k of A (make_A: edge_flags, common.hpp): +1 at a, -1 at b (-1: none)
    if (t < nu) {
        double *row = M + t * WC_LD;
        for (int k = 0; k < ne; k++) {
            const int2 e = sI[k];
            const uint8_t fl = edge_flags(e.x, e.y, f);
            const int a = (fl & EF_CJ) ? e.y - f : -1, b = (fl & EF_CI) ? e.x - f : -1;
            if (a != t && b != t) continue;
            const double d = sR[k].w;
            row[t] = fma(d, d, row[t]);
            if (a >= 0 && b >= 0) row[a == t ? b : a] -= d * d;
        }
    }
    __syncthreads();
    // ---- Jacobi scaling: unit diagonal, so the dead-pivot rule is the row's own
    if (t < nu) {
        const double dg = M[t * WC_LD + t];
        if (!(dg > 0.0) || !(dg < INFINITY)) sDead = 1;
        sc[t] = 1.0 / sqrt(dg);
    }
    __syncthreads();
    const int c = t & 63, r0 = t >> 6;  // the thread's column and first row (rows r0, r0 + 4, ...)
    if (c < nu)
        for (int r = r0; r < nu; r += 4) M[r * WC_LD + c] *= sc[r] * sc[c];
    __syncthreads();
    // ---- Gauss-Jordan in place, no pivoting (symmetric positive definite)
    for (int k = 0; k < nu && sDead == 0; k++) {
        const double p = M[k * WC_LD + k];
        if (!(p > 1e-13)) {  // every thread reads the same value: a uniform exit
            __syncthreads();
            if (t == 0) sDead = 1;
            break;
        }
        const double pinv = 1.0 / p;
        if (t < nu) colk[t] = M[t * WC_LD + k];
        else if (t >= 64 && t < 64 + nu) rowk[t - 64] = M[k * WC_LD + (t - 64)] * pinv;
        __syncthreads();
        if (c < nu) {
            const double rc = rowk[c];
            for (int r = r0; r < nu; r += 4) {
                double v;
                if (r == k) v = c == k ? pinv : rc;
                else if (c == k) v = -colk[r] * pinv;
                else v = fma(-colk[r], rc, M[r * WC_LD + c]);
                M[r * WC_LD + c] = v;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (c < nu)
        for (int r = r0; r < nu; r += 4) M[r * WC_LD + c] *= sc[r] * sc[c];
    __syncthreads();
    // ---- s^2 over the edges with a non-zero row of A: strided partials, then a tree (fixed order)
    {
        double a = 0.0, b = 0.0;
        for (int k = t; k < ne; k += WC_THREADS) {
            if (sI[k].y < f) continue;
            const double4 rr = sR[k];
            a = fma(rr.w * rr.w, wc_norm2(rr.x, rr.y, rr.z), a);
            b += 1.0;
        }
        red[t] = a;
        red[WC_THREADS + t] = b;
        __syncthreads();
        for (int o = WC_THREADS / 2; o > 0; o >>= 1) {
            if (t < o) {
                red[t] += red[t + o];
                red[WC_THREADS + t] += red[WC_THREADS + t + o];
            }
            __syncthreads();
        }
    }
    const double num = red[0], cnt = red[WC_THREADS];
    const double s2 = cnt > nu ? num / (3.0 * (cnt - nu)) : NAN;
    // ---- outputs
    if constexpr (IO::kUser) {
        // The caller's arrays are written only on success: every value that can raise the dead word is looked at first
        // (they all come from LDS), then the workgroup agrees, then it stores.
        if (t < nu && !(fabs(M[t * WC_LD + t]) < INFINITY)) sDead = 1;
        for (int k = t; k < ne; k += WC_THREADS)
            if (!(fabs(wc_edge_var(M, sI[k], f)) < INFINITY)) sDead = 1;
        if constexpr (IO::kCand)
            for (long long q = t; q < P.nc; q += WC_THREADS) {
                const int2 ab = io.cand_rows(q, f);
                if (!(fabs(wc_usu(M, ab.x, ab.y)) < INFINITY)) sDead = 1;
            }
        __syncthreads();
        if (sDead == 0 && io.U.var)
            for (int v = t; v < nv; v += WC_THREADS) io.U.var[io.voff + v] = v < f ? 0.0 : M[(v - f) * WC_LD + (v - f)];
    } else {
        double *var = reinterpret_cast<double *>(io.slot + oVar);
        if (t < nu) {
            const double v = M[t * WC_LD + t];
            if (!(fabs(v) < INFINITY)) sDead = 1;
            if (P.first) var[t] = v;
        }
    }
    const bool store = !IO::kUser || sDead == 0;  // (kUser: uniform, read behind the barrier above)
    constexpr bool kEdgeOut = !(IO::kUser && IO::kCand);  // the batched gate has no edge output: nothing to compute for one
    for (int k = t; k < (kEdgeOut && store && P.first ? ne : 0); k += WC_THREADS) {
        const double4 rr = sR[k];
        const double v = wc_edge_var(M, sI[k], f), w = rr.w * rr.w, l = w * v;
        if (!IO::kUser && !(fabs(v) < INFINITY)) sDead = 1;
        io.put_edge(k, v, l, w * wc_norm2(rr.x, rr.y, rr.z) / (s2 * fmax(0.0, fma(-w, v, 1.0))));
    }
    for (int q = t; q < (store ? P.np : 0); q += WC_THREADS) {
        const int2 ab = io.pair_rows(q, f);
        const bool in = ab.x >= -1 && ab.x < nu && ab.y >= -1 && ab.y < nu;
        io.put_pair(q, in ? wc_usu(M, ab.x, ab.y) : NAN);
    }
    if constexpr (IO::kCand) {
        // the candidates of the gate, a chunk of measurements at a time (kUser: through LDS; the staged form has them all
        // in its slot). The trip counts are uniform: P.nc and `store` are the workgroup's.
        double4 *sC = reinterpret_cast<double4 *>(lds + L.oC);
        for (long long c0 = 0; c0 < (store ? P.nc : 0); c0 += WC_MAX_C) {
            const int n = (int)min((long long)WC_MAX_C, P.nc - c0);
            const double4 *chunk = io.cand_stage(sC, c0, n);
            if constexpr (IO::kUser) __syncthreads();
            for (int k = t; k < n; k += WC_THREADS) {
                const int2 ab = io.cand_rows(c0 + k, f);
                const WinCovCand cd = io.cand(c0 + k, k, sQ, chunk);
                const bool in = ab.x >= -1 && ab.x < nu && ab.y >= -1 && ab.y < nu;
                const double v = in ? wc_usu(M, ab.x, ab.y) : NAN;
                double angle, chi2;
                wc_gate(cd, v, s2, sg2, angle, chi2);
                io.put_cand(c0 + k, angle, v, chi2);
            }
            if constexpr (IO::kUser) __syncthreads();
        }
    }
    __threadfence_system();
    __syncthreads();
    if (t == 0) wc_finish(res, sDead == 0 ? IROTAVG_OK : (sDead == 2 ? IROTAVG_ERR_BAD_ARG : IROTAVG_ERR_SOLVER), s2, P.seq);
}

// the staged form: blockIdx.x selects the slot of the staging block
__global__ __launch_bounds__(WC_THREADS) void k_window_cov(unsigned char *__restrict__ base, size_t stride) {
    unsigned char *slot = base + stride * blockIdx.x;
    const WinCovParams P = *reinterpret_cast<const WinCovParams *>(slot + oP);
    wincov_body(P, WcIoSlot{slot}, kLdsOwn, reinterpret_cast<WinCovResult *>(slot + oRes));
}

// Workgroup b takes the problem of descriptor b on the caller's packed arrays (irotavg_window_uncertainty_batch_dev):
// sizes and offsets from D[b], sigma / the weights switch / the sequence number from Pk, the result to R[D[b].d.idx].
__global__ __launch_bounds__(WC_THREADS) void k_window_cov_user(WinCovParams Pk, const WinCovDesc *__restrict__ D, WinCovUser U,
                                                                WinCovResult *__restrict__ R) {
    const WinCovDesc d = D[blockIdx.x];
    WinCovParams P = Pk;
    P.nv = d.d.nv;
    P.f = d.d.f;
    P.ne = d.d.ne;
    P.np = d.np;
    wincov_body(P, WcIoUser<false>{U, d.d.eoff, d.d.voff, d.poff, 0}, wincov_lds(d.d.nv, d.d.ne, d.d.nv - d.d.f, true), R + d.d.idx);
}

// The same with the candidates of descriptor b (irotavg_window_gate_batch_dev): a second instance of the body, so that
// the one above stays the code it was.
__global__ __launch_bounds__(WC_THREADS) void k_window_gate_user(WinCovParams Pk, const WinCovDesc *__restrict__ D, WinCovUser U,
                                                                 WinCovResult *__restrict__ R) {
    const WinCovDesc d = D[blockIdx.x];
    WinCovParams P = Pk;
    P.nv = d.d.nv;
    P.f = d.d.f;
    P.ne = d.d.ne;
    P.np = d.np;
    P.nc = d.nc;
    wincov_body(P, WcIoUser<true>{U, d.d.eoff, d.d.voff, d.poff, d.coff}, wincov_lds(d.d.nv, d.d.ne, d.d.nv - d.d.f, true, d.nc),
                R + d.d.idx);
}

}  // namespace

struct WinCov {
    hipStream_t stream = nullptr;
    MappedBlock blk;  // one slot
    int seq = 0;
    bool attr_set = false;
    ~WinCov() {
        if (stream) StreamPool::get().give(stream);
    }
};

WinCov *wincov_new() { return new WinCov(); }
void wincov_delete(WinCov *w) { delete w; }

int wincov_query(WinCov &wc, WinCovQuery &q) {
    if (!window_fits(q.nv, q.f, q.ne) || q.np < 0 || q.nc < 0) return IROTAVG_ERR_BAD_ARG;
    static_assert(sizeof(WinCovParams) <= oI, "the parameter record outgrew its place in the slot");
    static_assert(kLds <= WIN_MAX_LDS, "LDS of a gfx950 workgroup");
    if (!wc.stream) wc.stream = StreamPool::get().take();
    wc.blk.reserve(kSlot);
    if (!wc.attr_set) {
        IRH_CHECK(hipFuncSetAttribute((const void *)k_window_cov, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
        wc.attr_set = true;
    }
    unsigned char *h = wc.blk.host;
    std::memcpy(h + oI, q.I, sizeof(int32_t) * 2 * (size_t)q.ne);
    std::memcpy(h + oQQ, q.qq_aos, sizeof(double) * 4 * (size_t)q.ne);
    std::memcpy(h + oQ, q.Q_aos, sizeof(double) * 4 * (size_t)q.nv);
    if (q.weights) std::memcpy(h + oWt, q.weights, sizeof(double) * (size_t)q.ne);
    const int nu = q.nv - q.f;
    // pairs and candidates beyond what one launch stages: further launches of the same problem (bitwise the same Sigma)
    // that leave var and the edge outputs of the first one in the block; the caller's arrays are written after the last
    int p0 = 0, c0 = 0;
    bool first = true;
    while (first || p0 < q.np || c0 < q.nc) {
        const int np = std::min(WC_MAX_P, q.np - p0), nc = std::min(WC_MAX_C, q.nc - c0);
        WinCovParams P{q.nv, q.f, q.ne, np, nc, 0, first ? 1 : 0, q.weights ? 1 : 0, q.sigma};
        P.seq = next_seq(wc.seq);
        std::memcpy(h + oP, &P, sizeof(P));
        if (np > 0) std::memcpy(h + oPR, q.prow + 2 * (size_t)p0, sizeof(int32_t) * 2 * (size_t)np);
        if (nc > 0) {
            std::memcpy(h + oCR, q.crow + 2 * (size_t)c0, sizeof(int32_t) * 2 * (size_t)nc);
            std::memcpy(h + oCQ, q.cq + 12 * (size_t)c0, sizeof(double) * 12 * (size_t)nc);
        }
        WinCovResult *res = reinterpret_cast<WinCovResult *>(h + oRes);
        res->seq = 0;
        hipLaunchKernelGGL(k_window_cov, dim3(1), dim3(WC_THREADS), kLds, wc.stream, wc.blk.hdev, kSlot);
        IRH_CHECK(hipGetLastError());
        if (!wait_seq(&res->seq, 0, 1, P.seq, 2e-3)) IRH_CHECK(hipStreamSynchronize(wc.stream));
        if (res->status != IROTAVG_OK) return res->status;  // outputs untouched
        if (first) q.s2 = res->s2;
        if (np > 0) std::memcpy(q.pair_var + p0, h + oPv, sizeof(double) * (size_t)np);
        if (nc > 0) {
            const double *ca = reinterpret_cast<const double *>(h + oCa);
            std::memcpy(q.angle + c0, ca, sizeof(double) * (size_t)nc);
            std::memcpy(q.cand_var + c0, ca + WC_MAX_C, sizeof(double) * (size_t)nc);
            std::memcpy(q.cand_chi2 + c0, ca + 2 * WC_MAX_C, sizeof(double) * (size_t)nc);
        }
        p0 += np;
        c0 += nc;
        first = false;
    }
    if (q.var) std::memcpy(q.var, h + oVar, sizeof(double) * (size_t)nu);
    if (q.edge_var) std::memcpy(q.edge_var, h + oEv, sizeof(double) * (size_t)q.ne);
    if (q.leverage) std::memcpy(q.leverage, h + oLev, sizeof(double) * (size_t)q.ne);
    if (q.chi2) std::memcpy(q.chi2, h + oChi, sizeof(double) * (size_t)q.ne);
    return IROTAVG_OK;
}

// ---- irotavg_window_uncertainty_batch_dev: many problems on the caller's device arrays ------------------------------
// The block of records and descriptors, the sequence number and the lock: batchdev.hpp (one instance for both calls).
// k_window_cov_user / k_window_gate_user may use the LDS of a problem at the limits on this device (under the driver's lock)
static int wincov_attr_device[2] = {-1, -1};

// the arguments have been checked (devapi.hip) and `plan` made from the caller's sizes and pair counts (winbatch.hpp)
int wincov_batch_dev(const WinCovPlan &plan, int device, const WinCovArrays &A, double sigma, double *scale, int32_t *results,
                     hipStream_t stream) {
    auto &drv = BatchDev<WinCovResult, WinCovDesc>::get();
    const size_t nb = plan.desc.size();
    const auto s = drv.stage(plan.desc.data(), nb);
    const WinCovParams P{0, 0, 0, 0, 0, s.seq, 1, A.weights ? 1 : 0, sigma};
    const WinCovUser U{reinterpret_cast<const int2 *>(A.I), A.QQ, A.qq_rs, A.qq_cs, A.Q, A.q_rs, A.q_cs, A.weights, A.var,
                       reinterpret_cast<const int2 *>(A.pairs), A.pair_var, A.edge_var, A.leverage, A.chi2,
                       rows16(reinterpret_cast<uintptr_t>(A.QQ), A.qq_rs, A.qq_cs),
                       rows16(reinterpret_cast<uintptr_t>(A.Q), A.q_rs, A.q_cs),
                       reinterpret_cast<const int2 *>(A.cand), A.cand_QQ, A.cq_rs, A.cq_cs, A.angle, A.cand_var, A.cand_chi2,
                       A.cand_QQ ? rows16(reinterpret_cast<uintptr_t>(A.cand_QQ), A.cq_rs, A.cq_cs) : 0};
    const auto kernel = A.gate ? k_window_gate_user : k_window_cov_user;
    if (wincov_attr_device[A.gate] != device) {
        const size_t most = wincov_lds(WC_MAX_NV, WC_MAX_NE, WC_MAX_NU, true, A.gate ? WINCOV_CAND_CHUNK : 0).bytes;
        IRH_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        wincov_attr_device[A.gate] = device;
    }
    // the LDS of the largest problem of THIS batch: small problems share a compute unit
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(WC_THREADS), plan.lds, stream, P, s.D, U, s.Rd);
    IRH_CHECK(hipGetLastError());
    return drv.finish(s, stream, nb, [&](size_t b, const WinCovResult &r) {  // (record b is problem b: the plan keeps the caller's order)
        if (results) results[b] = r.status;
        if (scale && r.status == IROTAVG_OK) scale[b] = r.s2;
    });
}

}  // namespace irh
