// wincov.hip -- uncertainty of a window-size problem in ONE kernel launch (docs/viewgraph_uncertainty.md): what
// irotavg_viewgraph_rotation_variance / _edge_diagnostics / _gate_connections run for every problem window_fits accepts
// (<= 64 free views, <= 640 edges, <= 320 views: every rotAvg(10)). No handle is involved.
//
// One workgroup per problem (blockIdx.x selects the slot of the staging block, so a batched entry point can follow);
// everything stays in LDS: the quaternions (10 KB), per edge the endpoints, the residual and the weight (25 KB), the
// operator M = A' diag(d^2) A (33 KB), inverted in place.
//   1. residuals r_k (K1's formula) and weights d_k = 1 / (|r_k|^2 + sigma^2): Geman-McClure at a zero step
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

#include "graph.hpp"
#include "kernels.hpp"

namespace irh {
namespace {

constexpr int WC_MAX_NU = 64, WC_MAX_NV = 320, WC_MAX_NE = 640;  // window_fits' limits
constexpr int WC_MAX_P = 1024;                                   // pairs staged per launch
constexpr int WC_MAX_C = 256;                                    // candidates staged per launch
constexpr int WC_LD = WC_MAX_NU + 1;                             // row stride of M in LDS (bank spread)
constexpr int WC_THREADS = 256;

struct WinCovParams {
    int nv, f, ne, np, nc, seq;
    int first;  // 0: a further launch of the same problem for more pairs / candidates -- var and the edge outputs stay
    double sigma;
};
struct WinCovResult {
    int status, seq;
    double s2;
};
struct WinCovCand {  // a candidate connection (lo, hi, R): rows of its ends (-1 held, -2 not in the problem)
    double4 qi, qj, qq;
};

// the slot of one problem in the staging block
constexpr size_t oP = 0;
constexpr size_t oI = 64;
constexpr size_t oQQ = oI + sizeof(int2) * WC_MAX_NE;
constexpr size_t oQ = oQQ + sizeof(double4) * WC_MAX_NE;
constexpr size_t oPR = oQ + sizeof(double4) * WC_MAX_NV;       // pair rows
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

// LDS layout (dynamic: above the 64 KB a static allocation may take)
constexpr size_t sQ_ = 0;
constexpr size_t sR_ = sQ_ + sizeof(double4) * WC_MAX_NV;
constexpr size_t sM_ = sR_ + sizeof(double4) * WC_MAX_NE;
constexpr size_t sI_ = sM_ + sizeof(double) * WC_MAX_NU * WC_LD;
constexpr size_t sSc_ = sI_ + sizeof(int2) * WC_MAX_NE;
constexpr size_t sCol_ = sSc_ + sizeof(double) * WC_MAX_NU;
constexpr size_t sRow_ = sCol_ + sizeof(double) * WC_MAX_NU;
constexpr size_t sRed_ = sRow_ + sizeof(double) * WC_MAX_NU;
constexpr size_t kLds = sRed_ + sizeof(double) * 2 * WC_THREADS;

// u' Sigma u from the resident Sigma; a, b: the rows of the +1 / -1 coefficient (-1: none)
__device__ __forceinline__ double wc_usu(const double *M, int a, int b) {
    double v = 0.0;
    if (a >= 0) v += M[a * WC_LD + a];
    if (b >= 0) v += M[b * WC_LD + b];
    if (a >= 0 && b >= 0) v -= M[a * WC_LD + b] + M[b * WC_LD + a];
    return v;
}

__global__ __launch_bounds__(WC_THREADS) void k_window_cov(unsigned char *__restrict__ base, size_t stride) {
    extern __shared__ double4 wc_lds[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(wc_lds);
    double4 *sQ = reinterpret_cast<double4 *>(lds + sQ_);
    double4 *sR = reinterpret_cast<double4 *>(lds + sR_);  // (r_x, r_y, r_z, d)
    double *M = reinterpret_cast<double *>(lds + sM_);
    int2 *sI = reinterpret_cast<int2 *>(lds + sI_);
    double *sc = reinterpret_cast<double *>(lds + sSc_);
    double *colk = reinterpret_cast<double *>(lds + sCol_);
    double *rowk = reinterpret_cast<double *>(lds + sRow_);
    double *red = reinterpret_cast<double *>(lds + sRed_);
    __shared__ int sDead;

    unsigned char *slot = base + stride * blockIdx.x;
    const WinCovParams P = *reinterpret_cast<const WinCovParams *>(slot + oP);
    WinCovResult *res = reinterpret_cast<WinCovResult *>(slot + oRes);
    const int t = threadIdx.x, nv = P.nv, f = P.f, ne = P.ne, nu = nv - f;
    const bool ok = nv >= 1 && nv <= WC_MAX_NV && f >= 0 && nu >= 1 && nu <= WC_MAX_NU && ne >= 1 && ne <= WC_MAX_NE &&
                    P.np >= 0 && P.np <= WC_MAX_P && P.nc >= 0 && P.nc <= WC_MAX_C;
    if (!ok) {  // (the host checks the same before the launch)
        if (t == 0) {
            res->status = IROTAVG_ERR_BAD_ARG;
            res->s2 = NAN;
            __threadfence_system();
            __hip_atomic_store(&res->seq, P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (t == 0) sDead = 0;
    const double4 *Qg = reinterpret_cast<const double4 *>(slot + oQ);
    const double4 *QQg = reinterpret_cast<const double4 *>(slot + oQQ);
    const int2 *Ig = reinterpret_cast<const int2 *>(slot + oI);
    for (int v = t; v < nv; v += WC_THREADS) sQ[v] = Qg[v];
    for (int x = t; x < WC_MAX_NU * WC_LD; x += WC_THREADS) M[x] = 0.0;
    __syncthreads();
    // ---- residuals and weights
    const double sg2 = P.sigma * P.sigma;
    for (int k = t; k < ne; k += WC_THREADS) {
        int2 e = Ig[k];
        if ((unsigned)e.x >= (unsigned)nv || (unsigned)e.y >= (unsigned)nv) {  // never with the view-graph's own lists
            sDead = 2;
            e = make_int2(0, 0);
        }
        double rx, ry, rz;
        edge_log(sQ[e.x], sQ[e.y], QQg[k], rx, ry, rz);
        sI[k] = e;
        sR[k] = make_double4(rx, ry, rz, 1.0 / (rx * rx + ry * ry + rz * rz + sg2));
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
            const double d = sR[k].w, w = d * d;
            row[t] += w;
            if (a >= 0 && b >= 0) row[a == t ? b : a] -= w;
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
                else v = M[r * WC_LD + c] - colk[r] * rc;
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
            a += rr.w * rr.w * (rr.x * rr.x + rr.y * rr.y + rr.z * rr.z);
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
    double *var = reinterpret_cast<double *>(slot + oVar);
    if (t < nu) {
        const double v = M[t * WC_LD + t];
        if (!(fabs(v) < INFINITY)) sDead = 1;
        if (P.first) var[t] = v;
    }
    double *ev = reinterpret_cast<double *>(slot + oEv), *lev = reinterpret_cast<double *>(slot + oLev);
    double *chi = reinterpret_cast<double *>(slot + oChi);
    for (int k = t; k < (P.first ? ne : 0); k += WC_THREADS) {
        const int2 e = sI[k];
        const double4 rr = sR[k];
        const uint8_t fl = edge_flags(e.x, e.y, f);
        const int a = (fl & EF_CJ) ? e.y - f : -1, b = (fl & EF_CI) ? e.x - f : -1;
        const double v = wc_usu(M, a, b), w = rr.w * rr.w, l = w * v;
        if (!(fabs(v) < INFINITY)) sDead = 1;
        ev[k] = v;
        lev[k] = l;
        chi[k] = w * (rr.x * rr.x + rr.y * rr.y + rr.z * rr.z) / (s2 * fmax(0.0, 1.0 - l));
    }
    const int2 *pr = reinterpret_cast<const int2 *>(slot + oPR);
    double *pv = reinterpret_cast<double *>(slot + oPv);
    for (int q = t; q < P.np; q += WC_THREADS) {
        const int2 ab = pr[q];
        const bool in = ab.x >= -1 && ab.x < nu && ab.y >= -1 && ab.y < nu;
        pv[q] = in ? wc_usu(M, ab.x, ab.y) : NAN;
    }
    const int2 *cr = reinterpret_cast<const int2 *>(slot + oCR);
    const WinCovCand *cq = reinterpret_cast<const WinCovCand *>(slot + oCQ);
    double *ca = reinterpret_cast<double *>(slot + oCa);
    for (int q = t; q < P.nc; q += WC_THREADS) {
        const int2 ab = cr[q];
        const WinCovCand cd = cq[q];
        double rx, ry, rz;
        edge_log(cd.qi, cd.qj, cd.qq, rx, ry, rz);
        const double e2 = rx * rx + ry * ry + rz * rz;
        const bool in = ab.x >= -1 && ab.x < nu && ab.y >= -1 && ab.y < nu;
        const double v = in ? wc_usu(M, ab.x, ab.y) : NAN;
        ca[q] = sqrt(e2);
        ca[WC_MAX_C + q] = v;
        ca[2 * WC_MAX_C + q] = e2 / (s2 * (v + sg2 * sg2));  // sigma^4 = 1 / d0^2, d0 the weight of a zero residual
    }
    __threadfence_system();
    __syncthreads();
    if (t == 0) {
        res->status = sDead == 0 ? IROTAVG_OK : (sDead == 2 ? IROTAVG_ERR_BAD_ARG : IROTAVG_ERR_SOLVER);
        res->s2 = s2;
        __threadfence_system();
        __hip_atomic_store(&res->seq, P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
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
    static_assert(kLds <= 160 * 1024, "LDS of a gfx950 workgroup");
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
    const int nu = q.nv - q.f;
    // pairs and candidates beyond what one launch stages: further launches of the same problem (bitwise the same Sigma)
    // that leave var and the edge outputs of the first one in the block; the caller's arrays are written after the last
    int p0 = 0, c0 = 0;
    bool first = true;
    while (first || p0 < q.np || c0 < q.nc) {
        const int np = std::min(WC_MAX_P, q.np - p0), nc = std::min(WC_MAX_C, q.nc - c0);
        WinCovParams P{q.nv, q.f, q.ne, np, nc, 0, first ? 1 : 0, q.sigma};
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

}  // namespace irh
