// winbatch.hpp -- the host arithmetic of the window kernels, of irotavg_window_solve_batch_dev and of
// irotavg_window_uncertainty_batch_dev / irotavg_window_gate_batch_dev: size limits, the staging layout, the stride rule of
// the `_dev` API, the plan of a batch (offsets and descriptors from `sizes`), the LDS layout and the pair and candidate
// offsets of the uncertainty kernels. Plain C++ with no HIP
// type in it, so that a stand-alone program can run all of it under a sanitizer on a machine without a device
// (tools/winbatch_host_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace irh {

constexpr int WIN_MAX_NU = 64;    // free views
constexpr int WIN_MAX_NV = 320;   // all views of the sub-problem
constexpr int WIN_MAX_NE = 640;   // edges
constexpr int SM_MAX_NE = 64;     // the wave-resident kernel
constexpr int SM_MAX_NU = 16;
constexpr size_t WIN_MAX_LDS = 160 * 1024;
constexpr int64_t WIN_BATCH_MAX = 262144;  // problems of one irotavg_window_solve_batch_dev call

// dynamic LDS of the general kernel (32 = sizeof(double4), 8 = sizeof(int2): window.hip asserts both)
constexpr size_t win_lds_bytes(int nv, int ne, int nu) {
    return 32 * (size_t)nv +
           sizeof(double) * ((size_t)4 * ne + ne + 3 * nu + (size_t)nu * (nu + 1) + 3 * nu + 12 * (size_t)ne +
                             5 * nu + 16) +
           8 * (size_t)ne + (size_t)ne + 64;
}
// the batched general kernel also keeps the problem's measurements in LDS, one double4 per edge (see WinIoUser)
constexpr size_t win_lds_bytes_user(int nv, int ne, int nu) { return win_lds_bytes(nv, ne, nu) + 32 * (size_t)ne; }
static_assert(win_lds_bytes_user(WIN_MAX_NV, WIN_MAX_NE, WIN_MAX_NU) <= WIN_MAX_LDS,
              "every term grows with its size: a problem inside the limits fits");
inline bool win_fits_wave(int nv, int f, int ne) {
    const int64_t nu = (int64_t)nv - f;
    return nu >= 1 && nu <= SM_MAX_NU && nv <= WIN_MAX_NV && ne >= 1 && ne <= SM_MAX_NE;
}
inline bool win_fits(int nv, int f, int ne) {
    const int64_t nu = (int64_t)nv - f;
    return nu >= 1 && nu <= WIN_MAX_NU && nv <= WIN_MAX_NV && ne >= 1 && ne <= WIN_MAX_NE &&
           win_lds_bytes(nv, ne, (int)nu) <= WIN_MAX_LDS;
}

// what a workgroup of the window kernels is told and what it leaves (no HIP type: the staging layout below counts them)
struct WinParams {
    int nv, f, ne;
    int l1_max, irls_max, cost;
    double change_th, sigma;
    int seq;  // k_window_wave stores it into WinResult::seq LAST (system scope): the host polls for it
};
struct WinResult {
    int l1_iters, irls_iters, status, seq;
    double l1_score, irls_score;
    long long stamp[8];  // development aid (IROTAVG_WINDOW_STAMPS=1 prints them): s_memtime at the phase boundaries of k_window_wave
};
// The library's own staging of one problem, [I | QQ | Q | weights | result | params], for max_ne edges and WIN_MAX_NV
// views. window_solve: one problem, the block ends at oP (the parameters are a kernel argument); window_solve_batch: slots
// of `stride` bytes.
struct WinStage {
    size_t oI, oQQ, oQ, oW, oR, oP, stride;
};
constexpr WinStage win_stage(int max_ne) {
    const size_t oQQ = 8 * (size_t)max_ne, oQ = oQQ + 32 * (size_t)max_ne, oW = oQ + 32 * (size_t)WIN_MAX_NV;
    const size_t oR = oW + sizeof(double) * (size_t)max_ne, oP = oR + sizeof(WinResult);
    return WinStage{0, oQQ, oQ, oW, oR, oP, (oP + sizeof(WinParams) + 255) & ~(size_t)255};
}
constexpr WinStage kStageOwn = win_stage(WIN_MAX_NE), kStageBatch = win_stage(SM_MAX_NE);
static_assert(kStageOwn.oQQ == 5120 && kStageOwn.oQ == 25600 && kStageOwn.oW == 35840 && kStageOwn.oR == 40960 &&
                  kStageOwn.oP == 41056 && kStageBatch.oQQ == 512 && kStageBatch.oQ == 2560 && kStageBatch.oW == 12800 &&
                  kStageBatch.oR == 13312 && kStageBatch.oP == 13408 && kStageBatch.stride == 13568,
              "the byte offsets the kernels of both forms have always been given");

// Rows of four contiguous doubles behind a 16-byte aligned pointer: the one case in which the kernels of the `_dev` API
// move a row with 16-byte accesses (window.hip: ld_row / st_row, devapi.hip: the AoS path).
inline bool rows16(uintptr_t p, int64_t rs, int64_t cs) { return rs == 4 && cs == 1 && (p & 15) == 0; }

// A strided rows x cols matrix does not alias itself when its rows do not overlap (|rs| >= cols |cs|) or its columns
// do not (|cs| >= rows |rs|), both strides non-zero and at most 2^31: the rule include/irotavg_hip.h states.
inline bool strides_ok(int64_t rows, int cols, int64_t rs, int64_t cs) {
    const int64_t lim = (int64_t)1 << 31;
    if (rs == 0 || cs == 0 || rs > lim || rs < -lim || cs > lim || cs < -lim || rows <= 0 || rows > lim) return false;
    const int64_t a = rs < 0 ? -rs : rs, b = cs < 0 ? -cs : cs;
    return a >= (int64_t)cols * b || b >= rows * a;
}
// element offsets of the lowest and the highest element of such a matrix (negative strides reach below the pointer)
inline void matrix_span(int64_t rows, int cols, int64_t rs, int64_t cs, int64_t &lo, int64_t &hi) {
    const int64_t r = (rows - 1) * rs, c = (int64_t)(cols - 1) * cs;
    lo = (r < 0 ? r : 0) + (c < 0 ? c : 0);
    hi = (r > 0 ? r : 0) + (c > 0 ? c : 0);
}

// Are the bytes [first, end) covered by allocations without a gap? range(at, base, size) names the allocation around
// the address `at` (false: the asked party knows none). 1: yes, the allocation around `first` reaches `end`, or
// allocations that follow it without a gap do (a reservation mapped piece by piece; at most 64 of them); 0: no, a gap or
// nothing known before `end`, or end <= first; -1: not even the allocation around `first` could be named.
template <class Range>
inline int span_covered(uintptr_t first, uintptr_t end, Range &&range) {
    if (end <= first) return 0;
    uintptr_t at = first;
    for (int hops = 0; hops < 64; hops++) {
        uintptr_t base = 0;
        size_t size = 0;
        if (!range(at, base, size) || base > at || size <= at - base) return hops == 0 ? -1 : 0;
        if (end - base <= size) return 1;
        at = base + size;
    }
    return 0;
}

// one problem of a batch as its workgroup reads it: sizes, first row of its edges / views in the packed arrays, and its
// place in the caller's order (the row of `results`)
struct WinDesc {
    int nv, f, ne, idx;
    long long eoff, voff;
};
struct WinBatchPlan {
    std::vector<WinDesc> desc;  // the wave kernel's list, then the general kernel's, each in the caller's order
    int64_t nwave = 0;          // length of the first list
    int64_t sum_m = 0, sum_n = 0;
    size_t lds = 0;             // largest win_lds_bytes_user of the general list
};
// sizes = (n_total, f, m) per problem. kernel: 0 per problem as window_solve chooses, 1 / 2 one kernel for all.
// false: a bad count, a problem the kernels (or the forced kernel) do not take, or a kernel outside 0..2.
inline bool winbatch_plan(int64_t nb, const int32_t *sizes, int kernel, WinBatchPlan &out) {
    if (nb <= 0 || nb > WIN_BATCH_MAX || !sizes || kernel < 0 || kernel > 2) return false;
    int64_t nwave = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int nv = sizes[3 * b], f = sizes[3 * b + 1], ne = sizes[3 * b + 2];
        if (nv <= 0 || f < 0 || f >= nv || !win_fits(nv, f, ne)) return false;
        const bool fw = win_fits_wave(nv, f, ne);
        if (kernel == 2 && !fw) return false;
        if (kernel == 2 || (kernel == 0 && fw)) nwave++;
    }
    out.desc.assign((size_t)nb, WinDesc{});
    out.nwave = nwave;
    out.lds = 0;
    int64_t iw = 0, ig = nwave, eoff = 0, voff = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int nv = sizes[3 * b], f = sizes[3 * b + 1], ne = sizes[3 * b + 2];
        const bool wave = kernel == 2 || (kernel == 0 && win_fits_wave(nv, f, ne));
        WinDesc &d = out.desc[(size_t)(wave ? iw++ : ig++)];
        d = WinDesc{nv, f, ne, (int)b, (long long)eoff, (long long)voff};
        if (!wave) {
            const size_t l = win_lds_bytes_user(nv, ne, nv - f);
            if (l > out.lds) out.lds = l;
        }
        eoff += ne;
        voff += nv;
    }
    out.sum_m = eoff;
    out.sum_n = voff;
    return true;
}

// The pinned block of a batched call on device arrays (batchdev.hpp): nb result records of `rec` bytes, then nb
// descriptors of `desc` bytes at oD. A block that has to grow is allocated with half as much again.
struct BatchBlock {
    size_t oD, bytes, headroom;
};
constexpr BatchBlock batch_block(size_t rec, size_t desc, size_t nb) {
    return BatchBlock{rec * nb, (rec + desc) * nb, (rec + desc) * nb / 2};
}

// ---- the uncertainty of such problems: k_window_cov / k_window_cov_user (wincov.hip), irotavg_window_uncertainty[_batch_dev]
constexpr int WINCOV_THREADS = 256;
constexpr int WINCOV_LD = WIN_MAX_NU + 1;  // row stride of M in LDS (bank spread), whatever the problem's nu
constexpr int WINCOV_CAND_CHUNK = 256;     // candidate measurements the batched gate keeps in LDS at a time (8 KB)
// dynamic LDS of one workgroup, in bytes from its base: the quaternions, (stage: the measurements, as WinIoUser keeps
// them,) per edge the residual and the weight, M, the endpoints, three vectors of nu, the reduction scratch, (a batched
// problem with nc candidates: one chunk of their measurements)
struct WinCovLds {
    size_t oQ, oQQ, oR, oM, oI, oSc, oCol, oRow, oRed, oC, bytes;
};
constexpr WinCovLds wincov_lds(int nv, int ne, int nu, bool stage, int nc = 0) {
    const size_t oQQ = 32 * (size_t)nv, oR = oQQ + (stage ? 32 * (size_t)ne : 0), oM = oR + 32 * (size_t)ne;
    const size_t oI = oM + sizeof(double) * (size_t)nu * WINCOV_LD, oSc = oI + 8 * (size_t)ne;
    const size_t oCol = oSc + sizeof(double) * (size_t)nu, oRow = oCol + sizeof(double) * (size_t)nu;
    const size_t oRed = oRow + sizeof(double) * (size_t)nu;
    const size_t end = oRed + sizeof(double) * 2 * WINCOV_THREADS, rows = nc < WINCOV_CAND_CHUNK ? (nc > 0 ? nc : 0) : WINCOV_CAND_CHUNK;
    const size_t oC = (end + 31) & ~(size_t)31;  // double4 rows (the vectors before it leave `end` on 8 bytes)
    return WinCovLds{0, oQQ, oR, oM, oI, oSc, oCol, oRow, oRed, oC, rows ? oC + 32 * rows : end};
}
static_assert(wincov_lds(WIN_MAX_NV, WIN_MAX_NE, WIN_MAX_NU, true, 0x7fffffff).bytes <= WIN_MAX_LDS,
              "every term grows with its size: a problem inside the limits fits");

// what a workgroup of the uncertainty kernels leaves: the sequence number last, as WinResult::seq
struct WinCovResult {
    int status, seq;
    double s2;
};
// one problem of irotavg_window_uncertainty_batch_dev / irotavg_window_gate_batch_dev: the solve's descriptor, then its
// pairs in the packed pair arrays and its candidates in the packed candidate arrays
struct WinCovDesc {
    WinDesc d;
    long long poff, coff;
    int np, nc;
};
struct WinCovPlan {
    std::vector<WinCovDesc> desc;  // in the caller's order
    int64_t sum_m = 0, sum_n = 0, sum_p = 0, sum_c = 0;
    size_t lds = 0;  // largest wincov_lds(..., true, nc).bytes of the batch
};
// sizes as winbatch_plan takes them (the same limits); npairs / ncand: nb counts each or nullptr (none anywhere).
// false: what winbatch_plan refuses, or a negative count.
inline bool wincov_plan(int64_t nb, const int32_t *sizes, const int32_t *npairs, const int32_t *ncand, WinCovPlan &out) {
    WinBatchPlan base;
    if (!winbatch_plan(nb, sizes, 1, base)) return false;  // kernel 1: one list, in the caller's order
    for (int64_t b = 0; b < nb; b++)
        if ((npairs && npairs[b] < 0) || (ncand && ncand[b] < 0)) return false;
    out.desc.assign((size_t)nb, WinCovDesc{});
    out.lds = 0;
    int64_t poff = 0, coff = 0;
    for (int64_t b = 0; b < nb; b++) {
        const WinDesc &d = base.desc[(size_t)b];
        const int np = npairs ? npairs[b] : 0, nc = ncand ? ncand[b] : 0;
        out.desc[(size_t)b] = WinCovDesc{d, (long long)poff, (long long)coff, np, nc};
        const size_t l = wincov_lds(d.nv, d.ne, d.nv - d.f, true, nc).bytes;
        if (l > out.lds) out.lds = l;
        poff += np;
        coff += nc;
    }
    out.sum_m = base.sum_m;
    out.sum_n = base.sum_n;
    out.sum_p = poff;
    out.sum_c = coff;
    return true;
}
// A query must ask for something: pose variances, pair variances, an edge output or the scale. (Pairs are asked for by
// a positive count; the count needs both of its arrays.)
inline bool wincov_asked(bool var, int64_t pairs, bool pair_arrays, bool edge_var, bool leverage, bool chi2, bool scale) {
    if (pairs < 0 || (pairs > 0 && !pair_arrays)) return false;
    return var || pairs > 0 || edge_var || leverage || chi2 || scale;
}
// The gate must ask for something too: an output array with candidates to fill it, or the scale. (A positive count needs
// both candidate arrays.)
inline bool wingate_asked(int64_t cands, bool cand_arrays, bool angle, bool pair_var, bool chi2, bool scale) {
    if (cands < 0 || (cands > 0 && !cand_arrays)) return false;
    return (cands > 0 && (angle || pair_var || chi2)) || scale;
}

}  // namespace irh
