// asm0w.hpp -- K3, windowed form: the assembly of ONE 64-row slice of level 0 as a device function, so that the
// stand-alone kernel (k_assemble0w, solver.hip) and the level-0 reduction of the banded direct solver that assembles
// its own slices first (k_bcr_reduce<..., ASM = true>, bcr.hip) run the same instructions on the same inputs.
#pragma once
#include "kernels.hpp"

namespace irh {

constexpr int kAsmWin = 1664;  // edges staged per slice: (64 + 19) * 19 = 1577 at 100k views / 2M edges
constexpr int kAsmCW = 8;      // level-1 entries per row handled in the fused form
// (one pad word per 64: the rows of a wave read edges a constant stride apart -- 20 per row on the headline graph --,
// and a stride of 4 mod 16 doubles puts every fourth lane on the same banks)
constexpr int kAsmWinPad = kAsmWin + kAsmWin / 32 + 1;

// the slice's LDS, carved from one buffer: sT (planes of the staged window), part (partial row sums of the four
// waves), acc1 (level-1 accumulators, L1 only), sEx (the rows' excess, L1 only)
template <int MODE, bool L1>
struct Asm0wLds {
    static constexpr int NP = MODE == 0 ? 4 : (MODE == 2 ? 2 : 1);  // planes: w | w r_x | w r_y | w r_z
    static constexpr int oPart = NP * kAsmWinPad;
    static constexpr int oAcc1 = oPart + NP * 4 * 64;
    static constexpr int oEx = oAcc1 + (L1 ? 4 * kAsmCW * 64 : 0);
    static constexpr int doubles = oEx + (L1 ? 64 : 0);
};

// One slice by the first four waves of a workgroup of NT threads (NT > kRowBlock: the other waves only keep the
// barriers company). Two workgroup barriers (three with L1); the caller puts one more between two slices that share `lds`.
template <int MODE, bool L1, int NT>
__device__ __forceinline__ void asm0w_slice(
    const int sl, double *lds, int n, long long m, long long mpad, const int *__restrict__ sl_off,
    const uint32_t *__restrict__ slot_eid, const uint8_t *__restrict__ slot_cs,
    const int *__restrict__ tile_e0, const int *__restrict__ bptr, const uint32_t *__restrict__ beid,
    const uint8_t *__restrict__ bflag, const double *__restrict__ wsrc, const double *__restrict__ er,
    double *__restrict__ val, double *__restrict__ excess, double *__restrict__ diag,
    double *__restrict__ idg, double4 *__restrict__ rhs, double *__restrict__ bval, int n1,
    const int *__restrict__ sl_off1, double *__restrict__ val1, double *__restrict__ excess1,
    double *__restrict__ diag1, double *__restrict__ idg1) {
    typedef Asm0wLds<MODE, L1> Lds;
    double(*sT)[kAsmWinPad] = reinterpret_cast<double(*)[kAsmWinPad]>(lds);
    double(*part)[4][64] = reinterpret_cast<double(*)[4][64]>(lds + Lds::oPart);
    double(*acc1)[L1 ? kAsmCW : 1][64] = reinterpret_cast<double(*)[L1 ? kAsmCW : 1][64]>(lds + Lds::oAcc1);
    double *sEx = lds + Lds::oEx;
#define IRH_QI(q) ((q) + ((q) >> 5))
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = NT == kRowBlock || tid < kRowBlock;
    const int e0 = tile_e0[sl];
    const int row = sl * 64 + lane;
    const int o0 = sl_off[sl], np = on ? (sl_off[sl + 1] - o0) / 2 : 0;
    const uint2 *__restrict__ se_p = reinterpret_cast<const uint2 *>(slot_eid) + (size_t)(o0 / 2) * 64 + lane;
    const uint16_t *__restrict__ cs_p = reinterpret_cast<const uint16_t *>(slot_cs) + (size_t)(o0 / 2) * 64 + lane;
    double2 *__restrict__ v_p = reinterpret_cast<double2 *>(val) + (size_t)(o0 / 2) * 64 + lane;
    constexpr int PB = 6;  // pairs in flight per wave (rows of up to 48 entries in one batch)
    uint2 se[PB];
    uint32_t cc[PB];
    auto load_batch = [&](int p0) {  // entry pairs p0, p0 + 4, ... of this wave
#pragma unroll
        for (int u = 0; u < PB; u++) {
            const int p = p0 + 4 * u;
            se[u] = make_uint2(0xffffffffu, 0xffffffffu);
            cc[u] = 0xffffu;
            if (p < np) {
                se[u] = se_p[(size_t)p * 64];
                if (L1) cc[u] = cs_p[(size_t)p * 64];
            }
        }
    };
    load_batch(wave);  // in flight while the window is staged
    if (on) {
        constexpr int NQ = (kAsmWin + kRowBlock - 1) / kRowBlock;
        double rw[NQ], rx[NQ], ry[NQ], rz[NQ];
#pragma unroll
        for (int it = 0; it < NQ; it++) {  // all loads first
            const int q = tid + it * kRowBlock;
            const long long e = (long long)e0 + q;
            rw[it] = rx[it] = ry[it] = rz[it] = 0.0;
            if (q < kAsmWin && e < m) {
                rw[it] = wsrc[e];
                if (MODE == 0) {
                    rx[it] = er[e];
                    ry[it] = er[mpad + e];
                    rz[it] = er[2 * mpad + e];
                }
                if (MODE == 2) rx[it] = er[e];
            }
        }
#pragma unroll
        for (int it = 0; it < NQ; it++) {
            const int q = tid + it * kRowBlock;
            if (q < kAsmWin) {
                const double w = MODE == 0 ? rw[it] * rw[it] : rw[it];
                sT[0][IRH_QI(q)] = w;
                if (MODE == 0) {
                    sT[1][IRH_QI(q)] = w * rx[it];
                    sT[2][IRH_QI(q)] = w * ry[it];
                    sT[3][IRH_QI(q)] = w * rz[it];
                }
                if (MODE == 2) sT[1][IRH_QI(q)] = rx[it];
            }
        }
    }
    if (L1 && on) {
#pragma unroll
        for (int c = 0; c < kAsmCW; c++) acc1[wave][c][lane] = 0.0;
    }
    __syncthreads();
    auto fetch = [&](uint32_t e, double &w, double &x, double &y, double &z) {
        const uint32_t q = e - (uint32_t)e0;
        if (q < (uint32_t)kAsmWin) {
            w = sT[0][IRH_QI(q)];
            if (MODE == 0) {
                x = sT[1][IRH_QI(q)];
                y = sT[2][IRH_QI(q)];
                z = sT[3][IRH_QI(q)];
            }
            if (MODE == 2) x = sT[1][IRH_QI(q)];
        } else {
            w = wsrc[e];
            if (MODE == 0) {
                w *= w;
                x = w * er[e];
                y = w * er[mpad + e];
                z = w * er[2 * mpad + e];
            }
            if (MODE == 2) x = er[e];
        }
    };
    double sw = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int p0 = wave; p0 < np; p0 += 4 * PB) {
        if (p0 != wave) load_batch(p0);
#pragma unroll
        for (int u = 0; u < PB; u++) {
            const int p = p0 + 4 * u;
            if (p >= np) break;
            double wv[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t s = h ? se[u].y : se[u].x;
                double w = 0.0, x = 0.0, y = 0.0, z = 0.0;
                if (s != 0xffffffffu) fetch(s >> 1, w, x, y, z);
                if (MODE == 0) {
                    const double sg = (s & 1u) ? 1.0 : -1.0;
                    b0 += sg * x;
                    b1 += sg * y;
                    b2 += sg * z;
                }
                if (MODE == 2) b0 += (s & 1u) ? x : -x;
                sw += w;
                wv[h] = w;
                if (L1) {
                    const uint32_t c = (cc[u] >> (8 * h)) & 255u;
                    if (c < (uint32_t)kAsmCW) acc1[wave][c][lane] -= w;
                }
            }
            v_p[(size_t)p * 64] = make_double2(-wv[0], -wv[1]);
        }
    }
    if (on) {
        part[0][wave][lane] = sw;
        if (MODE == 0) {
            part[1][wave][lane] = b0;
            part[2][wave][lane] = b1;
            part[3][wave][lane] = b2;
        }
        if (MODE == 2) part[1][wave][lane] = b0;
    }
    __syncthreads();
    if (wave == 0) {
        double ex = 0.0;
        if (row < n) {
            sw = ((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane];
            if (MODE == 0) {
                b0 = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
                b1 = ((part[2][0][lane] + part[2][1][lane]) + part[2][2][lane]) + part[2][3][lane];
                b2 = ((part[3][0][lane] + part[3][1][lane]) + part[3][2][lane]) + part[3][3][lane];
            }
            if (MODE == 2) b0 = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
            for (int s = bptr[row]; s < bptr[row + 1]; s++) {
                const uint8_t fl = bflag[s];
                if (MODE == 2 && (fl & BF_IRLS) && !(fl & BF_L1H)) {  // (cannot happen: every make_A coefficient is one of make_AtA's)
                    double wk, x = 0.0, y = 0.0, z = 0.0;
                    const uint32_t se = beid[s];
                    fetch(se >> 1, wk, x, y, z);
                    b0 += (se & 1u) ? x : -x;
                }
                if (!(fl & (MODE == 0 ? BF_IRLS : BF_L1H))) {
                    bval[s] = 0.0;
                    continue;
                }
                const uint32_t se = beid[s];
                double wk, x = 0.0, y = 0.0, z = 0.0;
                fetch(se >> 1, wk, x, y, z);
                if (MODE == 2 && (fl & BF_IRLS)) b0 += (se & 1u) ? x : -x;  // make_A kept this coefficient: part of A' t
                if (MODE == 0) {
                    const double sg = (se & 1u) ? 1.0 : -1.0;
                    b0 += sg * x;
                    b1 += sg * y;
                    b2 += sg * z;
                } else if (fl & BF_NEG) {
                    wk = -wk;
                }
                bval[s] = wk;
                ex += wk;
            }
            const double d = sw + ex;
            excess[row] = ex;
            diag[row] = d;
            idg[row] = d > 0.0 ? 1.0 / d : 0.0;
            if (MODE == 0) rhs[row] = make_double4(b0, b1, b2, 0.0);
            if (MODE == 2) rhs[row] = make_double4(b0, 0.0, 0.0, 0.0);
        }
        if (L1) sEx[lane] = ex;
    }
#undef IRH_QI
    if (!L1) return;
    __syncthreads();
    if (wave == 0) {
        // lane = (aggregate a, level-1 entry c): sum of the 8 rows x 4 waves in a fixed order
        const int a = lane >> 3, c = lane & 7;
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
            for (int wv = 0; wv < 4; wv++) v += acc1[wv][c][a * 8 + r];
        const int I = sl * 8 + a;
        const bool liveI = I < n1;
        int o1 = 0, w1 = 0;
        if (liveI) {
            o1 = sl_off1[I >> 6];
            w1 = sl_off1[(I >> 6) + 1] - o1;
        }
        if (liveI && c < w1) val1[sell_pos(o1, c, I & 63)] = v;
        const double sv = seg_sum(v, 8);
        if (liveI && c == 0) {
            double ex = 0.0;
#pragma unroll
            for (int r = 0; r < 8; r++) ex += sEx[a * 8 + r];
            const double d = ex - sv;
            excess1[I] = ex;
            diag1[I] = d;
            idg1[I] = d > 0.0 ? 1.0 / d : 0.0;
        }
    }
}

}  // namespace irh
