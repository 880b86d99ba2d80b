// bcr.hip -- direct solve of a BANDED level-0 operator (a view sequence without loop closures: every view is
// linked to a bounded number of predecessors) by block cyclic reduction. Replaces the sparse factorisations
// of the reference on such graphs: SuiteSparseQR in irls (ral/l1_irls.cpp:536-556) and UMFPACK in
// l1decode_pd (ral/l1_irls.cpp:131-184) -- no iteration, no preconditioner, no tolerance.
//
// The operator A = A' D^2 A (IRLS) or the primal-dual Hessian (L1RA) of a graph whose edges (i, j) all have
// |i - j| <= b is a symmetric positive definite band matrix of half-bandwidth b. With B >= b rows per block
// it is block tridiagonal: D_i = A[i, i] (B x B), G_i = A[i, i + 1] (B x B). A workgroup takes a CHUNK of
// eight consecutive blocks and eliminates seven of them in nested-dissection order (0 2 4 6 | 1 5 | 3),
// one wave per block, leaving block 7 -- the separator -- coupled to the separator of the chunk before
// it. Eliminating block i between its current neighbours a (left) and c (right):
//     W = D_i^-1 [ P' | Q | R_i ],  P = A[a, i], Q = A[i, c]            (B x (2B + 3), kept for the way back)
//     D_a -= P W_P,  A[a, c] = -P W_Q,  R_a -= P W_R,   D_c -= Q' W_Q,  R_c -= Q' W_R
// The separators form a block tridiagonal system an eighth the size: the same kernel again, until at
// most eight blocks are left (100k views, B = 24: 4167 -> 521 -> 66 -> 9 -> 2 blocks). The way back is
// x_i = W_R - W_P x_a - W_Q x_c level by level. No host round trip anywhere: a solve is ~10 launches.
//
// What the hardware dictated: the B^3 work (five products per block) runs on the matrix cores
// (v_mfma_f64_16x16x4_f64: operands are distributed over the lanes, so no operand is broadcast through
// LDS -- with vector FMAs every value of P, Q and D^-1 would have to reach all 64 lanes, and eight waves
// per CU saturate the LDS port with that); the accumulator layout of one product IS the B-operand layout
// of the next (row = 4 reg + lane / 16), so W never leaves the registers between the two (the right-hand sides, three
// columns of a sixteen-column tile, run on v_mfma_f64_4x4x4_4b_f64 instead: BcrRs; so do the last eight rows of a block of
// 24 or 8, half a sixteen-row tile, into the very accumulator registers of that tile: BcrAop). D_i^-1 is
// formed by a symmetric sweep (Gauss-Jordan without pivoting: SPD), a column per lane, the pivot row
// broadcast through LDS (bcr_invert). A pivot not above kDeadTol x its original diagonal entry is dead
// (an isolated view, a floating component): its unknown solves to 0, as everywhere else in this library.
#include <atomic>

#include "graph.hpp"
#include "kernels.hpp"
#include "asm0w.hpp"
#include "bcr_route.hpp"

namespace irh {
// a direct solve with closures is repeated by conjugate gradients on the full operator when its relative residual is above
// the tolerance the ITERATIVE solver would have been held to (options.pcg_rtol, 1e-10 by default; at least this). A sound
// Woodbury solve: 1e-14 ... 2e-11 with a thousand closures at 100k views; what slipped through looser gates: fuzz seed
// 21 case 35 at 8e-9 (1.3e-6 rad off the oracle), seed 32 case 1 below 1e-9 (3e-8 rad).
constexpr double kBcrGateTolMin = 1e-12;

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));

constexpr int kTopMax = 16, kTopRounds = 6;
struct BcrTopSched {
    int n = 0, nr = 0, last = 0;   // blocks, rounds, the block that is left
    signed char ne[kTopRounds];    // eliminations of a round (<= 4)
    signed char i[kTopRounds][4], a[kTopRounds][4], c[kTopRounds][4];  // block, left / right neighbour (-1: none)
};

// (the arguments of k_bcr_reduce_up, see there). They live in device memory and are read by functions that are not inlined
// into the kernel: a pointer loaded from memory is GENERIC to the compiler (flat loads / stores, which also count on the
// LDS counter) unless its type says global -- so the fields are typed global for the device pass.
#if defined(__HIP_DEVICE_COMPILE__)
#define IRH_GPTR(T) T __attribute__((address_space(1))) *
#else
#define IRH_GPTR(T) T *
#endif
typedef IRH_GPTR(const double) gp_cd;
typedef IRH_GPTR(double) gp_d;
typedef IRH_GPTR(const int) gp_ci;
typedef IRH_GPTR(int) gp_i;
typedef IRH_GPTR(unsigned) gp_u;
typedef IRH_GPTR(const double4) gp_cd4;
struct BcrUpLevel {
    int nb, nred, nch;
    gp_cd inD, inR, inXD, inXR, inXG;  // from the level below
    gp_d W, sepD, sepR, extD, extR, extG;
    gp_d stD, stP, stQ;  // the unit-weight factor's operands of this level (BcrUnit; null: the handle keeps none)
};
struct BcrUpArgs {
    int nl;  // levels of the launch; lev[0] = level 1 of the solve
    BcrUpLevel lev[kUpLevels];
    // the level-0 operator, for the blocks of a mixed level 1 that no chunk reduced
    int n;
    gp_ci sl_off, col;
    gp_cd val, diag;
    gp_cd4 rhs;
    gp_d xtop;
    gp_u cnt;
    // round 5: the last level as ONE workgroup of up to sixteen blocks that also makes its way back (bcr_top_body):
    // top16 != 0, its schedule, where the solutions of its blocks go
    int top16;
    BcrTopSched top;
    gp_d xtop_all;
    // a wait that did not end: every workgroup that gives up says so here (cnt + kUpLevels), skips its chunk but still
    // counts itself -- nobody else waits a second for it --, and the top workgroup poisons the solution when the word is
    // set; the host then repeats the solve level by level (bcr_up_failed)
    gp_i fail;
    gp_d tst;  // the unit-weight factor's part of the single-workgroup top (BcrUnit::top)
};

struct BcrLevel {
    int nb = 0;   // blocks
    int nred = 0; // ... of which the first nred come from the level below (the others: raw level-0 blocks)
    int nch = 0;  // chunks of eight
    DevBuf<double> W;                             // nch * 7 blocks of B x (2B + 3)
    DevBuf<double> sepD, sepR, extD, extR, extG;  // per chunk: what the next level is assembled from
    DevBuf<double> x;                             // nch * 8 blocks of B x 3 (levels >= 1)
};
// The factor of the UNIT-WEIGHT operator (the first system of every irls call: weights.setOnes(), ral/l1_irls.cpp:577), kept
// from the first such solve of the handle on: per level and eliminated block the three A-operands of its products exactly as
// they read them (D_i^-1, P before phase 2 overwrites it, Q) and a private W whose W_P / W_Q the ways back read and whose W_R
// the right-hand-side-only pass rewrites; for the single-workgroup top per scheduled elimination r * 4 + e five blocks
// (D_i^-1, P, Q, W_P, W_Q) and, in slot kTopUnitLast, the inverse of the block that is left. Only run_irls's unit-weight
// solve writes or reads any of this.
constexpr int kTopUnitLast = 5 * 4 * kTopRounds;
struct BcrUnitLevel {
    DevBuf<double> Wu, Di, P, Q;
};
struct BcrUnit {
    std::vector<BcrUnitLevel> lev;
    DevBuf<double> top;
    DevBuf<BcrUpArgs> up_args;  // k_bcr_reduce_up's arguments with W = Wu and the operand arrays (written once)
    bool valid = false;         // a filling solve has ended with a finite score
    int last = 0;               // what the most recent solve did: 0 nothing, 1 filled, 2 was served from the store
    unsigned epoch = 0;         // bcr_unit_trim()'s count when the arrays were allocated
    int64_t solves = 0, bytes = 0;
    void release() {
        lev.clear();
        top.release();
        up_args.release();
        valid = false;
        last = 0;
        bytes = 0;
    }
};
struct BcrState {
    BcrUnit unit;
    int B = 0;
    int nfar = 0;  // long-range edges (loop closures) handled by the Woodbury correction
    std::vector<BcrLevel> lev;
    DevBuf<double> xtop;  // B x 3: the last separator
    DevBuf<int> far_e;    // edge id of the closures
    // the closures' part of a solve (bcr_closures): per level the inverse of every eliminated block, the step programs
    // of the closures' forward eliminations and what they record, the Woodbury system
    std::vector<DevBuf<double>> Dinv;
    DevBuf<double> topDinv;
    DevBuf<int> cl_off;          // nfar + 1: first step of a closure
    DevBuf<int4> cl_step;        // {level (-1: the top block), elimination inside the level, slots src | dstA << 8 | dstC << 16, sort key}
    DevBuf<int4> cl_init;        // {slot, row inside the block} of the two endpoints
    DevBuf<int> cl_owner;        // the closure of a step
    DevBuf<double> cl_R, cl_W;   // per step: the block's right-hand side when it was eliminated, and D^-1 times it
    DevBuf<double> cl_S, cl_T, lam;  // Woodbury system (npad x npad, npad x 3), its solution (nfar x 3)
    DevBuf<int> cl_alive;
    DevBuf<int> dead;            // dead pivots of the band factor of the last solve
    DevBuf<int> co_off, co_rec;  // per touched elimination: the steps that touch it ...
    DevBuf<int2> co_elim;        // ... and {level, elimination}
    int cl_nslots = 0, cl_nsteps = 0, cl_nelim = 0, cl_npad = 0, cl_maxsteps = 1, cl_ndense = 0;
    DevBuf<int> cl_dense;        // cl_ndense x nfar: the step of closure q on dense elimination d, or -1
    // a shard of a sharded sequence (dist.hip): the separator before the first chunk is the previous rank's
    int ext0 = 0;
    DevBuf<long long> stamps;  // development aid: bcr_stamp
    DevBuf<unsigned> up_cnt;   // k_bcr_reduce_up: arrivals per level boundary (they only grow: solve g waits for g x chunks);
                               // word kUpLevels: a wait gave up (bcr_up_failed)
    unsigned up_gen = 0;
    DevBuf<BcrUpArgs> up_args; // k_bcr_reduce_up's arguments (written once)
    BcrRoute last;             // the route of the most recent whole solve (a phase-1 + phase-2 pair is one solve)
    bool top16 = false;        // the last level is one workgroup of <= 16 blocks that makes its own way back (bcr_top_body)
    BcrTopSched tsched;
    DevBuf<BcrTopSched> tsched_dev;
    DevBuf<int> ghost_extcol;  // per ghost view: its row in the previous rank's last block, or -1
    DevBuf<double> remD, remR; // what this shard's eliminations subtract from that separator (sum over its levels)
    // closures on a shard: per local closure the slots that hold what is left on this rank's separator and on the one
    // before it {own, remote} (255: nothing), its number in the global list, who adds its 1 / w; the rows whose diagonal
    // loses the weight of a closure to a ghost view for the time of the reduction
    DevBuf<double> res_part;   // k_bcr_residual's partial sums (bcr_gate)
    DevBuf<int> res_zero;      // FL_COUNT zero words: the done flags the gate's SpMV runs behind
    DevBuf<int> gate_skip;     // k_bcr_gate's verdict as a skip word (1: do not touch weights / residuals)
    bool dead_clean = false;   // the dead-pivot counter is known to be zero (k_bcr_gate read and cleared it)
    DevBuf<int2> cl_fin;
    DevBuf<int> cl_gid;
    DevBuf<uint8_t> cl_own;
    DevBuf<int> fix_row, fix_off, fix_e;
    DevBuf<double> fix_saved;
    int nfix = 0;
};

void BcrDeleter::operator()(BcrState *p) const { delete p; }

// Sum over aligned groups of sixteen lanes, every lane gets it: the butterfly of __shfl_xor(1, 2, 4, 8) -- the same
// additions, bit for bit -- by DPP moves (quad permutes, then the mirrors of half a row and of a row: after two steps all
// four lanes of a quad hold the quad's sum, so WHICH lane of the other quad / half a lane adds does not matter) instead
// of ds_bpermute: a step costs ~20 clocks instead of an LDS round trip (round 5: the ways back are chains of such sums).
template <int CTRL>
__device__ __forceinline__ double bcr_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bcr_row16_sum(double v) {
    v += bcr_dpp<0xB1>(v);   // quad_perm [1 0 3 2]
    v += bcr_dpp<0x4E>(v);   // quad_perm [2 3 0 1]
    v += bcr_dpp<0x141>(v);  // row_half_mirror
    v += bcr_dpp<0x140>(v);  // row_mirror
    return v;
}

// In-place inverse of the SPD B x B matrix Dm (LDS, row-major) by one wave; B even, B <= 32. Symmetric sweep: after
// pivot k the registers hold -(inverse) on the swept part. Lane (c, h) = (lane % 32, lane / 32) holds the rows
// h HB .. h HB + HB - 1 of column c (HB = B / 2). The sweep stays symmetric, so column k IS row k: per pivot the lanes
// that hold row k write it to LDS (one store) and every lane reads back its own column's entry (the multiplier of the
// pivot row) and the HB entries of its rows (the pivot column) -- broadcast reads, no lane permutes, no address
// arithmetic (round 3 exchanged column k by 12 ds_bpermute on an 8 x 8-lane register tile and needed B % 8 == 0). The
// pivot and its dead-pivot reference travel through SGPRs (v_readlane), so the reciprocal starts before the LDS round
// trip of the row has finished. A wave issues in order -- about one instruction per 4.5 clocks, whatever it is -- so the
// chain of a pivot and the issue time of its updates ADD unless independent work stands between the links: the element
// of row k + 1 is updated first, written, its reciprocal started and the reads of row k + 1 issued; the other updates
// of pivot k follow and cover those latencies. (The empty asm statements pin that right-looking order: without them
// the compiler defers an element's updates until its row is the pivot row -- k dependent FMAs on the critical path.)
// LDS scratch: the first B doubles of the block itself (it lives in registers during the sweep). One wave alone:
// 0.85 / 2.3 / 4.2 / 6.9 us for B = 8 / 16 / 24 / 32 (tools/micro/sweep_cols.hip).
// dead: a counter of dead pivots (nullptr: not wanted); reg: a dead pivot is replaced by the row's own original
// diagonal entry (1 if that is not positive) instead of zeroing the unknown -- the regularised factorisation the guard of
// the closure path preconditions with (Graph::bcr_guard).
template <int B>
__device__ __forceinline__ void bcr_invert(double *Dm, int lane, int *dead = nullptr, bool reg = false) {
    static_assert(B % 2 == 0 && B <= 32, "block size");
    constexpr int HB = B / 2;
    const int c = lane & 31, h = lane >> 5;
    const bool act = c < B;
    const int cl = act ? c : B - 1;
    const v2d *Dh = reinterpret_cast<const v2d *>(Dm + h * HB);
    double t[HB];
#pragma unroll
    for (int i = 0; i < HB; i++) t[i] = Dm[(h * HB + i) * B + cl];
    const double dg = Dm[cl * B + cl];
    const double dgt = kDeadTol * dg;  // (the dead-pivot limit of the lane's row, formed once: a product per pivot less)
    int ndead = 0;
    auto pivot_inverse = [&](double tk, int k, int kh) {
        // reciprocal by v_rcp_f64 + two Newton steps (the IEEE division sequence is three times as long and sits on
        // the chain from pivot to pivot)
        const double p0 = readlane_d(tk, k + 32 * kh);
        const bool alive = p0 > readlane_d(dgt, k);
        ndead += alive ? 0 : 1;
        double p = p0;
        if (reg && !alive) {
            const double ref = readlane_d(dg, k);
            p = ref > 0.0 ? ref : 1.0;
        }
        double x = __builtin_amdgcn_rcp(p);
        x = fma(fma(-p, x, 1.0), x, x);
        x = fma(fma(-p, x, 1.0), x, x);
        return (alive || reg) ? x : 0.0;
    };
    // (the row's own diagonal position carries -1 instead of the pivot: nobody reads the pivot there -- it travels through
    // an SGPR --, and the lane of column k, which reads it as its multiplier of the pivot row, gets rowk pinv = -pinv, the
    // (k, k) entry of the swept matrix, without a select of its own)
    if (h == 0 && act) Dm[c] = c == 0 ? -1.0 : t[0];
    asm volatile("" ::: "memory");
    double pinv = pivot_inverse(t[0], 0, 0);
    double rowk = Dm[cl], colk[HB];
#pragma unroll
    for (int i = 0; i < HB; i += 2) {
        const v2d v = Dh[i / 2];
        colk[i] = v.x;
        colk[i + 1] = v.y;
    }
#pragma unroll
    for (int k = 0; k < B; k++) {
        const int kh = k / HB, ki = k - kh * HB;
        const int k1 = k + 1, kh1 = k1 / HB, ki1 = k1 - kh1 * HB;  // the next pivot (when k1 < B)
        const bool isk = c == k;
        const double f = rowk * pinv;
        const double g = f;
        // general element: t -= colk (rowk pinv); column k: colk pinv; row k: rowk pinv; (k, k): -pinv
        // (the lane of column k drops its old values by a product with 0, one instruction, not by a 64-bit select, two:
        // 24 of the ~105 instructions of a pivot; taking the LDS round trip of the row out of the pivot-to-pivot chain --
        // the element of row k + 1 updated from registers alone, its multiplier through an SGPR like the pivot -- cost ten
        // instructions per pivot and made the sweep slower, 11 600 instead of 10 150 clocks: the chain is the reciprocal's)
        const double keep = isk ? 0.0 : 1.0;
        auto upd = [&](int i) {
            const double a = t[i] * keep;
            double u = fma(-colk[i], g, a);
            if (i == ki) u = (h == kh) ? g : u;
            t[i] = u;
        };
        double pinv1 = 0.0, rowk1 = 0.0, colk1[HB];
        if (k1 < B) {
            upd(ki1);
            if (h == kh1 && act) Dm[c] = c == k1 ? -1.0 : t[ki1];
            asm volatile("" ::: "memory");
            pinv1 = pivot_inverse(t[ki1], k1, kh1);
            rowk1 = Dm[cl];
#pragma unroll
            for (int i = 0; i < HB; i += 2) {
                const v2d v = Dh[i / 2];
                colk1[i] = v.x;
                colk1[i + 1] = v.y;
            }
        }
#pragma unroll
        for (int i = 0; i < HB; i++)
            if (!(k1 < B && i == ki1)) upd(i);
#pragma unroll
        for (int i = 0; i < HB; i++) asm volatile("" : "+v"(t[i]));
        if (k1 < B) {
            pinv = pinv1;
            rowk = rowk1;
#pragma unroll
            for (int i = 0; i < HB; i++) colk[i] = colk1[i];
        }
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < HB; i++)
        if (act) Dm[(h * HB + i) * B + c] = -t[i];
    if (dead && ndead && lane == 0) atomicAdd(dead, ndead);
}

// development aid (IROTAVG_BCR_DBG & 64, irotavg_graph_time_kernel 200 + slot): shader-clock stamps of thread 0 of every
// workgroup of k_bcr_reduce at its phase boundaries, 16 slots per chunk
__device__ __forceinline__ void bcr_stamp(long long *st, int slot) {
    if (st && threadIdx.x == 0) st[(size_t)blockIdx.x * 16 + slot] = (long long)__builtin_readcyclecounter();
}

// NR: right-hand-side columns riding along (3: the three coordinates; 19: + 16 columns of the closures' incidence
// vectors, see bcr_solve)
template <int B, int NR = 3>
struct BcrDim {
    static constexpr int NC = 2 * B + NR;       // columns of W: P' | Q | R
    static constexpr int MT = (B + 15) / 16;    // 16-row tiles of a block
    static constexpr int NT = (NC + 15) / 16;   // 16-column tiles of W
    static constexpr int KS = B / 4;            // k-steps of a product over a block
    static constexpr int NT0 = B / 16;          // first column tile that holds a column of W_Q
};

// The A-operands of a wide product (sixteen columns per instruction), all row tiles and k-steps of the row-major B x B
// matrix M or of its transpose: a[mt][s] = element (16 mt + lane % 16, 4 s + lane / 16), the 16x16x4 operand. With
// B % 16 == 8 (B = 24, 8) the last row tile holds eight rows and eight rows of zeros: 64 pipe clocks for half a tile.
// That tile runs as TWO v_mfma_f64_4x4x4_4b_f64 per column tile and k-step instead (2 x ~18 clocks), one per group g of
// four rows, whose four blocks share the same A and are the four column groups of the 16-column tile (the layout: BcrRs
// below, tools/micro/mfma_f64_4x4x4_layout.hip prints this use as well):
//   A  M[16 (MT - 1) + 4 g + lane % 4][4 s + lane / 16] in every block -- the operand loaded here (a4);
//   B  B[k][4 block + j] in lane 16 k + 4 block + j: lane for lane the 16x16x4 B-operand, unchanged;
//   D  D[i][4 block + j] in lane 16 i + 4 block + j: register g of the 16x16x4 accumulator tile of that row tile (rows
//      16 (MT - 1) + 4 g + lane / 16). Registers 2 and 3 of the tile stay zero; they hold rows >= B, which nobody reads.
// So stores, puts and the use of an accumulator tile as the next product's B-operand are those of the 16x16x4 tile, and
// the sums are the same four-term k groups in the same order: bit for bit what the padded tile gave.
template <int B>
struct BcrAop {
    typedef BcrDim<B> Dm;
    static constexpr bool SMALL = B % 16 == 8;
    static constexpr int MW = SMALL ? Dm::MT - 1 : Dm::MT;  // row tiles on the 16x16x4 product
    double a[MW > 0 ? MW : 1][Dm::KS];
    double a4[2][Dm::KS];
    template <bool TRANS>
    __device__ __forceinline__ void load(const double *M, int lane) {
        const int li = lane & 15, lk = lane >> 4;
#pragma unroll
        for (int mt = 0; mt < MW; mt++) {
            // (rows beyond B read as zero)
            const int i = 16 * mt + li;
            const int ic = i < B ? i : B - 1;
#pragma unroll
            for (int s = 0; s < Dm::KS; s++) {
                const int k = 4 * s + lk;
                const double v = TRANS ? M[k * B + ic] : M[ic * B + k];
                a[mt][s] = i < B ? v : 0.0;
            }
        }
        if constexpr (SMALL) {
#pragma unroll
            for (int g = 0; g < 2; g++) {
                const int i = 16 * MW + 4 * g + (lane & 3);
#pragma unroll
                for (int s = 0; s < Dm::KS; s++) {
                    const int k = 4 * s + lk;
                    a4[g][s] = TRANS ? M[k * B + i] : M[i * B + k];
                }
            }
        }
    }
    // acc (the accumulator tile of row tile mt) += A(mt, k-step s) x bop
    __device__ __forceinline__ void mul(int mt, int s, double bop, v4d &acc) const {
        if (SMALL && mt == MW) {
            acc[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a4[0][s], bop, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a4[1][s], bop, acc[1], 0, 0, 0);
        } else {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mt][s], bop, acc, 0, 0, 0);
        }
    }
};

// out[mt][nt] += A (registers) x W (accumulator tiles of a previous product used as B-operands: register r of
// tile (mt, nt) holds the rows 16 mt + 4 r + lane / 16, i.e. k-step 4 mt + r)
template <int B, int NTA>
__device__ __forceinline__ void bcr_mul_w(const BcrAop<B> &aop, const v4d (&w)[BcrDim<B>::MT][BcrDim<B>::NT],
                                          v4d (&out)[BcrDim<B>::MT][BcrDim<B>::NT]) {
    typedef BcrDim<B> Dm;
#pragma unroll
    for (int nt = NTA; nt < Dm::NT; nt++)
#pragma unroll
        for (int s = 0; s < Dm::KS; s++) {
            const double bop = w[s >> 2][nt][s & 3];
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++) aop.mul(mt, s, bop, out[mt][nt]);
        }
}

// The right-hand sides as SMALL products. With three right-hand sides and 2 B a multiple of 16 (B = 8 / 16 / 24 / 32) the
// last 16-column tile of W holds W_R and thirteen columns of zeros: 3 MT KS products of 64 pipe clocks each for 3 useful
// columns of 16. v_mfma_f64_4x4x4_4b_f64 runs four independent 4 x 4 x 4 products per instruction at an issue every ~18
// clocks (tools/micro/mfma_f64.hip) and holds one double per lane for each of A, B and the accumulator; the layout is the
// 16x16x4 one with the sixteen columns cut into four blocks: block = (lane / 4) % 4 for all three, A[i][k] sits in lane
// 16 k + 4 block + i, B[k][j] in lane 16 k + 4 block + j, D[i][j] in lane 16 i + 4 block + j -- measured, it is documented
// nowhere (tools/micro/mfma_f64_4x4x4_layout.hip prints it). A block of the instruction is a ROW GROUP of four rows: instruction t
// of a product covers the row groups 4 t ... 4 t + 3 (B = 24: 4 + 2, B = 8: 2 -- the other blocks run on zeros), its A-operand
// of k-step s is the 4 x 4 block (group, s) of D_i^-1, Q' or P, its B-operand the rows 4 s ... 4 s + 3 of the B x 3 matrix on
// the right (column 3 reads as zero) in every block. MT = ceil(B / 16) instructions per k-step, KS k-steps: 12 instructions
// per product at B = 24. The matrix on the right of the second and third product is W_R itself: its owner writes it over
// R_i in LDS (nobody else reads R_i, and the single-workgroup top keeps W_R there anyway) and reads it back as an operand.
template <int B>
struct BcrRs {
    static constexpr int MT = (B + 15) / 16, KS = B / 4, NG = B / 4;
    int blk, ai, ak, bk, bj, di, dj;
    __device__ __forceinline__ explicit BcrRs(int lane)
        : blk((lane >> 2) & 3), ai(lane & 3), ak(lane >> 4), bk(lane >> 4), bj(lane & 3), di(lane >> 4), dj(lane & 3) {}
    // A-operands from the row-major B x B matrix M (or its transpose)
    template <bool TRANS>
    __device__ __forceinline__ void load_a(const double *M, double (&aop)[MT][KS]) const {
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const int g = 4 * t + blk;
            const int row = 4 * (g < NG ? g : NG - 1) + ai;
#pragma unroll
            for (int s = 0; s < KS; s++) {
                const int k = 4 * s + ak;
                const double v = TRANS ? M[k * B + row] : M[row * B + k];
                aop[t][s] = g < NG ? v : 0.0;
            }
        }
    }
    // B-operands from the row-major B x 3 matrix X
    __device__ __forceinline__ void load_b(const double *X, double (&bop)[KS]) const {
        const int j = bj < 3 ? bj : 2;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const double v = X[(4 * s + bk) * 3 + j];
            bop[s] = bj < 3 ? v : 0.0;
        }
    }
    // acc[t] = sum over the k-steps, in their order (k-steps outermost: the MT accumulators are independent chains)
    __device__ __forceinline__ void mul(const double (&aop)[MT][KS], const double (&bop)[KS], double (&acc)[MT]) const {
#pragma unroll
        for (int t = 0; t < MT; t++) acc[t] = 0.0;
#pragma unroll
        for (int s = 0; s < KS; s++)
#pragma unroll
            for (int t = 0; t < MT; t++) acc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(aop[t][s], bop[s], acc[t], 0, 0, 0);
    }
    // the lane's entry of instruction t: row (of B) and column (of 3), or row = -1
    __device__ __forceinline__ int row(int t) const {
        const int g = 4 * t + blk;
        return g < NG && dj < 3 ? 4 * g + di : -1;
    }
};

// W_R = D_i^-1 R_i over R_i (and to Wg: row stride 2 B + 3, columns 2 B ...), R_c -= Q' W_R
template <int B>
__device__ __forceinline__ void bcr_rs_phase1(const double *Di, const double *Q, double *Ri, double *Rc, double *Wg, int lane,
                                              bool hasQ) {
    typedef BcrRs<B> S_;
    const S_ S(lane);
    double aop[S_::MT][S_::KS], bop[S_::KS], acc[S_::MT];
    S.template load_a<true>(Di, aop);
    S.load_b(Ri, bop);
    S.mul(aop, bop, acc);
#pragma unroll
    for (int t = 0; t < S_::MT; t++) {
        const int row = S.row(t);
        if (row >= 0) {
            Ri[row * 3 + S.dj] = acc[t];
            if (Wg) Wg[row * (2 * B + 3) + 2 * B + S.dj] = acc[t];
        }
    }
    if (!hasQ) return;
    S.template load_a<true>(Q, aop);
    S.load_b(Ri, bop);
    S.mul(aop, bop, acc);
#pragma unroll
    for (int t = 0; t < S_::MT; t++) {
        const int row = S.row(t);
        if (row >= 0) Rc[row * 3 + S.dj] -= acc[t];
    }
}
// P W_R: the lane's entries of the (at most two) instructions
template <int B>
__device__ __forceinline__ v2d bcr_rs_pw(const double *P, const double *Wr, int lane) {
    typedef BcrRs<B> S_;
    static_assert(S_::MT <= 2, "two instructions per k-step");
    const S_ S(lane);
    double aop[S_::MT][S_::KS], bop[S_::KS], acc[S_::MT];
    S.template load_a<false>(P, aop);
    S.load_b(Wr, bop);
    S.mul(aop, bop, acc);
    return v2d{acc[0], S_::MT > 1 ? acc[S_::MT - 1] : 0.0};
}
// the same as FUNCTIONS, for the single-workgroup top: its body has no registers to spare (248 of 256 before the small
// products), and what a call costs -- the registers of the small products are the callee's -- is a few dozen clocks
template <int B>
__device__ __noinline__ void bcr_rs_phase1_call(const double *Di, const double *Q, double *Ri, double *Rc, int lane, bool hasQ) {
    bcr_rs_phase1<B>(Di, Q, Ri, Rc, nullptr, lane, hasQ);
}
template <int B>
__device__ __noinline__ v2d bcr_rs_pw_call(const double *P, const double *Wr, int lane) {
    return bcr_rs_pw<B>(P, Wr, lane);
}

// The matrix-core part of one block elimination. The 16-column tiles of W are independent of each other in all
// three products, so they are dealt to the waves of the elimination's group (one wave in the first round of a
// four-wave workgroup, two in the second, four in the third; four from the start in a sixteen-wave workgroup):
// this wave owns the tiles nt = part, part + WPE, ... and keeps them in w[][slot] between the phases (workgroup
// barriers lie in between). NTPW: slots of a wave.
// RSCALL: the small products of the right-hand sides are calls (bcr_top_body)
template <int B, int NR, int NTPW, bool RSCALL = false>
struct BcrElim {
    typedef BcrDim<B, NR> Dm;
    typedef BcrAop<B> Aop;
    v4d w[Dm::MT][NTPW];
    // the last column tile holds W_R alone: its owner runs it as small products (BcrRs), in every phase. With WPE waves
    // per elimination that is the wave of part (NT - 1) % WPE, in its slot (NT - 1) / WPE -- the same in all four functions
    static constexpr bool RS = NR == 3 && 16 * (Dm::NT - 1) == 2 * B;
    template <int WPE>
    __device__ __forceinline__ static bool rs_mine(int part) {
        return RS && part == (Dm::NT - 1) % WPE;
    }
#define IRH_RS_SKIP(sl) (SM && (sl) == (Dm::NT - 1) / WPE)

    // W = Di^-1 [P' | Q | R] (Di^-1 in LDS), W -> global (the way back reads it), and the right neighbour:
    // D_c -= Q' W_Q, R_c -= Q' W_R
    // (hasQ = false: the block has no right neighbour -- the last block of the single-workgroup top, bcr_top_body; Wg =
    // nullptr: W is not wanted in memory)
    template <int WPE>
    __device__ __forceinline__ void phase1(int part, const double *Di, const double *P, bool hasP, const double *Q,
                                           double *Ri, double *Dc, double *Rc, double *Wg, const double *zero,
                                           int lane, bool hasQ = true) {
        if (rs_mine<WPE>(part)) phase1_t<WPE, true>(part, Di, P, hasP, Q, Ri, Dc, Rc, Wg, zero, lane, hasQ);
        else phase1_t<WPE, false>(part, Di, P, hasP, Q, Ri, Dc, Rc, Wg, zero, lane, hasQ);
    }
    __device__ __forceinline__ void rs_phase1(const double *Di, const double *Q, double *Ri, double *Rc, double *Wg, int lane,
                                              bool hasQ) const {
        if constexpr (!RS) return;
        else if constexpr (RSCALL) bcr_rs_phase1_call<B>(Di, Q, Ri, Rc, lane, hasQ);
        else bcr_rs_phase1<B>(Di, Q, Ri, Rc, Wg, lane, hasQ);
    }
    template <int WPE, bool SM>
    __device__ __forceinline__ void phase1_t(int part, const double *Di, const double *P, bool hasP, const double *Q,
                                             double *Ri, double *Dc, double *Rc, double *Wg, const double *zero,
                                             int lane, bool hasQ) {
        constexpr int NS = (Dm::NT + WPE - 1) / WPE;
        static_assert(NS <= NTPW, "slots");
        if (SM) {
            rs_phase1(Di, Q, Ri, Rc, Wg, lane, hasQ);
            if (NS == 1) return;
            // (the wide tiles' operands are not requested while the small products' are live: the sixteen-block top
            // has no registers to spare)
            __builtin_amdgcn_sched_barrier(0);
        }
        Aop aop;
        // (the inverse is symmetric: read by columns -- consecutive lanes, consecutive words -- instead of by rows, whose
        // stride of 2 B words puts sixteen lanes on four banks)
        aop.template load<true>(Di, lane);
        const int lj = lane & 15, lk = lane >> 4;
        const double *base[NS];
        int stride[NS];
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            const int nt = part + sl * WPE;
            const int j = 16 * nt + lj;
            base[sl] = zero;
            stride[sl] = 0;
            if (nt < Dm::NT) {
                if (j < B) {
                    if (hasP) {
                        base[sl] = P + j * B;  // column j of P' = row j of P
                        stride[sl] = 1;
                    }
                } else if (j < 2 * B) {
                    if (hasQ) {
                        base[sl] = Q + (j - B);
                        stride[sl] = B;
                    }
                } else if (j < Dm::NC) {
                    base[sl] = Ri + (j - 2 * B);
                    stride[sl] = NR;
                }
            }
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++) w[mt][sl] = v4d{0.0, 0.0, 0.0, 0.0};
        }
        // k-steps outermost: the MT x NS accumulator tiles are independent chains, and a chain of dependent
        // f64 MFMAs issues one instruction per result latency, not per issue slot
#pragma unroll
        for (int s = 0; s < Dm::KS; s++) {
            double bop[NS];
#pragma unroll
            for (int sl = 0; sl < NS; sl++) bop[sl] = base[sl][(4 * s + lk) * stride[sl]];
#pragma unroll
            for (int sl = 0; sl < NS; sl++) {
                if (IRH_RS_SKIP(sl)) continue;
#pragma unroll
                for (int mt = 0; mt < Dm::MT; mt++) aop.mul(mt, s, bop[sl], w[mt][sl]);
            }
        }
        if (Wg) {
#pragma unroll
            for (int sl = 0; sl < NS; sl++) {
                if (IRH_RS_SKIP(sl)) continue;
                const int j = 16 * (part + sl * WPE) + lj;
#pragma unroll
                for (int mt = 0; mt < Dm::MT; mt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = 16 * mt + 4 * r + lk;
                        if (row < B && j < Dm::NC) Wg[row * Dm::NC + j] = w[mt][sl][r];
                    }
            }
        }
        if (!hasQ) return;
        aop.template load<true>(Q, lane);
        v4d out[Dm::MT][NS];
#pragma unroll
        for (int sl = 0; sl < NS; sl++)
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++) out[mt][sl] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < Dm::KS; s++)
#pragma unroll
            for (int sl = 0; sl < NS; sl++) {
                const int nt = part + sl * WPE;
                if (nt >= Dm::NT || nt < Dm::NT0 || IRH_RS_SKIP(sl)) continue;
#pragma unroll
                for (int mt = 0; mt < Dm::MT; mt++) aop.mul(mt, s, w[s >> 2][sl][s & 3], out[mt][sl]);
            }
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            const int nt = part + sl * WPE;
            if (nt >= Dm::NT || nt < Dm::NT0 || IRH_RS_SKIP(sl)) continue;
            const int c = 16 * nt + lj;
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = 16 * mt + 4 * r + lk;
                    if (row < B) {
                        if (c >= B && c < 2 * B)
                            Dc[row * B + c - B] -= out[mt][sl][r];
                        else if (c >= 2 * B && c < Dm::NC)
                            Rc[row * NR + c - 2 * B] -= out[mt][sl][r];
                    }
                }
        }
    }

    // the single-workgroup top keeps W in LDS for its way back, in the places its elimination has freed: W_P over
    // D_i^-1, W_Q over Q, W_R over R_i (after the barrier behind phase1: nobody reads those any more)
    template <int WPE>
    __device__ __forceinline__ void keep_w(int part, double *Di, double *Q, bool hasQ, double *Ri, int lane) const {
        // (the small products have left W_R over R_i already)
        if (rs_mine<WPE>(part)) keep_w_t<WPE, true>(part, Di, Q, hasQ, Ri, lane);
        else keep_w_t<WPE, false>(part, Di, Q, hasQ, Ri, lane);
    }
    template <int WPE, bool SM>
    __device__ __forceinline__ void keep_w_t(int part, double *Di, double *Q, bool hasQ, double *Ri, int lane) const {
        constexpr int NS = (Dm::NT + WPE - 1) / WPE;
        const int lj = lane & 15, lk = lane >> 4;
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            const int nt = part + sl * WPE;
            if (nt >= Dm::NT || IRH_RS_SKIP(sl)) continue;
            const int j = 16 * nt + lj;
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = 16 * mt + 4 * r + lk;
                    if (row < B) {
                        const double v = w[mt][sl][r];
                        if (j < B)
                            Di[row * B + j] = v;
                        else if (j < 2 * B) {
                            if (hasQ) Q[row * B + j - B] = v;
                        } else if (j < Dm::NC)
                            Ri[row * NR + j - 2 * B] = v;
                    }
                }
        }
    }

    // left neighbour, first half: the products P W (P is read by every wave of the group, and overwritten in
    // the second half -- a barrier lies in between when the group has more than one wave)
    // (Wr: where phase1 left W_R -- the place of R_i)
    template <int WPE>
    __device__ __forceinline__ void phase2_mul(int part, const double *P, const double *Wr, v4d (&out)[Dm::MT][NTPW], int lane) {
        if (rs_mine<WPE>(part)) phase2_mul_t<WPE, true>(part, P, Wr, out, lane);
        else phase2_mul_t<WPE, false>(part, P, Wr, out, lane);
    }
    template <int WPE, bool SM>
    __device__ __forceinline__ void phase2_mul_t(int part, const double *P, const double *Wr, v4d (&out)[Dm::MT][NTPW], int lane) {
        constexpr int NS = (Dm::NT + WPE - 1) / WPE;
        if (SM) {
            // P W_R: the lane's entry of instruction t travels in out[t][slot][0]
            if constexpr (RS) {
                const v2d acc = RSCALL ? bcr_rs_pw_call<B>(P, Wr, lane) : bcr_rs_pw<B>(P, Wr, lane);
#pragma unroll
                for (int t = 0; t < Dm::MT; t++) out[t][(Dm::NT - 1) / WPE][0] = acc[t];  // (the other three: not read)
            }
            if (NS == 1) return;
            __builtin_amdgcn_sched_barrier(0);
        }
        Aop aop;
        aop.template load<false>(P, lane);
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            if (IRH_RS_SKIP(sl)) continue;
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++) out[mt][sl] = v4d{0.0, 0.0, 0.0, 0.0};
        }
#pragma unroll
        for (int s = 0; s < Dm::KS; s++)
#pragma unroll
            for (int sl = 0; sl < NS; sl++) {
                if (part + sl * WPE >= Dm::NT || IRH_RS_SKIP(sl)) continue;
#pragma unroll
                for (int mt = 0; mt < Dm::MT; mt++) aop.mul(mt, s, w[s >> 2][sl][s & 3], out[mt][sl]);
            }
    }
    // second half: D_a -= P W_P (assigned when `assign`: the chunk's first contribution to the separator before
    // it), A[a, c] = -P W_Q written over P, R_a -= P W_R
    template <int WPE>
    __device__ __forceinline__ void phase2_put(int part, const v4d (&out)[Dm::MT][NTPW], double *P, double *Da,
                                               bool assign, double *Ra, int lane) {
        if (rs_mine<WPE>(part)) phase2_put_t<WPE, true>(part, out, P, Da, assign, Ra, lane);
        else phase2_put_t<WPE, false>(part, out, P, Da, assign, Ra, lane);
    }
    template <int WPE, bool SM>
    __device__ __forceinline__ void phase2_put_t(int part, const v4d (&out)[Dm::MT][NTPW], double *P, double *Da,
                                                 bool assign, double *Ra, int lane) {
        constexpr int NS = (Dm::NT + WPE - 1) / WPE;
        if (SM) {
            if constexpr (RS) {
                const BcrRs<B> S(lane);
#pragma unroll
                for (int t = 0; t < Dm::MT; t++) {
                    const int row = S.row(t);
                    if (row >= 0) Ra[row * NR + S.dj] -= out[t][(Dm::NT - 1) / WPE][0];
                }
            }
            if (NS == 1) return;
        }
        const int lj = lane & 15, lk = lane >> 4;
#pragma unroll
        for (int sl = 0; sl < NS; sl++) {
            const int nt = part + sl * WPE;
            if (nt >= Dm::NT || IRH_RS_SKIP(sl)) continue;
            const int c = 16 * nt + lj;
#pragma unroll
            for (int mt = 0; mt < Dm::MT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = 16 * mt + 4 * r + lk;
                    if (row < B) {
                        const double v = out[mt][sl][r];
                        if (c < B)
                            Da[row * B + c] = assign ? -v : Da[row * B + c] - v;
                        else if (c < 2 * B)
                            P[row * B + c - B] = -v;
                        else if (c < Dm::NC)
                            Ra[row * NR + c - 2 * B] -= v;
                    }
                }
        }
    }
#undef IRH_RS_SKIP
};

// One row of the level-0 operator into the block arrays of a chunk: `row` lies in block lb (rows lb B ...), r = its
// row inside the block. Entries in block lb -> Dblk (with the diagonal), entries in block lb + 1 -> Gnext (the
// coupling lb -> lb + 1; nullptr: not wanted), entries in block lb - 1 -> GprevT, stored transposed (the coupling
// lb - 1 -> lb as the rows of block lb see it, by symmetry; nullptr: not wanted). The right-hand side -> Rblk.
// A thread owns its row (and, in GprevT, its column): plain read-modify-writes.
// Entries further away than the neighbouring blocks belong to long-range edges (loop closures): they are not part
// of the band operator this solver factorises -- their weight is taken back out of the diagonal (the entry is
// -w, the diagonal holds +w) and the closures re-enter by the Woodbury correction (bcr_solve). nfar > 0: the
// right-hand-side columns 3 .. 3 + nfar of the row get the incidence vectors of the closures of this pass.
template <int B, int NR, int NBT = 12>
__device__ __forceinline__ void bcr_gather_row(int row, int lb, int r, const int *__restrict__ sl_off,
                                               const int *__restrict__ col, const double *__restrict__ val,
                                               const double *__restrict__ diag, const double4 *__restrict__ rhs,
                                               double *blocks, int oD, int oGnext, int oGprevT, double *Rblk, int nfar,
                                               const int *__restrict__ far_i, const int *__restrict__ far_j) {
    // (Dblk, Gnext, GprevT = blocks + oD, + oGnext, + oGprevT; a negative offset: not wanted)
    double *Dblk = blocks + oD;
    const int sl = row >> 6, ln = row & 63;
    const int o0 = sl_off[sl], w = sl_off[sl + 1] - o0;
    const v2i *__restrict__ cp = reinterpret_cast<const v2i *>(col) + (size_t)(o0 / 2) * 64 + ln;
    const v2d *__restrict__ vp = reinterpret_cast<const v2d *>(val) + (size_t)(o0 / 2) * 64 + ln;
    const int c0 = lb * B;
    // (diagonal and right-hand side are requested ahead of the entries: behind them they were a memory round trip of
    // their own)
    const double dgv = diag[row];
    const double4 bb = rhs[row];
    // the row's entries in batches of NBT pairs: all loads of a batch are issued before the first value is
    // scattered (a load per scatter was a memory round trip per pair). NBT = 24: the raw blocks of a mixed level 1 inside
    // the single-launch upper reduction, where nine workgroups gather while sixty-four wait for them -- a row of the
    // headline graph (42 entries) is then ONE batch, one memory round trip less
    for (int q0 = 0; q0 < w / 2; q0 += NBT) {
        v2i cc[NBT];
        v2d vv[NBT];
#pragma unroll
        for (int u = 0; u < NBT; u++) {
            const int q = q0 + u < w / 2 ? q0 + u : w / 2 - 1;
            cc[u] = __builtin_nontemporal_load(&cp[(size_t)q * 64]);
            vv[u] = __builtin_nontemporal_load(&vp[(size_t)q * 64]);
        }
        // branch-free scatter by LDS adds without return (ds_add_f64: issued back to back, executed in program order, so
        // the sum of a row's duplicates keeps its order; a read-modify-write per entry was an LDS round trip and four
        // divergent branches each: a third of the load phase)
#pragma unroll
        for (int u = 0; u < NBT; u++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int c = h ? cc[u].y : cc[u].x;
                const double v = h ? vv[u].y : vv[u].x;
                const int gc = c - c0;
                // the target as an index: selects, no branches
                const bool inD = gc >= 0 && gc < B, inN = gc >= B && gc < 2 * B, inP = gc < 0 && gc >= -B;
                int idx = oD + r * B + r;  // long-range entry: its weight back out of the diagonal
                idx = inD ? oD + r * B + gc : idx;
                idx = inN ? oGnext + r * B + gc - B : idx;
                idx = inP ? oGprevT + (gc + B) * B + r : idx;
                const bool keep = q0 + u < w / 2 && v != 0.0 && !(inN && oGnext < 0) && !(inP && oGprevT < 0);  // (zero: padding)
                double *dst = blocks + idx;
                if (keep) atomicAdd(dst, v);
            }
        }
    }
    Dblk[r * B + r] += dgv;
    Rblk[r * NR + 0] = bb.x;
    Rblk[r * NR + 1] = bb.y;
    Rblk[r * NR + 2] = bb.z;
    if (NR > 3)
        for (int q = 0; q < nfar; q++) {
            const int fi = far_i[q], fj = far_j[q];
            if (fi == row || fj == row) Rblk[r * NR + 3 + q] = (fi == row ? 1.0 : 0.0) - (fj == row ? 1.0 : 0.0);
        }
}

// Where the k real blocks of a PARTIAL chunk sit among its eight positions. By default the first k (the rest is
// padding: identity blocks without couplings, whose eliminations are skipped) -- the chunk's separator, position 7, is
// then padding and its last real block is eliminated like any other: fine when nothing lies to its right. A SHARD's
// last block is coupled to the next rank and must survive as the separator at every level: its partial chunks place
// their blocks such that the last one sits at position 7 and every padding position is eliminated (= skipped) before
// it would be the neighbour of a real elimination in the (0 2 4 6)(1 5)(3) schedule. The coupling of the real block at
// position p to the next real block lives in slot p + 1, the one to the separator before the chunk in slot 0.
__constant__ signed char kBcrPlace[9][8] = {{-1, -1, -1, -1, -1, -1, -1, -1}, {7, -1, -1, -1, -1, -1, -1, -1},
                                             {3, 7, -1, -1, -1, -1, -1, -1},   {3, 5, 7, -1, -1, -1, -1, -1},
                                             {1, 3, 5, 7, -1, -1, -1, -1},     {1, 3, 5, 6, 7, -1, -1, -1},
                                             {1, 3, 4, 5, 6, 7, -1, -1},       {1, 2, 3, 4, 5, 6, 7, -1},
                                             {0, 1, 2, 3, 4, 5, 6, 7}};
__device__ __forceinline__ int bcr_pos(bool placed, int k, int t) { return placed ? (int)kBcrPlace[k][t] : t; }
__device__ __forceinline__ int bcr_ridx(bool placed, int k, int i) {
    if (!placed) return i < k ? i : -1;
    for (int t = 0; t < k; t++)
        if (kBcrPlace[k][t] == i) return t;
    return -1;
}

// One chunk of eight blocks per workgroup of NW waves (4, or 8 when the level has so few chunks that every
// workgroup has a CU to itself: the column tiles of W are then dealt to two waves in the first round and four afterwards).
// L0: the blocks are gathered from the level-0 SELL operator (off-diagonals), its diagonal and right-hand side;
// otherwise from the separator data of the level below (block j of this level = chunk j of that one):
//   D_j = sepD[j] + extD[j + 1],  R_j = sepR[j] + extR[j + 1],  G_j = extG[j + 1].
// Output per chunk c: W (seven blocks), sepD / sepR (block 7 after the eliminations), extD / extR (what the
// chunk's eliminations subtract from the separator of chunk c - 1), extG (coupling of that separator to block 7).
// TOP (one chunk, nothing before it): block 7 is solved and written to xtop.
// What one level writes for the next inside ONE launch (k_bcr_reduce_up) crosses the XCDs' L2s: device-scope atomic
// stores / loads (write-through, read at the coherence point) instead of fences -- a device-scope release writes back a
// whole L2, and tools/micro/xcdbar.hip measures a counter barrier + exchange among sixteen workgroups at 1.2 us this way.
template <bool COH>
__device__ __forceinline__ double bcr_ld(const double *p) {
    if (!COH) return *p;
    const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double((long long)v);
}
template <bool COH>
__device__ __forceinline__ void bcr_st(double *p, double v) {
    if (!COH)
        *p = v;
    else
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// The reduction of one chunk (the body of k_bcr_reduce; k_bcr_reduce_up runs it for the chunks of several levels in
// turn). sDG: 16 blocks, sR: 9 right-hand-side slots, sZ: 2 doubles of LDS. COH: the level below was written, and this
// level's separator data is read, inside the same launch (bcr_ld / bcr_st).
// UF (the unit-weight factor, BcrUnit): 1 = the full reduction also keeps the operands of its products (Dinvg, stP, stQ; W is
// the store's Wu); 2 = the RIGHT-HAND-SIDE-ONLY pass over a kept factor: the gather takes the right-hand sides alone, no
// sweep -- D_i^-1, P and Q are the stored bits, read from memory as the products' A-operands --, and the three phases run
// for the one column tile that holds W_R (nt = NT - 1 = 2 B / 16: for B = 8 / 16 / 24 it holds nothing else, and runs as
// small products: BcrRs), on the wave that owns the elimination's sweep in the full form. The right-hand-side products do
// not depend on the other tiles, the functions, their K order and the subtractions of the puts are the same code: R_a, R_c,
// W_R, sepR, extR come out bit for bit.
template <int B, int NR, bool L0, bool TOP, int NW, bool COH, int UF = 0>
__device__ __forceinline__ void bcr_reduce_body(
    const int chunk, double (*sDG)[B * B], double (*sR)[B * NR], double *sZ,

    int nb, int nred, int n, const int *__restrict__ sl_off, const int *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ diag, const double4 *__restrict__ rhs, const double *__restrict__ inD,
    const double *__restrict__ inR, const double *__restrict__ inXD, const double *__restrict__ inXR,
    const double *__restrict__ inXG, double *__restrict__ W, double *__restrict__ sepD, double *__restrict__ sepR,
    double *__restrict__ extD, double *__restrict__ extR, double *__restrict__ extG, double *__restrict__ xtop, int dbg,
    int nfar, const int *__restrict__ far_i, const int *__restrict__ far_j, int ext0, const int *__restrict__ bptr,
    const int *__restrict__ bghost, const double *__restrict__ bval, const int *__restrict__ ghost_extcol, int place,
    long long *__restrict__ stamps, double *__restrict__ Dinvg, double *__restrict__ topDinv, int *__restrict__ deadctr,
    int reg, double *__restrict__ stP = nullptr, double *__restrict__ stQ = nullptr) {
    typedef BcrDim<B, NR> Dm;
    constexpr int BB = B * B;
    double(*sD)[BB] = sDG;       // sD[0] becomes the chunk's contribution to the separator before it
    double(*sG)[BB] = sDG + 8;   // slot 0: coupling (separator before the chunk) -> block 0; slot j + 1: block j -> j + 1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ext0: this handle is a SHARD of a sequence (dist.hip) and the separator before its first chunk is the last block
    // of the rank before it -- same algebra, the coupling comes from the boundary slots of the ghost views
    const bool hasExt = chunk > 0 || ext0;
    constexpr int NT_ = NW * 64;  // threads
    const int kreal = nb - chunk * 8 < 8 ? nb - chunk * 8 : 8;  // real blocks of this chunk
    const bool placed = place && kreal < 8;                      // ... placed so that the last one is the separator

    if constexpr (UF == 2) {
        static_assert(NR == 3 && !TOP && 16 * (Dm::NT - 1) == 2 * B, "the last column tile holds the right-hand sides alone");
        constexpr int XB = B * NR;
        for (int e = tid; e < 9 * XB; e += NT_) (&sR[0][0])[e] = 0.0;
        if (tid < 2) sZ[tid] = 0.0;
        __syncthreads();
        if (L0) {
            const int row0 = chunk * 8 * B;
            for (int t = tid; t < kreal * B; t += NT_) {
                const int row = row0 + t;
                if (row < n) {
                    const double4 bb = rhs[row];
                    double *Rb = &sR[1][0] + t * NR;
                    Rb[0] = bb.x;
                    Rb[1] = bb.y;
                    Rb[2] = bb.z;
                }
            }
        } else {
            // R_j = sepR[j] + extR[j + 1] of the level below; the raw blocks of a mixed level 1 take theirs from rhs
            constexpr int NIR = (8 * XB + NT_ - 1) / NT_;
            double vr[NIR], vy[NIR];
#pragma unroll
            for (int u = 0; u < NIR; u++) {
                const int e = tid + NT_ * u, i = e / XB, el = e - i * XB, gb = chunk * 8 + i;
                const bool ok = e < 8 * XB && i < kreal && gb < nred;
                vr[u] = ok ? bcr_ld<COH>(inR + (size_t)gb * XB + el) : 0.0;
                vy[u] = ok && gb + 1 < nred ? bcr_ld<COH>(inXR + (size_t)(gb + 1) * XB + el) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < NIR; u++) {
                const int e = tid + NT_ * u, i = e / XB, gb = chunk * 8 + i;
                if (e < 8 * XB && i < kreal && gb < nred) (&sR[1][0])[e] = vr[u] + vy[u];
            }
            if (chunk * 8 + 8 > nred && nred < nb)
                for (int t = tid; t < 8 * B; t += NT_) {
                    const int i = t / B, gb = chunk * 8 + i;
                    if (gb >= nred && gb < nb) {
                        const int row = (8 * nred + (gb - nred)) * B + (t - i * B);
                        if (row < n) {
                            const double4 bb = rhs[row];
                            double *Rb = &sR[1][0] + t * NR;
                            Rb[0] = bb.x;
                            Rb[1] = bb.y;
                            Rb[2] = bb.z;
                        }
                    }
                }
        }
        __syncthreads();
        BcrElim<B, NR, 1> E;
        v4d out[Dm::MT][1];
#define IRH_BCR_ROUND_RHS(RND)                                                                                      \
    {                                                                                                               \
        constexpr int NE = 4 >> RND;                                                                                \
        int i = -1, a = -1, c = 7;                                                                                  \
        if (wave < NE) {                                                                                            \
            if (RND == 0) {                                                                                         \
                i = 2 * wave;                                                                                       \
                a = i - 1;                                                                                          \
                c = i + 1;                                                                                          \
            } else if (RND == 1) {                                                                                  \
                i = 1 + 4 * wave;                                                                                   \
                a = wave == 0 ? -1 : 3;                                                                             \
                c = wave == 0 ? 3 : 7;                                                                              \
            } else {                                                                                                \
                i = 3;                                                                                              \
            }                                                                                                       \
        }                                                                                                           \
        const bool active = i >= 0 && bcr_ridx(placed, kreal, i) >= 0;                                              \
        const bool hasP = a >= 0 || hasExt;                                                                         \
        const size_t el = (size_t)chunk * 7 + (i >= 0 ? i : 0);                                                     \
        if (active)                                                                                                 \
            E.template phase1<Dm::NT>(Dm::NT - 1, Dinvg + el * BB, stP + el * BB, hasP, stQ + el * BB, sR[i + 1], sZ, \
                                      sR[c + 1], W + el * B * Dm::NC, sZ, lane);                                    \
        __syncthreads();                                                                                            \
        if (active && hasP) {                                                                                       \
            E.template phase2_mul<Dm::NT>(Dm::NT - 1, stP + el * BB, sR[i + 1], out, lane);                         \
            E.template phase2_put<Dm::NT>(Dm::NT - 1, out, sZ, sZ, false, sR[a + 1], lane);                         \
        }                                                                                                           \
        __syncthreads();                                                                                            \
    }
        IRH_BCR_ROUND_RHS(0)
        IRH_BCR_ROUND_RHS(1)
        IRH_BCR_ROUND_RHS(2)
#undef IRH_BCR_ROUND_RHS
        for (int e = tid; e < XB; e += NT_) {
            bcr_st<COH>(sepR + (size_t)chunk * XB + e, sR[8][e]);
            if (hasExt) bcr_st<COH>(extR + (size_t)chunk * XB + e, sR[0][e]);
        }
        return;
    }

    // ---- load ----
    // A chunk of an upper level whose blocks all come from the level below and sit at their own positions (every chunk
    // but a shard's partial ones and those of a mixed level 1 that hold raw level-0 blocks) is loaded by the FAST path
    // below: every word of LDS is written exactly once -- value, identity or zero -- so LDS is not cleared first (18
    // stores per thread and a barrier in front of the first load), the right-hand sides are requested together with the
    // blocks (they were a second memory round trip) and the index arithmetic is that of a contiguous copy (round 5: the
    // load phase of an upper level took 8 500 clocks, half of it address arithmetic of the general mapping).
    const bool fastload = !L0 && !placed && !(chunk * 8 + 8 > nred && nred < nb);
    if (!fastload) {
        for (int e = tid; e < 8 * BB; e += NT_) {
            (&sD[0][0])[e] = 0.0;
            (&sG[0][0])[e] = 0.0;
        }
        for (int e = tid; e < 9 * B * NR; e += NT_) (&sR[0][0])[e] = 0.0;
        if (tid < 2) sZ[tid] = 0.0;
    }
    bcr_stamp(stamps, 0);
    if (!fastload) __syncthreads();
    bcr_stamp(stamps, 1);
    if (!L0 && fastload) {
        // block gb = chunk 8 + i of this level = chunk gb of the level below; (gb BB + el) = chunk 8 BB + e: contiguous
        constexpr int NIT = (8 * BB + NT_ - 1) / NT_, U = NIT <= 12 ? NIT : 8;
        constexpr int NIR = (8 * B * NR + NT_ - 1) / NT_;
        const size_t cb = (size_t)chunk * 8 * BB, cr = (size_t)chunk * 8 * B * NR;
        double vr[NIR], vy[NIR];
#pragma unroll
        for (int u = 0; u < NIR; u++) {
            const int e = tid + NT_ * u, i = e / (B * NR);
            const bool ok = e < 8 * B * NR && i < kreal;
            vr[u] = ok ? bcr_ld<COH>(inR + cr + e) : 0.0;
            vy[u] = ok && chunk * 8 + i + 1 < nred ? bcr_ld<COH>(inXR + cr + B * NR + e) : 0.0;
        }
        for (int u0 = 0; u0 < NIT; u0 += U) {
            double vd[U], vx[U], vg[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = tid + NT_ * (u0 + u), i = e / BB;
                const bool ok = e < 8 * BB && i < kreal;
                vd[u] = ok ? bcr_ld<COH>(inD + cb + e) : 0.0;
                vx[u] = ok && chunk * 8 + i + 1 < nred ? bcr_ld<COH>(inXD + cb + BB + e) : 0.0;
                vg[u] = ok && (chunk * 8 + i > 0 || ext0) ? bcr_ld<COH>(inXG + cb + e) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = tid + NT_ * (u0 + u), i = e / BB, el = e - i * BB;
                if (e >= 8 * BB) continue;
                // (a position without a block: the identity, its eliminations are skipped)
                (&sD[0][0])[e] = i < kreal ? vd[u] + vx[u] : (el % (B + 1) == 0 ? 1.0 : 0.0);
                (&sG[0][0])[e] = vg[u];
            }
        }
#pragma unroll
        for (int u = 0; u < NIR; u++) {
            const int e = tid + NT_ * u;
            if (e < 8 * B * NR) (&sR[1][0])[e] = vr[u] + vy[u];
        }
        for (int e = tid; e < B * NR; e += NT_) sR[0][e] = 0.0;
        if (tid < 2) sZ[tid] = 0.0;
    } else if (L0) {
        const int row0 = chunk * 8 * B;
        for (int t = tid; t < kreal * B; t += NT_) {
            const int row = row0 + t, blk = t / B, r = t - blk * B;
            const int ps = bcr_pos(placed, kreal, blk);
            if (row < n)
                bcr_gather_row<B, NR>(row, chunk * 8 + blk, r, sl_off, col, val, diag, rhs, &sDG[0][0], ps * BB,
                                      ps < 7 ? (8 + ps + 1) * BB : -1, blk == 0 ? 8 * BB : -1, sR[ps + 1], nfar, far_i,
                                      far_j);
            else
                sD[ps][r * B + r] = 1.0;
        }
        // (position 0 of a placed chunk stays zero: sD[0] collects the chunk's contribution to the separator before it,
        // and nothing assigns it first when no real block sits there)
        for (int i = placed ? 1 : 0; i < 8; i++)
            if (bcr_ridx(placed, kreal, i) < 0)
                for (int e = tid; e < B; e += NT_) sD[i][e * B + e] = 1.0;
        if (ext0 && chunk == 0) {
            // coupling (last block of the previous rank) -> block 0: the ghost entries of block 0's rows, -w each
            // (k_assemble0w leaves the weight of every boundary slot in bval); a thread owns column r of sG[0]
            for (int r = tid; r < B && r < n; r += NT_)
                for (int sl = bptr[r]; sl < bptr[r + 1]; sl++) {
                    const int gi = bghost[sl];
                    const int ec = gi >= 0 ? ghost_extcol[gi] : -1;
                    if (ec >= 0) sG[0][ec * B + r] -= bval[sl];
                }
        }
    } else {
        // blocks below nred come from the level below; the others (a mixed level 1, see bcr_alloc) are blocks of
        // the level-0 operator that no chunk reduced: block gb is level-0 block 8 nred + (gb - nred). Every block
        // brings the coupling from its predecessor along (slot i; slot 0: from the separator before the chunk).
        // every load of the launch is requested before the first value is used (a loop over the eight positions with
        // its loads inside was a memory round trip per position: 5 of the 8 us a launch costs before its first sweep)
        auto where = [&](int i, int &gb, int &slot) {
            const int t = bcr_ridx(placed, kreal, i);
            gb = t >= 0 ? chunk * 8 + t : -1;
            slot = t > 0 ? bcr_pos(placed, kreal, t - 1) + 1 : 0;
            return t;
        };
        constexpr int NIT = (8 * BB + NT_ - 1) / NT_, U = NIT <= 12 ? NIT : 8;
        // (a chunk of a mixed level that holds raw level-0 blocks only has nothing to fetch from the level below: the
        // positions without a block become the identity and the walk over the eight positions is skipped -- nine such
        // workgroups are what the sixty-four others of level 1 wait for at 100k views)
        const bool allraw = !placed && chunk * 8 >= nred;
        if (allraw)
            for (int e = tid; e < (8 - kreal) * B; e += NT_) sD[kreal + e / B][(e % B) * (B + 1)] = 1.0;
        for (int u0 = 0; u0 < NIT && !allraw; u0 += U) {
            double vd[U], vx[U], vg[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = tid + NT_ * (u0 + u), i = e / BB, el = e - i * BB;
                int gb, slot;
                const int t = e < 8 * BB ? where(i, gb, slot) : -1;
                const bool ok = t >= 0 && gb < nred;
                vd[u] = ok ? bcr_ld<COH>(inD + (size_t)gb * BB + el) : 0.0;
                vx[u] = ok && gb + 1 < nred ? bcr_ld<COH>(inXD + (size_t)(gb + 1) * BB + el) : 0.0;
                vg[u] = ok && (gb > 0 || ext0) ? bcr_ld<COH>(inXG + (size_t)gb * BB + el) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = tid + NT_ * (u0 + u), i = e / BB, el = e - i * BB;
                if (e >= 8 * BB) continue;
                int gb, slot;
                const int t = where(i, gb, slot);
                if (t >= 0 && gb < nred) {
                    sD[i][el] = vd[u] + vx[u];
                    if (gb > 0 || ext0) sG[slot][el] = vg[u];
                } else if (t < 0 && !(placed && i == 0) && el / B == el % B) {  // (sD[0] of a placed chunk: see the level-0 branch)
                    sD[i][el] = 1.0;
                }
            }
        }
        if (!allraw) {
            constexpr int NIR = (8 * B * NR + NT_ - 1) / NT_;
            double vr[NIR], vy[NIR];
#pragma unroll
            for (int u = 0; u < NIR; u++) {
                const int e = tid + NT_ * u, i = e / (B * NR), el = e - i * (B * NR);
                int gb, slot;
                const int t = e < 8 * B * NR ? where(i, gb, slot) : -1;
                const bool ok = t >= 0 && gb < nred;
                vr[u] = ok ? bcr_ld<COH>(inR + (size_t)gb * B * NR + el) : 0.0;
                vy[u] = ok && gb + 1 < nred ? bcr_ld<COH>(inXR + (size_t)(gb + 1) * B * NR + el) : 0.0;
                if (ok) sR[i + 1][el] = vr[u] + vy[u];
            }
        }
        if (chunk * 8 + 8 > nred && nred < nb) {
            for (int t = tid; t < 8 * B; t += NT_) {
                const int i = t / B, r = t - i * B, gb = chunk * 8 + i;
                if (gb >= nred && gb < nb) {
                    const int lb = 8 * nred + (gb - nred), row = lb * B + r;
                    if (row < n)
                        bcr_gather_row<B, NR, (NW == 8 && B <= 24 ? 24 : 12)>(row, lb, r, sl_off, col, val, diag, rhs, &sDG[0][0],
                                                                            i * BB, -1, gb > 0 ? (8 + i) * BB : -1, sR[i + 1],
                                                                            nfar, far_i, far_j);
                    else
                        sD[i][r * B + r] = 1.0;
                }
            }
        }
    }
    __syncthreads();
    bcr_stamp(stamps, 2);

    // ---- three rounds of eliminations: (0 2 4 6) (1 5) (3) ----
    constexpr int WPE0 = NW / 4 < Dm::NT ? NW / 4 : Dm::NT;  // waves per elimination in the first round
    constexpr int NTPW = (Dm::NT + WPE0 - 1) / WPE0;
    BcrElim<B, NR, NTPW> E;
    v4d out[Dm::MT][NTPW];
#define IRH_BCR_ROUND(RND)                                                                                          \
    {                                                                                                               \
        constexpr int NE = 4 >> RND;                                                                                \
        constexpr int WPE = NW / NE < Dm::NT ? NW / NE : Dm::NT;                                                    \
        /* (two waves per elimination, four eliminations: the wave that owns the column tiles 1 and 3 issues 72 products, */ \
        /* the other one 60, and wave w sits on SIMD w % 4 -- the roles are swapped in eliminations 2 and 3 so that every */ \
        /* SIMD gets one wave of each kind: 132 instead of 144 / 120 products of 64 clocks per SIMD)                      */ \
        const int e = wave / WPE, part0 = wave - e * WPE;                                                           \
        const int part = (WPE == 2 && NE == 4) ? (part0 ^ ((e >> 1) & 1)) : part0;                                  \
        int i = -1, a = -1, c = 7;                                                                                  \
        if (e < NE) {                                                                                               \
            if (RND == 0) {                                                                                         \
                i = 2 * e;                                                                                          \
                a = i - 1;                                                                                          \
                c = i + 1;                                                                                          \
            } else if (RND == 1) {                                                                                  \
                i = 1 + 4 * e;                                                                                      \
                a = e == 0 ? -1 : 3;                                                                                \
                c = e == 0 ? 3 : 7;                                                                                 \
            } else {                                                                                                \
                i = 3;                                                                                              \
            }                                                                                                       \
        }                                                                                                           \
        const bool active = i >= 0 && bcr_ridx(placed, kreal, i) >= 0;                                              \
        const bool hasP = a >= 0 || hasExt;                                                                         \
        /* the sweep of elimination e runs on wave e: the first four waves of a workgroup sit on four different */   \
        /* SIMDs (waves e WPE of an eight-wave workgroup share two, and two sweeps on one SIMD take 7 us, not 4) */  \
        const int isw = wave < NE ? (RND == 0 ? 2 * wave : RND == 1 ? 1 + 4 * wave : 3) : -1;                       \
        if (isw >= 0 && bcr_ridx(placed, kreal, isw) >= 0 && !(dbg & 1))                                            \
            bcr_invert<B>(sD[isw], lane, deadctr, reg != 0);                                                        \
        __syncthreads();                                                                                            \
        /* closures: the inverse of every eliminated block is kept (bcr_closures) */                                \
        if (Dinvg && active && part == 0)                                                                           \
            for (int o = lane; o < BB; o += 64) Dinvg[((size_t)chunk * 7 + i) * BB + o] = sD[i][o];                 \
        if constexpr (UF == 1)                                                                                      \
            if (active && part == 0)                                                                                \
                for (int o = lane; o < BB; o += 64) {                                                               \
                    stP[((size_t)chunk * 7 + i) * BB + o] = sG[a + 1][o];                                           \
                    stQ[((size_t)chunk * 7 + i) * BB + o] = sG[i + 1][o];                                           \
                }                                                                                                   \
        bcr_stamp(stamps, 3 + 4 * RND);                                                                             \
        if (active && !(dbg & 2))                                                                                   \
            E.template phase1<WPE>(part, sD[i], sG[a + 1], hasP, sG[i + 1], sR[i + 1], sD[c], sR[c + 1],            \
                                   W + ((size_t)chunk * 7 + i) * B * Dm::NC, sZ, lane);                             \
        __syncthreads();                                                                                            \
        bcr_stamp(stamps, 4 + 4 * RND);                                                                             \
        if (active && hasP && !(dbg & 4)) E.template phase2_mul<WPE>(part, sG[a + 1], sR[i + 1], out, lane);        \
        if (WPE > 1) __syncthreads();                                                                               \
        bcr_stamp(stamps, 5 + 4 * RND);                                                                             \
        if (active && hasP && !(dbg & 4))                                                                           \
            E.template phase2_put<WPE>(part, out, sG[a + 1], a >= 0 ? sD[a] : sD[0], a < 0 && RND == 0, sR[a + 1],  \
                                       lane);                                                                       \
        __syncthreads();                                                                                            \
        bcr_stamp(stamps, 6 + 4 * RND);                                                                             \
    }
    IRH_BCR_ROUND(0)
    IRH_BCR_ROUND(1)
    IRH_BCR_ROUND(2)
#undef IRH_BCR_ROUND

    // ---- store ----
    if (TOP) {
        if (wave == 0) {
            if (bcr_ridx(placed, kreal, 7) >= 0) {
                bcr_invert<B>(sD[7], lane, deadctr, reg != 0);
                if (topDinv)
                    for (int o = lane; o < BB; o += 64) topDinv[o] = sD[7][o];
                for (int o = lane; o < B * NR; o += 64) {
                    const int k = o / NR, q = o - NR * k;
                    double s = 0.0;
                    for (int cidx = 0; cidx < B; cidx++) s += sD[7][k * B + cidx] * sR[8][cidx * NR + q];
                    xtop[o] = s;
                }
            } else {
                for (int o = lane; o < B * NR; o += 64) xtop[o] = 0.0;
            }
        }
    } else {
        for (int e = tid; e < BB; e += NT_) {
            bcr_st<COH>(sepD + (size_t)chunk * BB + e, sD[7][e]);
            if (hasExt) {
                bcr_st<COH>(extD + (size_t)chunk * BB + e, sD[0][e]);
                bcr_st<COH>(extG + (size_t)chunk * BB + e, sG[0][e]);
            }
        }
        for (int e = tid; e < B * NR; e += NT_) {
            bcr_st<COH>(sepR + (size_t)chunk * B * NR + e, sR[8][e]);
            if (hasExt) bcr_st<COH>(extR + (size_t)chunk * B * NR + e, sR[0][e]);
        }
    }
    bcr_stamp(stamps, 15);
}

// ASM (level 0 of a plain banded handle, 8 B a multiple of 64: ls_solve): the workgroup ASSEMBLES the slices of its
// chunk first -- K3's body (asm0w.hpp: MODE 0, no level 1) for the 8 B / 64 slices that are exactly the chunk's rows --
// and then reduces the chunk. What bcr_gather_row reads (values, diagonal and right-hand side of the chunk's own rows)
// this very workgroup wrote: a workgroup barrier lies in between, no workgroup waits for another, and the launch of
// k_assemble0w in front of the solve is gone -- with it the fourth round of K3's workgroups (1568 on 512 slots at 100k
// views), a launch boundary behind 32 MB of dirty values, and a gather from memory (the values are hot in L2 now). The
// two phases use the same LDS one after the other. The slices under no chunk (the raw blocks of a mixed level 1) are
// assembled by extra workgroups behind the chunks', one slice each; the upper levels' launch gathers them. Everything K3
// writes is written as before (the ways back, the edge diagnostics and the residual read it).
struct BcrAsmArgs {
    int nch, nsl;
    long long m, mpad;
    const uint32_t *slot_eid;
    const int *tile_e0;
    const uint32_t *beid;
    const uint8_t *bflag;
    const double *wsrc, *er;
    double *excess, *idg, *bval;
    double *stP, *stQ;  // the unit-weight factor's P and Q of level 0 (UF != 0)
};
// (ASM: the kernel itself writes val / diag / rhs -- they are no read-only arguments of its)
template <bool ASM>
struct BcrL0Ptr {
    typedef const double *__restrict__ d;
    typedef const double4 *__restrict__ d4;
};
template <>
struct BcrL0Ptr<true> {
    typedef double *d;
    typedef double4 *d4;
};

template <int B, int NR, bool L0, bool TOP, int NW, bool ASM = false, int UF = 0>
__global__ __launch_bounds__(NW * 64, (NW == 4 && B <= 24 && NR == 3 ? 2 : 1)) void k_bcr_reduce(

    int nb, int nred, int n, const int *__restrict__ sl_off, const int *__restrict__ col, typename BcrL0Ptr<ASM>::d val,
    typename BcrL0Ptr<ASM>::d diag, typename BcrL0Ptr<ASM>::d4 rhs, const double *__restrict__ inD,
    const double *__restrict__ inR, const double *__restrict__ inXD, const double *__restrict__ inXR,
    const double *__restrict__ inXG, double *__restrict__ W, double *__restrict__ sepD, double *__restrict__ sepR,
    double *__restrict__ extD, double *__restrict__ extR, double *__restrict__ extG, double *__restrict__ xtop, int dbg,
    int nfar, const int *__restrict__ far_i, const int *__restrict__ far_j, int ext0, const int *__restrict__ bptr,
    const int *__restrict__ bghost, const double *__restrict__ bval, const int *__restrict__ ghost_extcol, int place,
    long long *__restrict__ stamps, double *__restrict__ Dinvg, double *__restrict__ topDinv, int *__restrict__ deadctr,
    int reg, BcrAsmArgs A) {
    // one buffer: the reduction's blocks, right-hand sides and two flags -- and, before them, K3's window of a slice
    constexpr int kRed = 16 * B * B + 9 * B * NR + 2, kAsm = ASM ? Asm0wLds<0, false>::doubles : 0;
    __shared__ double lds[kRed > kAsm ? kRed : kAsm];
    double(*sDG)[B * B] = reinterpret_cast<double(*)[B * B]>(lds);
    double(*sR)[B * NR] = reinterpret_cast<double(*)[B * NR]>(lds + 16 * B * B);  // slot 0: contribution to the right-hand side of the separator before the chunk
    double *sZ = lds + 16 * B * B + 9 * B * NR;
    if constexpr (ASM) {
        static_assert(L0 && NR == 3 && (8 * B) % 64 == 0, "a chunk's rows are whole slices");
        constexpr int SPC = 8 * B / 64;  // slices per chunk
#define IRH_BCR_ASM_SLICE(sl_)                                                                                           \
    asm0w_slice<0, false, NW * 64>(sl_, lds, n, A.m, A.mpad, sl_off, A.slot_eid, (const uint8_t *)nullptr, A.tile_e0, bptr, \
                                   A.beid, A.bflag, A.wsrc, A.er, val, A.excess, diag, A.idg, rhs, A.bval, 0,            \
                                   (const int *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr,        \
                                   (double *)nullptr)
        if ((int)blockIdx.x >= A.nch) {
            // a slice under no chunk of this level
            const int sl = A.nch * SPC + ((int)blockIdx.x - A.nch);
            if (sl < A.nsl) IRH_BCR_ASM_SLICE(sl);
            return;
        }
        for (int k = 0; k < SPC; k++) {
            const int sl = (int)blockIdx.x * SPC + k;
            if (sl >= A.nsl) break;
            IRH_BCR_ASM_SLICE(sl);
            __syncthreads();  // (the last wave-0 reads of this slice's window and partial sums | the next use of the LDS)
        }
#undef IRH_BCR_ASM_SLICE
        // the chunk's rows are in memory as far as THIS workgroup is concerned (its waves share one L1; a device-scope
        // release would write back the whole L2): stores issued and complete, then the barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    static_assert(UF == 0 || ASM, "the unit-weight factor rides on the assembling launch");
    bcr_reduce_body<B, NR, L0, TOP, NW, false, UF>(blockIdx.x, sDG, sR, sZ, nb, nred, n, sl_off, col, val, diag, rhs, inD, inR, inXD, inXR,
                                                   inXG, W, sepD, sepR, extD, extR, extG, xtop, dbg, nfar, far_i, far_j, ext0, bptr,
                                                   bghost, bval, ghost_extcol, place, stamps, Dinvg, topDinv, deadctr, reg, A.stP,
                                                   A.stQ);
}

// ---------------------------------------------------------------------------------------------
// The top of the hierarchy in ONE workgroup: up to sixteen blocks (round 5; until then a level of 9 ... 64 blocks was
// reduced by chunks of eight to a top of <= 8 -- at 100k views the last two levels held 10 and 2 blocks and cost a load,
// four rounds, a store and a level boundary more than the 10 blocks need). The blocks of the top level are loaded once;
// every round eliminates up to four blocks no two of which are neighbours (four sweeps on four SIMDs, their products
// dealt to the eight waves as in a chunk), by a schedule the host writes (bcr_top_schedule: the first four even positions
// of the list of blocks still alive -- 10 blocks: 10 -> 6 -> 3 -> 1 in three rounds, 16: five); the block that is left
// is solved. W stays in LDS, in the places an elimination frees (W_P over D_i^-1, W_Q over the coupling to the right
// neighbour, W_R over R_i), so the way back of the top level follows at once: the workgroup writes the solutions of ALL
// its blocks, and the ways back of the levels below start from them (k_bcr_back_top / k_bcr_back: one level less).
// The coupling of block x to the next block alive lives in sG[x]; a fill-in A[a, c] takes the place of A[a, i].
// Three right-hand sides, B <= 24 (LDS: (2 n - 1) blocks + 2 n right-hand-side slots = 158 KB for n = 16, B = 24), no
// closures (their step programs know chunks only), not a shard.
// ---------------------------------------------------------------------------------------------
static BcrTopSched bcr_top_schedule(int n) {
    BcrTopSched T;
    memset(&T, 0, sizeof(T));
    T.n = n;
    std::vector<int> alive(n);
    for (int k = 0; k < n; k++) alive[k] = k;
    while (alive.size() > 1 && T.nr < kTopRounds) {
        const int r = T.nr++;
        std::vector<int> next;
        int ne = 0;
        for (size_t p = 0; p < alive.size(); p++) {
            if (p % 2 == 0 && ne < 4) {
                T.i[r][ne] = (signed char)alive[p];
                T.a[r][ne] = (signed char)(p > 0 ? alive[p - 1] : -1);
                T.c[r][ne] = (signed char)(p + 1 < alive.size() ? alive[p + 1] : -1);
                ne++;
            } else {
                next.push_back(alive[p]);
            }
        }
        T.ne[r] = (signed char)ne;
        alive.swap(next);
    }
    T.last = alive[0];
    return T;
}
static size_t bcr_top_lds(int B, int n) {
    return ((size_t)(2 * n - 1) * B * B + (size_t)2 * n * B * 3 + 2) * sizeof(double) + sizeof(BcrTopSched);
}

// (the filling solve's copies of a block into the store, as a function: see bcr_rs_phase1_call)
template <int BB>
__device__ __noinline__ void bcr_top_keep(double *dst, const double *src, bool have, int lane) {
    for (int o = lane; o < BB; o += 64) dst[o] = have ? src[o] : 0.0;
}

// UF (BcrUnit::top): 1 = the operands of every scheduled elimination, what it leaves for the way back and the inverse of the
// block that is left are also written to tst; 2 = the right-hand-side-only pass: they are read from there (see bcr_reduce_body)
template <int B, int NW, bool COH, int UF = 0>
__device__ __forceinline__ void bcr_top_body(double *smem, const BcrTopSched *__restrict__ Tg, const double *__restrict__ inD,
                                             const double *__restrict__ inR, const double *__restrict__ inXD,
                                             const double *__restrict__ inXR, const double *__restrict__ inXG,
                                             double *__restrict__ xout, int dbg, long long *__restrict__ stamps,
                                             double *__restrict__ tst = nullptr) {
    constexpr int NR = 3;
    typedef BcrDim<B, NR> Dm;
    constexpr int BB = B * B, XB = B * NR, NT_ = NW * 64;
    static_assert(NW == 8, "eight waves");
    const int n = Tg->n;
    double(*sD)[BB] = reinterpret_cast<double(*)[BB]>(smem);
    double(*sG)[BB] = sD + n;  // n - 1 slots
    double(*sR)[XB] = reinterpret_cast<double(*)[XB]>(smem + (size_t)(2 * n - 1) * BB);
    double(*sX)[XB] = sR + n;
    double *sZ = &sX[n][0];
    // (the schedule is read with indices that are not known at compile time, by every wave, in every round: LDS)
    BcrTopSched &T = *reinterpret_cast<BcrTopSched *>(sZ + 2);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    static_assert(sizeof(BcrTopSched) % 4 == 0, "copied by words");
    if (tid < (int)(sizeof(BcrTopSched) / 4)) reinterpret_cast<int *>(&T)[tid] = reinterpret_cast<const int *>(Tg)[tid];
    bcr_stamp(stamps, 0);
    // ---- load: D_j = sepD[j] + extD[j + 1], R_j = sepR[j] + extR[j + 1], coupling j - 1 -> j = extG[j] ----
    {
        constexpr int U = 6;
        const int nD = n * BB, nG = (n - 1) * BB, nR = n * XB;
        for (int e0 = 0; e0 < nD && UF != 2; e0 += U * NT_) {
            double vd[U], vx[U], vg[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = e0 + tid + NT_ * u;
                vd[u] = e < nD ? bcr_ld<COH>(inD + e) : 0.0;
                vx[u] = e < nG ? bcr_ld<COH>(inXD + BB + e) : 0.0;
                vg[u] = e < nG ? bcr_ld<COH>(inXG + BB + e) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = e0 + tid + NT_ * u;
                if (e < nD) (&sD[0][0])[e] = vd[u] + vx[u];
                if (e < nG) (&sG[0][0])[e] = vg[u];
            }
        }
        for (int e = tid; e < nR; e += NT_) {
            const double vr = bcr_ld<COH>(inR + e);
            const double vy = e < nR - XB ? bcr_ld<COH>(inXR + XB + e) : 0.0;
            (&sR[0][0])[e] = vr + vy;
        }
        if (tid < 2) sZ[tid] = 0.0;
    }
    __syncthreads();
    bcr_stamp(stamps, 1);
    // ---- the rounds ----
    for (int r = 0; r < T.nr; r++) {
        const int ne = T.ne[r];
        // (the lane number as the round sees it is opaque: what the products derive from it -- dozens of offsets per
        // instantiation -- is formed again in every round instead of living in registers across the whole loop)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if constexpr (UF == 2) {
            const bool active = wave < ne;
            const int i = active ? T.i[r][wave] : 0, a = active ? T.a[r][wave] : -1, c = active ? T.c[r][wave] : -1;
            const bool hasP = a >= 0, hasQ = c >= 0;
            const double *op = tst + (size_t)5 * (4 * r + (active ? wave : 0)) * BB;  // D_i^-1, P, Q
            BcrElim<B, NR, 1, true> E;
            v4d out[Dm::MT][1];
            if (active)
                E.template phase1<Dm::NT>(Dm::NT - 1, op, op + BB, hasP, op + 2 * BB, sR[i], sZ, hasQ ? sR[c] : sR[i],
                                          (double *)nullptr, sZ, ln, hasQ);
            __syncthreads();
            if (active && hasP) E.template phase2_mul<Dm::NT>(Dm::NT - 1, op + BB, sR[i], out, ln);
            if (active) E.template keep_w<Dm::NT>(Dm::NT - 1, sZ, sZ, hasQ, sR[i], ln);
            __syncthreads();
            if (active && hasP) E.template phase2_put<Dm::NT>(Dm::NT - 1, out, sZ, sZ, false, sR[a], ln);
            __syncthreads();
            continue;
        }
        if (wave < ne && !(dbg & 1)) bcr_invert<B>(sD[T.i[r][wave]], ln);
        __syncthreads();
        bcr_stamp(stamps, 2 + 2 * r);
        auto products = [&](auto wpe_tag) {
            constexpr int WPE = decltype(wpe_tag)::value;
            const int e = wave / WPE, part0 = wave - e * WPE;
            const int part = WPE == 2 ? (part0 ^ ((e >> 1) & 1)) : part0;
            const bool active = e < ne;
            const int i = active ? T.i[r][e] : 0, a = active ? T.a[r][e] : -1, c = active ? T.c[r][e] : -1;
            const bool hasP = a >= 0, hasQ = c >= 0;
            BcrElim<B, NR, 2, true> E;
            v4d out[Dm::MT][2];
            double *op = UF == 1 ? tst + (size_t)5 * (4 * r + (active ? e : 0)) * BB : nullptr;
            if constexpr (UF == 1)
                if (active && part == 0) {
                    bcr_top_keep<BB>(op, sD[i], true, ln);
                    bcr_top_keep<BB>(op + BB, hasP ? sG[a] : sZ, hasP, ln);
                    bcr_top_keep<BB>(op + 2 * BB, hasQ ? sG[i] : sZ, hasQ, ln);
                }
            if (active && !(dbg & 2))
                E.template phase1<WPE>(part, sD[i], hasP ? sG[a] : sZ, hasP, hasQ ? sG[i] : sZ, sR[i], hasQ ? sD[c] : sD[i],
                                       hasQ ? sR[c] : sR[i], (double *)nullptr, sZ, ln, hasQ);
            __syncthreads();
            if (active && hasP && !(dbg & 4)) E.template phase2_mul<WPE>(part, sG[a], sR[i], out, ln);
            if (active && !(dbg & 2)) E.template keep_w<WPE>(part, sD[i], hasQ ? sG[i] : sZ, hasQ, sR[i], ln);
            __syncthreads();
            if (active && hasP && !(dbg & 4)) E.template phase2_put<WPE>(part, out, sG[a], sD[a], false, sR[a], ln);
            __syncthreads();
            // (what keep_w left: nobody writes the places of an eliminated block any more)
            if constexpr (UF == 1)
                if (active && part == 0) {
                    bcr_top_keep<BB>(op + 3 * BB, sD[i], true, ln);
                    bcr_top_keep<BB>(op + 4 * BB, hasQ ? sG[i] : sZ, hasQ, ln);
                }
        };
        if (ne > 2) products(std::integral_constant<int, 2>());
        else products(std::integral_constant<int, 4>());
        bcr_stamp(stamps, 3 + 2 * r);
    }
    // ---- the block that is left ----
    const int last = T.last;
    if (wave == 0) {
        if constexpr (UF != 2) bcr_invert<B>(sD[last], lane);
        const double *Dl = UF == 2 ? tst + (size_t)kTopUnitLast * BB : sD[last];
        for (int o = lane; o < XB; o += 64) {
            const int k = o / NR, q = o - NR * k;
            double acc = 0.0;
            for (int cidx = 0; cidx < B; cidx++) acc += Dl[k * B + cidx] * sR[last][cidx * NR + q];
            sX[last][o] = acc;
        }
    }
    __syncthreads();
    // (behind the barrier, like every other record: nothing writes the block that is left any more)
    if constexpr (UF == 1)
        for (int o = tid; o < BB; o += NT_) tst[(size_t)kTopUnitLast * BB + o] = sD[last][o];
    bcr_stamp(stamps, 14);
    // ---- the way back: x_i = W_R - W_P x_a - W_Q x_c, rounds in reverse; a unit of work = four rows of a block ----
    {
        constexpr int UPB = B / 4, NCT = (2 * B + 15) / 16;
        const int lk = lane >> 4, lp = lane & 15;
        for (int r = T.nr - 1; r >= 0; r--) {
            const int ne = T.ne[r];
            for (int u = wave; u < ne * UPB; u += NW) {
                const int e = u / UPB, it = u - e * UPB;
                const int i = T.i[r][e], a = T.a[r][e], c = T.c[r][e];
                const double *xa = sX[a >= 0 ? a : 0], *xc = sX[c >= 0 ? c : 0];
                const double *wP = UF == 2 ? tst + ((size_t)5 * (4 * r + e) + 3) * BB : sD[i];
                const double *wQ = UF == 2 ? tst + ((size_t)5 * (4 * r + e) + 4) * BB : sG[i];
                const int k = 4 * it + lk;
                double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int t = 0; t < NCT; t++) {
                    const int cidx = lp + 16 * t;
                    if (cidx < B) {
                        if (a >= 0) {
                            const double wv = wP[k * B + cidx];
                            s0 += wv * xa[cidx * 3 + 0];
                            s1 += wv * xa[cidx * 3 + 1];
                            s2 += wv * xa[cidx * 3 + 2];
                        }
                    } else if (cidx < 2 * B) {
                        if (c >= 0) {
                            const double wv = wQ[k * B + cidx - B];
                            s0 += wv * xc[(cidx - B) * 3 + 0];
                            s1 += wv * xc[(cidx - B) * 3 + 1];
                            s2 += wv * xc[(cidx - B) * 3 + 2];
                        }
                    }
                }
                s0 = bcr_row16_sum(s0);
                s1 = bcr_row16_sum(s1);
                s2 = bcr_row16_sum(s2);
                if (lp == 0) {
                    sX[i][k * 3 + 0] = sR[i][k * 3 + 0] - s0;
                    sX[i][k * 3 + 1] = sR[i][k * 3 + 1] - s1;
                    sX[i][k * 3 + 2] = sR[i][k * 3 + 2] - s2;
                }
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < n * XB; e += NT_) xout[e] = (&sX[0][0])[e];
    bcr_stamp(stamps, 15);
}

// the top alone (a launch of its own: timing of single levels, a handle whose single-launch reduction was not admitted)
template <int B>
__global__ __launch_bounds__(512, 1) void k_bcr_top(const BcrTopSched *__restrict__ T, const double *__restrict__ inD, const double *__restrict__ inR,
                                                    const double *__restrict__ inXD, const double *__restrict__ inXR,
                                                    const double *__restrict__ inXG, double *__restrict__ xout, int dbg,
                                                    long long *__restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) double top_smem[];
    bcr_top_body<B, 8, false>(top_smem, T, inD, inR, inXD, inXR, inXG, xout, dbg, stamps);
}

// The reductions of ALL levels above level 0 in ONE launch (round 4). Those levels hold 1.6 % of the rows; each was a
// launch of 73 / 10 / 2 / 1 workgroups that spends ~5 us of its 20 - 38 us starting, filling and draining. Here workgroup c
// runs chunk c of every level that has one, level after level; between two levels the workgroups that go on wait for a
// counter every workgroup of the level before has passed. What the first attempt at this lost (round 3: 325 instead of
// 290 us per solve) was the way the data crossed the level boundary -- a device-scope release and acquire per workgroup
// and boundary, i.e. L2 write-backs and invalidates, 7 us each. Now the separator data is WRITTEN by device-scope
// atomic stores and READ by device-scope atomic loads (bcr_st / bcr_ld: the coherence point of the eight L2s, no
// fence), the counter is a relaxed atomic: ~1.2 us per boundary (tools/micro/xcdbar.hip, sixteen workgroups on eight
// XCDs). All workgroups of the launch fit the chip at once (one per CU), so nobody waits for a workgroup that cannot
// start. A wait that does not end (~1 s) poisons the top separator: the solve then fails with IROTAVG_ERR_SOLVER at the
// next score instead of hanging the device. W goes to memory as before: the ways back are later launches.
// The bodies of the levels are separate FUNCTIONS (round 5): inlined into one kernel the three of them -- a chunk, a chunk
// that is the top, the sixteen-block top -- shared one register allocation with the level loop around them, and the
// kernel spilled (36 registers in round 4, 155 with the sixteen-block top) where each body alone needs 124 - 212 and
// spills nothing. A call per level costs nothing against 30 us of work. Their arguments live in device memory (written
// once per handle: only the generation, the debug word and the stamp array change from solve to solve and travel as
// kernel arguments); LDS is the launch's dynamic allocation, named by the functions themselves.
// (16-byte alignment: the sweeps read LDS by ds_read_b128; behind the kernel's one static word an 8-byte-aligned base made
// every such read a split one and a sweep 3.5 x slower)
extern __shared__ __attribute__((aligned(16))) double up_smem[];
typedef IRH_GPTR(const BcrUpArgs) gp_args;
template <int B, bool TOP, int UF = 0>
__device__ __noinline__ void bcr_up_chunk(gp_args A, int i, int dbg, long long *stl) {
    constexpr int NR = 3;
    IRH_GPTR(const BcrUpLevel) L = &A->lev[i];
    double(*sDG)[B * B] = reinterpret_cast<double(*)[B * B]>(up_smem);
    double(*sR)[B * NR] = reinterpret_cast<double(*)[B * NR]>(up_smem + 16 * B * B);
    double *sZ = up_smem + 16 * B * B + 9 * B * NR;
    bcr_reduce_body<B, NR, false, TOP, 8, true, UF>(
        blockIdx.x, sDG, sR, sZ, L->nb, L->nred, A->n, (const int *)A->sl_off, (const int *)A->col, (const double *)A->val,
        (const double *)A->diag, (const double4 *)A->rhs, (const double *)L->inD, (const double *)L->inR, (const double *)L->inXD,
        (const double *)L->inXR, (const double *)L->inXG, (double *)L->W, (double *)L->sepD, (double *)L->sepR, (double *)L->extD,
        (double *)L->extR, (double *)L->extG, (double *)A->xtop, dbg, 0, (const int *)nullptr, (const int *)nullptr, 0, (const int *)nullptr, (const int *)nullptr,
        (const double *)nullptr, (const int *)nullptr, 0, stl ? stl - (size_t)blockIdx.x * 16 : nullptr,
        UF ? (double *)L->stD : (double *)nullptr, (double *)nullptr, (int *)nullptr, 0, UF ? (double *)L->stP : (double *)nullptr,
        UF ? (double *)L->stQ : (double *)nullptr);   // (bcr_stamp adds 16 x the workgroup's number)
}
template <int B, int UF = 0>
__device__ __noinline__ void bcr_up_top(gp_args A, int i, int dbg, long long *stl) {
    IRH_GPTR(const BcrUpLevel) L = &A->lev[i];
    bcr_top_body<B, 8, true, UF>(up_smem, (const BcrTopSched *)&A->top, (const double *)L->inD, (const double *)L->inR,
                                 (const double *)L->inXD, (const double *)L->inXR, (const double *)L->inXG, (double *)A->xtop_all, dbg,
                                 stl ? stl - (size_t)blockIdx.x * 16 : nullptr, UF ? (double *)A->tst : (double *)nullptr);
}
// UF != 0 (the unit-weight factor: the launch that fills it, the right-hand-side-only launch): a sixteen-block top only
template <int B, int UF = 0>
__global__ __launch_bounds__(512, 1) void k_bcr_reduce_up(const BcrUpArgs *__restrict__ Ap, unsigned gen, int dbg,
                                                          long long *__restrict__ stamps) {
    constexpr int NR = 3;
    __shared__ int s_ok;
    const gp_args Ag = (gp_args)Ap;
    const BcrUpArgs &A = *Ap;
    const int wg = blockIdx.x;
    const int nl = A.nl;
    bool fine = true;
    for (int i = 0; i < nl; i++) {
        if (wg >= A.lev[i].nch) break;  // (the chunk counts shrink level by level)
        long long *stl = stamps && wg == (dbg >> 8) ? stamps + 32 * i : nullptr;  // (the workgroup that stamps: dbg >> 8)
        if (stl && threadIdx.x == 0) stl[16] = (long long)__builtin_readcyclecounter();
        // (slots 20 ...: where the workgroup's waves sit -- HW_ID: wave [3:0], SIMD [5:4], CU [11:8], SE [15:13])
        if (stl && (threadIdx.x & 63) == 0) stl[20 + (threadIdx.x >> 6)] = 0x10000 + (long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
        if (i > 0) {
            if (threadIdx.x == 0) {
                const unsigned target = gen * (unsigned)A.lev[i - 1].nch;
                int good = 0;
                for (int spin = 0; spin < (1 << 21); spin++) {
                    // (a difference: the counter may wrap)
                    if ((int)(__hip_atomic_load((const unsigned *)A.cnt + (i - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) {
                        good = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (!good) __hip_atomic_store((int *)A.fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_ok = good;
            }
            __syncthreads();
            fine = fine && s_ok != 0;
        }
        if (stl && threadIdx.x == 0) stl[17] = (long long)__builtin_readcyclecounter();
        if (i == nl - 1) {
            // (the top workgroup has waited for every workgroup of the level below, and a workgroup sets the word before it
            // counts itself)
            const bool bad = !fine || __hip_atomic_load((const int *)A.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
            // bad: NaN into every entry -- it then reaches every solution row on the ways back, no view takes a step
            // (step_apply leaves a rotation alone when its step is not finite) and the score is NaN
            if (A.top16) {
                if (!bad) bcr_up_top<B, UF>(Ag, i, dbg, stl);
                else
                    for (int e = threadIdx.x; e < A.top.n * B * NR; e += 512) A.xtop_all[e] = __builtin_nan("");
            } else {
                if constexpr (UF == 0) {
                    if (!bad) bcr_up_chunk<B, true>(Ag, i, dbg, stl);
                }
                if (bad)
                    for (int e = threadIdx.x; e < B * NR; e += 512) A.xtop[e] = __builtin_nan("");
            }
        } else {
            if (fine) bcr_up_chunk<B, false, UF>(Ag, i, dbg, stl);
            if (stl && threadIdx.x == 0) stl[18] = (long long)__builtin_readcyclecounter();
            // every thread's separator stores have been acknowledged before the workgroup is counted
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_fetch_add((unsigned *)A.cnt + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (stl && threadIdx.x == 0) stl[19] = (long long)__builtin_readcyclecounter();
        }
    }
}

// k_bcr_reduce_up's workgroups WAIT for each other, so all workgroups of a launch must be resident at the same time -- and
// so must those of every other such launch that is dispatched next to it (l1ra's three chains, other handles, other
// sessions): two launches that each hold a part of the device and spin for the rest would wait until the bounded spin
// gives up. The launches of one process therefore RESERVE their share of the device first: a launch of N workgroups
// costs N / (workgroups of this kernel that fit the device, from the occupancy query) and is admitted while the sum over
// all handles stays within the device; a handle keeps its share (its launches are ordered on its stream: the largest
// counts, not the sum) until it is idle. A launch that is not admitted runs level by level, as before round 4.
// IROTAVG_BCR_UP_CAP: the capacity in 1/1024ths (tests).
template <int B>
static size_t bcr_up_lds(int ntop) {
    const size_t chunk = ((size_t)16 * B * B + 9 * B * 3 + 2) * sizeof(double);
    return ntop > 0 ? std::max(chunk, bcr_top_lds(B, ntop)) : chunk;
}
namespace {
std::atomic<unsigned> g_unit_epoch{0};  // irotavg_trim_memory's count: a store allocated under an older one is released
std::atomic<int> g_up_used[16];
template <int B>
int bcr_up_capacity(int dev) {
    static std::atomic<int> cap[16];
    const int d = dev & 15;
    int c = cap[d].load(std::memory_order_relaxed);
    if (c == 0) {
        int per_cu = 0, cus = 0;
        // (dynamic LDS: at least a chunk's; a sixteen-block top asks for more, still one workgroup per CU either way)
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bcr_reduce_up<B>, 512, bcr_up_lds<B>(0)) != hipSuccess) per_cu = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        (void)hipGetLastError();
        c = per_cu > 0 && cus > 0 ? per_cu * cus : -1;
        cap[d].store(c, std::memory_order_relaxed);
    }
    return c;
}
template <int B>
bool bcr_up_reserve(Graph &g, int nwg) {
    const int capwg = bcr_up_capacity<B>(g.device);
    if (capwg <= 0) return false;
    const int total = g.sw.bcr_up_cap;
    const int cost = (int)(((long long)nwg * 1024 + capwg - 1) / capwg);
    const int need = cost - g.bcr_up_held;
    if (need <= 0) return true;
    std::atomic<int> &used = g_up_used[g.device & 15];
    const int before = used.fetch_add(need, std::memory_order_acq_rel);
    if (before + need > total) {
        used.fetch_sub(need, std::memory_order_acq_rel);
        return false;
    }
    g.bcr_up_held += need;
    return true;
}
}  // namespace
void bcr_up_release(Graph &g) noexcept {
    if (g.bcr_up_held > 0) {
        g_up_used[g.device & 15].fetch_sub(g.bcr_up_held, std::memory_order_acq_rel);
        g.bcr_up_held = 0;
    }
}

// The three rounds of the way back of one chunk: its W in sW, the solutions of the separator before it and of its own
// separator in sX[0] and sX[8], the other slots zero. Ends with a workgroup barrier. 256 threads. mask: the positions
// wanted (bit i; closed under what a position depends on, bcr_back_mask) -- the others are not computed.
// Three right-hand sides: a unit of work is four rows of one block (sixteen lanes per row of W, three accumulators
// each); the units of a round are dealt to the four waves, so the single block of round 2 and the two of round 1 do not
// leave three / two waves idle.
__device__ __forceinline__ int bcr_back_mask(int m) {
    if (m & 0x05) m |= 0x02;   // 0, 2 need 1
    if (m & 0x50) m |= 0x20;   // 4, 6 need 5
    if (m & 0x36) m |= 0x08;   // 1, 2, 4, 5 need 3
    return m;
}
template <int B, int NR, int NWB = 4>
__device__ __forceinline__ void bcr_back_rounds(const double *sW, double (*sX)[B * NR], bool placed, int kreal, int wave,
                                                int lane, int mask = 0x7f) {
    typedef BcrDim<B, NR> Dm;
    constexpr int WB = B * Dm::NC;
    const int lk = lane >> 4, lp = lane & 15;
#pragma unroll
    for (int rnd = 2; rnd >= 0; rnd--) {
        if (NR == 3) {
            constexpr int UPB = B / 4;                  // units per block
            const int nbk = 4 >> rnd;                   // blocks of the round: 3 | 1 5 | 0 2 4 6
            for (int u = wave; u < nbk * UPB; u += NWB) {
                const int e = u / UPB, it = u - e * UPB;
                int i, a, c;
                if (rnd == 0) {
                    i = 2 * e;
                    a = i - 1;
                    c = i + 1;
                } else if (rnd == 1) {
                    i = 1 + 4 * e;
                    a = e == 0 ? -1 : 3;
                    c = e == 0 ? 3 : 7;
                } else {
                    i = 3;
                    a = -1;
                    c = 7;
                }
                if (!((mask >> i) & 1) || bcr_ridx(placed, kreal, i) < 0) continue;
                const double *Wi = sW + i * WB;
                const double *xa = sX[a + 1], *xcn = sX[c + 1];
                const int k = 4 * it + lk;
                double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int t = 0; t < Dm::NT; t++) {
                    const int cidx = lp + 16 * t;
                    if (cidx < Dm::NC) {
                        const double wv = Wi[k * Dm::NC + cidx];
                        if (cidx < B) {
                            s0 -= wv * xa[cidx * 3 + 0];
                            s1 -= wv * xa[cidx * 3 + 1];
                            s2 -= wv * xa[cidx * 3 + 2];
                        } else if (cidx < 2 * B) {
                            s0 -= wv * xcn[(cidx - B) * 3 + 0];
                            s1 -= wv * xcn[(cidx - B) * 3 + 1];
                            s2 -= wv * xcn[(cidx - B) * 3 + 2];
                        } else {
                            const int q = cidx - 2 * B;
                            s0 += q == 0 ? wv : 0.0;
                            s1 += q == 1 ? wv : 0.0;
                            s2 += q == 2 ? wv : 0.0;
                        }
                    }
                }
                s0 = bcr_row16_sum(s0);
                s1 = bcr_row16_sum(s1);
                s2 = bcr_row16_sum(s2);
                if (lp == 0) {
                    sX[i + 1][k * 3 + 0] = s0;
                    sX[i + 1][k * 3 + 1] = s1;
                    sX[i + 1][k * 3 + 2] = s2;
                }
            }
        } else {
            static_assert(NR == 3 || NWB == 4, "the closures' right-hand sides ride on four-wave workgroups");
            int i = -1, a = -1, c = 7;
            if (rnd == 0) {
                i = 2 * wave;
                a = i - 1;
                c = i + 1;
            } else if (rnd == 1) {
                if (wave < 2) {
                    i = 1 + 4 * wave;
                    a = wave == 0 ? -1 : 3;
                    c = wave == 0 ? 3 : 7;
                }
            } else if (wave == 0) {
                i = 3;
            }
            if (i >= 0 && bcr_ridx(placed, kreal, i) >= 0) {
                const double *Wi = sW + i * WB;
                const double *xa = sX[a + 1], *xcn = sX[c + 1];
                // a lane per (row, right-hand side)
                for (int o = lane; o < B * NR; o += 64) {
                    const int k = o / NR, q = o - NR * k;
                    const double *wr = Wi + k * Dm::NC;
                    double sacc = wr[2 * B + q];
#pragma unroll 4
                    for (int cidx = 0; cidx < B; cidx++)
                        sacc -= wr[cidx] * xa[cidx * NR + q] + wr[B + cidx] * xcn[cidx * NR + q];
                    sX[i + 1][o] = sacc;
                }
            }
        }
        __syncthreads();
    }
}

// K6 inside the way back (run_irls on the plain direct path; BcrRequest::apply): the threads that write a view's solution
// row also make its step (step_apply) and sum ||x||; the workgroup's sum goes to slot `slot` of the partial array (a
// DOUBLE per workgroup, not a row of four: level 0 at 100k views has 512 workgroups and level 1 another 73, the pinned
// block 512 rows), summed by the host in slot order like k_apply_step's partials.
__device__ __forceinline__ void bcr_apply_sum(double acc, double *__restrict__ part, int slot) {
    __shared__ double sm[16];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += sm[w];   // fixed order
        part[slot] = t;
    }
}

// The way back for one chunk: x_7 and the separator before the chunk come from the coarser level. The chunk's
// W (7 blocks of B x (2B + 3)) is staged in LDS first -- every load of the launch is in flight at once; read row
// by row behind the three dependent rounds it cost a memory round trip per four rows.
template <int B, int NR, bool L0>
__global__ __launch_bounds__(256) void k_bcr_back(int nb, int nred, int n, const double *__restrict__ W,
                                                   const double *__restrict__ xc, double *__restrict__ xl,
                                                   double4 *__restrict__ X, double *__restrict__ Z, int zstride,
                                                   int zoff, int nfar, const double *__restrict__ xext, int place,
                                                   double4 *__restrict__ Qap = nullptr, int fap = 0,
                                                   double *__restrict__ part_ap = nullptr, int slot0 = 0) {
    typedef BcrDim<B, NR> Dm;
    constexpr int WB = B * Dm::NC;     // doubles of one W block
    __shared__ double sW[7 * WB];
    __shared__ double sX[9][B * NR];  // slot 0: separator before the chunk; slot j + 1: block j
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = blockIdx.x;
    const int kreal = nb - chunk * 8 < 8 ? nb - chunk * 8 : 8;
    const bool placed = place && kreal < 8;  // see kBcrPlace
    const int nblk = placed || kreal > 7 ? 7 : kreal;  // W blocks to stage (the separator, position 7, has none)
    // x of the two separators (from the coarser level) and W are requested together: one memory round trip, not two
    constexpr int NQ = (B * NR + 255) / 256;
    double x8[NQ], x0[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const int e = tid + 256 * q;
        x8[q] = 0.0;
        x0[q] = 0.0;
        if (e < B * NR) {
            x8[q] = xc[(size_t)chunk * B * NR + e];
            if (chunk > 0) x0[q] = xc[(size_t)(chunk - 1) * B * NR + e];
            else if (xext) x0[q] = xext[e];   // a shard: the separator of the rank before it (dist.hip)
        }
    }
    {
        // (every piece of W requested before the first one is put down: a loop of load -> LDS store pairs left it to the
        // compiler how many round trips that became)
        const v2d *__restrict__ src = reinterpret_cast<const v2d *>(W + (size_t)chunk * 7 * WB);
        v2d *dst = reinterpret_cast<v2d *>(sW);
        const int cnt = nblk * WB / 2;  // B is a multiple of 8: WB is even
        constexpr int NVW = (7 * WB / 2 + 255) / 256;
        v2d wreg[NVW];
#pragma unroll
        for (int v = 0; v < NVW; v++) {
            const int e = tid + 256 * v;
            wreg[v] = e < cnt ? __builtin_nontemporal_load(&src[e]) : v2d{0.0, 0.0};
        }
#pragma unroll
        for (int v = 0; v < NVW; v++) {
            const int e = tid + 256 * v;
            if (e < cnt) dst[e] = wreg[v];
        }
    }
    for (int e = tid; e < 7 * B * NR; e += 256) (&sX[1][0])[e] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const int e = tid + 256 * q;
        if (e < B * NR) {
            sX[8][e] = x8[q];
            sX[0][e] = x0[q];
        }
    }
    __syncthreads();
    bcr_back_rounds<B, NR>(sW, sX, placed, kreal, wave, lane);
    double acc_ap = 0.0;
    auto put_row = [&](int row, int t) {
        const double *xs = &sX[1][0] + t * NR;
        X[row] = double4{xs[0], xs[1], xs[2], 0.0};
        if (NR > 3)
            for (int q = 0; q < nfar; q++) Z[(size_t)row * zstride + zoff + q] = xs[3 + q];
        if (NR == 3 && Qap) acc_ap += step_apply(xs[0], xs[1], xs[2], Qap, row + fap, true);
    };
    if (L0) {
        const int row0 = chunk * 8 * B;
        for (int t = tid; t < kreal * B; t += 256) {
            const int row = row0 + t, blk = t / B;
            if (row < n) put_row(row, bcr_pos(placed, kreal, blk) * B + (t - blk * B));
        }
    } else {
        for (int e = tid; e < 8 * B * NR; e += 256) {
            const int blk = e / (B * NR);
            xl[(size_t)chunk * 8 * B * NR + e] =
                blk < kreal ? (&sX[1][0])[bcr_pos(placed, kreal, blk) * B * NR + (e - blk * B * NR)] : 0.0;
        }
        // blocks of a mixed level that are level-0 blocks themselves: their solution rows
        if (chunk * 8 + 8 > nred && nred < nb)
            for (int t = tid; t < 8 * B; t += 256) {
                const int i = t / B, r = t - i * B, gb = chunk * 8 + i;
                if (gb >= nred && gb < nb) {
                    const int row = (8 * nred + (gb - nred)) * B + r;
                    if (row < n) put_row(row, t);
                }
            }
    }
    if (NR == 3 && Qap) bcr_apply_sum(acc_ap, part_ap, slot0 + chunk);
}

// The ways back of ALL levels above level 0 in one launch (round 4; they were a launch per level, 11 - 16 us each for
// a handful of workgroups). A workgroup = a chunk of level `base`. What it needs from the level above are the solutions
// of two neighbouring blocks, i.e. the way back of the one or two chunks of that level that hold them, which in turn
// need at most two chunks of the level above them, ... up to the single chunk of the top level: at most two ways back
// per level, computed REDUNDANTLY by every workgroup that needs them -- no workgroup waits for another, nothing is
// exchanged through memory. The solutions of the (<= 16) blocks solved at a level stay in LDS for the level below.
struct BcrBackPlan {
    const double *W[kMaxLevels];
    int nb[kMaxLevels];
    int top, base;
};
// (eight waves: the rounds of a chunk are 24 / 12 / 6 units of four rows, and a workgroup has a CU to itself)
constexpr int kBackTopThreads = 512;
template <int B>
__global__ __launch_bounds__(kBackTopThreads) void k_bcr_back_top(BcrBackPlan P, const double *__restrict__ xtop, double *__restrict__ xl,
                                                       double4 *__restrict__ X, int n, int nred,
                                                       double4 *__restrict__ Qap = nullptr, int fap = 0,
                                                       double *__restrict__ part_ap = nullptr, int slot0 = 0,
                                                       int top_all = 0) {
    // top_all: xtop holds the solutions of ALL blocks of the level above P.top (the single-workgroup top, bcr_top_body,
    // made its own way back): chunk q of level P.top takes blocks q and q - 1 of it
    constexpr int NR = 3;
    typedef BcrDim<B, NR> Dm;
    constexpr int WB = B * Dm::NC, XB = B * NR;
    constexpr int NV = (7 * WB / 2 + kBackTopThreads - 1) / kBackTopThreads;   // 16-byte pieces of a chunk's W per thread
    __shared__ double sW[7 * WB];
    __shared__ double sX[9][XB];
    __shared__ double sWin[2][16][XB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cbase = blockIdx.x;
    // the chunks [lo, hi] of level L this workgroup solves (hi - lo <= 1)
    auto range = [&](int L, int &lo, int &hi) {
        lo = hi = cbase;
        for (int l = P.base; l < L; l++) {
            lo = (lo > 0 ? lo - 1 : 0) >> 3;
            hi >>= 3;
        }
    };
    // the positions of chunk q of level L whose solutions are wanted: all at the base level; above it the blocks the
    // chunks of the level below need (the separators of those chunks and the one before the first), plus what they
    // depend on inside the chunk
    auto wanted = [&](int L, int q) {
        if (L == P.base) return 0x7f;
        int lo, hi, m = 0;
        range(L - 1, lo, hi);
        for (int j = (lo > 0 ? lo - 1 : 0); j <= hi; j++)
            if ((j >> 3) == q && (j & 7) < 7) m |= 1 << (j & 7);
        return bcr_back_mask(m);
    };
    // W of the next chunk is requested while this one is solved: pieces of 16 bytes in registers
    v2d wreg[NV];
    auto request = [&](int L, int q) {
        const int kreal = P.nb[L] - q * 8 < 8 ? P.nb[L] - q * 8 : 8;
        const int nblk = kreal > 7 ? 7 : kreal;
        const int mask = wanted(L, q);
        const v2d *__restrict__ src = reinterpret_cast<const v2d *>(P.W[L] + (size_t)q * 7 * WB);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const int e = tid + kBackTopThreads * v, blk = e / (WB / 2);
            wreg[v] = (blk < nblk && ((mask >> blk) & 1)) ? __builtin_nontemporal_load(&src[e]) : v2d{0.0, 0.0};
        }
    };
    auto deposit = [&]() {
        v2d *dst = reinterpret_cast<v2d *>(sW);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const int e = tid + kBackTopThreads * v;
            if (e < 7 * WB / 2) dst[e] = wreg[v];
        }
    };
    double acc_ap = 0.0;
    int L = P.top, lo, hi;
    range(L, lo, hi);
    int q = lo;
    request(L, q);
    while (true) {
        int plo = 0, phi = 0;
        if (L < P.top) range(L + 1, plo, phi);
        const double(*winP)[XB] = sWin[(L + 1) & 1];
        double(*winC)[XB] = sWin[L & 1];
        const int kreal = P.nb[L] - q * 8 < 8 ? P.nb[L] - q * 8 : 8;
        const int mask = wanted(L, q);
        deposit();
        for (int e = tid; e < 7 * XB; e += kBackTopThreads) (&sX[1][0])[e] = 0.0;
        for (int e = tid; e < XB; e += kBackTopThreads) {
            sX[8][e] = L == P.top ? xtop[(top_all ? q * XB : 0) + e] : winP[q - 8 * plo][e];
            sX[0][e] = q == 0 ? 0.0 : L == P.top ? (top_all ? xtop[(q - 1) * XB + e] : 0.0) : winP[q - 1 - 8 * plo][e];
        }
        // the next chunk: the same level's second chunk, else the first of the level below
        int Ln = L, qn = q + 1;
        if (qn > hi) {
            Ln = L - 1;
            if (Ln >= P.base) {
                range(Ln, lo, hi);
                qn = lo;
            }
        }
        if (Ln >= P.base) request(Ln, qn);
        __syncthreads();
        bcr_back_rounds<B, NR, kBackTopThreads / 64>(sW, sX, false, kreal, wave, lane, mask);
        if (L > P.base) {
            int clo, chi;
            range(L, clo, chi);
            for (int e = tid; e < 8 * XB; e += kBackTopThreads) {
                const int blk = e / XB;
                winC[(q - clo) * 8 + blk][e - blk * XB] = blk < kreal ? (&sX[1][0])[e] : 0.0;
            }
        } else {
            for (int e = tid; e < 8 * XB; e += kBackTopThreads) {
                const int blk = e / XB;
                xl[(size_t)q * 8 * XB + e] = blk < kreal ? (&sX[1][0])[e] : 0.0;
            }
            // blocks of a mixed level that are level-0 blocks themselves: their solution rows
            if (q * 8 + 8 > nred && nred < P.nb[L])
                for (int t = tid; t < 8 * B; t += kBackTopThreads) {
                    const int i = t / B, r = t - i * B, gb = q * 8 + i;
                    if (gb >= nred && gb < P.nb[L]) {
                        const int row = (8 * nred + (gb - nred)) * B + r;
                        const double *xs = &sX[1][0] + t * NR;
                        if (row < n) {
                            X[row] = double4{xs[0], xs[1], xs[2], 0.0};
                            if (Qap) acc_ap += step_apply(xs[0], xs[1], xs[2], Qap, row + fap, true);
                        }
                    }
                }
        }
        if (Ln < P.base) break;
        __syncthreads();
        L = Ln;
        q = qn;
    }
    if (Qap) bcr_apply_sum(acc_ap, part_ap, slot0 + cbase);
}

// ---------------------------------------------------------------------------------------------
// The closures' part of a solve (round 4). The operator is A = A_b + V C V' (A_b: the band part the reduction
// factorised, column q of V = e_i - e_j for closure q, C = diag(w_q)), so with Y = A_b^-1 b
//     x = Y - A_b^-1 V lambda,    (C^-1 + V' A_b^-1 V) lambda = V' Y        (Sherman-Morrison-Woodbury).
// Round 3 got A_b^-1 V by riding sixteen incidence vectors at a time through a whole re-factorisation (0.3 ms per
// sixteen closures, at most 64). But a column of V has TWO non-zeros, and the block elimination is a nested dissection:
// the forward elimination of e_i only ever touches the blocks on the path from i's block up the elimination tree -- three
// eliminations per level and endpoint, plus what spills into the separator before the chunk. And nothing but the
// forward elimination is needed: with R_g(v) = the right-hand side of block g when it is eliminated,
//     u' A_b^-1 v = sum over the eliminated blocks g of R_g(u)' D_g^-1 R_g(v),
// so S = C^-1 + V' A_b^-1 V and T = V' Y are sums over the blocks two closures' paths share (Y's forward elimination
// is what the reduction stored as W_R), and x = A_b^-1 (b - V lambda) is the ordinary way back from right-hand
// sides corrected by sum_q lambda_q D_g^-1 R_g(v_q) on the blocks of the paths. Which blocks a closure touches
// depends on the positions of its endpoints only: the host writes a STEP PROGRAM per closure once (bcr_closure_plan),
// a wave executes it per solve (k_bcr_closure_forward), pairs of closures are joined on the blocks they share
// (k_bcr_closure_S), the Woodbury system is solved in LDS (<= 96 closures) or by the blocked Gauss-Jordan sweep of
// dense.hip, and one launch corrects the stored right-hand sides (k_bcr_closure_correct) before the ways back.
// No second pass over the matrix, no n x r array: 2048 closures instead of 64.
// ---------------------------------------------------------------------------------------------
struct BcrClPlan {
    const double *W[kMaxLevels], *Dinv[kMaxLevels];
    double *Wrw[kMaxLevels];  // the same W, writable (k_bcr_closure_correct)
    const double *topDinv;
    double *xtop;
};

// One WORKGROUP per closure: its step program. A step eliminates one block g of the path: R = slot[src];
// slot[dstA] -= W_P' R, slot[dstC] -= W_Q' R (the block's W = D^-1 [P' | Q | R_main]), T += R' W_R(main),
// and R and D^-1 R are recorded. The chain of steps is sequential in R (LDS) only: a step's block columns
// ([W_P | W_Q | W_R | D^-1]: 14 KB at B = 24) do not depend on the step before. Round 4 ran a wave per closure that
// fetched its block at every step -- ~40 memory round trips in sequence, 61 us whatever the number of closures; round
// 5: the four waves of the workgroup stage the blocks of FOUR steps in LDS per round trip (each wave one step) and then
// run the four steps from LDS together -- thread (column, part) sums a part of its column's rows, the parts meet in LDS
// (one wave doing a step alone is two chains of B dependent multiply-adds: ~1 us, as long as the round trip it replaced).
template <int B, int NWF = 4>
__global__ __launch_bounds__(64 * NWF) void k_bcr_closure_forward(BcrClPlan P, int r, int nslots, const int *__restrict__ off,
                                                              const int4 *__restrict__ steps,
                                                              const int4 *__restrict__ init, double *__restrict__ recR,
                                                              double *__restrict__ recW, double *__restrict__ T,
                                                              const double *__restrict__ slot_init = nullptr,
                                                              const int2 *__restrict__ fin = nullptr,
                                                              const int *__restrict__ gid = nullptr,
                                                              double *__restrict__ dep = nullptr, int world = 0,
                                                              int rank = 0) {
    constexpr int NR = 3, NC = 2 * B + NR, BB = B * B, NCOL = NC + B, NE = B * NCOL;
    constexpr int NLD = (NE + 63) / 64;
    constexpr int KP = B == 24 ? 3 : (NCOL * 4 <= 256 ? 4 : 2), KB = B / KP;  // parts of a column's rows, rows per part
    static_assert(B % KP == 0 && NCOL * KP <= 256, "thread (col, part)");
    // NWF waves = NWF steps staged per memory round trip (four; eight measured slower, see bcr_launch_forward)
    extern __shared__ double smem[];  // [NWF][B][NCOL] staged blocks, KP x NCOL partial sums, then nslots x B slots
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.x;
    double *stage = smem + (size_t)wave * NE;
    double *spart = smem + (size_t)NWF * NE;
    double *slots = spart + KP * NCOL;
    if (wave == 0) {
        if (slot_init) {
            // the separator system of a sharded sequence: the column starts from what the ranks' eliminations left there
            for (int e = lane; e < nslots * B; e += 64) slots[e] = slot_init[(size_t)q * nslots * B + e];
        } else {
            for (int e = lane; e < nslots * B; e += 64) slots[e] = 0.0;
            const int4 in = init[q];
            if (lane == 0) {  // (a slot of 255: that endpoint is a row of another rank)
                if (in.x != 255) slots[in.x * B + in.y] += 1.0;
                if (in.z != 255) slots[in.z * B + in.w] -= 1.0;
            }
        }
    }
    double tacc = 0.0;  // threads 2B .. 2B + 2: a coordinate of T each
    const int s0 = off[q], s1 = off[q + 1];
    __syncthreads();  // (the slots' start values)
    for (int g0 = s0; g0 < s1; g0 += NWF) {
        // ---- every wave: the block of step g0 + wave into its stage, element (k, col) at k NCOL + col ----
        const int st_w = g0 + wave;
        if (st_w < s1) {
            const int4 sp = steps[st_w];
            const int lvl = __builtin_amdgcn_readfirstlane(sp.x), spy = __builtin_amdgcn_readfirstlane(sp.y);
            const double *Wb = lvl >= 0 ? P.W[lvl] + (size_t)spy * B * NC : P.topDinv;
            const double *Db = lvl >= 0 ? P.Dinv[lvl] + (size_t)spy * BB : P.topDinv;
            double v[NLD];
#pragma unroll
            for (int u = 0; u < NLD; u++) {
                const int e = lane + 64 * u;
                const int k = e / NCOL, col = e - k * NCOL;
                // (an address that is valid for every lane; what is not wanted is zeroed by a select below)
                const double *src = Db;
                if (e < NE) {
                    if (col >= NC)
                        src = Db + k * B + (col - NC);
                    else if (lvl >= 0)
                        src = Wb + k * NC + col;
                    else if (col >= 2 * B)
                        src = P.xtop + k * NR + (col - 2 * B);  // the top block: nothing beside it; its part of Y is xtop
                }
                v[u] = *src;
            }
#pragma unroll
            for (int u = 0; u < NLD; u++) {
                const int e = lane + 64 * u;
                const int k = e / NCOL, col = e - k * NCOL;
                const bool zero = lvl < 0 && col < 2 * B;
                if (e < NE) stage[e] = zero ? 0.0 : v[u];
            }
        }
        __syncthreads();
        // ---- all four waves: the (up to) four steps from LDS. Thread (col, part) sums its share of the rows of column
        // col (a wave alone took ~1 us per step: two chains of B dependent multiply-adds), the parts meet in LDS ----
        for (int w = 0; w < NWF && g0 + w < s1; w++) {
            const int st = g0 + w;
            const int spz = __builtin_amdgcn_readfirstlane(steps[st].z);
            const int src = spz & 255, dA = (spz >> 8) & 255, dC = (spz >> 16) & 255;
            const double *blk = smem + (size_t)w * NE;
            const int tcol = threadIdx.x % NCOL, tpart = threadIdx.x / NCOL;
            if (tpart < KP) {
                const double *rs = slots + src * B + tpart * KB;
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < KB; k++) acc = fma(blk[(tpart * KB + k) * NCOL + tcol], rs[k], acc);
                spart[tpart * NCOL + tcol] = acc;
            }
            if (threadIdx.x < B) recR[(size_t)st * B + threadIdx.x] = slots[src * B + threadIdx.x];
            __syncthreads();
            if (threadIdx.x < NCOL) {
                const int col = threadIdx.x;
                double acc = spart[col];
#pragma unroll
                for (int pp = 1; pp < KP; pp++) acc += spart[pp * NCOL + col];
                if (col < B) {
                    if (dA != 255) slots[dA * B + col] -= acc;
                } else if (col < 2 * B) {
                    if (dC != 255) slots[dC * B + col - B] -= acc;
                } else if (col < NC) {
                    tacc += acc;
                } else {
                    recW[(size_t)st * B + col - NC] = acc;
                }
            }
            __syncthreads();  // (slots and spart before the next step; the stages before the next group)
        }
    }
    // the T threads: column 2B + c is thread 2B + c in every step
    if (threadIdx.x >= 2 * B && threadIdx.x < 2 * B + 3) T[(size_t)q * 3 + (threadIdx.x - 2 * B)] = tacc;
    if (wave != 0) return;
    // a shard: what the column leaves on this rank's separator (block `rank` of the separator system) and on the one
    // before it (block rank - 1) is ADDED to the ranks' common buffer (the loopback's shards run one after the other)
    if (dep) {
        const int2 fn = fin[q];
        double *d = dep + (size_t)gid[q] * world * B;
        if (lane < B) {
            if (fn.x != 255) d[rank * B + lane] += slots[fn.x * B + lane];
            if (fn.y != 255 && rank > 0) d[(rank - 1) * B + lane] += slots[fn.y * B + lane];
        }
    }
}

// The same step programs, one WAVE per closure and the block fetched at every step (round 4's kernel): small in LDS, so
// that a thousand closures run side by side -- the form for many closures, where the machine is filled by their number.
// One wave per closure: its step program. A step eliminates one block g of the path: R = slot[src];
// slot[dstA] -= W_P' R, slot[dstC] -= W_Q' R (the block's W = D^-1 [P' | Q | R_main]), T += R' W_R(main),
// and R and D^-1 R are recorded. Every lane owns one column of [W_P | W_Q | W_R | D^-1] per pass.
template <int B>
__global__ __launch_bounds__(256) void k_bcr_closure_forward_wave(BcrClPlan P, int r, int nslots, const int *__restrict__ off,
                                                              const int4 *__restrict__ steps,
                                                              const int4 *__restrict__ init, double *__restrict__ recR,
                                                              double *__restrict__ recW, double *__restrict__ T,
                                                              const double *__restrict__ slot_init = nullptr,
                                                              const int2 *__restrict__ fin = nullptr,
                                                              const int *__restrict__ gid = nullptr,
                                                              double *__restrict__ dep = nullptr, int world = 0,
                                                              int rank = 0) {
    constexpr int NR = 3, NC = 2 * B + NR, BB = B * B, NCOL = NC + B;
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * (blockDim.x >> 6) + wave;
    if (q >= r) return;  // (no workgroup barrier below)
    double *slots = smem + (size_t)wave * nslots * B;
    if (slot_init) {
        // the separator system of a sharded sequence: the column starts from what the ranks' eliminations left there
        for (int e = lane; e < nslots * B; e += 64) slots[e] = slot_init[(size_t)q * nslots * B + e];
    } else {
        for (int e = lane; e < nslots * B; e += 64) slots[e] = 0.0;
        const int4 in = init[q];
        if (lane == 0) {  // (a slot of 255: that endpoint is a row of another rank)
            if (in.x != 255) slots[in.x * B + in.y] += 1.0;
            if (in.z != 255) slots[in.z * B + in.w] -= 1.0;
        }
    }
    double tacc = 0.0;  // lanes 2B .. 2B + 2 of the first pass: a coordinate of T each
    for (int st = off[q]; st < off[q + 1]; st++) {
        const int4 sp = steps[st];
        const int lvl = sp.x, src = sp.z & 255, dA = (sp.z >> 8) & 255, dC = (sp.z >> 16) & 255;
        const double *Wb = lvl >= 0 ? P.W[lvl] + (size_t)sp.y * B * NC : nullptr;
        const double *Db = lvl >= 0 ? P.Dinv[lvl] + (size_t)sp.y * BB : P.topDinv;
        double R[B];
        {
            const v2d *rs = reinterpret_cast<const v2d *>(slots + src * B);
#pragma unroll
            for (int k = 0; k < B / 2; k++) {
                const v2d v = rs[k];
                R[2 * k] = v.x;
                R[2 * k + 1] = v.y;
            }
        }
        if (lane < B) recR[(size_t)st * B + lane] = slots[src * B + lane];
        // the columns of both passes are requested before the first is used: one memory round trip per step
        constexpr int NPASS = (NCOL + 63) / 64;
        double m[NPASS][B];
        bool have[NPASS];
#pragma unroll
        for (int pass = 0; pass < NPASS; pass++) {
            const int col = pass * 64 + lane;
            const double *base = Db;
            int stride = B;
            have[pass] = col < NCOL;
            if (col < NC) {
                if (lvl >= 0) {
                    base = Wb + col;
                    stride = NC;
                } else {  // the top block: nothing beside it; its part of Y is xtop
                    base = P.xtop + (col - 2 * B);
                    stride = NR;
                    have[pass] = col >= 2 * B;
                }
            } else {
                base = Db + (col - NC);
            }
#pragma unroll
            for (int k = 0; k < B; k++) m[pass][k] = have[pass] ? base[(size_t)k * stride] : 0.0;
        }
#pragma unroll
        for (int pass = 0; pass < NPASS; pass++) {
            const int col = pass * 64 + lane;
            if (col >= NCOL) continue;
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < B; k++) acc = fma(m[pass][k], R[k], acc);
            if (col < B) {
                if (dA != 255) slots[dA * B + col] -= acc;
            } else if (col < 2 * B) {
                if (dC != 255) slots[dC * B + col - B] -= acc;
            } else if (col < NC) {
                tacc += acc;
            } else {
                recW[(size_t)st * B + col - NC] = acc;
            }
        }
    }
    // the T lanes: column 2B + c sits in pass (2B + c) / 64, lane (2B + c) % 64 -- the same lane in every step
    {
        const int c0 = 2 * B;
        for (int c = 0; c < 3; c++)
            if (((c0 + c) & 63) == lane) T[(size_t)q * 3 + c] = tacc;
    }
    // a shard: what the column leaves on this rank's separator (block `rank` of the separator system) and on the one
    // before it (block rank - 1) is ADDED to the ranks' common buffer (the loopback's shards run one after the other)
    if (dep) {
        const int2 fn = fin[q];
        double *d = dep + (size_t)gid[q] * world * B;
        if (lane < B) {
            if (fn.x != 255) d[rank * B + lane] += slots[fn.x * B + lane];
            if (fn.y != 255 && rank > 0) d[(rank - 1) * B + lane] += slots[fn.y * B + lane];
        }
    }
}

// S = C^-1 + V' A_b^-1 V: entry (p, q) = sum over the steps of p and q on the same block of R_p . (D^-1 R_q); the
// step lists are sorted by block. A workgroup per 16 x 16 tile of the upper triangle, the keys of its 32 closures in
// LDS (a merge that fetched every key from memory was a dependent load per step: 270 us at a thousand closures); a
// closure of weight 0 (Talwar) is not there: its row and column are the identity's, its T is 0.
template <int B>
__global__ __launch_bounds__(256) void k_bcr_closure_S(int r, int npad, int maxsteps, int ndense,
                                                        const int *__restrict__ dense, const int *__restrict__ off,
                                                        const int4 *__restrict__ steps, const double *__restrict__ recR,
                                                        const double *__restrict__ recW, const int *__restrict__ far_e,
                                                        const double *__restrict__ wsrc, int wsquare,
                                                        double *__restrict__ S, double *__restrict__ T,
                                                        int *__restrict__ alive, const int *__restrict__ gid = nullptr,
                                                        const uint8_t *__restrict__ own = nullptr, int npadG = 0,
                                                        double *__restrict__ Tx = nullptr,
                                                        double *__restrict__ deadx = nullptr) {
    extern __shared__ int skey[];  // [32][maxsteps]: rows 0..15 the tile's p, 16..31 its q
    constexpr int DB = 4;          // dense eliminations per batch
    __shared__ double sx[DB][16][B + 1], sy[DB][16][B + 1];
    if (blockIdx.x < blockIdx.y) return;
    const int tp = threadIdx.x >> 4, tq = threadIdx.x & 15;
    const int p = blockIdx.y * 16 + tp, q = blockIdx.x * 16 + tq;
    for (int e = threadIdx.x; e < 32 * maxsteps; e += 256) {
        const int who = e / maxsteps, k = e - who * maxsteps;
        const int cl = who < 16 ? blockIdx.y * 16 + who : blockIdx.x * 16 + who - 16;
        int key = 0x7fffffff;
        if (cl < r && k < off[cl + 1] - off[cl]) key = steps[off[cl] + k].w;
        skey[e] = key;
    }
    __syncthreads();
    // the dense eliminations (the blocks of the top levels, on almost every closure's path): the records of the tile's
    // sixteen p and sixteen q through LDS -- each is used sixteen times. DB eliminations per batch: their records are
    // requested together (one elimination per round was one memory round trip per elimination: 36 of this kernel's
    // 51 us at a hundred closures).
    double sum = 0.0;
    {
        constexpr int NE = 32 * (B / 2), NU = (DB * NE + 255) / 256;  // pairs of doubles per elimination; per thread and batch
        for (int d0 = 0; d0 < ndense; d0 += DB) {
            v2d v[NU];
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const int e = threadIdx.x + 256 * u;
                const int dd = e / NE, e1 = e - dd * NE;
                const int who = e1 / (B / 2), k2 = e1 - who * (B / 2);
                const int cl = who < 16 ? blockIdx.y * 16 + who : blockIdx.x * 16 + who - 16;
                int st = -1;
                if (dd < DB && d0 + dd < ndense && cl < r) st = dense[(size_t)(d0 + dd) * r + cl];
                v[u] = v2d{0.0, 0.0};
                if (st >= 0) v[u] = *reinterpret_cast<const v2d *>((who < 16 ? recR : recW) + (size_t)st * B + 2 * k2);
            }
            __syncthreads();  // (the previous batch has been read)
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const int e = threadIdx.x + 256 * u;
                const int dd = e / NE, e1 = e - dd * NE;
                const int who = e1 / (B / 2), k2 = e1 - who * (B / 2);
                if (dd < DB) {
                    double *dst = who < 16 ? &sx[dd][who][2 * k2] : &sy[dd][who - 16][2 * k2];
                    dst[0] = v[u].x;
                    dst[1] = v[u].y;
                }
            }
            __syncthreads();
#pragma unroll
            for (int dd = 0; dd < DB; dd++) {
                if (d0 + dd >= ndense) break;
                const double *x = sx[dd][tp], *y = sy[dd][tq];
                double d0s = 0.0, d1s = 0.0;
#pragma unroll
                for (int k = 0; k < B; k += 2) {
                    d0s = fma(x[k], y[k], d0s);
                    d1s = fma(x[k + 1], y[k + 1], d1s);
                }
                sum += d0s + d1s;
            }
        }
    }
    if (p >= npad || q >= npad || q < p) return;
    if (p >= r || q >= r) {  // padding of the inversion
        if (!gid) S[(size_t)p * npad + q] = S[(size_t)q * npad + p] = p == q ? 1.0 : 0.0;
        return;
    }
    double wp = wsrc[far_e[p]], wq = wsrc[far_e[q]];
    if (wsquare) {
        wp *= wp;
        wq *= wq;
    }
    if (wp > 0.0 && wq > 0.0) {
        const int *ka = skey + tp * maxsteps, *kb = skey + (16 + tq) * maxsteps;
        const int na = off[p + 1] - off[p], nb = off[q + 1] - off[q];
        const double *x0 = recR + (size_t)off[p] * B, *y0 = recW + (size_t)off[q] * B;
        int a = 0, b = 0;
        while (a < na && b < nb) {
            const int va = ka[a], vb = kb[b];
            if (va == vb) {
                if (!(va & 1)) {  // (a dense elimination: summed above)
                    const double *x = x0 + (size_t)a * B, *y = y0 + (size_t)b * B;
                    double d0 = 0.0, d1 = 0.0;
#pragma unroll
                    for (int k = 0; k < B; k += 2) {
                        d0 = fma(x[k], y[k], d0);
                        d1 = fma(x[k + 1], y[k + 1], d1);
                    }
                    sum += d0 + d1;
                }
                a++;
                b++;
            } else if (va < vb) {
                a++;
            } else {
                b++;
            }
        }
        if (p == q && (!gid || own[p])) sum += 1.0 / wp;
    } else {
        sum = p == q ? 1.0 : 0.0;
    }
    if (gid) {
        // a shard: this rank's share of the system is ADDED at the closures' places in the global list (dist.hip sums
        // the ranks' buffers); a closure of weight 0 is flagged by its owner and settled after the sum
        const int gp = gid[p], gq = gid[q];
        const bool live = wp > 0.0 && wq > 0.0;
        if (live) {
            S[(size_t)gp * npadG + gq] += sum;
            if (p != q) S[(size_t)gq * npadG + gp] += sum;
        }
        if (p == q) {
            if (live) {
                for (int c = 0; c < 3; c++) Tx[3 * gp + c] += T[3 * p + c];
            } else if (own[p]) {
                deadx[gp] += 1.0;
            }
        }
        return;
    }
    S[(size_t)p * npad + q] = sum;
    S[(size_t)q * npad + p] = sum;
    if (p == q) {
        alive[p] = wp > 0.0;
        if (!(wp > 0.0)) T[3 * p] = T[3 * p + 1] = T[3 * p + 2] = 0.0;
    }
}

// The same sums for FEW closures (round 6), a WAVE per pair (p, q), p <= q. With a tile of 16 x 16 pairs per workgroup
// thirty closures are three workgroups -- three CUs of 256 -- and every thread walks its pair's merge alone, 24 doubles of
// two records per shared block out of global memory: 34 us of an IRLS iteration that has thirty closures, most of it
// latency. Here the wave looks every key of p's list up in q's list (a binary search in LDS, 64 keys at a time), lists
// the matches, and eight groups of eight lanes take a match each per round -- lane e of a group the elements e, e + 8, ...
// of the two records -- so that eight matches' loads are in flight together; one sum over the wave at the end. All
// eliminations alike: the dense ones (the top levels' blocks, an odd key) need no table here. Same entries as
// k_bcr_closure_S up to the order of the additions; single GPU only (a shard adds into the ranks' common buffer).
constexpr int kClosurePairsMax = 192;  // closures up to which the pair kernel is used (above: the tiles' shared keys pay)
template <int B>
__global__ __launch_bounds__(256) void k_bcr_closure_S_pairs(int r, int npad, int maxsteps, const int *__restrict__ off,
                                                              const int4 *__restrict__ steps, const double *__restrict__ recR,
                                                              const double *__restrict__ recW, const int *__restrict__ far_e,
                                                              const double *__restrict__ wsrc, int wsquare,
                                                              double *__restrict__ S, double *__restrict__ T,
                                                              int *__restrict__ alive) {
    extern __shared__ int spairs[];  // per wave: maxsteps keys of q, then 64 matches (a | b << 16)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = blockIdx.y, q = blockIdx.x * 4 + wave;
    if (q < p || q >= npad || p >= npad) return;   // (whole waves leave: no barrier below)
    if (p >= r || q >= r) {  // padding of the inversion
        if (lane == 0) S[(size_t)p * npad + q] = S[(size_t)q * npad + p] = p == q ? 1.0 : 0.0;
        return;
    }
    double wp = wsrc[far_e[p]], wq = wsrc[far_e[q]];
    if (wsquare) {
        wp *= wp;
        wq *= wq;
    }
    double sum = 0.0;
    if (wp > 0.0 && wq > 0.0) {
        int *kb = spairs + (size_t)wave * (maxsteps + 64);
        int *ml = kb + maxsteps;
        const int na = off[p + 1] - off[p], nb = off[q + 1] - off[q];
        for (int k = lane; k < nb; k += 64) kb[k] = steps[off[q] + k].w;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const double *x0 = recR + (size_t)off[p] * B, *y0 = recW + (size_t)off[q] * B;
        const int grp = lane >> 3, e = lane & 7;
        double acc = 0.0;
        for (int a0 = 0; a0 < na; a0 += 64) {
            const int a = a0 + lane;
            int found = -1;
            if (a < na) {
                const int ka = steps[off[p] + a].w;
                int lo = 0, hi = nb;  // first index whose key is >= ka
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (kb[mid] < ka) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < nb && kb[lo] == ka) found = lo;
            }
            const unsigned long long mask = __ballot(found >= 0);
            const int nm = __popcll(mask);
            if (found >= 0) ml[__popcll(mask & ((1ull << lane) - 1ull))] = a | (found << 16);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int i = grp; i < nm; i += 8) {
                const int ab = ml[i];
                const double *x = x0 + (size_t)(ab & 0xffff) * B, *y = y0 + (size_t)(ab >> 16) * B;
#pragma unroll
                for (int k = 0; k < (B + 7) / 8; k++)
                    if (e + 8 * k < B) acc = fma(x[e + 8 * k], y[e + 8 * k], acc);
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        sum = acc;
        if (p == q) sum += 1.0 / wp;
    } else {
        sum = p == q ? 1.0 : 0.0;
    }
    if (lane != 0) return;
    S[(size_t)p * npad + q] = sum;
    S[(size_t)q * npad + p] = sum;
    if (p == q) {
        alive[p] = wp > 0.0;
        if (!(wp > 0.0)) T[3 * p] = T[3 * p + 1] = T[3 * p + 2] = 0.0;
    }
}

// lambda = S^-1 T for at most 96 closures: one workgroup, [S | T] in LDS, Gauss-Jordan without pivoting (SPD). Thread
// (row p, class c) updates the columns q = c, c + 4, ... BEHIND the pivot of its row: the row's factor is formed once,
// nobody writes the pivot's row or column during its step, so ONE barrier per pivot. (Round 4's form -- an element per
// thread found by an integer division, three barriers per pivot, every column -- took 225 us at sixty closures, a third
// of such an IRLS iteration and more than the blocked sweep of dense.hip needs for a hundred: round 5, ~25 us; the time
// grows with r^2 and meets the blocked sweep's 92 us at about a hundred closures.)
constexpr int kSolveLdsMax = 96;  // (measured at 100k views: the blocked sweep of dense.hip takes over at ~ 100 closures: 92 us there)
__global__ __launch_bounds__(512) void k_bcr_closure_solve_lds(int r, int npad, const double *__restrict__ Sg,
                                                                const double *__restrict__ Tg, double *__restrict__ lam) {
    extern __shared__ double A[];  // r x ld
    const int nc = r + 3, ld = nc | 1;
    const int tid = threadIdx.x, p = tid >> 2, c = tid & 3;
    for (int e = tid; e < r * nc; e += blockDim.x) {
        const int pp = e / nc, q = e - pp * nc;
        A[pp * ld + q] = q < r ? Sg[(size_t)pp * npad + q] : Tg[3 * pp + (q - r)];
    }
    __syncthreads();
    for (int k = 0; k < r; k++) {
        if (p < r && p != k) {
            const double f = A[p * ld + k] / A[k * ld + k];
            const double *rk = A + k * ld;
            double *rp = A + p * ld;
            for (int q = k + 1 + ((c - (k + 1)) & 3); q < nc; q += 4) rp[q] = fma(-f, rk[q], rp[q]);
        }
        __syncthreads();
    }
    if (p < r && c < 3) lam[3 * p + c] = A[p * ld + r + c] / A[p * ld + p];
}
static void bcr_launch_solve_lds(hipStream_t st, int r, int npad, const double *S, const double *T, double *lam) {
    const size_t lds = (size_t)r * ((r + 3) | 1) * sizeof(double);
    static std::atomic<size_t> lds_set[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds > 64 * 1024 && lds_set[dev & 15].load() < lds) {
        IRH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bcr_closure_solve_lds),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set[dev & 15].store(lds);
    }
    hipLaunchKernelGGL(k_bcr_closure_solve_lds, dim3(1), dim3(r <= 64 ? 256 : 512), lds, st, r, npad, S, T, lam);
}

// lambda = Sinv T (more than 96 closures: Sinv from the blocked Gauss-Jordan sweep); a wave per row
__global__ __launch_bounds__(256) void k_bcr_closure_lambda(int r, int npad, const double *__restrict__ Sinv,
                                                             const double *__restrict__ T, double *__restrict__ lam) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= r) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = lane; q < r; q += 64) {
        const double v = Sinv[(size_t)p * npad + q];
        s0 = fma(v, T[3 * q], s0);
        s1 = fma(v, T[3 * q + 1], s1);
        s2 = fma(v, T[3 * q + 2], s2);
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        lam[3 * p] = s0;
        lam[3 * p + 1] = s1;
        lam[3 * p + 2] = s2;
    }
}

// W_R of every block a closure touches -= sum over the steps on it of (D^-1 R_q) lambda_q' (the top block: xtop):
// a workgroup per block. The top blocks lie on every closure's path (a thousand steps each): the list is dealt to
// PARTS groups of threads whose partial sums are added in a fixed order.
template <int B>
__global__ __launch_bounds__(1024) void k_bcr_closure_correct(BcrClPlan P, const int *__restrict__ eoff,
                                                               const int *__restrict__ erec, const int2 *__restrict__ elim,
                                                               const int *__restrict__ owner,
                                                               const double *__restrict__ recW,
                                                               const double *__restrict__ lam) {
    constexpr int NR = 3, NC = 2 * B + NR, NO = B * 3, PARTS = 1024 / NO;
    __shared__ double part[PARTS][NO];
    const int g = blockIdx.x, t = threadIdx.x;
    const int pt = t / NO, o = t - pt * NO;
    const int row = o / 3, c = o - 3 * row;
    const int k0 = eoff[g], k1 = eoff[g + 1];
    if (pt < PARTS) {
        double acc = 0.0;
        if (k1 - k0 > pt) {
#pragma unroll 4
            for (int k = k0 + pt; k < k1; k += PARTS) {
                const int st = erec[k];
                acc = fma(recW[(size_t)st * B + row], lam[3 * owner[st] + c], acc);
            }
        }
        part[pt][o] = acc;
    }
    __syncthreads();
    if (t >= NO) return;
    double acc = 0.0;
    const int np = k1 - k0 < PARTS ? k1 - k0 : PARTS;
    for (int q = 0; q < np; q++) acc += part[q][o];
    const int2 el = elim[g];
    if (el.x >= 0)
        P.Wrw[el.x][(size_t)el.y * B * NC + (size_t)row * NC + 2 * B + c] -= acc;
    else
        P.xtop[row * NR + c] -= acc;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The step programs of the closures (see "The closures' part of a solve"): a symbolic forward elimination of
// e_i - e_j per closure. Blocks are tracked as (level, block of that level) -> slot; a chunk's eliminations run in the
// kernel's order (0 2 4 6)(1 5)(3); what an elimination subtracts from the separator before its chunk is kept in the
// slot of that separator's block of the NEXT level (the reduction adds sepR[j] + extR[j + 1] there as well).
// Where the real block t of a chunk with kreal blocks sits (host mirror of bcr_pos / kBcrPlace)
static const signed char kBcrPlaceHost[9][8] = {{-1, -1, -1, -1, -1, -1, -1, -1}, {7, -1, -1, -1, -1, -1, -1, -1},
                                                {3, 7, -1, -1, -1, -1, -1, -1},   {3, 5, 7, -1, -1, -1, -1, -1},
                                                {1, 3, 5, 7, -1, -1, -1, -1},     {1, 3, 5, 6, 7, -1, -1, -1},
                                                {1, 3, 4, 5, 6, 7, -1, -1},       {1, 2, 3, 4, 5, 6, 7, -1},
                                                {0, 1, 2, 3, 4, 5, 6, 7}};
// A SHARD's plan (round 5): the partial chunks are placed (the last block sits at position 7 and survives as the
// separator at every level), chunk 0 of every level subtracts from the separator of the rank before this one (one slot
// per closure that lives through all levels), the last level is not solved -- what is left at its position 7 and in that
// slot goes to the separator system (cl_fin), and an endpoint may be a row of another rank (row -1: no start value here).
static void bcr_closure_plan(Graph &g) {
    BcrState &S = *g.bcr;
    const int B = S.B, nl = (int)S.lev.size(), r = S.nfar;
    const int nch0 = S.lev[0].nch;
    const bool shard = g.bcr_shard;
    std::vector<int> off(1, 0), owner;
    std::vector<int4> steps, init((size_t)r);
    std::vector<int2> fin((size_t)r);
    std::vector<long long> koff((size_t)nl + 1, 0);  // sort keys: (level, chunk, rank in the schedule)
    for (int l = 0; l < nl; l++) koff[(size_t)l + 1] = koff[(size_t)l] + (long long)S.lev[l].nch * 8;
    static const int rank_of[7] = {0, 4, 1, 6, 2, 5, 3}, sched[7] = {0, 2, 4, 6, 1, 5, 3};
    int nslots = 2;
    for (int q = 0; q < r; q++) {
        std::vector<std::map<int, int>> nz((size_t)nl + 1);  // per level: block -> slot
        std::vector<int> freelist;
        int next = 0;
        auto take = [&]() {
            if (!freelist.empty()) {
                const int t = freelist.back();
                freelist.pop_back();
                return t;
            }
            return next++;
        };
        auto slot_of = [&](int l, int blk) {
            auto it = nz[(size_t)l].find(blk);
            if (it != nz[(size_t)l].end()) return it->second;
            const int t = take();
            nz[(size_t)l][blk] = t;
            return t;
        };
        int4 in;
        in.x = in.z = 255;
        in.y = in.w = 0;
        for (int e = 0; e < 2; e++) {
            const int row = e ? g.bcr_far_j[(size_t)q] : g.bcr_far_i[(size_t)q];
            if (row < 0) continue;  // (a row of another rank)
            const int b = row / B;
            int l = 0, blk = b;
            if (nl > 1 && b >= 8 * nch0) {  // a block no chunk of level 0 reduces: a block of the mixed level 1
                l = 1;
                blk = S.lev[1].nred + (b - 8 * nch0);
            }
            const int t = slot_of(l, blk);
            if (e == 0) {
                in.x = t;
                in.y = row - b * B;
            } else {
                in.z = t;
                in.w = row - b * B;
            }
        }
        init[(size_t)q] = in;
        int remote = -1, own = -1;  // a shard: the slots of the two separators this rank's eliminations add to
        for (int l = 0; l < nl; l++) {
            const bool top = l == nl - 1 && !shard;
            // chunks with non-zero blocks, ascending (std::map is ordered)
            while (!nz[(size_t)l].empty()) {
                const int chunk = nz[(size_t)l].begin()->first / 8;
                const int kreal = std::min(8, S.lev[l].nb - chunk * 8);
                const bool placed = shard && kreal < 8;
                auto pos_of = [&](int t) { return placed ? (int)kBcrPlaceHost[kreal][t] : t; };
                bool real[8];
                for (int i = 0; i < 8; i++) real[i] = false;
                for (int t = 0; t < kreal; t++) real[pos_of(t)] = true;
                int slot[9];  // positions 0..7, [8] = the separator before the chunk
                for (int i = 0; i < 9; i++) slot[i] = -1;
                for (int t = 0; t < kreal; t++) {
                    auto it = nz[(size_t)l].find(chunk * 8 + t);
                    if (it != nz[(size_t)l].end()) {
                        slot[pos_of(t)] = it->second;
                        nz[(size_t)l].erase(it);
                    }
                }
                const bool ext_remote = shard && chunk == 0 && S.ext0;
                const bool has_ext = chunk > 0 || ext_remote;
                for (int k = 0; k < 7; k++) {
                    const int i = sched[k];
                    if (!real[i] || slot[i] < 0) continue;
                    int a, c;
                    if (k < 4) {
                        a = i - 1;
                        c = i + 1;
                    } else if (k < 6) {
                        a = i == 1 ? -1 : 3;
                        c = i == 1 ? 3 : 7;
                    } else {
                        a = -1;
                        c = 7;
                    }
                    int dA = 255, dC = 255;
                    if (a >= 0) {
                        // (a placed chunk: every padding position has been skipped before it would be a neighbour)
                        if (!real[a]) throw HipError{hipErrorUnknown};
                        if (slot[a] < 0) slot[a] = take();
                        dA = slot[a];
                    } else if (has_ext) {
                        if (slot[8] < 0) {
                            if (ext_remote) {
                                if (remote < 0) remote = take();
                                slot[8] = remote;
                            } else {
                                // the separator before the chunk = block chunk - 1 of the next level (it may hold a value)
                                slot[8] = slot_of(l + 1, chunk - 1);
                            }
                        }
                        dA = slot[8];
                    }
                    if (real[c]) {
                        if (slot[c] < 0) slot[c] = take();
                        dC = slot[c];
                    }
                    int4 sp;
                    sp.x = l;
                    sp.y = chunk * 7 + i;
                    sp.z = slot[i] | (dA << 8) | (dC << 16);
                    sp.w = (int)(koff[(size_t)l] + (long long)chunk * 8 + rank_of[i]);
                    steps.push_back(sp);
                    owner.push_back(q);
                    slot[i] = -1;  // (its slot is not reused: a new slot must start from zero)
                }
                // what is left: the separator (position 7 when the chunk is full or placed)
                if (real[7] && slot[7] >= 0) {
                    if (top) {  // solved on the spot
                        int4 sp;
                        sp.x = -1;
                        sp.y = 0;
                        sp.z = slot[7] | (255 << 8) | (255 << 16);
                        sp.w = (int)(koff[(size_t)l] + (long long)chunk * 8 + 7);
                        steps.push_back(sp);
                        owner.push_back(q);
                    } else if (l == nl - 1) {  // a shard's last level: this rank's block of the separator system
                        own = slot[7];
                    } else {
                        auto it = nz[(size_t)l + 1].find(chunk);
                        if (it == nz[(size_t)l + 1].end()) {
                            nz[(size_t)l + 1][chunk] = slot[7];
                        } else {
                            // the block of the next level already has a slot (the chunk after this one subtracted from
                            // it first): cannot happen -- chunks run in ascending order and only chunk + 1 writes there
                            throw HipError{hipErrorUnknown};
                        }
                    }
                }
            }
        }
        fin[(size_t)q] = int2{own < 0 ? 255 : own, remote < 0 ? 255 : remote};
        nslots = std::max(nslots, next);
        S.cl_maxsteps = std::max(S.cl_maxsteps, (int)steps.size() - off.back());
        off.push_back((int)steps.size());
    }
    if (nslots > 250) throw HipError{hipErrorUnknown};
    // the steps of every touched elimination, in step order
    std::map<int, std::vector<int>> by_key;
    for (size_t k = 0; k < steps.size(); k++) by_key[steps[k].w].push_back((int)k);
    std::vector<int> eoff(1, 0), erec;
    std::vector<int2> elim;
    for (auto &kv : by_key) {
        const int4 sp = steps[(size_t)kv.second[0]];
        int2 el;
        el.x = sp.x;
        el.y = sp.y;
        elim.push_back(el);
        for (int k : kv.second) erec.push_back(k);
        eoff.push_back((int)erec.size());
    }
    // eliminations on (almost) every closure's path -- the blocks of the top levels: their part of S is a dense
    // product, done tile-wise from LDS (k_bcr_closure_S); the key of a step carries the mark in its lowest bit
    std::vector<int> dense;
    for (size_t k = 0; k < steps.size(); k++) steps[k].w *= 2;
    if (r >= 8) {  // (round 5: also for the Woodbury systems that are solved in LDS -- the merge is a memory round trip per match)
        int d = 0;
        for (auto &kv : by_key)
            if ((long long)kv.second.size() * 4 >= r) {
                dense.resize((size_t)(d + 1) * r, -1);
                for (int k : kv.second) {
                    dense[(size_t)d * r + owner[(size_t)k]] = k;
                    steps[(size_t)k].w |= 1;
                }
                d++;
            }
        S.cl_ndense = d;
    }
    if (dense.empty()) dense.push_back(-1);
    S.cl_dense.upload(dense, g.stream);
    S.cl_nslots = nslots;
    S.cl_nsteps = (int)steps.size();
    S.cl_nelim = (int)elim.size();
    S.cl_npad = r <= kSolveLdsMax ? r : (r + 63) / 64 * 64;
    S.far_e.upload(g.bcr_far_e, g.stream);
    S.cl_off.upload(off, g.stream);
    S.cl_step.upload(steps, g.stream);
    S.cl_init.upload(init, g.stream);
    if (shard) {
        // (the steps' owners as the correction reads them: numbers in the global list, where lambda lives)
        std::vector<int> gowner(owner.size());
        for (size_t k = 0; k < owner.size(); k++) gowner[k] = g.bcr_far_gid[(size_t)owner[k]];
        if (gowner.empty()) gowner.push_back(0);
        S.cl_owner.upload(gowner, g.stream);
        S.cl_fin.upload(fin, g.stream);
        S.cl_gid.upload(g.bcr_far_gid, g.stream);
        S.cl_own.upload(g.bcr_far_own, g.stream);
    } else {
        S.cl_owner.upload(owner, g.stream);
    }
    S.co_off.upload(eoff, g.stream);
    S.co_rec.upload(erec, g.stream);
    S.co_elim.upload(elim, g.stream);
    S.cl_R.alloc(steps.size() * (size_t)B);
    S.cl_W.alloc(steps.size() * (size_t)B);
    if (!shard) S.cl_S.alloc((size_t)S.cl_npad * S.cl_npad);  // (a shard's share goes straight into the ranks' common buffer)
    S.cl_T.alloc((size_t)S.cl_npad * 3);
    S.lam.alloc((size_t)S.cl_npad * 3);
    S.cl_alive.alloc((size_t)S.cl_npad);
    S.Dinv.resize((size_t)nl);
    for (int l = 0; l < nl; l++) S.Dinv[(size_t)l].alloc((size_t)S.lev[l].nch * 7 * B * B);
    S.topDinv.alloc((size_t)B * B);
    S.dead.alloc(1);
    IRH_CHECK(hipMemsetAsync(S.topDinv.p, 0, sizeof(double) * (size_t)B * B, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));  // the host vectors go away
}

static void bcr_alloc(Graph &g) {
    if (g.bcr) return;
    g.bcr.reset(new BcrState());
    BcrState &S = *g.bcr;
    S.B = g.bcr_B;
    S.nfar = (int)g.bcr_far_e.size();
    constexpr int NR = 3;
    const int B = S.B, NC = 2 * B + NR;
    const int nb0 = (g.levels[0].n + B - 1) / B;
    int nch0 = (nb0 + 7) / 8;
    // The level-0 reduction keeps two workgroups per CU resident (one for B = 32 or with closure columns: LDS). A
    // chunk count slightly above a multiple of that capacity would cost a whole extra round of workgroups for a
    // handful of chunks (100k views, B = 24: 521 chunks on 512 slots): the chunks beyond the multiple are not
    // reduced at all -- their blocks enter level 1 as they are (a MIXED level 1: k_bcr_reduce's loader), where
    // there is room.
    int nraw = 0;
    {
        int ncu = 256;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, g.device);
        if (ncu <= 0) ncu = 256;
        const int cap = ncu * (B <= 24 && NR == 3 ? 2 : 1);
        const int full = nch0 / cap * cap, rem = nch0 - full;
        if (full > 0 && rem > 0 && rem <= cap / 4 && !g.bcr_shard && !g.sw.bcr_no_mixed) {
            nraw = nb0 - 8 * full;
            nch0 = full;
        }
    }
    // the last level: one chunk of <= 8 blocks, or (round 5) one workgroup of <= 16 blocks that also makes its way back
    // -- three right-hand sides, blocks up to 24 rows (LDS), no closures (their step programs know chunks), not a shard
    S.top16 = B <= 24 && S.nfar == 0 && !g.bcr_shard && !g.sw.bcr_no_top16;
    const int topmax = S.top16 ? kTopMax : 8;
    int nb = nb0, nch = nch0;
    for (int l = 0;; l++) {
        S.lev.emplace_back();
        BcrLevel &L = S.lev.back();
        L.nb = nb;
        L.nch = nch;
        L.nred = (l == 1 && nraw > 0) ? nb - nraw : nb;
        const bool last = nb <= topmax && !g.bcr_shard && l > 0;
        if (last && S.top16) {
            // (a level 0 of <= 16 blocks keeps the chunk form: its blocks are gathered from the operator)
            L.x.alloc((size_t)L.nch * 8 * B * NR);
            S.tsched = bcr_top_schedule(nb);
            S.tsched_dev.alloc(1);
            IRH_CHECK(hipMemcpyAsync(S.tsched_dev.p, &S.tsched, sizeof(BcrTopSched), hipMemcpyHostToDevice, g.stream));
            IRH_CHECK(hipStreamSynchronize(g.stream));
            break;
        }
        if (l == 0 && nb <= 8) S.top16 = false;
        L.W.alloc((size_t)L.nch * 7 * B * NC);
        if (l > 0) L.x.alloc((size_t)L.nch * 8 * B * NR);
        if (nb <= 8 && !g.bcr_shard) {
            S.top16 = false;
            break;
        }
        L.sepD.alloc((size_t)L.nch * B * B);
        L.extD.alloc((size_t)L.nch * B * B);
        L.extG.alloc((size_t)L.nch * B * B);
        L.sepR.alloc((size_t)L.nch * B * NR);
        L.extR.alloc((size_t)L.nch * B * NR);
        if (nb <= 8) break;
        nb = L.nch + (l == 0 ? nraw : 0);
        nch = (nb + 7) / 8;
    }
    if (g.bcr_shard) {
        S.ext0 = g.bcr_ext0;
        S.ghost_extcol.upload(g.bcr_ghost_extcol, g.stream);
        S.remD.alloc((size_t)B * B);
        S.remR.alloc((size_t)B * NR);
        IRH_CHECK(hipStreamSynchronize(g.stream));
    }
    S.xtop.alloc((size_t)B * NR);
    if (S.nfar > 0) bcr_closure_plan(g);
    if (g.bcr_shard && !g.bcr_fix_row.empty()) {
        S.nfix = (int)g.bcr_fix_row.size();
        S.fix_row.upload(g.bcr_fix_row, g.stream);
        S.fix_off.upload(g.bcr_fix_off, g.stream);
        S.fix_e.upload(g.bcr_fix_e, g.stream);
        S.fix_saved.alloc((size_t)S.nfix);
        IRH_CHECK(hipStreamSynchronize(g.stream));
    }
}

// ---------------------------------------------------------------------------------------------
// One solve on the host: shape -> route (bcr_route.hpp) -> reductions -> ways back. Every function below makes one kind
// of launch; which of them run, and as which instantiation, is the route's business alone.
// ---------------------------------------------------------------------------------------------
static_assert(kBcrMaxLevels == kMaxLevels && kBcrApplySlotsMax == 4 * kMaxParts, "bcr_route.hpp restates these");

BcrShape bcr_shape(const Graph &g) {
    BcrShape s;
    s.B = g.bcr_B;
    s.nfar = (int)g.bcr_far_e.size();
    s.shard = g.bcr_shard;
    s.ng = g.ng;
    s.guard = g.bcr_guard;
    s.asm_windowed = g.asm_windowed != 0;
    s.dbg = g.sw.bcr_dbg;
    s.no_fused_asm = g.sw.bcr_no_fused_asm;
    s.no_unit_factor = g.sw.bcr_no_unit_factor;
    s.no_fused_up = g.bcr_no_fused_up;
    if (g.bcr) {
        const BcrState &S = *g.bcr;
        s.nl = (int)S.lev.size();
        for (int l = 0; l < s.nl; l++) s.nch[l] = S.lev[l].nch;
        s.top16 = S.top16;
        s.unit_valid = S.unit.valid;
    }
    return s;
}

// the unit-weight store, allocated by the handle's first filling solve (lazily: a handle that never makes such a solve -- a
// solver clone, l1ra alone -- keeps nothing)
static void bcr_unit_alloc(BcrState &S) {
    BcrUnit &U = S.unit;
    const int nl = (int)S.lev.size();
    const size_t B = (size_t)S.B, NC = 2 * B + 3;
    U.epoch = g_unit_epoch.load(std::memory_order_acquire);
    U.lev.resize((size_t)nl - 1);
    size_t words = 0;
    for (int l = 0; l + 1 < nl; l++) {
        const size_t ne = (size_t)S.lev[l].nch * 7;
        U.lev[(size_t)l].Wu.alloc(ne * B * NC);
        U.lev[(size_t)l].Di.alloc(ne * B * B);
        U.lev[(size_t)l].P.alloc(ne * B * B);
        U.lev[(size_t)l].Q.alloc(ne * B * B);
        words += ne * B * (NC + 3 * B);
    }
    U.top.alloc((size_t)(kTopUnitLast + 1) * B * B);
    words += (size_t)(kTopUnitLast + 1) * B * B;
    U.bytes = (int64_t)(words * sizeof(double));
    // (a partial chunk skips its padding positions: their slots are never written, and never read)
}

// k_bcr_reduce_up's arguments and its arrival counters: written once per handle
static void bcr_up_args_write(Graph &g) {
    BcrState &S = *g.bcr;
    Level &L0 = g.levels[0];
    hipStream_t st = g.stream;
    const int nl = (int)S.lev.size();
    if (S.up_cnt.n < (size_t)kUpLevels + 1) {
        S.up_cnt.alloc(kUpLevels + 1);
        S.up_cnt.zero(st);
        S.up_gen = 0;
    }
    if (S.up_args.p) return;
    BcrUpArgs A;
    memset(&A, 0, sizeof(A));
    A.nl = nl - 1;
    for (int i = 0; i < A.nl; i++) {
        BcrLevel &Li = S.lev[1 + i], &Fi = S.lev[i];
        A.lev[i] = BcrUpLevel{Li.nb,          Li.nred,        Li.nch,         (gp_cd)Fi.sepD.p, (gp_cd)Fi.sepR.p,
                              (gp_cd)Fi.extD.p, (gp_cd)Fi.extR.p, (gp_cd)Fi.extG.p, (gp_d)Li.W.p,   (gp_d)Li.sepD.p,
                              (gp_d)Li.sepR.p, (gp_d)Li.extD.p, (gp_d)Li.extR.p, (gp_d)Li.extG.p};
    }
    A.n = L0.n;
    A.sl_off = (gp_ci)L0.sl_off.p;
    A.col = (gp_ci)L0.col.p;
    A.val = (gp_cd)L0.val.p;
    A.diag = (gp_cd)L0.diag.p;
    A.rhs = (gp_cd4)L0.b.p;
    A.xtop = (gp_d)S.xtop.p;
    A.cnt = (gp_u)S.up_cnt.p;
    A.top16 = S.top16;
    A.top = S.tsched;
    A.xtop_all = (gp_d)S.lev[nl - 1].x.p;
    A.fail = (gp_i) reinterpret_cast<int *>(S.up_cnt.p + kUpLevels);
    S.up_args.alloc(1);
    IRH_CHECK(hipMemcpyAsync(S.up_args.p, &A, sizeof(A), hipMemcpyHostToDevice, st));
    IRH_CHECK(hipStreamSynchronize(st));  // (A is on this stack)
}
// ... and the store's copy: the same arguments with W = the store's and the operand arrays
static void bcr_up_args_write_unit(BcrState &S, hipStream_t st) {
    BcrUnit &U = S.unit;
    if (U.up_args.p) return;
    BcrUpArgs A;
    IRH_CHECK(hipMemcpyAsync(&A, S.up_args.p, sizeof(A), hipMemcpyDeviceToHost, st));
    IRH_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i + 1 < A.nl; i++) {
        BcrUnitLevel &Ui = U.lev[(size_t)i + 1];
        A.lev[i].W = (gp_d)Ui.Wu.p;
        A.lev[i].stD = (gp_d)Ui.Di.p;
        A.lev[i].stP = (gp_d)Ui.P.p;
        A.lev[i].stQ = (gp_d)Ui.Q.p;
    }
    A.tst = (gp_d)U.top.p;
    U.up_args.alloc(1);
    IRH_CHECK(hipMemcpyAsync(U.up_args.p, &A, sizeof(A), hipMemcpyHostToDevice, st));
    IRH_CHECK(hipStreamSynchronize(st));  // (A is on this stack)
}

// the upper launch: the reductions of all levels above level 0 (and, on a sixteen-block top, its way back)
template <int B, int UF>
static void bcr_launch_up_as(Graph &g, const BcrUpArgs *args, int dbg) {
    BcrState &S = *g.bcr;
    const int nl = (int)S.lev.size();
    const size_t lds = bcr_up_lds<B>(S.top16 ? S.lev[nl - 1].nb : 0);
    static std::atomic<size_t> lds_set[16];
    if (lds_set[g.device & 15].load() < lds) {
        IRH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bcr_reduce_up<B, UF>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set[g.device & 15].store(lds);
    }
    hipLaunchKernelGGL((k_bcr_reduce_up<B, UF>), dim3(S.lev[1].nch), dim3(512), lds, g.stream, args, ++S.up_gen, dbg,
                       (dbg & 128) ? S.stamps.p : (long long *)nullptr);
}
template <int B>
static void bcr_launch_up(Graph &g, const BcrRoute &R, int dbg) {
    if constexpr (B <= 24) {
        BcrState &S = *g.bcr;
        bcr_up_args_write(g);
        // (tests: the give-up path without a second process -- the word is set as if a wait had timed out)
        if (g.sw.bcr_fake_up_fail && g.stats.direct_up_fallbacks == 0)
            IRH_CHECK(hipMemsetAsync(S.up_cnt.p + kUpLevels, 1, sizeof(int), g.stream));
        if constexpr (B == 8 || B == 16 || B == 24) {
            if (R.uf) {
                bcr_up_args_write_unit(S, g.stream);
                if (R.uf == 2) bcr_launch_up_as<B, 2>(g, S.unit.up_args.p, dbg);
                else bcr_launch_up_as<B, 1>(g, S.unit.up_args.p, dbg);
                return;
            }
        }
        if (R.uf) throw HipError{hipErrorInvalidValue};
        return bcr_launch_up_as<B, 0>(g, S.up_args.p, dbg);
    }
    throw HipError{hipErrorInvalidValue};  // (the route takes the upper launch for blocks up to 24 only)
}

// the single-workgroup top in a launch of its own
template <int B>
static void bcr_launch_top(Graph &g, int dbg, long long *stamps) {
    if constexpr (B <= 24) {
        BcrState &S = *g.bcr;
        const int l = (int)S.lev.size() - 1;
        const BcrLevel &F = S.lev[l - 1];
        const size_t lds = bcr_top_lds(B, S.lev[l].nb);
        static std::atomic<size_t> lds_set[16];
        if (lds_set[g.device & 15].load() < lds) {
            IRH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bcr_top<B>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            lds_set[g.device & 15].store(lds);
        }
        hipLaunchKernelGGL((k_bcr_top<B>), dim3(1), dim3(512), lds, g.stream, S.tsched_dev.p, F.sepD.p, F.sepR.p, F.extD.p,
                           F.extR.p, F.extG.p, S.lev[l].x.p, dbg, stamps);
        return;
    }
    throw HipError{hipErrorInvalidValue};  // (a sixteen-block top: blocks up to 24 only)
}

// The instantiation of k_bcr_reduce a route entry names, handed to go(kernel, waves). Only these exist: eight waves for
// blocks up to 24; the assembling launch at level 0 when a chunk's rows are whole slices; the unit-weight factor on the
// assembling launch below the top for blocks of 8 / 16 / 24. Anything else the route cannot ask for
// (tools/bcr_route_host_check.cpp) and is an error here.
template <int B, class Go>
static void bcr_reduce_kernel(const BcrLaunch &k, Go go) {
    auto waves = [&](auto l0, auto top, auto as, auto uf) {
        constexpr bool L = decltype(l0)::value, T = decltype(top)::value, A = decltype(as)::value;
        constexpr int U = decltype(uf)::value;
        if constexpr (B <= 24) {
            if (k.wide) return go(&k_bcr_reduce<B, 3, L, T, 8, A, U>, 8);
        }
        if (k.wide) throw HipError{hipErrorInvalidValue};
        go(&k_bcr_reduce<B, 3, L, T, 4, A, U>, 4);
    };
    using Y = std::true_type;
    using N = std::false_type;
    using U0 = std::integral_constant<int, 0>;
    if (k.uf) {
        if constexpr (B == 8 || B == 16 || B == 24) {
            if (k.l0 && !k.top && k.assemble && k.uf == 1) return waves(Y(), N(), Y(), std::integral_constant<int, 1>());
            if (k.l0 && !k.top && k.assemble && k.uf == 2) return waves(Y(), N(), Y(), std::integral_constant<int, 2>());
        }
        throw HipError{hipErrorInvalidValue};
    }
    if (k.assemble) {
        if constexpr ((8 * B) % 64 == 0) {
            if (k.l0) return k.top ? waves(Y(), Y(), Y(), U0()) : waves(Y(), N(), Y(), U0());
        }
        throw HipError{hipErrorInvalidValue};
    }
    if (k.l0) k.top ? waves(Y(), Y(), N(), U0()) : waves(Y(), N(), N(), U0());
    else k.top ? waves(N(), Y(), N(), U0()) : waves(N(), N(), N(), U0());
}
// one level's reduction in a launch of its own (the closure columns nothing instantiates -- nfar, far_i, far_j -- are literals)
template <int B>
static void bcr_reduce_level(Graph &g, const BcrRoute &R, int l, int dbg, long long *stamps) {
    BcrState &S = *g.bcr;
    Level &L0 = g.levels[0];
    BcrLevel &L = S.lev[l];
    const BcrLevel *F = l > 0 ? &S.lev[l - 1] : nullptr;
    const BcrLaunch &k = R.own[l];
    const bool far = S.nfar > 0;
    // (the unit-weight factor: level 0's W, inverses and operands are the store's)
    const BcrUnitLevel *U = k.uf ? &S.unit.lev[0] : nullptr;
    double *W = U ? U->Wu.p : L.W.p, *Dinv = U ? U->Di.p : far ? S.Dinv[(size_t)l].p : nullptr;
    BcrAsmArgs A{};
    int grid = L.nch;
    if (k.assemble) {
        // level 0 assembles its own slices first: the chunks' workgroups, then one per slice under no chunk
        A = BcrAsmArgs{L.nch,   L0.nsl,    (long long)g.m, (long long)g.mpad, g.slot_eid.p, g.tile_e0.p, g.beid.p,
                       g.bflag.p, g.bcr_wsrc, g.er.p,         L0.excess.p,       L0.idg.p,     g.bval.p};
        grid += std::max(0, L0.nsl - L.nch * (8 * B / 64));
        if (U) A.stP = U->P.p, A.stQ = U->Q.p;
    }
    bcr_reduce_kernel<B>(k, [&](auto kernel, int waves) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), 0, g.stream, L.nb, L.nred, L0.n, L0.sl_off.p, L0.col.p,
                           L0.val.p, L0.diag.p, L0.b.p, F ? F->sepD.p : nullptr, F ? F->sepR.p : nullptr,
                           F ? F->extD.p : nullptr, F ? F->extR.p : nullptr, F ? F->extG.p : nullptr, W, L.sepD.p, L.sepR.p,
                           L.extD.p, L.extR.p, L.extG.p, S.xtop.p, dbg, 0, (const int *)nullptr, (const int *)nullptr, S.ext0,
                           g.bptr.p, g.bghost.p, g.bval.p, S.ghost_extcol.p, (int)g.bcr_shard, stamps, Dinv,
                           far ? S.topDinv.p : nullptr, far ? S.dead.p : nullptr, (int)g.bcr_guard, A);
    });
}

// the ways back: of the levels above level 0 in one launch (k_bcr_back_top) unless this is a shard or the closures'
// columns ride along; xc_top / xext (a shard): the solution of its open top and of the previous rank's separator
template <int B>
static void bcr_ways_back(Graph &g, const BcrRoute &R, double4 *Xout, const double *xc_top, const double *xext) {
    BcrState &S = *g.bcr;
    Level &L0 = g.levels[0];
    hipStream_t st = g.stream;
    const int nl = (int)S.lev.size();
    const BcrUnit &U = S.unit;
    double4 *Qap = R.apply ? g.Q.p : (double4 *)nullptr;
    for (int l = nl - 1; l >= 0; l--) {
        BcrLevel &L = S.lev[l];
        if (R.back[l] == kBackTop && l == 1) {
            BcrBackPlan P;
            for (int k = 0; k < nl; k++) {
                P.W[k] = R.uf && k + 1 < nl ? U.lev[(size_t)k].Wu.p : S.lev[k].W.p;
                P.nb[k] = S.lev[k].nb;
            }
            P.top = S.top16 ? nl - 2 : nl - 1;
            P.base = 1;
            hipLaunchKernelGGL((k_bcr_back_top<B>), dim3(L.nch), dim3(kBackTopThreads), 0, st, P,
                               S.top16 ? S.lev[nl - 1].x.p : S.xtop.p, L.x.p, Xout, L0.n, L.nred, Qap, g.f, g.part_score.p,
                               S.lev[0].nch, (int)S.top16);
        }
        if (R.back[l] != kBackOwn) continue;
        const double *xc = l == nl - 1 ? (xc_top ? xc_top : S.xtop.p) : S.lev[l + 1].x.p;
        if (l == 0)
            hipLaunchKernelGGL((k_bcr_back<B, 3, true>), dim3(L.nch), dim3(256), 0, st, L.nb, L.nred, L0.n,
                               R.uf ? U.lev[0].Wu.p : L.W.p, xc, (double *)nullptr, Xout, (double *)nullptr, 0, 0, 0, xext,
                               (int)g.bcr_shard, Qap, g.f, g.part_score.p, 0);
        else
            hipLaunchKernelGGL((k_bcr_back<B, 3, false>), dim3(L.nch), dim3(256), 0, st, L.nb, L.nred, L0.n, L.W.p, xc,
                               L.x.p, Xout, (double *)nullptr, 0, 0, 0, xext, (int)g.bcr_shard);
    }
}

// One pass of a solve (BcrRequest::phase; a solve without closures on one GPU is one pass). The two side effects between
// the predicates keep their places: the upper launch's share of the device is asked for once it is wanted, a trimmed
// unit-weight store is released before the route reads whether one is valid, and allocated after it said "fill".
template <int B>
static void bcr_pass(Graph &g, const BcrRequest &rq, const double *xc_top = nullptr, const double *xext = nullptr) {
    BcrState &S = *g.bcr;
    BcrUnit &U = S.unit;
    BcrShape sh = bcr_shape(g);
    const int dbg = bcr_dbg(sh, rq), nl = sh.nl;
    long long *stamps = nullptr;
    if (dbg & 64) {
        if (!S.stamps.p) S.stamps.alloc((size_t)S.lev[0].nch * 16);
        stamps = S.stamps.p;
    }
    bool up = bcr_wants_up(sh, rq);
    if constexpr (B <= 24) {
        if ((dbg & 128) && !S.stamps.p) S.stamps.alloc((size_t)std::max(S.lev[0].nch * 16, 32 * kUpLevels));
        if (up) up = bcr_up_reserve<B>(g, S.lev[1].nch);
    }
    if (bcr_wants_unit(sh, rq, up)) {
        if (!U.lev.empty() && U.epoch != g_unit_epoch.load(std::memory_order_acquire)) U.release();
        sh.unit_valid = U.valid;
    }
    const BcrRoute R = bcr_route(sh, rq, up);
    // (ls_solve skipped K3 exactly when it asked level 0 to assemble: both or neither)
    if (R.asm0 != rq.assemble || (rq.open_top && rq.phase == 2) != (xc_top != nullptr)) throw HipError{hipErrorInvalidValue};
    if (rq.only < 0 && rq.phase != 2) S.last = R;
    U.last = R.uf;
    if (R.uf == 1 && U.lev.empty()) bcr_unit_alloc(S);
    for (int l = 0; l < nl; l++) {
        if (R.red[l] == kRedOwn) bcr_reduce_level<B>(g, R, l, dbg, stamps);
        else if (R.red[l] == kRedUp && l == 1) bcr_launch_up<B>(g, R, dbg);
        else if (R.red[l] == kRedTopAlone) bcr_launch_top<B>(g, dbg, stamps);
    }
    bcr_ways_back<B>(g, R, rq.out ? static_cast<double4 *>(rq.out) : g.X.p + g.ng, xc_top, xext);
}

// ---------------------------------------------------------------------------------------------
// the sharded form (dist.hip): a rank's range of the sequence is reduced to its last block; the separators of the
// `world` <= 8 ranks are one chunk, solved redundantly by every rank after ONE gather
// ---------------------------------------------------------------------------------------------
struct BcrPtrs {
    const double *d[kMaxLevels], *r[kMaxLevels];
    int n;
};
// remote contributions summed over the shard's levels (chunk 0 of each) and, with the top level's separator data,
// written into this rank's slices of the top buffer
template <int B>
__global__ __launch_bounds__(256) void k_bcr_pack_top(BcrPtrs P, int ext0, const double *__restrict__ sepD,
                                                      const double *__restrict__ sepR, const double *__restrict__ extG,
                                                      double *__restrict__ buf, int world, int rank) {
    constexpr int BB = B * B, BR = B * 3;
    double *oD = buf + (size_t)rank * BB, *oXD = buf + (size_t)world * BB + (size_t)rank * BB,
           *oXG = buf + (size_t)2 * world * BB + (size_t)rank * BB,
           *oR = buf + (size_t)3 * world * BB + (size_t)rank * BR,
           *oXR = buf + (size_t)3 * world * BB + (size_t)world * BR + (size_t)rank * BR;
    for (int e = threadIdx.x; e < BB; e += 256) {
        oD[e] = sepD[e];
        double sacc = 0.0;
        if (ext0)
            for (int l = 0; l < P.n; l++) sacc += P.d[l][e];
        oXD[e] = sacc;
        oXG[e] = ext0 ? extG[e] : 0.0;
    }
    for (int e = threadIdx.x; e < BR; e += 256) {
        oR[e] = sepR[e];
        double sacc = 0.0;
        if (ext0)
            for (int l = 0; l < P.n; l++) sacc += P.r[l][e];
        oXR[e] = sacc;
    }
}

// rec (rank-major records of one rank's five slices, what ncclAllGather moves) <-> buf (array-major, what the separator
// system is read from): mine >= 0: buf's slices of rank `mine` -> its record; mine < 0: every record -> buf
__global__ __launch_bounds__(256) void k_bcr_top_records(int B, int world, int mine, double *__restrict__ buf, double *__restrict__ rec) {
    const int BB = B * B, BR = B * 3, RS = 3 * BB + 2 * BR;
    const int r0 = mine >= 0 ? mine : 0, r1 = mine >= 0 ? mine + 1 : world;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < (r1 - r0) * RS; idx += gridDim.x * 256) {
        const int rank = r0 + idx / RS, e = idx % RS;
        size_t b;   // position in buf
        if (e < 3 * BB) b = (size_t)(e / BB) * world * BB + (size_t)rank * BB + e % BB;
        else {
            const int q = e - 3 * BB;
            b = (size_t)3 * world * BB + (size_t)(q / BR) * world * BR + (size_t)rank * BR + q % BR;
        }
        if (mine >= 0) rec[(size_t)rank * RS + e] = buf[b];
        else buf[b] = rec[(size_t)rank * RS + e];
    }
}
void bcr_top_to_record(BcrTop &T, int rank, hipStream_t st) {
    hipLaunchKernelGGL(k_bcr_top_records, dim3(8), dim3(256), 0, st, T.B, T.world, rank, T.buf.p, T.rec.p);
}
void bcr_top_from_records(BcrTop &T, hipStream_t st) {
    hipLaunchKernelGGL(k_bcr_top_records, dim3(8 * T.world), dim3(256), 0, st, T.B, T.world, -1, T.buf.p, T.rec.p);
}

void bcr_top_alloc(BcrTop &T, int B, int world) {
    T.B = B;
    T.world = world;
    T.buf.alloc(T.n_doubles());
    T.rec.alloc(T.n_doubles());
    T.W.alloc((size_t)7 * B * (2 * B + 3));
    T.x.alloc((size_t)8 * B * 3);
    T.xtop.alloc((size_t)B * 3);
}

// ---- loop closures on a sharded sequence (round 5) -------------------------------------------------------------
// The Woodbury correction of "The closures' part of a solve" with the elimination tree cut at the ranks' separators:
// a closure's incidence column is eliminated through the levels of the rank(s) that hold its endpoints
// (k_bcr_closure_forward on the shard's own step programs), what it leaves on the rank's separator and on the one
// before it is the column's right-hand side of the separator system, which every rank eliminates for ALL closures
// after the ranks' buffers have been summed; S = C^-1 + V' A_b^-1 V and T = V' Y are sums over eliminated blocks --
// a rank's blocks (its share, added to the same buffer) and the separator system's (added by everybody after the sum);
// lambda is solved by every rank, the corrections of the stored right-hand sides are local again.

// the rows with a closure to a GHOST view: their diagonal holds that closure's weight (a ghost edge is Dirichlet mass
// on a shard) -- the band operator loses it for the time of the reduction as bcr_gather_row takes a local far entry out
__global__ __launch_bounds__(256) void k_bcr_fix_diag(int nfix, const int *__restrict__ row, const int *__restrict__ off,
                                                       const int *__restrict__ e, const double *__restrict__ wsrc, int wsquare,
                                                       double *__restrict__ diag, double *__restrict__ saved, int restore) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nfix) return;
    const int rw = row[k];
    if (restore) {
        diag[rw] = saved[k];
        return;
    }
    const double d = diag[rw];
    saved[k] = d;
    double s = 0.0;
    for (int t = off[k]; t < off[k + 1]; t++) {
        const double w = wsrc[e[t]];
        s += wsquare ? w * w : w;
    }
    diag[rw] = d - s;
}

__global__ void k_bcr_add_dead(const int *__restrict__ dead, double *__restrict__ sum) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *sum += (double)*dead;
}

// After the sum over the ranks: S += the separator system's share (sum over its eliminations of R_p . D^-1 R_q: every
// closure has a record on every one of them -- a product of two r x (nst B) arrays), T += its share; a closure its owner
// flagged as dead (weight 0) gets the identity's row and column and T = 0; the padding of the inversion.
template <int B>
__global__ __launch_bounds__(256) void k_bcr_top_closure_S(int r, int npad, int nst, const double *__restrict__ recR,
                                                            const double *__restrict__ recW, const double *__restrict__ Ttop,
                                                            double *__restrict__ S, double *__restrict__ T,
                                                            const double *__restrict__ deadx) {
    __shared__ double sx[16][65], sy[16][65];
    if (blockIdx.x < blockIdx.y) return;
    const int tp = threadIdx.x >> 4, tq = threadIdx.x & 15;
    const int p = blockIdx.y * 16 + tp, q = blockIdx.x * 16 + tq;
    const int K = nst * B;
    double sum = 0.0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        for (int e = threadIdx.x; e < 32 * 64; e += 256) {
            const int who = e >> 6, k = e & 63;
            const int cl = who < 16 ? blockIdx.y * 16 + who : blockIdx.x * 16 + who - 16;
            double v = 0.0;
            if (cl < r && k0 + k < K) v = (who < 16 ? recR : recW)[(size_t)cl * K + k0 + k];
            if (who < 16)
                sx[who][k] = v;
            else
                sy[who - 16][k] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 64; k++) sum = fma(sx[tp][k], sy[tq][k], sum);
        __syncthreads();
    }
    if (p >= npad || q >= npad || q < p) return;
    if (p >= r || q >= r) {
        S[(size_t)p * npad + q] = S[(size_t)q * npad + p] = p == q ? 1.0 : 0.0;
        return;
    }
    const bool live = !(deadx[p] > 0.0) && !(deadx[q] > 0.0);
    const double v = live ? S[(size_t)p * npad + q] + sum : (p == q ? 1.0 : 0.0);
    S[(size_t)p * npad + q] = v;
    S[(size_t)q * npad + p] = v;
    if (p == q)
        for (int c = 0; c < 3; c++) T[3 * p + c] = live ? T[3 * p + c] + Ttop[3 * p + c] : 0.0;
}

template <int B>
static BcrClPlan bcr_local_clplan(BcrState &S) {
    BcrClPlan P;
    const int nl = (int)S.lev.size();
    for (int l = 0; l < kMaxLevels; l++) {
        P.W[l] = P.Wrw[l] = l < nl ? S.lev[l].W.p : nullptr;
        P.Dinv[l] = l < nl && l < (int)S.Dinv.size() ? S.Dinv[(size_t)l].p : nullptr;
    }
    P.topDinv = S.topDinv.p;
    P.xtop = S.xtop.p;
    return P;
}

template <int B>
static void bcr_launch_forward(hipStream_t st, const BcrClPlan &P, int r, int nslots, const int *off, const int4 *steps,
                               const int4 *init, double *recR, double *recW, double *T, const double *slot_init,
                               const int2 *fin, const int *gid, double *dep, int world, int rank) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    // Few closures: one workgroup per closure, four staged blocks of B x (3B + 3) doubles (58 KB at B = 24, 100 KB at
    // B = 32) + the slots -- the chain of a closure's steps is what takes the time, and two such workgroups fill a CU.
    // Many closures (more than two per CU): a wave per closure, LDS for the slots only (measured at a thousand closures:
    // 65 us against 100).
    const size_t lds_wg = ((size_t)4 * B * (3 * B + 3) + (size_t)4 * (3 * B + 3) + (size_t)nslots * B) * sizeof(double);
    // (blocks of 32: 100 KB, one workgroup per CU -- the chip takes 256 closures at a time then)
    const int r_wg = lds_wg * 2 <= 150 * 1024 ? 400 : 256;
    // (EIGHT steps per round trip -- eight waves, twice the stages -- measured 50 us against 35.5 at thirty closures in
    // round 6: the steps are bound by their two barriers each, not by the round trips. DESIGN.md 5b keeps the record.)
    if (r <= r_wg && lds_wg <= 150 * 1024) {
        static std::atomic<size_t> lds_set[16];
        if (lds_wg > 64 * 1024 && lds_set[dev & 15].load() < lds_wg) {
            IRH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bcr_closure_forward<B>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wg));
            lds_set[dev & 15].store(lds_wg);
        }
        hipLaunchKernelGGL((k_bcr_closure_forward<B>), dim3(r), dim3(256), lds_wg, st, P, r, nslots, off, steps, init, recR, recW,
                           T, slot_init, fin, gid, dep, world, rank);
        return;
    }
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * nslots * B * sizeof(double) > 60 * 1024) wpb >>= 1;
    const size_t lds = (size_t)wpb * nslots * B * sizeof(double);
    if (lds > 64 * 1024)
        IRH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bcr_closure_forward_wave<B>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_bcr_closure_forward_wave<B>), dim3((r + wpb - 1) / wpb), dim3(64 * wpb), lds, st, P, r, nslots, off,
                       steps, init, recR, recW, T, slot_init, fin, gid, dep, world, rank);
}

template <int B>
static void bcr_shard_reduce_t(Graph &g, BcrTop &T, int rank) {
    BcrState &S = *g.bcr;
    if (S.nfar > 0) IRH_CHECK(hipMemsetAsync(S.dead.p, 0, sizeof(int), g.stream));
    if (S.nfix > 0)
        hipLaunchKernelGGL(k_bcr_fix_diag, dim3((S.nfix + 255) / 256), dim3(256), 0, g.stream, S.nfix, S.fix_row.p, S.fix_off.p,
                           S.fix_e.p, g.bcr_wsrc, g.bcr_wsquare, g.levels[0].diag.p, S.fix_saved.p, 0);
    BcrRequest rq;
    rq.phase = 1;
    rq.open_top = true;
    bcr_pass<B>(g, rq);
    if (S.nfix > 0)
        hipLaunchKernelGGL(k_bcr_fix_diag, dim3((S.nfix + 255) / 256), dim3(256), 0, g.stream, S.nfix, S.fix_row.p, S.fix_off.p,
                           S.fix_e.p, g.bcr_wsrc, g.bcr_wsquare, g.levels[0].diag.p, S.fix_saved.p, 1);
    BcrPtrs P;
    P.n = (int)S.lev.size();
    for (int l = 0; l < P.n; l++) {
        P.d[l] = S.lev[l].extD.p;  // chunk 0 of every level
        P.r[l] = S.lev[l].extR.p;
    }
    BcrLevel &L = S.lev.back();
    hipLaunchKernelGGL((k_bcr_pack_top<B>), dim3(1), dim3(256), 0, g.stream, P, S.ext0, L.sepD.p, L.sepR.p, L.extG.p,
                       T.buf.p, T.world, rank);
}
template <int B>
static void bcr_top_reduce_launch(Graph &g, BcrTop &T, double *Dinv, double *topDinv, int *dead, int reg = 0) {
    const int W = T.world;
    const size_t BB = (size_t)B * B, BR = (size_t)B * 3;
    double *buf = T.buf.p;
    const double *nul = nullptr;
    hipLaunchKernelGGL((k_bcr_reduce<B, 3, false, true, 4>), dim3(1), dim3(256), 0, g.stream, W, W, 0, (const int *)nullptr,
                       (const int *)nullptr, nul, nul, (const double4 *)nullptr, buf, buf + 3 * W * BB, buf + W * BB,
                       buf + 3 * W * BB + W * BR, buf + 2 * W * BB, T.W.p, (double *)nullptr, (double *)nullptr,
                       (double *)nullptr, (double *)nullptr, (double *)nullptr, T.xtop.p, 0, 0, (const int *)nullptr,
                       (const int *)nullptr, 0, (const int *)nullptr, (const int *)nullptr, nul, (const int *)nullptr, 0,
                       (long long *)nullptr, Dinv, topDinv, dead, reg, BcrAsmArgs{});
}
template <int B>
static void bcr_top_back_launch(Graph &g, BcrTop &T) {
    const int W = T.world;
    const double *nul = nullptr;
    hipLaunchKernelGGL((k_bcr_back<B, 3, false>), dim3(1), dim3(256), 0, g.stream, W, W, 0, T.W.p, T.xtop.p, T.x.p,
                       (double4 *)nullptr, (double *)nullptr, 0, 0, 0, nul, 0);
}
template <int B>
static void bcr_top_solve_t(Graph &g, BcrTop &T) {
    bcr_top_reduce_launch<B>(g, T, nullptr, nullptr, nullptr);
    bcr_top_back_launch<B>(g, T);
}
template <int B>
static void bcr_shard_back_t(Graph &g, BcrTop &T, int rank) {
    const double *xs = T.x.p + (size_t)rank * B * 3;
    BcrRequest rq;
    rq.phase = 2;
    rq.open_top = true;
    bcr_pass<B>(g, rq, xs, rank > 0 ? xs - (size_t)B * 3 : nullptr);
}

// this rank's closures: their forward eliminations through its levels, its share of S and T and its dead pivots -> T.xbuf
template <int B>
static void bcr_shard_closures_forward_t(Graph &g, BcrTop &T, int rank) {
    BcrState &S = *g.bcr;
    if (S.nfar == 0) return;
    hipStream_t st = g.stream;
    const BcrClPlan P = bcr_local_clplan<B>(S);
    const int r = S.nfar;
    bcr_launch_forward<B>(st, P, r, S.cl_nslots, S.cl_off.p, S.cl_step.p, S.cl_init.p, S.cl_R.p, S.cl_W.p, S.cl_T.p, nullptr,
                          S.cl_fin.p, S.cl_gid.p, T.xbuf.p + T.x_dep(), T.world, rank);
    const int nt = (S.cl_npad + 15) / 16;
    hipLaunchKernelGGL((k_bcr_closure_S<B>), dim3(nt, nt), dim3(256), (size_t)32 * S.cl_maxsteps * sizeof(int), st, r,
                       S.cl_npad, S.cl_maxsteps, S.cl_ndense, S.cl_dense.p, S.cl_off.p, S.cl_step.p, S.cl_R.p, S.cl_W.p,
                       S.far_e.p, g.bcr_wsrc, g.bcr_wsquare, T.xbuf.p + T.x_S(), S.cl_T.p, S.cl_alive.p, S.cl_gid.p,
                       S.cl_own.p, T.npad, T.xbuf.p + T.x_T(), T.xbuf.p + T.x_dead());
    hipLaunchKernelGGL(k_bcr_add_dead, dim3(1), dim3(64), 0, st, S.dead.p, T.xbuf.p + T.x_pivots());
}

// the separator system with the closures' columns (every rank, after the sum of the ranks' buffers): factor, the columns'
// forward eliminations, S and T completed, lambda, the corrected right-hand sides, the separators' solution
template <int B>
static void bcr_top_solve_closures_t(Graph &g, BcrTop &T) {
    hipStream_t st = g.stream;
    const int r = T.r, npad = T.npad, W = T.world;
    IRH_CHECK(hipMemsetAsync(T.dead.p, 0, sizeof(int), st));
    bcr_top_reduce_launch<B>(g, T, T.Dinv.p, T.topDinv.p, T.dead.p, (int)g.bcr_guard);
    BcrClPlan P;
    for (int l = 0; l < kMaxLevels; l++) {
        P.W[l] = P.Wrw[l] = l == 0 ? T.W.p : nullptr;
        P.Dinv[l] = l == 0 ? T.Dinv.p : nullptr;
    }
    P.topDinv = T.topDinv.p;
    P.xtop = T.xtop.p;
    double *xb = T.xbuf.p;
    bcr_launch_forward<B>(st, P, r, W, T.cl_off.p, T.cl_step.p, nullptr, T.recR.p, T.recW.p, T.Ttop.p, xb + T.x_dep(), nullptr,
                          nullptr, nullptr, 0, 0);
    const int nt = (npad + 15) / 16;
    hipLaunchKernelGGL((k_bcr_top_closure_S<B>), dim3(nt, nt), dim3(256), 0, st, r, npad, T.nst, T.recR.p, T.recW.p, T.Ttop.p,
                       xb + T.x_S(), xb + T.x_T(), xb + T.x_dead());
    if (r <= kSolveLdsMax) {
        bcr_launch_solve_lds(st, r, npad, xb + T.x_S(), xb + T.x_T(), T.lam.p);
    } else {
        dense_invert_spd(g, xb + T.x_S(), npad);
        hipLaunchKernelGGL(k_bcr_closure_lambda, dim3((r + 3) / 4), dim3(256), 0, st, r, npad, xb + T.x_S(), xb + T.x_T(),
                           T.lam.p);
    }
    hipLaunchKernelGGL((k_bcr_closure_correct<B>), dim3(T.nst), dim3(1024), 0, st, P, T.co_off.p, T.co_rec.p, T.co_elim.p,
                       T.cl_owner.p, T.recW.p, T.lam.p);
    bcr_top_back_launch<B>(g, T);
}

// the stored right-hand sides of this rank's blocks on the closures' paths -= sum_q (D^-1 R_q) lambda_q'
template <int B>
static void bcr_shard_closures_correct_t(Graph &g, BcrTop &T) {
    BcrState &S = *g.bcr;
    if (S.nfar == 0 || S.cl_nelim == 0) return;
    const BcrClPlan P = bcr_local_clplan<B>(S);
    hipLaunchKernelGGL((k_bcr_closure_correct<B>), dim3(S.cl_nelim), dim3(1024), 0, g.stream, P, S.co_off.p, S.co_rec.p,
                       S.co_elim.p, S.cl_owner.p, S.cl_W.p, T.lam.p);
}

// the separator system's step program: one chunk of `world` blocks at their own positions, nothing before it; every
// closure runs every elimination (slot t = block t, started from the summed deposits); the eighth block is solved
void bcr_top_closures_alloc(Graph &g0, BcrTop &T, int r) {
    T.r = r;
    if (r <= 0) return;
    const int B = T.B, W = T.world;
    T.npad = r <= kSolveLdsMax ? r : (r + 63) / 64 * 64;
    static const int sched[7] = {0, 2, 4, 6, 1, 5, 3};
    std::vector<int4> prog;
    std::vector<int2> elim;
    for (int k = 0; k < 7; k++) {
        const int i = sched[k];
        if (i >= W) continue;
        int a, c;
        if (k < 4) {
            a = i - 1;
            c = i + 1;
        } else if (k < 6) {
            a = i == 1 ? -1 : 3;
            c = i == 1 ? 3 : 7;
        } else {
            a = -1;
            c = 7;
        }
        const int dA = a >= 0 ? a : 255, dC = c < W ? c : 255;
        prog.push_back(int4{0, i, i | (dA << 8) | (dC << 16), 0});
        elim.push_back(int2{0, i});
    }
    if (W == 8) {
        prog.push_back(int4{-1, 0, 7 | (255 << 8) | (255 << 16), 0});
        elim.push_back(int2{-1, 0});
    }
    const int nst = (int)prog.size();
    T.nst = nst;
    std::vector<int> off((size_t)r + 1), owner((size_t)r * nst), eoff((size_t)nst + 1), erec((size_t)r * nst);
    std::vector<int4> steps((size_t)r * nst);
    for (int q = 0; q <= r; q++) off[(size_t)q] = q * nst;
    for (int q = 0; q < r; q++)
        for (int d = 0; d < nst; d++) {
            steps[(size_t)q * nst + d] = prog[(size_t)d];
            owner[(size_t)q * nst + d] = q;
        }
    for (int d = 0; d <= nst; d++) eoff[(size_t)d] = d * r;
    for (int d = 0; d < nst; d++)
        for (int q = 0; q < r; q++) erec[(size_t)d * r + q] = q * nst + d;
    hipStream_t st = g0.stream;
    T.cl_off.upload(off, st);
    T.cl_step.upload(steps, st);
    T.cl_owner.upload(owner, st);
    T.co_off.upload(eoff, st);
    T.co_rec.upload(erec, st);
    T.co_elim.upload(elim, st);
    T.xbuf.alloc(T.x_doubles());
    T.Dinv.alloc((size_t)7 * B * B);
    T.topDinv.alloc((size_t)B * B);
    T.recR.alloc((size_t)r * nst * B);
    T.recW.alloc((size_t)r * nst * B);
    T.Ttop.alloc((size_t)r * 3);
    T.lam.alloc((size_t)T.npad * 3);
    T.dead.alloc(1);
    IRH_CHECK(hipMemsetAsync(T.topDinv.p, 0, sizeof(double) * (size_t)B * B, st));
    IRH_CHECK(hipMemsetAsync(T.xbuf.p, 0, sizeof(double) * T.x_doubles(), st));
    IRH_CHECK(hipStreamSynchronize(st));  // the host vectors go away
}
#define IRH_BCR_DISPATCH(fn, ...)              \
    switch (g.bcr_B) {                         \
    case 8: fn<8>(__VA_ARGS__); break;         \
    case 16: fn<16>(__VA_ARGS__); break;       \
    case 24: fn<24>(__VA_ARGS__); break;       \
    default: fn<32>(__VA_ARGS__); break;       \
    }
void bcr_shard_reduce(Graph &g, BcrTop &T, int rank) {
    bcr_alloc(g);
    IRH_BCR_DISPATCH(bcr_shard_reduce_t, g, T, rank)
}
void bcr_top_solve(Graph &g, BcrTop &T) { IRH_BCR_DISPATCH(bcr_top_solve_t, g, T) }
void bcr_shard_back(Graph &g, BcrTop &T, int rank) {
    IRH_BCR_DISPATCH(bcr_shard_back_t, g, T, rank)
    g.stats.direct_solves += 1;
}
void bcr_shard_closures_forward(Graph &g, BcrTop &T, int rank) { IRH_BCR_DISPATCH(bcr_shard_closures_forward_t, g, T, rank) }
void bcr_top_solve_closures(Graph &g, BcrTop &T) { IRH_BCR_DISPATCH(bcr_top_solve_closures_t, g, T) }
void bcr_shard_closures_correct(Graph &g, BcrTop &T) { IRH_BCR_DISPATCH(bcr_shard_closures_correct_t, g, T) }

template <int B>
static void bcr_solve_t(Graph &g, const BcrRequest &rq) {
    BcrState &S = *g.bcr;
    if (S.nfar == 0 || rq.only >= 0) {
        bcr_pass<B>(g, rq);
        return;
    }
    // closures: the reduction (which keeps the inverses of the eliminated blocks), the closures' forward eliminations,
    // the Woodbury system, the corrected right-hand sides, the ways back
    hipStream_t st = g.stream;
    const int r = S.nfar, npad = S.cl_npad, nl = (int)S.lev.size();
    if (!S.dead_clean) IRH_CHECK(hipMemsetAsync(S.dead.p, 0, sizeof(int), st));
    S.dead_clean = false;
    BcrRequest part = rq;
    part.phase = 1;
    bcr_pass<B>(g, part);
    BcrClPlan P;
    for (int l = 0; l < nl; l++) {
        P.W[l] = S.lev[l].W.p;
        P.Wrw[l] = S.lev[l].W.p;
        P.Dinv[l] = S.Dinv[(size_t)l].p;
    }
    P.topDinv = S.topDinv.p;
    P.xtop = S.xtop.p;
    bcr_launch_forward<B>(st, P, r, S.cl_nslots, S.cl_off.p, S.cl_step.p, S.cl_init.p, S.cl_R.p, S.cl_W.p, S.cl_T.p, nullptr,
                          nullptr, nullptr, nullptr, 0, 0);
    const int nt = (npad + 15) / 16;
    const size_t lds_pairs = (size_t)4 * (S.cl_maxsteps + 64) * sizeof(int);
    if (r <= kClosurePairsMax && S.cl_maxsteps < 32768 && lds_pairs <= 60 * 1024 && !g.sw.bcr_s_tiles)  // (the switch: the tile kernel for every closure count)
        hipLaunchKernelGGL((k_bcr_closure_S_pairs<B>), dim3((npad + 3) / 4, npad), dim3(256), lds_pairs, st, r, npad,
                           S.cl_maxsteps, S.cl_off.p, S.cl_step.p, S.cl_R.p, S.cl_W.p, S.far_e.p, g.bcr_wsrc, g.bcr_wsquare,
                           S.cl_S.p, S.cl_T.p, S.cl_alive.p);
    else
    hipLaunchKernelGGL((k_bcr_closure_S<B>), dim3(nt, nt), dim3(256), (size_t)32 * S.cl_maxsteps * sizeof(int), st, r, npad,
                       S.cl_maxsteps, S.cl_ndense, S.cl_dense.p, S.cl_off.p, S.cl_step.p, S.cl_R.p,
                       S.cl_W.p, S.far_e.p, g.bcr_wsrc, g.bcr_wsquare, S.cl_S.p, S.cl_T.p, S.cl_alive.p);
    if (r <= kSolveLdsMax) {
        bcr_launch_solve_lds(st, r, npad, S.cl_S.p, S.cl_T.p, S.lam.p);
    } else {
        dense_invert_spd(g, S.cl_S.p, npad);
        hipLaunchKernelGGL(k_bcr_closure_lambda, dim3((r + 3) / 4), dim3(256), 0, st, r, npad, S.cl_S.p, S.cl_T.p,
                           S.lam.p);
    }
    hipLaunchKernelGGL((k_bcr_closure_correct<B>), dim3(S.cl_nelim), dim3(1024), 0, st, P, S.co_off.p, S.co_rec.p,
                       S.co_elim.p, S.cl_owner.p, S.cl_W.p, S.lam.p);
    part.phase = 2;
    bcr_pass<B>(g, part);
}

// levels[0] values, diagonal and right-hand side (assemble_values) -> g.X. Asynchronous; only >= 0 launches one
// kernel alone (bench: 0.. the reductions, 100.. the ways back).
int bcr_solve(Graph &g, const BcrRequest &rq) {
    if (!g.bcr_B || rq.phase != 0 || rq.open_top) return IROTAVG_ERR_BAD_ARG;  // (the passes of a shard: bcr_shard_*)
    bcr_alloc(g);
    switch (g.bcr_B) {
    case 8: bcr_solve_t<8>(g, rq); break;
    case 12: bcr_solve_t<12>(g, rq); break;
    case 16: bcr_solve_t<16>(g, rq); break;
    case 20: bcr_solve_t<20>(g, rq); break;
    case 24: bcr_solve_t<24>(g, rq); break;
    case 28: bcr_solve_t<28>(g, rq); break;
    case 32: bcr_solve_t<32>(g, rq); break;
    default: return IROTAVG_ERR_BAD_ARG;
    }
    if (rq.only < 0) g.stats.direct_solves += 1;
    return IROTAVG_OK;
}

// ||b - A x||^2 and ||b||^2 per coordinate of the level-0 system as it stands (values and diagonal of the last assembly,
// its right-hand side, g.X): a row per thread walks its SELL-64 row like bcr_gather_row does. The loop closures' entries
// are part of these rows, so the Woodbury correction is checked as well.
__global__ __launch_bounds__(256) void k_bcr_residual(int n, const int *__restrict__ sl_off, const int *__restrict__ col,
                                                       const double *__restrict__ val, const double *__restrict__ diag,
                                                       const double4 *__restrict__ rhs, const double4 *__restrict__ X,
                                                       double *__restrict__ part) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (row < n) {
        const int sl = row >> 6, ln = row & 63;
        const int o0 = sl_off[sl], w = sl_off[sl + 1] - o0;
        const v2i *__restrict__ cp = reinterpret_cast<const v2i *>(col) + (size_t)(o0 / 2) * 64 + ln;
        const v2d *__restrict__ vp = reinterpret_cast<const v2d *>(val) + (size_t)(o0 / 2) * 64 + ln;
        const double4 x = X[row], bb = rhs[row];
        const double d = diag[row];
        double s0 = d * x.x, s1 = d * x.y, s2 = d * x.z;
        for (int q = 0; q < w / 2; q++) {
            const v2i cc = cp[(size_t)q * 64];
            const v2d vv = vp[(size_t)q * 64];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const double v = h ? vv.y : vv.x;
                const int c = h ? cc.y : cc.x;
                if (v != 0.0) {  // (zero: padding)
                    const double4 xc = X[c];
                    s0 += v * xc.x;
                    s1 += v * xc.y;
                    s2 += v * xc.z;
                }
            }
        }
        r0 = (bb.x - s0) * (bb.x - s0);
        r1 = (bb.y - s1) * (bb.y - s1);
        r2 = (bb.z - s2) * (bb.z - s2);
        b0 = bb.x * bb.x;
        b1 = bb.y * bb.y;
        b2 = bb.z * bb.z;
    }
    block_sum3_store(r0, r1, r2, part + 8 * blockIdx.x);
    __syncthreads();
    block_sum3_store(b0, b1, b2, part + 8 * blockIdx.x + 4);
}

// a direct solve has no residual test of its own. On demand (one pass over level 0, a host round trip):
// ||b - A x|| / ||b|| per coordinate of the handle's most recent direct solve -> relres[3] and stats.last_relres.
int bcr_residual(Graph &g, double *relres) {
    if (!g.bcr_B || g.stats.direct_solves == 0 || g.levels.empty()) return IROTAVG_ERR_BAD_ARG;
    // not for a shard (its rows sit behind the ghost views, and a rank's rows are no system of their own) ...
    if (g.ng > 0 || g.bcr_shard) return IROTAVG_ERR_BAD_ARG;
    // ... and after a GUARDED solve (run_irls: a dead pivot of the band part -> conjugate gradients on the full operator,
    // preconditioned by the regularised direct solve) the right-hand side array holds that iteration's residual vector,
    // not b: what it reached is in stats.last_relres already (its own convergence test); nothing to evaluate here
    if (g.bcr_last_guarded) {
        for (int c = 0; c < 3; c++) relres[c] = g.stats.last_relres[c];
        return IROTAVG_OK;
    }
    Level &L0 = g.levels[0];
    const int grid = (L0.n + 255) / 256;
    DevBuf<double> part;
    part.alloc((size_t)grid * 8);
    hipLaunchKernelGGL(k_bcr_residual, dim3(grid), dim3(256), 0, g.stream, L0.n, L0.sl_off.p, L0.col.p, L0.val.p, L0.diag.p,
                       L0.b.p, g.X.p, part.p);
    IRH_CHECK(hipGetLastError());
    std::vector<double> h((size_t)grid * 8);
    IRH_CHECK(hipMemcpyAsync(h.data(), part.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
    double rr[3] = {0, 0, 0}, bb[3] = {0, 0, 0};
    for (int b = 0; b < grid; b++)
        for (int c = 0; c < 3; c++) {
            rr[c] += h[(size_t)b * 8 + c];
            bb[c] += h[(size_t)b * 8 + 4 + c];
        }
    for (int c = 0; c < 3; c++) {
        relres[c] = bb[c] > 0.0 ? std::sqrt(rr[c] / bb[c]) : (rr[c] > 0.0 ? HUGE_VAL : 0.0);
        g.stats.last_relres[c] = relres[c];
    }
    return IROTAVG_OK;
}

int bcr_info(Graph &g, int64_t *out, int cap) {
    int k = 0;
    auto put = [&](int64_t v) {
        if (k < cap) out[k++] = v;
    };
    put(g.bcr_B);
    if (!g.bcr_B) return k;
    bcr_alloc(g);
    put((int64_t)g.bcr->lev.size());
    for (const BcrLevel &L : g.bcr->lev) {
        put(L.nb);
        put(L.nch);
        put(L.nred);
    }
    put(g.bcr->nfar);
    put(g.bcr_asm_fused_last ? 1 : 0);  // the most recent assembly + solve (ls_solve) was ONE launch at level 0
    // the unit-weight factor: 0 none / 1 stored, solves served from it, its bytes
    const bool stored = bcr_unit_valid(g);
    put(stored ? 1 : 0);
    put(g.bcr->unit.solves);
    put(stored ? g.bcr->unit.bytes : 0);
    return k;
}

// development aid: a whole solve with stamps inside the single-launch upper reduction (IROTAVG_BCR_DBG & 128): out[32 i + k] =
// shader clocks of workgroup 0 at level i of the launch relative to the launch's first stamp -- k < 16: the body's phases,
// 16: level entered, 17: the wait for the level below is over, 18: body done, 19: counted; -1: not stamped
int bcr_stamps_up(Graph &g, double *out) {
    if (!g.bcr_B) return IROTAVG_ERR_BAD_ARG;
    bcr_alloc(g);
    BcrState &S = *g.bcr;
    BcrRequest rq;
    rq.dbg = 128 + 256 * g.sw.bcr_stamp_chunk;
    const size_t cnt = (size_t)std::max(S.lev[0].nch * 16, 32 * kUpLevels);
    if (!S.stamps.p) S.stamps.alloc(cnt);
    IRH_CHECK(hipMemsetAsync(S.stamps.p, 0, sizeof(long long) * cnt, g.stream));
    const int rc = bcr_solve(g, rq);
    if (rc != IROTAVG_OK) return rc;
    long long h[32 * kUpLevels];
    IRH_CHECK(hipMemcpyAsync(h, S.stamps.p, sizeof(h), hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
    bcr_up_release(g);
    for (int k = 0; k < 32 * kUpLevels; k++) out[k] = !h[k] ? -1.0 : (k & 31) >= 20 ? (double)h[k] : (double)(h[k] - h[16]);
    return S.last.fused_up ? IROTAVG_OK : IROTAVG_ERR_BAD_ARG;
}

// development aid: the reduction of `level` once with stamps on; out[0..16) = shader clocks of chunk `chunk` relative to
// its first stamp
int bcr_stamps(Graph &g, int level, int chunk, double *out) {
    if (!g.bcr_B) return IROTAVG_ERR_BAD_ARG;
    bcr_alloc(g);
    BcrState &S = *g.bcr;
    if (level < 0 || level >= (int)S.lev.size() || chunk < 0 || chunk >= S.lev[level].nch) return IROTAVG_ERR_BAD_ARG;
    BcrRequest rq;
    rq.only = level;
    rq.dbg = 64;
    if (!S.stamps.p) S.stamps.alloc((size_t)S.lev[0].nch * 16);
    IRH_CHECK(hipMemsetAsync(S.stamps.p, 0, sizeof(long long) * (size_t)S.lev[0].nch * 16, g.stream));
    const int rc = bcr_solve(g, rq);
    if (rc != IROTAVG_OK) return rc;
    long long h[16];
    IRH_CHECK(hipMemcpyAsync(h, S.stamps.p + (size_t)chunk * 16, sizeof(h), hipMemcpyDeviceToHost, g.stream));
    IRH_CHECK(hipStreamSynchronize(g.stream));
    for (int k = 0; k < 16; k++) out[k] = h[k] ? (double)(h[k] - h[0]) : -1.0;
    return IROTAVG_OK;
}

// diagnostic (irotavg_bcr_rhs_products): ONE wave through the right-hand-side products of an elimination, as the
// right-hand-side-only pass calls them (operands in memory, right-hand sides in LDS)
template <int B>
__global__ __launch_bounds__(64) void k_bcr_rhs_products(const double *__restrict__ Dinv, const double *__restrict__ P,
                                                         const double *__restrict__ Q, const double *__restrict__ R, int hasP,
                                                         int hasQ, double *__restrict__ WR, double *__restrict__ Ra,
                                                         double *__restrict__ Rc) {
    constexpr int NR = 3, XB = B * NR;
    typedef BcrDim<B, NR> Dm;
    __shared__ double sR[3][XB], sZ[2];
    const int lane = threadIdx.x;
    for (int e = lane; e < XB; e += 64) {
        sR[0][e] = R[e];
        sR[1][e] = Ra[e];
        sR[2][e] = Rc[e];
    }
    if (lane < 2) sZ[lane] = 0.0;
    __syncthreads();
    BcrElim<B, NR, 1> E;
    v4d out[Dm::MT][1];
    E.template phase1<Dm::NT>(Dm::NT - 1, Dinv, P, hasP != 0, Q, sR[0], sZ, sR[2], (double *)nullptr, sZ, lane, hasQ != 0);
    __syncthreads();
    if (hasP) {
        E.template phase2_mul<Dm::NT>(Dm::NT - 1, P, sR[0], out, lane);
        E.template phase2_put<Dm::NT>(Dm::NT - 1, out, sZ, sZ, false, sR[1], lane);
    }
    __syncthreads();
    for (int e = lane; e < XB; e += 64) {
        WR[e] = sR[0][e];
        Ra[e] = sR[1][e];
        Rc[e] = sR[2][e];
    }
}
template <int B>
static void bcr_rhs_products_run(const double *d, int hasP, int hasQ, hipStream_t s) {
    constexpr int BB = B * B, XB = B * 3;
    static_assert(BcrElim<B, 3, 1>::RS, "block size");
    double *o = const_cast<double *>(d) + 3 * BB + XB;
    k_bcr_rhs_products<B><<<1, 64, 0, s>>>(d, d + BB, d + 2 * BB, d + 3 * BB, hasP, hasQ, o, o + XB, o + 2 * XB);
    IRH_CHECK(hipGetLastError());
}
int bcr_rhs_products(int B, const double *Dinv, const double *P, const double *Q, const double *R, int hasP, int hasQ,
                     double *WR, double *Ra, double *Rc) {
    if (B != 8 && B != 16 && B != 24 && B != 32) return IROTAVG_ERR_BAD_ARG;
    hipStream_t s = nullptr;
    const size_t BB = (size_t)B * B, XB = (size_t)B * 3;
    DevBuf<double> d;  // D^-1 | P | Q | R | W_R | R_a | R_c
    d.alloc(3 * BB + 4 * XB);
    IRH_CHECK(hipMemcpyAsync(d.p, Dinv, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + BB, P, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 2 * BB, Q, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 3 * BB, R, XB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 3 * BB + 2 * XB, Ra, XB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 3 * BB + 3 * XB, Rc, XB * sizeof(double), hipMemcpyHostToDevice, s));
    switch (B) {
    case 8: bcr_rhs_products_run<8>(d.p, hasP, hasQ, s); break;
    case 16: bcr_rhs_products_run<16>(d.p, hasP, hasQ, s); break;
    case 24: bcr_rhs_products_run<24>(d.p, hasP, hasQ, s); break;
    default: bcr_rhs_products_run<32>(d.p, hasP, hasQ, s); break;
    }
    IRH_CHECK(hipMemcpyAsync(WR, d.p + 3 * BB + XB, XB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipMemcpyAsync(Ra, d.p + 3 * BB + 2 * XB, XB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipMemcpyAsync(Rc, d.p + 3 * BB + 3 * XB, XB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    return IROTAVG_OK;
}

// diagnostic (irotavg_bcr_block_products): ONE elimination's wide products by a workgroup of WPE waves, through the
// member functions of BcrElim the reduction kernels call, operands in LDS as there: W = D^-1 [P' | Q | R] (to memory),
// D_c -= Q' W_Q, D_a -= P W_P, the fill A[a, c] = -P W_Q over P
template <int B, int WPE>
__global__ __launch_bounds__(64 * WPE) void k_bcr_block_products(const double *__restrict__ Dinv, double *__restrict__ P,
                                                                 const double *__restrict__ Q, const double *__restrict__ R,
                                                                 int hasP, int hasQ, double *__restrict__ Dc,
                                                                 double *__restrict__ Da, double *__restrict__ W) {
    constexpr int NR = 3, BB = B * B, XB = B * NR;
    typedef BcrDim<B, NR> Dm;
    static_assert(WPE <= Dm::NT, "a wave per column tile at the most");
    constexpr int NTPW = (Dm::NT + WPE - 1) / WPE;
    __shared__ double sD[3][BB], sG[2][BB], sR[3][XB], sZ[2];  // D^-1, D_c, D_a | P, Q | R, R_c, R_a
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < BB; e += 64 * WPE) {
        sD[0][e] = Dinv[e];
        sD[1][e] = Dc[e];
        sD[2][e] = Da[e];
        sG[0][e] = P[e];
        sG[1][e] = Q[e];
    }
    for (int e = tid; e < XB; e += 64 * WPE) {
        sR[0][e] = R[e];
        sR[1][e] = 0.0;
        sR[2][e] = 0.0;
    }
    if (tid < 2) sZ[tid] = 0.0;
    __syncthreads();
    BcrElim<B, NR, NTPW> E;
    v4d out[Dm::MT][NTPW];
    E.template phase1<WPE>(wave, sD[0], sG[0], hasP != 0, sG[1], sR[0], sD[1], sR[1], W, sZ, lane, hasQ != 0);
    __syncthreads();
    if (hasP) E.template phase2_mul<WPE>(wave, sG[0], sR[0], out, lane);
    __syncthreads();
    if (hasP) E.template phase2_put<WPE>(wave, out, sG[0], sD[2], false, sR[2], lane);
    __syncthreads();
    for (int e = tid; e < BB; e += 64 * WPE) {
        Dc[e] = sD[1][e];
        Da[e] = sD[2][e];
        P[e] = sG[0][e];
    }
}
template <int B, int WPE>
static void bcr_block_products_run(double *d, int hasP, int hasQ, hipStream_t s) {
    constexpr int BB = B * B;
    static_assert(BcrAop<B>::SMALL, "block size");
    k_bcr_block_products<B, WPE><<<1, 64 * WPE, 0, s>>>(d, d + BB, d + 2 * BB, d + 5 * BB, hasP, hasQ, d + 3 * BB, d + 4 * BB,
                                                       d + 5 * BB + 3 * B);
    IRH_CHECK(hipGetLastError());
}
int bcr_block_products(int B, int wpe, const double *Dinv, const double *P, const double *Q, const double *R, int hasP,
                       int hasQ, double *Dc, double *Da, double *W, double *fill) {
    // (the block sizes whose last row tile runs as small products; two column tiles at B = 8)
    if (!((B == 24 && (wpe == 1 || wpe == 2 || wpe == 4)) || (B == 8 && (wpe == 1 || wpe == 2)))) return IROTAVG_ERR_BAD_ARG;
    hipStream_t s = nullptr;
    const size_t BB = (size_t)B * B, XB = (size_t)B * 3, WB = (size_t)B * (2 * B + 3);
    DevBuf<double> d;  // D^-1 | P | Q | D_c | D_a | R | W
    d.alloc(5 * BB + XB + WB);
    IRH_CHECK(hipMemcpyAsync(d.p, Dinv, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + BB, P, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 2 * BB, Q, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 3 * BB, Dc, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 4 * BB, Da, BB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemcpyAsync(d.p + 5 * BB, R, XB * sizeof(double), hipMemcpyHostToDevice, s));
    IRH_CHECK(hipMemsetAsync(d.p + 5 * BB + XB, 0xff, WB * sizeof(double), s));  // (NaN: every entry of W is written)
    if (B == 24) {
        if (wpe == 1) bcr_block_products_run<24, 1>(d.p, hasP, hasQ, s);
        else if (wpe == 2) bcr_block_products_run<24, 2>(d.p, hasP, hasQ, s);
        else bcr_block_products_run<24, 4>(d.p, hasP, hasQ, s);
    } else {
        if (wpe == 1) bcr_block_products_run<8, 1>(d.p, hasP, hasQ, s);
        else bcr_block_products_run<8, 2>(d.p, hasP, hasQ, s);
    }
    IRH_CHECK(hipMemcpyAsync(fill, d.p + BB, BB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipMemcpyAsync(Dc, d.p + 3 * BB, BB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipMemcpyAsync(Da, d.p + 4 * BB, BB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipMemcpyAsync(W, d.p + 5 * BB + XB, WB * sizeof(double), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    return IROTAVG_OK;
}

// ||b - Ax||^2 and ||b||^2 per coordinate from A x (partial sums in k_bcr_residual's layout)
__global__ __launch_bounds__(256) void k_bcr_resid_norms(int n, const double4 *__restrict__ b, const double4 *__restrict__ Ax,
                                                          double *__restrict__ part) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (row < n) {
        const double4 bb = b[row], a = Ax[row];
        r0 = (bb.x - a.x) * (bb.x - a.x);
        r1 = (bb.y - a.y) * (bb.y - a.y);
        r2 = (bb.z - a.z) * (bb.z - a.z);
        b0 = bb.x * bb.x;
        b1 = bb.y * bb.y;
        b2 = bb.z * bb.z;
    }
    block_sum3_store(r0, r1, r2, part + 8 * blockIdx.x);
    __syncthreads();
    block_sum3_store(b0, b1, b2, part + 8 * blockIdx.x + 4);
}

// The verdict on a direct solve with closures, taken on the device: no dead pivot of the band part AND a residual of the
// FULL system (k_bcr_residual's partial sums: one pass over level 0) within tol. The Woodbury form is exact in exact
// arithmetic only: where robust weights leave a stretch of the band nearly free and the closures hold it, Y = A_b^-1 b is
// huge along that stretch and the correction cancels it (fuzz seed 21 case 46: Welsch, 365 closures, weights^2 down to
// 1e-8 -- relative residual 4e-7 where the band-only solve reaches 1e-12). flags[1] = 1: the residual was the reason.
__global__ __launch_bounds__(256) void k_bcr_gate(int *__restrict__ dead, int *__restrict__ flags,
                                                  const double *__restrict__ part, int nparts, double tol2,
                                                  int *__restrict__ skip_out, int *__restrict__ flags_copy) {
    __shared__ double sh[4][6];
    const int t = threadIdx.x;
    double a[6] = {0, 0, 0, 0, 0, 0};
    if (part)
        for (int b = t; b < nparts; b += 256) {
            for (int c = 0; c < 3; c++) {
                a[c] += part[(size_t)b * 8 + c];
                a[3 + c] += part[(size_t)b * 8 + 4 + c];
            }
        }
    // (the sums of the 256 threads: by wave shuffles, then over the four waves -- one thread adding 1536 LDS words took 8 us)
    for (int c = 0; c < 6; c++) {
        double v = a[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((t & 63) == 0) sh[t >> 6][c] = v;
    }
    __syncthreads();
    if (t != 0) return;
    bool ok = true;
    if (part) {
        for (int c = 0; c < 6; c++) a[c] = sh[0][c] + sh[1][c] + sh[2][c] + sh[3][c];
        for (int c = 0; c < 3; c++) ok = ok && (a[c] <= tol2 * a[3 + c]);  // (NaN: not ok)
    }
    const int d = dead ? dead[0] : 0;
    flags[FL_DONE] = d == 0 && ok ? 1 : 0;
    flags[FL_ITERS] = d == 0 && !ok ? 1 : 0;
    flags[3] = d;
    // (round 6) the same verdict as a skip word for k_weights_then_residual, and the four flag words once more behind the
    // score's partial sums, so that ONE publication -- that kernel's first workgroup -- carries score and verdict
    if (dead) dead[0] = 0;  // (read: the next reduction counts from zero without a memset in front of it, BcrState::dead_clean)
    if (skip_out) skip_out[0] = d == 0 && ok ? 0 : 1;
    if (flags_copy) {
        flags_copy[FL_DONE] = d == 0 && ok ? 1 : 0;
        flags_copy[FL_ITERS] = d == 0 && !ok ? 1 : 0;
        flags_copy[FL_STALE] = 0;
        flags_copy[3] = d;
    }
}
const int *bcr_gate_skip_word(Graph &g) {
    BcrState *S = g.bcr.get();
    if (!S) return nullptr;
    if (!S->gate_skip.p) {
        S->gate_skip.alloc(1);
        S->gate_skip.zero(g.stream);
    }
    return S->gate_skip.p;
}
void bcr_gate(Graph &g, double *flags_copy) {
    BcrState *S = g.bcr.get();
    int *dead = S && S->nfar > 0 ? S->dead.p : nullptr;
    if (dead) S->dead_clean = true;  // (the gate kernel leaves the counter at zero)
    const double *part = nullptr;
    int grid = 0;
    if (S && S->nfar > 0 && g.ng == 0 && !g.bcr_shard) {
        // A x by the iterative solver's SpMV (13 us at 2M edges; a row per thread walking its SELL row, k_bcr_residual,
        // took 45), then b - A x and the two norms in one small pass over the rows
        Level &L0 = g.levels[0];
        grid = (L0.n + 255) / 256;
        if (S->res_part.n < (size_t)grid * 8) {
            S->res_part.alloc((size_t)grid * 8);
            S->res_zero.alloc(FL_COUNT);
            S->res_zero.zero(g.stream);  // (the SpMV skips its work behind a FL_DONE that is set: it gets words that never are)
        }
        launch_spmv(g, g.X.p, nullptr, S->res_zero.p);
        hipLaunchKernelGGL(k_bcr_resid_norms, dim3(grid), dim3(256), 0, g.stream, L0.n, L0.b.p, g.AP.p, S->res_part.p);
        part = S->res_part.p;
    }
    // (IROTAVG_BCR_FAKE_GIVE_UP, tests: no residual passes the gate)
    const double gate = std::max(g.opt.pcg_rtol, kBcrGateTolMin);
    const double tol = g.sw.bcr_fake_give_up ? -1.0 : gate * gate;
    int *skip_out = (S && flags_copy) ? const_cast<int *>(bcr_gate_skip_word(g)) : nullptr;
    hipLaunchKernelGGL(k_bcr_gate, dim3(1), dim3(256), 0, g.stream, dead, g.flags.p, part, grid, tol, skip_out,
                       reinterpret_cast<int *>(flags_copy));
}

int bcr_closures(Graph &g) { return g.bcr_B ? (int)g.bcr_far_e.size() : 0; }

// partial sums of the score a solve with BcrRequest::apply leaves in part_score, or 0 (bcr_route.hpp)
int bcr_apply_slots(Graph &g) {
    if (!g.bcr_B || !g.bcr_far_e.empty() || g.bcr_shard || g.ng != 0) return 0;  // (nothing to allocate for)
    bcr_alloc(g);
    return bcr_apply_slots(bcr_shape(g));
}
const BcrRoute &bcr_last_route(Graph &g) {
    static const BcrRoute none;
    return g.bcr ? g.bcr->last : none;
}

const int *bcr_fail_word(Graph &g) {
    if (!g.bcr || !g.bcr->last.fused_up || g.bcr->up_cnt.n < (size_t)kUpLevels + 1) return nullptr;
    return reinterpret_cast<const int *>(g.bcr->up_cnt.p + kUpLevels);
}
bool bcr_up_failed(Graph &g) {
    const int *w = bcr_fail_word(g);
    if (!w) return false;
    int h = 0;
    if (hipMemcpyAsync(&h, w, sizeof(int), hipMemcpyDeviceToHost, g.stream) != hipSuccess) return false;
    if (hipStreamSynchronize(g.stream) != hipSuccess) return false;
    if (!h) return false;
    (void)hipMemsetAsync(const_cast<int *>(w), 0, sizeof(int), g.stream);
    g.bcr_no_fused_up = true;
    g.stats.direct_up_fallbacks += 1;
    bcr_up_release(g);
    return true;
}

// the unit-weight factor (BcrUnit). bcr_unit_commit: run_irls has the score of the solve it announced -- a finite one makes a
// filling solve's store valid and counts a solve served from it; a filling solve that failed gives its arrays back.
void bcr_unit_commit(Graph &g, bool finite) {
    if (!g.bcr) return;
    BcrUnit &U = g.bcr->unit;
    if (U.last == 1) {
        if (finite) U.valid = true;
        else U.release();
    } else if (U.last == 2 && finite) {
        U.solves += 1;
    }
    U.last = 0;
}
int bcr_unit_last(Graph &g) { return g.bcr ? g.bcr->unit.last : 0; }
bool bcr_unit_valid(Graph &g) {
    return g.bcr && g.bcr->unit.valid && g.bcr->unit.epoch == g_unit_epoch.load(std::memory_order_acquire);
}
// irotavg_trim_memory: every handle's store is invalid from now on; a handle gives its arrays back to the pool when it next
// looks (on its own thread, between its own solves -- not under a solve another thread may be running on it)
void bcr_unit_trim() noexcept { g_unit_epoch.fetch_add(1, std::memory_order_acq_rel); }

int bcr_levels(Graph &g) {
    if (!g.bcr_B) return 0;
    bcr_alloc(g);
    return (int)g.bcr->lev.size();
}

// Called BEFORE the build (capi.cpp): a handle that solves directly gets no multigrid hierarchy at all.
// Decides whether the handle's solves run here: one GPU, every edge between two free views within 32 views
// (ral's I is 0-based; row = view - f) except for at most kBcrMaxFar long-range edges (loop closures: Woodbury
// correction, bcr_solve), enough rows for the hierarchy of the iterative solver to exist at all (smaller graphs
// are one dense level = a direct solve already). opt.band_direct: 0 choose, 1 whenever the band allows, -1 never;
// IROTAVG_BAND_DIRECT overrides the option.
constexpr int kBcrMaxFar = 2048;

// Is the BAND part of the operator positive definite -- is every free view tied to a fixed one through edges that are
// not closures (free-free edges within 32 views or between neighbouring blocks, and the edges from a fixed view that
// make_A keeps)? Exact (union-find over the free views); the callers try the cheap sufficient rule first.
bool bcr_band_part_anchored(int64_t m, int f, int64_t nu, int B, const int32_t *I) {
    std::vector<int> parent((size_t)nu);
    for (int64_t r = 0; r < nu; r++) parent[(size_t)r] = (int)r;
    std::vector<uint8_t> anch((size_t)nu, 0);
    auto find = [&](int x) {
        while (parent[(size_t)x] != x) {
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    };
    for (int64_t k = 0; k < m; k++) {
        const int i = I[2 * k], j = I[2 * k + 1];
        if (i >= f && j >= f) {
            if (i == j) continue;
            if (std::abs(i - j) > 32 && std::abs((i - f) / B - (j - f) / B) >= 2) continue;  // a closure
            const int a = find(i - f), b = find(j - f);
            if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
        } else if (i < f && j >= f) {
            anch[(size_t)(j - f)] = 1;
        }
    }
    for (int64_t r = 0; r < nu; r++)
        if (anch[(size_t)r]) anch[(size_t)find((int)r)] = 1;
    for (int64_t r = 0; r < nu; r++)
        if (!anch[(size_t)find((int)r)]) return false;
    return true;
}

// The two plans (edge list on the host: bcr_plan; on the device: bcr_plan_dev) differ in how they scan the edges, not in
// what they decide. Before the scan: nothing is planned; false = this handle solves iteratively whatever its edges are.
static bool bcr_plan_begin(Graph &g, int *mode) {
    g.bcr_B = 0;
    g.band0 = -1;
    g.bcr_far_i.clear();
    g.bcr_far_j.clear();
    g.bcr_far_e.clear();
    *mode = g.sw.has_band_direct ? g.sw.band_direct : g.opt.band_direct;
    return *mode >= 0 && g.ng == 0 && g.no >= 1;
}
// After the scan (band: widest span <= 32, bandall: widest span, nfar: spans > 32, all between free views): records the
// half-bandwidth and returns the block size of the direct solver, or 0 = iterative
static int bcr_plan_block(Graph &g, int mode, int band, int bandall, long long nfar) {
    g.band0 = bandall;
    // closures cost the direct path 0.06 ms + 0.55 us r + 0.15 ns r^2 per solve (forward eliminations, inversion of the
    // r x r Woodbury system, its assembly; measured at r = 12 ... 1000), the iterative solver ~0.9 ms per solve at 3000
    // views with loop edges and ~2.2 ms at 20k ... 100k: up to 2048 closures stay direct, up to 1024 on small graphs
    if (nfar > (g.no < 8192 ? kBcrMaxFar / 2 : kBcrMaxFar)) return 0;
    if (mode == 0 && g.no <= 2048) return 0;
    // blocks of 8, 12, ... 32 rows: the smallest multiple of four that holds the band (a shard of a sharded sequence
    // keeps 8 / 16 / 24 / 32: its range is a multiple of 192 rows, dist.hip)
    return band <= 8 ? 8 : (band + 3) / 4 * 4;
}

void bcr_plan(Graph &g, const int32_t *I) {
    int mode = 0;
    if (!bcr_plan_begin(g, &mode)) return;
    const int f = g.f;
    std::atomic<int> band(0), bandall(0);
    std::atomic<long long> nfar(0);
    std::atomic<bool> bad(false);
    const int64_t nt = g.n_total;
    parallel_for(g.m, 65536, [&](int64_t k0, int64_t k1, int) {
        int bmax = 0, ball = 0;
        long long far = 0;
        for (int64_t k = k0; k < k1; k++) {
            const int i = I[2 * k], j = I[2 * k + 1];
            if (i < 0 || j < 0 || i >= nt || j >= nt) {
                bad = true;
                return;
            }
            if (i >= f && j >= f) {
                const int d = std::abs(i - j);
                ball = std::max(ball, d);
                if (d <= 32) bmax = std::max(bmax, d);
                else far++;
            }
        }
        int cur = band.load();
        while (bmax > cur && !band.compare_exchange_weak(cur, bmax)) {
        }
        cur = bandall.load();
        while (ball > cur && !bandall.compare_exchange_weak(cur, ball)) {
        }
        nfar += far;
    });
    if (bad.load()) return;
    const int B = bcr_plan_block(g, mode, band.load(), bandall.load(), nfar.load());
    if (!B) return;
    if (nfar.load() > 0) {
        // long-range edges = those whose endpoints lie in blocks that are not neighbours (an edge of more than 32
        // views between neighbouring blocks is part of the block tridiagonal operator as it is)
        for (int64_t k = 0; k < g.m; k++) {
            const int i = I[2 * k], j = I[2 * k + 1];
            if (i >= f && j >= f && std::abs(i - j) > 32 && std::abs((i - f) / B - (j - f) / B) >= 2) {
                g.bcr_far_i.push_back(i - f);
                g.bcr_far_j.push_back(j - f);
                g.bcr_far_e.push_back((int)k);
            }
        }
        bool refuse = !g.bcr_far_e.empty() && g.sw.bcr_no_closures;
        if (!g.bcr_far_e.empty() && !refuse) {
            // The Woodbury correction needs the BAND part alone to be positive definite: every free view must be
            // tied to a fixed one through band edges. Sufficient and cheap: every view has a band edge to an earlier
            // view or an edge to a fixed view that the IRLS system keeps (make_A drops an edge whose SECOND endpoint
            // is fixed, ral/l1_irls.cpp:770-771). A sequence whose band part falls apart (a stretch that only a
            // closure ties to the rest) is left to the iterative solver.
            std::vector<uint8_t> ok((size_t)g.no, 0);
            parallel_for(g.m, 65536, [&](int64_t k0, int64_t k1, int) {
                for (int64_t k = k0; k < k1; k++) {
                    const int i = I[2 * k], j = I[2 * k + 1];
                    if (i >= f && j >= f) {
                        if (i != j && std::abs(i - j) <= 32) ok[(size_t)(std::max(i, j) - f)] = 1;  // benign race: all write 1
                    } else if (i < f && j >= f) {
                        ok[(size_t)(j - f)] = 1;
                    }
                }
            });
            for (int r = 0; r < g.no && !refuse; r++) refuse = !ok[(size_t)r];
            // (the rule is sufficient, not necessary -- e.g. the first free view of a sequence whose fixed views lie
            // further on is tied through LATER views only: the exact test decides then)
            if (refuse) refuse = !bcr_band_part_anchored(g.m, f, g.no, B, I);
        }
        if (refuse) {
            g.bcr_far_i.clear();
            g.bcr_far_j.clear();
            g.bcr_far_e.clear();
            return;
        }
    }
    g.bcr_B = B;
}

// ---- the same plan from an edge list that lives on the device (a resident view-graph, resident.hip) --------------
namespace {
// out: [0] widest span <= 32, [1] widest span, [2] index out of range; nfar: spans > 32 between free views
__global__ __launch_bounds__(256) void k_plan_stats(long long m, int f, int nt, const int2 *__restrict__ I,
                                                    const int *__restrict__ relabel, int *__restrict__ out,
                                                    unsigned long long *__restrict__ nfar) {
    __shared__ int sb[3][4];
    __shared__ unsigned long long sf[4];
    int band = 0, ball = 0, bad = 0;
    unsigned long long far = 0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < m; k += (long long)gridDim.x * 256) {
        const int2 e = I[k];
        int i = e.x, j = e.y;
        if (i < 0 || j < 0 || i >= nt || j >= nt) {
            bad = 1;
            continue;
        }
        if (relabel) {
            i = relabel[i];
            j = relabel[j];
        }
        if (i >= f && j >= f) {
            const int d = abs(i - j);
            ball = max(ball, d);
            if (d <= 32) band = max(band, d);
            else far++;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        band = max(band, __shfl_xor(band, o));
        ball = max(ball, __shfl_xor(ball, o));
        bad |= __shfl_xor(bad, o);
        far += __shfl_xor(far, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sb[0][w] = band;
        sb[1][w] = ball;
        sb[2][w] = bad;
        sf[w] = far;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(out, max(max(sb[0][0], sb[0][1]), max(sb[0][2], sb[0][3])));
        atomicMax(out + 1, max(max(sb[1][0], sb[1][1]), max(sb[1][2], sb[1][3])));
        if (sb[2][0] | sb[2][1] | sb[2][2] | sb[2][3]) atomicOr(out + 2, 1);
        const unsigned long long t = sf[0] + sf[1] + sf[2] + sf[3];
        if (t) atomicAdd(nfar, t);
    }
}
// the long-range edges (rows, edge id; any order: the host sorts them by edge id) and the coverage of the band part:
// ok[r] = 1 when row r has a band edge to an earlier view or an edge to a fixed view that the IRLS system keeps
__global__ __launch_bounds__(256) void k_plan_far(long long m, int f, int B, const int2 *__restrict__ I,
                                                  const int *__restrict__ relabel, int cap, int *__restrict__ cnt,
                                                  int *__restrict__ fi, int *__restrict__ fj, int *__restrict__ fe,
                                                  uint8_t *__restrict__ ok) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const int2 e = I[k];
    const int i = relabel ? relabel[e.x] : e.x, j = relabel ? relabel[e.y] : e.y;
    if (i >= f && j >= f) {
        const int d = abs(i - j);
        if (d > 32 && abs((i - f) / B - (j - f) / B) >= 2) {
            const int q = atomicAdd(cnt, 1);
            if (q < cap) {
                fi[q] = i - f;
                fj[q] = j - f;
                fe[q] = (int)k;
            }
        }
        if (i != j && d <= 32) ok[max(i, j) - f] = 1;
    } else if (i < f && j >= f) {
        ok[j - f] = 1;
    }
}
__global__ __launch_bounds__(256) void k_plan_uncovered(int no, const uint8_t *__restrict__ ok, int *__restrict__ cnt) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < no && !ok[r]) atomicAdd(cnt, 1);
}
}  // namespace

void bcr_plan_dev(Graph &g, const DevEdgeSrc &src) {
    int mode = 0;
    if (!bcr_plan_begin(g, &mode)) return;
    const int f = g.f;
    hipStream_t s = g.stream;
    int *h = reinterpret_cast<int *>(PinPool::get().take());
    struct PinGuard {
        int *p;
        ~PinGuard() { PinPool::get().give(p); }
    } pin_guard{h};
    DevBuf<int> out;  // [0..2] the statistics, [4..5] the far count (64 bit), [6] far-list length, [7] uncovered rows
    out.alloc(8);
    out.zero(s);
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(1024, (g.m + 255) / 256));
    hipLaunchKernelGGL(k_plan_stats, dim3(grid), dim3(256), 0, s, (long long)g.m, f, (int)g.n_total, src.I, src.relabel, out.p,
                       reinterpret_cast<unsigned long long *>(out.p + 4));
    IRH_CHECK(hipMemcpyAsync(h, out.p, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
    IRH_CHECK(hipStreamSynchronize(s));
    if (h[2]) return;
    const long long nfar = (long long)*reinterpret_cast<unsigned long long *>(h + 4);
    const int B = bcr_plan_block(g, mode, h[0], h[1], nfar);
    if (!B) return;
    if (nfar > 0) {
        DevBuf<int> fl;
        DevBuf<uint8_t> ok;
        fl.alloc((size_t)3 * kBcrMaxFar);
        ok.alloc((size_t)g.no);
        ok.zero(s);
        hipLaunchKernelGGL(k_plan_far, dim3((unsigned)((g.m + 255) / 256)), dim3(256), 0, s, (long long)g.m, f, B, src.I,
                           src.relabel, kBcrMaxFar, out.p + 6, fl.p, fl.p + kBcrMaxFar, fl.p + 2 * kBcrMaxFar, ok.p);
        hipLaunchKernelGGL(k_plan_uncovered, dim3((unsigned)((g.no + 255) / 256)), dim3(256), 0, s, g.no, ok.p, out.p + 7);
        IRH_CHECK(hipMemcpyAsync(h, out.p + 6, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        IRH_CHECK(hipStreamSynchronize(s));
        const int nl = h[0], uncovered = h[1];
        if (nl > kBcrMaxFar) return;  // (cannot happen: nl <= nfar)
        if (nl > 0) {
            if (g.sw.bcr_no_closures) return;
            if (uncovered > 0) {
                // see bcr_plan: the band part must be SPD alone, and the coverage rule is sufficient, not necessary. The
                // exact test runs on the host (rare: one copy of the edge list, in the labels the plan uses)
                std::vector<int32_t> hI((size_t)2 * g.m);
                IRH_CHECK(hipMemcpyAsync(hI.data(), src.I, sizeof(int32_t) * hI.size(), hipMemcpyDeviceToHost, s));
                std::vector<int> hrel;
                if (src.relabel) {
                    hrel.resize((size_t)g.n_total);
                    IRH_CHECK(hipMemcpyAsync(hrel.data(), src.relabel, sizeof(int) * hrel.size(), hipMemcpyDeviceToHost, s));
                }
                IRH_CHECK(hipStreamSynchronize(s));
                if (src.relabel)
                    for (int32_t &v : hI) v = hrel[(size_t)v];  // (k_plan_stats found every index inside [0, n_total))
                if (!bcr_band_part_anchored(g.m, f, g.no, B, hI.data())) return;
            }
            std::vector<int> hl((size_t)3 * kBcrMaxFar);
            IRH_CHECK(hipMemcpyAsync(hl.data(), fl.p, sizeof(int) * hl.size(), hipMemcpyDeviceToHost, s));
            IRH_CHECK(hipStreamSynchronize(s));
            std::vector<int> order((size_t)nl);
            for (int q = 0; q < nl; q++) order[(size_t)q] = q;
            std::sort(order.begin(), order.end(),
                      [&](int a, int b) { return hl[(size_t)2 * kBcrMaxFar + a] < hl[(size_t)2 * kBcrMaxFar + b]; });
            for (int q : order) {  // edge order, as the host plan lists them
                g.bcr_far_i.push_back(hl[(size_t)q]);
                g.bcr_far_j.push_back(hl[(size_t)kBcrMaxFar + q]);
                g.bcr_far_e.push_back(hl[(size_t)2 * kBcrMaxFar + q]);
            }
        }
    }
    g.bcr_B = B;
}

}  // namespace irh
