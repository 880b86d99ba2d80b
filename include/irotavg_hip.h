/*
 * irotavg_hip.h -- C ABI of libirotavg_hip.so, the MI355X (gfx950) rotation-averaging core that
 * replaces the RAL library of ajparra/iRotAvg on the solve path.
 *
 * The reference has no FFI/plugin registry: its boundary is the C++ free-function API of
 * `namespace irotavg` in ral/l1_irls.hpp:81-112, called from ral/test.cpp:285-302 and
 * src/ViewGraph.cpp:1400-1417. Every entry point below names the reference interface it
 * replaces. include/irotavg/l1_irls.hpp is a header-only C++ shim with the reference's names on
 * top of this ABI; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Data layout (identical to the reference's Eigen types, ral/l1_irls.hpp:43-51):
 *   Mat  : column-major fp64, leading dimension ld >= rows; quaternion columns [x, y, z, w];
 *   I_t  : m pairs of int32 (first = i, second = j), 0-based; the first f rows of Q are fixed;
 *   Vec  : contiguous fp64.
 * All pointers in this header are HOST pointers unless a name ends in `_dev`.
 *
 * Error convention: the reference prints to stderr and calls exit(-1); this ABI returns one of
 * the negative codes below and never throws or exits. There is NO CPU fallback: if no HIP
 * device is usable every compute entry point returns IROTAVG_ERR_NO_DEVICE.
 *
 * Environment: the IROTAVG_* variables this header names (README.md lists all of them) are read when the
 * handle, the sharded handle or the view-graph is created -- once per call by the one-shot entry points -- and
 * hold for that object's life; IROTAVG_ONESHOT_CACHE and IROTAVG_POOL_LIMIT_MB are read once per process.
 */
#ifndef IROTAVG_HIP_H
#define IROTAVG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IROTAVG_OK 0
#define IROTAVG_ERR_BAD_ARG (-1)
#define IROTAVG_ERR_NOT_SPANNING (-2) /* ral/l1_irls.cpp:970-977 */
#define IROTAVG_ERR_SOLVER (-3)       /* ral/l1_irls.cpp:149-177 (UMFPACK failure) / PCG breakdown */
#define IROTAVG_ERR_UNKNOWN_COST (-4) /* ral/l1_irls.cpp:723-726 */
#define IROTAVG_ERR_NOMEM (-5)
#define IROTAVG_ERR_HIP (-6)
#define IROTAVG_ERR_NO_DEVICE (-7)
#define IROTAVG_ERR_NOT_CONVERGED (-8) /* inner PCG hit its iteration cap -- after irls has re-inverted a re-used
                                          coarse inverse and, on a single level of <= 1024 views, tried the dense
                                          Cholesky solve; the iterate reached so far is left in place */
#define IROTAVG_ERR_UNSUPPORTED (-9)  /* the query is not available on this kind of handle (irotavg_graph_rotation_variance,
                                         irotavg_graph_edge_diagnostics, the view-graph queries built on them) */

/* ral/l1_irls.hpp:56-57 -- the integer values are ABI */
enum irotavg_cost {
    IROTAVG_L2 = 0, IROTAVG_L1, IROTAVG_L15, IROTAVG_L05, IROTAVG_GEMAN_MCCLURE, IROTAVG_HUBER,
    IROTAVG_PSEUDO_HUBER, IROTAVG_ANDREWS, IROTAVG_BISQUARE, IROTAVG_CAUCHY, IROTAVG_FAIR,
    IROTAVG_LOGISTIC, IROTAVG_TALWAR, IROTAVG_WELSCH
};

/* Solver knobs that have no counterpart in the reference (it uses direct factorisations). */
typedef struct irotavg_options {
    double pcg_rtol;     /* stop when ||r||_2 <= pcg_rtol * ||b||_2 for every column; default 1e-10 */
    int pcg_max_iters;   /* default 2000 */
    int pcg_check_every; /* PCG iterations enqueued between host polls of the done flag; default 8 */
    int mg_levels_max;   /* cap on multigrid levels (1 = plain Jacobi-PCG); default 16 */
    int mg_agg0;         /* aggregate size of the finest level (0 = choose: 8, or the smallest power of two
                            that reaches the dense level) */
    int mg_agg;          /* aggregate size of the other levels (0 = choose; default) */
    int mg_dense_max;    /* coarsening stops at <= this many rows; that level is inverted densely
                            (blocked Gauss-Jordan on the GPU) and applied exactly; cap 2048;
                            0 (default) = chosen from the graph: 2048, or 1100 for a graph with
                            loop closures and <= 70k views (the sweep runs in most IRLS iterations) */
    double mg_omega;     /* damped-Jacobi factor; default 0.7 */
    double mg_kc;        /* coarse-correction scale (over-correction of the piecewise-constant aggregates);
                            0 (default) = choose: 2.0 for a graph without loop closures, 1.6 otherwise */
    int device;          /* HIP device ordinal; -1 = current device */
    int mg_multiplicative_top; /* 1: multiplicative V-cycle on level 0 (default 0: additive top level) */
    int dense_always_refresh;  /* 1: re-invert the dense coarse level at every solve (default 0: adaptive) */
    int no_window_kernel;      /* 1: irotavg_viewgraph_rot_avg never uses the single-kernel window path */
    int pcg_stall_accept;      /* a solve whose residual has stalled (not halved in 64 iterations: the
                                  attainable accuracy of an ill-conditioned system) is accepted if
                                  ||r||/||b|| <= 1e-6 (0, default) or <= 10^-k (k > 0); -1 = never: such
                                  a solve ends in IROTAVG_ERR_NOT_CONVERGED at pcg_max_iters */
    int no_fused_pspmv;        /* 1: no kernel fusion inside the PCG iteration (default 0: on one GPU the
                                  p-update runs inside the SpMV and, on graphs without loop closures, the
                                  level-1 down-sweep inside the update kernel) */
    int no_lowrank_repair;     /* 1: a non-uniformly changed coarse operator is always re-inverted (default 0:
                                  <= 64 deviating long-range entries are repaired by a low-rank update) */
    int pcg_classic;           /* 1: the PCG iteration always runs as separate launches (default 0: on one
                                  GPU a graph without loop closures runs it as two launches, cgcg.hip) */
    int band_direct;           /* a graph whose edges between free views all span <= 32 views -- a view sequence --
                                  except for at most 2048 long-range edges (loop closures) has a banded operator plus
                                  a low-rank part; its linear systems are then solved DIRECTLY -- on one GPU and on shards -- (block
                                  cyclic reduction + Woodbury correction, bcr.hip) instead of the PCG:
                                  0 (default) = when it has more than 2048 free views (smaller graphs are one
                                  dense level already), 1 = whenever the band allows, -1 = never */
    int inexact_outer;         /* 1: irls on the ITERATIVE solver solves the linear systems of its early iterations only as
                                  accurately as the outer iteration can use (round 5): while the last step was above
                                  50 x change_th the relative residual asked for is 0.01 change_th / last step (at most
                                  1e-4, never below pcg_rtol), i.e. the step is exact to ~1 % of change_th; the iterations
                                  near the fixed point -- the one that decides the stop and leaves the weights -- and the
                                  last one allowed are solved to pcg_rtol. 100k views / 2M edges with 2 % loop edges:
                                  27.8 -> 16.6 PCG iterations per solve, 13.4 -> 10.3 ms per irls, the same outer
                                  iterations, final rotations within 5e-8 rad (mean) of the all-exact run. 0 (default):
                                  every system to pcg_rtol, like the reference's QR (ral/l1_irls.cpp:536-556).
                                  IROTAVG_INEXACT=1 / 0 in the environment overrides the option. A direct solve
                                  (band_direct) has no tolerance and is not affected. */
} irotavg_options;

void irotavg_default_options(irotavg_options *opt);

/* Cumulative counters of a graph handle (since creation or the last reset). */
typedef struct irotavg_stats {
    int64_t pcg_solves;
    int64_t pcg_iters;       /* total PCG iterations over all solves */
    int64_t pcg_iters_last;  /* iterations of the most recent solve */
    int64_t outer_iters;     /* IRLS + L1RA outer iterations */
    int64_t edge_updates;    /* m * (IRLS outer iterations) */
    double seconds_irls;     /* wall seconds inside irotavg_graph_irls */
    double seconds_l1ra;
    int levels;              /* multigrid levels in use */
    int64_t level_rows[16];
    int64_t level_nnz[16];
    double last_relres[3];   /* ||r||/||b|| per column at the end of the last solve */
    int64_t pcg_stagnated;   /* solves accepted at a stalled residual above pcg_rtol (see pcg_stall_accept) */
    int64_t dense_inversions; /* full inversions of the dense coarse level */
    int64_t dense_repairs;    /* low-rank (Woodbury) repairs of that inverse instead of an inversion */
    int64_t pcg_handed_over;  /* solves whose single-reduction (Chronopoulos-Gear) recurrences stalled and that were
                                 repeated with the classic recurrences from the saved right-hand side */
    int64_t direct_solves;    /* linear systems solved by the banded direct solver (options.band_direct) */
    int64_t band;             /* half-bandwidth of the operator found at creation (-1: not looked at), and ... */
    int64_t band_block;       /* ... the block size of the direct solver (0: the solves run through the PCG) */
    int64_t direct_guarded;   /* direct solves with loop closures whose BAND part lost a pivot (a cost with exact-zero
                                 weights cut a view off its band neighbours while a closure may still hold it): repeated as a
                                 conjugate-gradient solve of the full operator preconditioned by the regularised direct solve */
    int64_t direct_dead_pivots; /* dead pivots of the band factor seen by the last such solve */
    int64_t direct_up_fallbacks; /* direct solves repeated level by level because a workgroup of the single-launch upper
                                    reduction gave up waiting for the others (another process held the device): the handle
                                    keeps the level-by-level launches from then on */
} irotavg_stats;

/* ---------------------------------------------------------------------------------------------
 * One-shot drop-ins: same arguments as the reference functions, host pointers in, host
 * pointers out. `A` of the reference signatures is derivable from (n, f, I) and is not passed.
 * ------------------------------------------------------------------------------------------ */

/* replaces irotavg::init_mst (ral/l1_irls.hpp:89, ral/l1_irls.cpp:915-979). Sequential sweep
 * semantics (result depends on edge order) -- runs on the host by design. */
int irotavg_init_mst(int64_t n, int64_t m, double *Q, int64_t ldq, const double *QQ,
                     int64_t ldqq, const int32_t *I, int f);

/* replaces irotavg::make_A (ral/l1_irls.hpp:91, ral/l1_irls.cpp:755-780): CSC arrays of the
 * m x (n-f) incidence matrix incl. the edge-drop quirk of :770-771. colptr: n-f+1 entries,
 * rowidx/vals: capacity 2m. Returns nnz or a negative error. */
int64_t irotavg_make_A(int n, int f, int64_t m, const int32_t *I, int64_t *colptr,
                       int64_t *rowidx, double *vals);

/* replaces irotavg::l1ra (ral/l1_irls.hpp:100-102, ral/l1_irls.cpp:851-912) */
int irotavg_l1ra(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ,
                 int64_t ldqq, double *Q, int64_t ldq, int max_iters, double change_th, int *iter,
                 double *runtime);

/* replaces irotavg::irls (ral/l1_irls.hpp:104-107, ral/l1_irls.cpp:559-752). `weights` must
 * hold m doubles. `runtime` is WALL seconds (the reference reports clock() CPU seconds). */
int irotavg_irls(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ,
                 int64_t ldqq, int cost, double sigma, double *Q, int64_t ldq, int max_iters,
                 double change_th, double *weights, int *iters, double *runtime);

/* replaces irotavg::quat_normalised (ral/l1_irls.hpp:112, ral/l1_irls.cpp:982-991) */
int irotavg_quat_normalised(int64_t n, double *Q, int64_t ldq, int f);

/* The reference's callers pass the SAME (I, QQ) to l1ra and then to irls (src/ViewGraph.cpp:1400-1417,
 * ral/test.cpp:295-301). irotavg_l1ra / irotavg_irls therefore KEEP the handle of their last call (one slot per
 * process): a following one-shot call with the same pointers, sizes and f whose content hashes equal (64 bits over every
 * word of I and of the four columns of QQ, computed from the caller's arrays on all host cores at every call -- an array
 * changed in place is a different graph) uploads Q only. A call in flight owns its handle (a concurrent call from another
 * thread builds its own); the kept handle holds device memory until irotavg_oneshot_cache_clear(), a call with another
 * graph, or process exit. irotavg_oneshot_cache(0) or IROTAVG_ONESHOT_CACHE=0 in the environment: every call builds and
 * destroys its handle as before round 5. */
void irotavg_oneshot_cache(int enable);
void irotavg_oneshot_cache_clear(void);
void irotavg_oneshot_cache_stats(int64_t *hits, int64_t *misses);

/* ---------------------------------------------------------------------------------------------
 * Handle API: the graph (edges, relative rotations, adjacency, multigrid hierarchy, work
 * vectors) stays resident in HBM across calls. One HIP stream per handle; a handle is not
 * thread-safe, distinct handles are independent.
 * ------------------------------------------------------------------------------------------ */
typedef struct irotavg_graph irotavg_graph;

/* Uploads I and QQ, builds the adjacency and the hierarchy. opt may be NULL. */
int irotavg_graph_create(irotavg_graph **g, int64_t m, int64_t n_total, int f, const int32_t *I,
                         const double *QQ, int64_t ldqq, const irotavg_options *opt);
void irotavg_graph_destroy(irotavg_graph *g);

int irotavg_graph_set_rotations(irotavg_graph *g, const double *Q, int64_t ldq); /* H2D, all n_total rows */
int irotavg_graph_get_rotations(irotavg_graph *g, double *Q, int64_t ldq);       /* D2H */
/* device-side snapshot / restore of the n_total rotations (e.g. to re-run a solve from the same
 * initial rotations without a host round trip) */
int irotavg_graph_snapshot_rotations(irotavg_graph *g);
int irotavg_graph_restore_rotations(irotavg_graph *g);
int irotavg_graph_get_weights(irotavg_graph *g, double *weights);                /* D2H, m */
int irotavg_graph_set_weights(irotavg_graph *g, const double *weights);          /* H2D, m */

/* irls / l1ra / quat_normalised on the resident graph (same semantics as the one-shot calls).
 * A handle on the banded direct solver that carries loop closures checks every closure solve against the FULL system
 * (relative residual options.pcg_rtol, 1e-10 by default; repaired by conjugate gradients with the direct solve as the preconditioner when it is
 * above). IROTAVG_ERR_SOLVER from irls then means: the band part alone is next to singular under the closures (robust
 * weights at their floor over whole stretches of a thin chain) and the repair stalled above 1e-8 -- the rotations are
 * what the last good iteration left; such a graph belongs to the iterative solver (options.band_direct = -1). The
 * one-shot irotavg_irls and irotavg_viewgraph_rot_avg repeat the call that way by themselves; the handle API and the
 * sharded handle (irotavg_dist_irls: the same check, by iterative refinement on the sharded operator) report it. */
int irotavg_graph_irls(irotavg_graph *g, int cost, double sigma, int max_iters, double change_th,
                       int *iters, double *runtime, double *score_trace /* may be NULL */);
int irotavg_graph_l1ra(irotavg_graph *g, int max_iters, double change_th, int *iter,
                       double *runtime, double *score_trace /* may be NULL */);
int irotavg_graph_quat_normalised(irotavg_graph *g);

int irotavg_graph_get_stats(irotavg_graph *g, irotavg_stats *out);
void irotavg_graph_reset_stats(irotavg_graph *g);
int irotavg_graph_synchronize(irotavg_graph *g);

/* ---------------------------------------------------------------------------------------------
 * Stage-level entry points on the resident graph (used by the parity tests, which check every
 * kernel against the oracle, and by bench.py's roofline leg).
 * ------------------------------------------------------------------------------------------ */

/* K1: r_k = log(Qinv_j (x) QQ_k (x) Q_i) for every edge (ral/l1_irls.cpp:109-127 + :498-532). */
int irotavg_graph_edge_residual(irotavg_graph *g);
/* K1 and K2 at a zero step in one pass over the edges: the residuals of the handle's current rotations go into the
 * residual planes (bit for bit what irotavg_graph_edge_residual leaves) and the weights become the cost's weights of those
 * residuals (all 14 costs; L2 and Huber inliers keep the handle's current value, as irotavg_graph_update_weights does).
 * "The uncertainty at these rotations" for irotavg_graph_rotation_variance / _edge_diagnostics without an irls. */
int irotavg_graph_pose_weights(irotavg_graph *g, int cost, double sigma);
/* D2H of the residual rows: out is m x 3 column-major, ld >= m. They are what the last irotavg_graph_edge_residual call
 * computed; irotavg_graph_irls / _l1ra use the planes as scratch and leave them unspecified (the residuals of the
 * rotations before OR after the last step, depending on the solver path). */
int irotavg_graph_get_residuals(irotavg_graph *g, double *out, int64_t ld);
/* one weighted least-squares solve with the current weights and residuals
 * (ral/l1_irls.cpp:596-612); X is n_u x 3 column-major (ld >= n_u), may be NULL. */
int irotavg_graph_ls_solve(irotavg_graph *g, double *X, int64_t ldx);
/* weight update from the current X and residuals (ral/l1_irls.cpp:614-727) */
int irotavg_graph_update_weights(irotavg_graph *g, int cost, double sigma);
/* score + exp map + Q update (ral/l1_irls.cpp:729-737); returns the score */
int irotavg_graph_apply_step(irotavg_graph *g, double *score);
/* one coordinate of the primal-dual LP (ral/l1_irls.cpp:228-468) on the resident graph:
 * y is a host vector of m entries, x receives n_u entries. */
int irotavg_graph_l1decode_pd(irotavg_graph *g, const double *y, int pdmaxiter, double *x,
                              int *stuck);

/* Times `reps` back-to-back launches of one kernel with HIP events on the handle's stream and
 * returns the mean milliseconds per launch. which: 1 = K1 edge_residual, 2 = K2 weight update
 * (Geman-McClure), 3 = matrix assembly (all levels, without the dense inversion), 4 = level-0 SpMV
 * (q = L p), 5 = one preconditioner application, 6 = so(3) step kernel (non-destructive variant),
 * 7 = dense coarse-level inversion (blocked Gauss-Jordan), 8 = the PCG p-update fused into the
 * level-0 SpMV (what a single-GPU solve of a graph without far entries runs instead of 4;
 * IROTAVG_ERR_BAD_ARG if this graph's PCG does not use it), 11 = K2 and the next iteration's K1 in one pass over the
 * edges (what the direct solver's irls loop runs from its second iteration on), 12 = K1 and the weights of a zero step in
 * one pass (irotavg_graph_pose_weights). */
int irotavg_graph_time_kernel(irotavg_graph *g, int which, int reps, double *ms_per_launch);

/* The banded direct solver of this handle (options.band_direct; irotavg_amd/csrc/bcr.hip): info[0] = block size (0: the
 * handle's systems run through the PCG -- nothing else is written), info[1] = levels L, then per level l < L three
 * values: blocks, chunks of eight blocks (= workgroups of its two launches), blocks that come from the level below
 * (fewer than `blocks` only on a mixed level 1, whose other blocks are level-0 blocks no chunk reduced); after the
 * levels the long-range edges (loop closures) the solver handles by its Woodbury correction, then 1 if the level-0
 * reduction of the handle's most recent assembly + solve (an IRLS iteration, irotavg_graph_ls_solve) assembled level 0
 * itself -- one launch instead of K3 and the reduction: a handle without closures whose chunks of eight blocks are whole
 * 64-row slices (blocks of 8 / 16 / 24 / 32), IROTAVG_BCR_NO_FUSED_ASM=1 not set -- and 0 if it did not. Three more
 * values follow, about the factor of the UNIT-WEIGHT operator: irls starts from weights of one, so the first system of
 * every irls call on a handle has the same operator, and a handle of three or more levels with blocks of 8 / 16 / 24 and
 * no closures keeps that factor from its first irls on (the first solve of every later call is a pass over the
 * right-hand sides alone, bit-identical to the full solve; IROTAVG_BCR_NO_UNIT_FACTOR=1: never kept;
 * irotavg_trim_memory releases it, the next irls rebuilds it): 1 if the handle holds a valid factor else 0, the solves
 * served from it so far, its bytes of device memory. which of
 * irotavg_graph_time_kernel: 19 = a whole solve (2 L launches, always the FULL reduction), 20 + l = the reduction of
 * level l, 40 + l = its way back; 17 = the right-hand-side-only solve over the kept unit-weight factor (all four
 * launches, level 0 assembling its slices as in irls), 18 = its upper launch alone -- both IROTAVG_ERR_BAD_ARG on a
 * handle without a valid factor. Returns the number of values written (<= cap) or a negative error. */
int irotavg_graph_direct_info(irotavg_graph *g, int64_t *info, int cap);

/* The direct solver has no tolerance and no residual test of its own (SuiteSparseQR / UMFPACK in ral/l1_irls.cpp:131-184,
 * 536-556 have none either). On demand: relres[c] = ||b - A x||_2 / ||b||_2 for the three coordinates of the handle's most
 * recent direct solve -- the level-0 operator as last assembled (loop closures included), its right-hand side, the
 * solution the last step was made from; one pass over level 0 and a host round trip, also stored in
 * irotavg_stats.last_relres. IROTAVG_ERR_BAD_ARG if the handle's systems do not run through the direct solver or none
 * has been solved yet. */
int irotavg_graph_direct_residual(irotavg_graph *g, double *relres);

/* Diagnostic: the right-hand-side part of ONE block elimination of the direct solver, run by one wave through the device
 * functions every reduction kernel uses for it (the small matrix-core products of irotavg_amd/csrc/bcr.hip, BcrRs), on
 * host arrays: Dinv (symmetric), P, Q are B x B row-major, R, WR, Ra, Rc are B x 3 row-major, B = 8 / 16 / 24 / 32
 * (any other: IROTAVG_ERR_BAD_ARG). On return WR = Dinv R; Rc = Rc - Q' WR unless hasQ = 0; Ra = Ra - P WR unless
 * hasP = 0 -- a skipped update leaves its array as it was. */
int irotavg_bcr_rhs_products(int B, const double *Dinv, const double *P, const double *Q, const double *R, int hasP,
                             int hasQ, double *WR, double *Ra, double *Rc);

/* Diagnostic: the wide matrix-core products of ONE block elimination of the direct solver, run by one workgroup of wpe
 * waves (the column tiles of W are dealt to them) through the device functions every reduction kernel uses (BcrElim in
 * irotavg_amd/csrc/bcr.hip), on host arrays, all row-major: Dinv (symmetric), P, Q, Dc, Da, fill are B x B, R is B x 3,
 * W is B x (2 B + 3). B = 24 with wpe = 1 / 2 / 4 or B = 8 with wpe = 1 / 2 -- the block sizes whose eight-row tile runs
 * as 4 x 4 x 4 products (any other: IROTAVG_ERR_BAD_ARG). On return W = Dinv [P' | Q | R] (the columns of P' are zero if
 * hasP = 0, those of Q if hasQ = 0); Dc = Dc - Q' W_Q unless hasQ = 0; Da = Da - P W_P and fill = -P W_Q unless
 * hasP = 0 -- then Da stays as it was and fill = P. */
int irotavg_bcr_block_products(int B, int wpe, const double *Dinv, const double *P, const double *Q, const double *R,
                               int hasP, int hasQ, double *Dc, double *Da, double *W, double *fill);

/* Uncertainty of the IRLS solution (docs/rotation_variance.md). M = A' diag(d^2) A with A = irotavg_make_A's
 * incidence (m x nu, nu = n_total - f) and d = the handle's current weights (irotavg_graph_get_weights), Sigma = M^-1:
 *   var[v]      = Sigma_{v-f, v-f} for a free view v, 0 for a fixed one (n_total entries; NULL: not asked for);
 *   pair_var[t] = u' Sigma u, u = e_i - e_j over the free ones of (pairs[2t], pairs[2t+1]) (0 for two fixed views, i == j);
 *   scale       = s^2 = sum_k d_k^2 |r_k|^2 / (3 (m_A - nu)) over the m_A edges with a nonzero row of A, r_k the edge
 *                 residuals of the current rotations (NaN when m_A <= nu). Covariance of view v's rotation vector under
 *                 the reference's linearisation: s^2 var[v] I_3; of log(R_j R_i') for a pair: s^2 pair_var I_3.
 * One factorisation serves both outputs. Routes: nu <= 2048 -- a dense inverse; the banded direct solver's handles
 * (stats.band_block > 0) -- block-tridiagonal selected inversion + Woodbury correction for the loop closures; any other
 * (multigrid-PCG) handle: pairs only (var == NULL), three pairs per solve of the handle's own PCG to pcg_rtol; var != NULL
 * there gives IROTAVG_ERR_UNSUPPORTED. Read-only: rotations, weights, residuals, stats and every later result of the
 * handle are as if the call had not run. Deterministic (bitwise). A singular M (a view that no weighted edge ties to a
 * fixed one: a pivot not above 1e-13 x its row's diagonal in M, or a PCG breakdown) gives IROTAVG_ERR_SOLVER (or the
 * PCG's IROTAVG_ERR_NOT_CONVERGED); outputs are written only on success. Out-of-range ids / npairs < 0:
 * IROTAVG_ERR_BAD_ARG before any device work. */
int irotavg_graph_rotation_variance(irotavg_graph *g, double *var /* n_total, or NULL */, int64_t npairs,
                                    const int32_t *pairs /* 2*npairs view ids */, double *pair_var /* npairs */,
                                    double *scale /* may be NULL */);
/* The same query without a handle (e.g. after irotavg_irls in src/ViewGraph.cpp:1400-1417): Q and weights are what
 * irls returned. Goes through the one-shot calls' kept handle (irotavg_oneshot_cache), so a call after irotavg_irls on
 * the same I, QQ does not rebuild. */
int irotavg_rotation_variance(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq,
                              const double *Q, int64_t ldq, const double *weights, double *var, int64_t npairs,
                              const int32_t *pairs, double *pair_var, double *scale);

/* Diagnostics of every measurement (docs/edge_diagnostics.md), with A, d, M, Sigma, r_k and s^2 as above and u_k = row k
 * of A. For every edge k < m:
 *   edge_var[k] = u_k' Sigma u_k (0 for a zero row of A: an edge whose second view is fixed);
 *   leverage[k] = d_k^2 edge_var[k], the diagonal of the hat matrix of the IRLS system: in [0, 1] up to rounding, summing
 *                 to nu; 1 - leverage is the edge's redundancy (0: an error in this measurement could never be seen);
 *   chi2[k]     = d_k^2 |r_k|^2 / (s^2 max(0, 1 - leverage[k])) in plain IEEE arithmetic (+inf for a residual on an edge
 *                 without redundancy, NaN for 0/0 and whenever s^2 is NaN); approximately chi-square with 3 degrees of
 *                 freedom under the reference's linearisation and Gaussian noise. Read leverage next to it.
 * Each array has m entries or is NULL (not computed, not copied); scale receives s^2 and may be NULL; nothing asked for:
 * IROTAVG_ERR_BAD_ARG before any device work. Routes: nu <= 2048 -- the dense inverse; the banded direct solver's handles
 * (stats.band_block > 0) -- gathers from the block-tridiagonal selected inverse, Woodbury-corrected for the loop closures;
 * any other (multigrid-PCG) handle: IROTAVG_ERR_UNSUPPORTED (irotavg_graph_rotation_variance's pairs serve a chosen
 * few there). Read-only, deterministic (bitwise), singular M -> IROTAVG_ERR_SOLVER, outputs written only on success:
 * all as irotavg_graph_rotation_variance. */
int irotavg_graph_edge_diagnostics(irotavg_graph *g, double *edge_var /* m or NULL */, double *leverage /* m or NULL */,
                                   double *chi2 /* m or NULL */, double *scale /* may be NULL */);
/* The same query without a handle, through the one-shot calls' kept handle (as irotavg_rotation_variance). */
int irotavg_edge_diagnostics(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq,
                             const double *Q, int64_t ldq, const double *weights, double *edge_var, double *leverage,
                             double *chi2, double *scale);

/* ---------------------------------------------------------------------------------------------
 * Device-pointer handle API (docs/device_api.md): the same handle, fed from and read into arrays that live in HBM
 * already -- no host round trip. Every DATA pointer below is a DEVICE pointer on the handle's device (`scale` alone is
 * a host pointer); `stream` is the caller's hipStream_t (NULL = the null stream).
 *
 * Ordering: on entry the handle's stream waits for an event recorded on `stream`; before returning, `stream` waits for
 * an event recorded on the handle's stream. The caller never needs a host synchronise before or after a call: inputs
 * may still be in flight on `stream`, outputs are ready for whatever is enqueued on `stream` next. The copy calls
 * (set / get) never block the host; create, the solves and the two queries read small results back and do.
 *
 * A strided matrix is (ptr, row_stride, col_stride) in ELEMENTS: element (k, c) lives at ptr[k * row_stride +
 * c * col_stride]; quaternion columns are [x, y, z, w]. Column-major planes are (1, ld), a contiguous (rows, 4) array
 * is (4, 1), strides may be negative. Accepted are exactly the stride pairs with
 *     rs != 0, cs != 0, and (|rs| >= cols * |cs|  or  |cs| >= rows * |rs|)
 * (rows that do not overlap, or columns that do not): anything else could alias and is IROTAVG_ERR_BAD_ARG, like a NULL
 * pointer, a pointer that is not 8-byte aligned, and a matrix whose lowest or highest element hipPointerGetAttributes
 * does not report as device memory of the handle's device. All of these are checked before any device work is enqueued.
 * ------------------------------------------------------------------------------------------ */

/* irotavg_graph_create from arrays on the device: I_dev = m pairs of int32 (8-byte aligned), QQ_dev = strided m x 4.
 * The handle is built on the device from the caller's arrays as they are (no relabelling; the build code of
 * IROTAVG_HOST_BUILD=0) and keeps its own copies: the caller's buffers are only read and are free again on return.
 * opt->device (or the current device) is the handle's device. An edge index outside [0, n_total) is found by the
 * build's first kernel: IROTAVG_ERR_BAD_ARG, *g stays NULL. No HIP device: IROTAVG_ERR_NO_DEVICE. init_mst has no
 * device form at handle size (window-size problems: irotavg_window_init_mst_batch_dev below); irotavg_init_tree_dev
 * below initialises on device arrays along another tree. Bring initial rotations with irotavg_graph_set_rotations_dev. */
int irotavg_graph_create_dev(irotavg_graph **g, int64_t m, int64_t n_total, int f, const int32_t *I_dev,
                             const double *QQ_dev, int64_t qq_rs, int64_t qq_cs, const irotavg_options *opt,
                             void *stream);
/* all n_total rows, strided n_total x 4 */
int irotavg_graph_set_rotations_dev(irotavg_graph *g, const double *Q_dev, int64_t rs, int64_t cs, void *stream);
int irotavg_graph_get_rotations_dev(irotavg_graph *g, double *Q_dev, int64_t rs, int64_t cs, void *stream);
/* m contiguous doubles */
int irotavg_graph_set_weights_dev(irotavg_graph *g, const double *w_dev, void *stream);
int irotavg_graph_get_weights_dev(irotavg_graph *g, double *w_dev, void *stream);
/* the m x 3 residuals of irotavg_graph_get_residuals, strided */
int irotavg_graph_get_residuals_dev(irotavg_graph *g, double *out_dev, int64_t rs, int64_t cs, void *stream);
/* irotavg_graph_rotation_variance's marginals (var_dev: n_total contiguous doubles, required) and scale (HOST, may be
 * NULL); pairs stay with the host call. Same routes, errors and read-only guarantee; var_dev is written only on success. */
int irotavg_graph_rotation_variance_dev(irotavg_graph *g, double *var_dev, double *scale, void *stream);
/* irotavg_graph_edge_diagnostics with the three arrays on the device (m contiguous doubles each, or NULL); scale is a
 * HOST pointer and may be NULL. Same definitions, routes, error codes and read-only guarantee; written only on success. */
int irotavg_graph_edge_diagnostics_dev(irotavg_graph *g, double *edge_var_dev, double *leverage_dev, double *chi2_dev,
                                       double *scale, void *stream);

/* Many small problems in one call, on arrays that live on the device (docs/window_batch.md): nb independent problems,
 * each l1ra(l1_iters) then irls(cost, sigma, irls_iters) as irotavg_window_solve runs them, one workgroup per problem.
 * Problem b has sizes[3b .. 3b+2] = (n_total, f, m) and must fit the window kernels (<= 64 free views, <= 320 views,
 * <= 640 edges). The problems are packed: problem b's edges are the rows sum_{a<b} m_a .. of I_dev / QQ_dev /
 * weights_dev, its views the rows sum_{a<b} n_total_a .. of Q_dev; the ids of I_dev are LOCAL to their problem
 * (0 .. n_total_b - 1). DATA pointers are DEVICE pointers on the calling thread's current device and follow the rules
 * above (strided matrices, 8-byte alignment, lowest / highest element); `sizes` and `results` are HOST pointers.
 *   kernel      0: per problem what irotavg_window_solve chooses, 1: the general LDS kernel for all, 2: the wave-resident
 *               kernel for all (a problem it does not take: IROTAVG_ERR_BAD_ARG)
 *   Q_dev       in and out; the rows of fixed views (< f of their problem) are never written
 *   weights_dev sum(m) contiguous doubles, or NULL
 *   results     4 per problem: status, l1ra iterations, irls iterations, kernel used (1 / 2); or NULL
 * IROTAVG_ERR_BAD_ARG before any device work: nb <= 0 or above 262144, NULL sizes, a problem with f outside
 * [0, n_total) or beyond the limits, kernel outside 0..2, a pointer / stride / alignment the rules refuse; a cost outside
 * the enum is IROTAVG_ERR_UNKNOWN_COST; no HIP device: IROTAVG_ERR_NO_DEVICE. The edge ids are read on the device alone:
 * the workgroup of a problem with an id outside [0, n_total) reports IROTAVG_ERR_BAD_ARG with zero iterations in
 * `results` and leaves that problem's rows of Q_dev and weights_dev as they are; the other problems are solved.
 * At most two launches go on `stream` itself; inputs may still be in flight there, Q_dev and weights_dev are ready for
 * whatever is enqueued on it next. The call blocks until every result record has arrived and returns the first
 * non-zero status in problem order. Results are bitwise those of irotavg_window_solve_kernel on each problem alone. */
int irotavg_window_solve_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev,
                                   int64_t qq_rs, int64_t qq_cs, double *Q_dev, int64_t q_rs, int64_t q_cs, int cost,
                                   double sigma, int l1_iters, int irls_iters, double change_th, double *weights_dev,
                                   int32_t *results, int kernel, void *stream);

/* irotavg_window_uncertainty for many small problems in one call, on arrays that live on the device
 * (docs/window_uncertainty_batch.md): one workgroup per problem, ONE launch. sizes, packing, limits, the stride rule,
 * alignment and the lowest / highest-element check are those of irotavg_window_solve_batch_dev, so the Q_dev and
 * weights_dev it leaves can be passed on as they are; Q_dev is only read.
 *   weights_dev  sum(m) contiguous doubles, or NULL for the weights of the poses (see irotavg_window_uncertainty)
 *   var_dev      sum(n_total) contiguous doubles or NULL; 0 for fixed views
 *   npairs       HOST, nb counts or NULL (no pairs); problem b's pairs are the rows sum_{a<b} npairs_a .. of pairs_dev
 *                (pairs of int32 view ids LOCAL to the problem, 8-byte aligned) and pair_var_dev
 *   edge_var_dev / leverage_dev / chi2_dev  sum(m) contiguous doubles each, or NULL
 *   scale        HOST, nb doubles or NULL; results: HOST, nb statuses or NULL
 * IROTAVG_ERR_BAD_ARG before any device work: what irotavg_window_solve_batch_dev refuses of nb, sizes, pointers, strides
 * and alignment, a negative pair count, pairs counted without both pair arrays, or nothing asked for (no output array, no
 * pairs, no scale); no HIP device: IROTAVG_ERR_NO_DEVICE. Edge and pair ids are read on the device alone: the workgroup
 * of a problem with an id outside [0, n_total) reports IROTAVG_ERR_BAD_ARG and indexes nothing with it; a singular
 * problem reports IROTAVG_ERR_SOLVER. A problem that fails leaves its rows of every output array, and its entry of
 * scale, exactly as they were; the other problems are computed. The launch goes on `stream` itself: inputs may still be
 * in flight there, outputs are ready for whatever is enqueued on it next. The call blocks until every result record has
 * arrived and returns the first non-zero status in problem order. Results are bitwise those of
 * irotavg_window_uncertainty on each problem alone. */
int irotavg_window_uncertainty_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev,
                                         int64_t qq_rs, int64_t qq_cs, const double *Q_dev, int64_t q_rs, int64_t q_cs,
                                         const double *weights_dev, double sigma, double *var_dev, const int32_t *npairs,
                                         const int32_t *pairs_dev, double *pair_var_dev, double *edge_var_dev,
                                         double *leverage_dev, double *chi2_dev, double *scale, int32_t *results,
                                         void *stream);

/* The closure gate for many small problems in one call, on arrays that live on the device (docs/window_gate_batch.md):
 * irotavg_window_gate on every problem, one workgroup per problem, ONE launch. nb .. sigma are exactly those of
 * irotavg_window_uncertainty_batch_dev (Q_dev is only read), so the Q_dev and weights_dev a batched solve leaves can be
 * passed on as they are.
 *   ncand        HOST, nb counts (each >= 0; no cap per problem); problem b's candidates are the rows
 *                sum_{a<b} ncand_a .. of cand_I_dev, cand_QQ_dev and the three outputs (offsets formed in 64 bits)
 *   cand_I_dev   sum(ncand) pairs of int32 view ids LOCAL to the problem, 8-byte aligned
 *   cand_QQ_dev  strided sum(ncand) x 4 (cq_rs, cq_cs): the stride rule above
 *   angle_dev / pair_var_dev / chi2_dev  sum(ncand) contiguous doubles each, or NULL
 *   scale        HOST, nb doubles or NULL; results: HOST, nb statuses or NULL
 * IROTAVG_ERR_BAD_ARG before any device work: what irotavg_window_uncertainty_batch_dev refuses of the shared arguments, a
 * negative count, candidates counted without both candidate arrays, a pointer / stride / alignment of the candidate
 * arrays the rules refuse, or nothing asked for (no candidates and no scale, or no output pointer at all); no HIP
 * device: IROTAVG_ERR_NO_DEVICE. Edge and candidate ids are read on the device alone: the workgroup of a problem with an
 * id outside [0, n_total), or a candidate with i == j, reports IROTAVG_ERR_BAD_ARG and indexes nothing with it; a
 * singular problem (also: a candidate pair_var that is not finite) reports IROTAVG_ERR_SOLVER. A problem that fails leaves
 * its rows of the three outputs, and its entry of scale, exactly as they were; the other problems are computed. The
 * launch goes on `stream` itself; the call blocks until every result record has arrived and returns the first non-zero
 * status in problem order. Results are bitwise those of irotavg_window_gate on each problem alone. */
int irotavg_window_gate_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev,
                                  int64_t qq_rs, int64_t qq_cs, const double *Q_dev, int64_t q_rs, int64_t q_cs,
                                  const double *weights_dev, double sigma, const int32_t *ncand, const int32_t *cand_I_dev,
                                  const double *cand_QQ_dev, int64_t cq_rs, int64_t cq_cs, double *angle_dev,
                                  double *pair_var_dev, double *chi2_dev, double *scale, int32_t *results, void *stream);

/* irotavg_init_mst for many small problems in one call, on arrays that live on the device (docs/window_init_batch.md):
 * the first link of init -> solve -> gate, one workgroup per problem, ONE launch. sizes, packing, limits, the stride
 * rule, alignment and the lowest / highest-element check are those of irotavg_window_solve_batch_dev, so the Q_dev this
 * call leaves can be passed on as it is.
 *   Q_dev       the rows of fixed views (< f of their problem) are read and never written; the rows of free views are
 *               written and never read, so they may be uninitialised (NaN included)
 *   results     HOST, nb statuses, or NULL
 * IROTAVG_ERR_BAD_ARG before any device work: what irotavg_window_solve_batch_dev refuses of nb, sizes, pointers, strides
 * and alignment, and a problem with f < 1 (irotavg_init_mst refuses f <= 0: view 0 is the anchor and must be fixed); no
 * HIP device: IROTAVG_ERR_NO_DEVICE. The edge ids are read on the device alone: the workgroup of a problem with an id
 * outside [0, n_total) reports IROTAVG_ERR_BAD_ARG and indexes nothing with it; a problem with a view no edge reaches
 * from view 0 reports IROTAVG_ERR_NOT_SPANNING (as on the host, a fixed view other than 0 counts as seen only once an
 * edge reaches it). A problem that fails keeps every byte of its rows of Q_dev -- irotavg_init_mst itself may have
 * written some of them before it fails --; the other problems are computed. The launch goes on `stream` itself: inputs
 * may still be in flight there, Q_dev is ready for whatever is enqueued on it next. The call blocks until every result
 * record has arrived and returns the first non-zero status in problem order. On success every problem's rows are
 * bitwise those irotavg_init_mst leaves on that problem alone. */
int irotavg_window_init_mst_batch_dev(int64_t nb, const int32_t *sizes, const int32_t *I_dev, const double *QQ_dev,
                                      int64_t qq_rs, int64_t qq_cs, double *Q_dev, int64_t q_rs, int64_t q_cs,
                                      int32_t *results, void *stream);

/* Cycle-consistency screening of relative rotations before any solve (docs/cycle_check.md): for every edge k = (a, b) the
 * triangles it closes with two other edges, (k1, k2) with k1 joining b and c, k2 joining c and a, c outside {a, b}, no
 * self loop among the three; parallel edges are distinct, every pair counts. The error of a triangle is the angle of
 * q(k2, c->a) (x) q(k1, b->c) (x) q(k, a->b), wrapped into [-pi, pi) as the edge residual is, in absolute value;
 * q(k, a_k->b_k) = QQ_k and q(k, b_k->a_k) is QQ_k with w negated. No poses, no weights, no fixed views, any topology.
 *   I           m pairs of ids in [0, n_total)
 *   QQ, ldqq    m x 4 column-major [x y z w], ldqq >= m; taken as given, not normalised
 *   threshold   radians, >= 0 (+inf accepted)
 *   tri_count   m int32 or NULL: triangles of edge k (a count above 2^31 - 1 is stored as 2^31 - 1)
 *   tri_ok      m int32 or NULL: those with error <= threshold
 *   tri_min     m doubles or NULL: the smallest error, +inf without a triangle
 *   summary     4 int64 on the HOST or NULL: sum of tri_count; edges with tri_ok >= 1; edges with tri_count >= 1 and
 *               tri_ok == 0; edges with tri_count == 0
 * A triangle whose error is not finite counts, is never ok and leaves tri_min alone. A self loop gets 0, 0, +inf.
 * IROTAVG_ERR_BAD_ARG before any device work: NULL I or QQ, m <= 0 or above 0x3fffffff, n_total <= 0 or above 0x7fffffff,
 * a threshold that is NaN or negative, ldqq < m. No HIP device: IROTAVG_ERR_NO_DEVICE. An id outside [0, n_total) is found
 * on the device before anything is indexed with it: IROTAVG_ERR_BAD_ARG. Outputs are written on success alone; with all
 * four NULL the call is the id check. Memory is O(m) whatever n_total is. Deterministic: two calls give the same bytes. */
int irotavg_cycle_check(int64_t m, int64_t n_total, const int32_t *I, const double *QQ, int64_t ldqq, double threshold,
                        int32_t *tri_count, int32_t *tri_ok, double *tri_min, int64_t summary[4]);
/* The same on arrays that live on the device: I_dev m pairs (8-byte aligned), QQ_dev a strided m x 4 matrix under the
 * stride rule above, tri_min_dev 8-byte and the count arrays 4-byte aligned, the lowest and highest element of every array
 * device memory of the current device (else IROTAVG_ERR_BAD_ARG, before any kernel). The kernels go on `stream` itself:
 * inputs may still be in flight there, the outputs are ready for whatever is enqueued on it next. The call blocks until
 * the error word and the summary are back. Bitwise the host call. */
int irotavg_cycle_check_dev(int64_t m, int64_t n_total, const int32_t *I_dev, const double *QQ_dev, int64_t qq_rs,
                            int64_t qq_cs, double threshold, int32_t *tri_count_dev, int32_t *tri_ok_dev,
                            double *tri_min_dev, int64_t summary[4] /* HOST */, void *stream);
/* Testing and measuring aid, NOT a stable interface (it may change or go without notice): the lanes that share one edge
 * in the triangle kernel, 8, 16, 32 or 64; 0 gives the default back. Process-wide. The results do not depend on it. Returns the width in force before the call, IROTAVG_ERR_BAD_ARG for any other value. */
int irotavg_cycle_check_group(int lanes);

/* An order-free spanning-tree initialiser, a second one next to irotavg_init_mst (docs/init_tree.md): the tree is the
 * minimum spanning forest under the keys (rank[k], k), ordered lexicographically -- distinct, so the forest is unique and
 * depends on no launch geometry; k alone decides between parallel and reversed duplicates. T(0) = Q[0];
 * T(b) = QQ_k (x) T(a) along a tree edge k = (a, b) walked from a, T(a) = QQ_k* (x) T(b) walked from b (QQ_k*: w negated).
 * Every free view v >= f gets Q[v] = +-T(v) up to rounding; the sign and the association of the products are not
 * specified. Computed on the device by Boruvka rounds, the rotations as labels of a union-find composed by pointer
 * jumping: the number of launches grows with log(n_total), not with the depth of the tree.
 *   I           m pairs of ids in [0, n_total); self loops are never used
 *   QQ, ldqq    m x 4 column-major [x y z w], ldqq >= m; taken as given, not normalised
 *   rank        m int32 or NULL (all zero); rank[k] < 0: edge k is never used
 *   Q, ldq      n_total x 4 column-major, ldq >= n_total: row 0 is read, the rows from f on are written and never read (they
 *               may hold NaN), rows 1 .. f-1 are neither read nor written (irotavg_init_mst re-anchors at a fixed view it
 *               passes; this call does not)
 *   in_tree     m int32 or NULL: 1 for a tree edge, 0 otherwise
 *   info        4 int64 on the HOST or NULL: Boruvka rounds run; components left (1: spanning); tree edges with rank > 0;
 *               the largest rank in the tree
 * IROTAVG_ERR_NOT_SPANNING unless the forest is one tree over all n_total views, fixed ones included; info is written then
 * too (the diagnosis), nothing else. IROTAVG_ERR_BAD_ARG before any device work: NULL I, QQ or Q, m <= 0 or above
 * 0x7fffffff, n_total <= 0 or above 0x7fffffff, f < 1 or f > n_total, ldqq < m, ldq < n_total. No HIP device:
 * IROTAVG_ERR_NO_DEVICE. An id outside [0, n_total) is found on the device before anything is indexed with it:
 * IROTAVG_ERR_BAD_ARG, every output byte untouched. Q and in_tree are written on success alone. Memory is O(n_total)
 * from the device pool. IROTAVG_ERR_SOLVER: a round or pass bound of the implementation was passed (an internal error that
 * no input should reach). Deterministic: two calls give the same bytes. */
int irotavg_init_tree(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq, const int32_t *rank,
                      double *Q, int64_t ldq, int32_t *in_tree, int64_t info[4]);
/* The same on arrays that live on the device: I_dev m pairs (8-byte aligned), QQ_dev and Q_dev strided m x 4 and
 * n_total x 4 matrices under the stride rule above (8-byte aligned), rank_dev and in_tree_dev 4-byte aligned, the lowest
 * and highest element of every array device memory of the current device (else IROTAVG_ERR_BAD_ARG, before any kernel).
 * The kernels go on `stream` itself: inputs may still be in flight there, the outputs are ready for whatever is enqueued
 * on it next. The call blocks until the status and info are back. Q is bitwise the host call's. */
int irotavg_init_tree_dev(int64_t m, int64_t n_total, int f, const int32_t *I_dev, const double *QQ_dev, int64_t qq_rs,
                          int64_t qq_cs, const int32_t *rank_dev, double *Q_dev, int64_t q_rs, int64_t q_cs,
                          int32_t *in_tree_dev, int64_t *info /* HOST */, void *stream);
/* Testing and measuring aid, NOT a stable interface: of the calling thread's most recent irotavg_init_tree[_dev], out[0] =
 * the kernels and fills it put on the stream, out[1] = the most pointer-jumping passes of one round that moved a pointer. */
void irotavg_init_tree_counters(int64_t out[2]);

/* Testing aid: fingerprint of the handle's static structure -- every index array the build produces (edge
 * streams, boundary slots, per level the SELL-64 pattern and the value-refresh maps) as one 64-bit FNV-1a hash
 * each, followed by the scalars that choose kernels (level shapes, far-entry count, fused-assembly / two-launch
 * flags, dense level size and bandwidth). The handle is built on the device (irotavg_amd/csrc/gbuild.hip) or,
 * with IROTAVG_HOST_BUILD=1, for shards and for small graphs, on the host (build.cpp): both must give the same
 * fingerprint (tests/test_gpu_build.py). Returns the number of values written (<= cap) or a negative error. */
int irotavg_graph_fingerprint(irotavg_graph *g, uint64_t *out, int cap);

/* ---------------------------------------------------------------------------------------------
 * View-graph side: OpenCV-free counterpart of ViewGraph / Pose (src/ViewGraph.hpp:54-75,
 * src/Pose.hpp:35-59). Rotations are row-major 3x3 doubles (cv::Matx33d layout). Connections
 * carry R_ij with R_j = R_ij R_i for the pair (i < j). The ORB / essential-matrix front-end that
 * produces them is not part of this library.
 * ------------------------------------------------------------------------------------------ */
typedef struct irotavg_viewgraph irotavg_viewgraph;

typedef struct irotavg_rotavg_info {
    int skipped;       /* 0 solved; 1 fewer than 2 views (:1270); 2 too few edges (:1313);
                          3 too few vertices (:1318); 4 no free view left */
    int n_views, n_edges, n_fixed;  /* size of the extracted sub-problem */
    int l1_iters, irls_iters;
    double l1_runtime, irls_runtime;
} irotavg_rotavg_info;

int irotavg_viewgraph_create(irotavg_viewgraph **vg, const irotavg_options *opt /* may be NULL */);
void irotavg_viewgraph_destroy(irotavg_viewgraph *vg);
/* appends a view with absolute rotation R (NULL = identity, Pose() default); returns its index,
 * which plays the role of frame().id() (ids only advance for admitted frames, src/IRotAvg.cpp:280-284) */
int irotavg_viewgraph_add_view(irotavg_viewgraph *vg, const double R[9]);
int irotavg_viewgraph_num_views(const irotavg_viewgraph *vg);
/* replaces View::connect (src/View.hpp:92, src/ViewGraph.cpp:1438-1455): returns 1 if the
 * connection was added, 0 if the pair was already connected. Rij is the rotation from view i to
 * view j (R_j = R_ij R_i); the pair is kept under (min, max), so a call with i > j stores Rij^T */
int irotavg_viewgraph_connect(irotavg_viewgraph *vg, int i, int j, const double Rij[9]);
/* replace ViewGraph::fixPose / isPoseFixed / countFixedPoses (src/ViewGraph.hpp:69-73) */
int irotavg_viewgraph_fix_pose(irotavg_viewgraph *vg, int idx, const double R[9]);
int irotavg_viewgraph_is_pose_fixed(const irotavg_viewgraph *vg, int idx);
int irotavg_viewgraph_count_fixed_poses(const irotavg_viewgraph *vg);
/* Pose::R() / Pose::setR() (src/Pose.hpp:47-51) */
int irotavg_viewgraph_get_pose(const irotavg_viewgraph *vg, int idx, double R[9]);
int irotavg_viewgraph_set_pose(irotavg_viewgraph *vg, int idx, const double R[9]);
/* replaces ViewGraph::rotAvg(int winSize) (src/ViewGraph.hpp:75, src/ViewGraph.cpp:1263-1435).
 * Sub-problems with <= 64 free views / <= 640 edges (every rotAvg(10) call) run as ONE kernel
 * launch (irotavg_amd/csrc/window.hip); larger ones through the graph handle path. */
int irotavg_viewgraph_rot_avg(irotavg_viewgraph *vg, int win_size, irotavg_rotavg_info *info);
/* Global re-solves (win_size >= the number of views: rotAvg(5000000) after a loop closure, src/IRotAvg.cpp:371-378) of a
 * graph with >= 20000 connections run on a DEVICE-RESIDENT, growing copy of the graph (irotavg_amd/csrc/resident.hip):
 * edge records, poses and the fixed mask stay in HBM between calls and a call sends only what changed since the last one
 * (views admitted, poses moved by sliding windows, new connections); results are bit-identical to extracting and
 * rebuilding the whole problem (IROTAVG_NO_RESIDENT=1 in the environment forces that).
 * irotavg_viewgraph_prepare runs that pipeline once on the graph as it is and drops the result (no pose changes): the
 * one-time costs of a process (device allocations, kernel code loads, streams) are then paid before the first loop
 * closure instead of inside it. Optional; IROTAVG_OK also when there is nothing to prepare. */
int irotavg_viewgraph_prepare(irotavg_viewgraph *vg);
/* The same for n DIFFERENT view-graphs at once (a server that tracks many sequences; the reference has one graph
 * per process, src/IRotAvg.cpp). The windows of different graphs are independent: those that fit the wave-resident
 * kernel (every rotAvg(10) of a sequence linked to <= 4 predecessors) are solved by ONE launch with a workgroup per
 * window -- one window alone keeps 1 of the 256 compute units busy --, the others run one by one. Results are
 * those of n separate irotavg_viewgraph_rot_avg calls. infos: n entries or NULL. Returns the first error. */
int irotavg_viewgraph_rot_avg_batch(irotavg_viewgraph *const *vgs, int n, int win_size, irotavg_rotavg_info *infos);

/* Uncertainty queries on the view-graph (docs/viewgraph_uncertainty.md). All three are defined on the problem
 * irotavg_viewgraph_rot_avg(win_size) would solve NOW -- the same connections in the same order, the touched views
 * relabelled fixed-first, a global problem when win_size >= the number of views -- at the current poses, with the weights
 * d_k = 1 / (|r_k|^2 + sigma^2) (Geman-McClure, sigma = 5 degrees: rot_avg's cost at a zero step), and M, Sigma, s^2,
 * edge_var, leverage, chi2 as irotavg_graph_rotation_variance / irotavg_graph_edge_diagnostics define them. None moves a
 * pose; the answers depend on the view-graph's state alone (poses, connections, fixed mask). A problem without a fixed
 * pose holds its row 0 at the pose it has (rot_avg would hold it at the identity). Where rot_avg would skip: IROTAVG_OK,
 * info->skipped set, every output NaN (conn: -1). Window-size problems (<= 64 free views, <= 640 edges, <= 320 views) run
 * as ONE kernel launch (irotavg_amd/csrc/wincov.hip), larger ones through a graph handle -- built on the device from
 * rot_avg's resident records where a global re-solve would run there, with the same delta upload -- and the handle queries (their
 * routes and errors: IROTAVG_ERR_UNSUPPORTED for var / edge diagnostics on a multigrid-PCG graph, IROTAVG_ERR_SOLVER for a
 * singular M, outputs untouched). Bad ids / counts: IROTAVG_ERR_BAD_ARG before any device work. */
typedef struct irotavg_uncertainty_info {
    int skipped, n_views, n_edges, n_fixed; /* as irotavg_rotavg_info */
    int route;                              /* 1 window kernel, 2 dense inverse, 3 banded direct solver, 4 PCG (pairs only) */
    int closures;                           /* loop closures the band route carried */
    double scale;                           /* s^2 */
} irotavg_uncertainty_info;
/* var[v] (num_views entries, caller's view ids, or NULL): Sigma's entry of a free view of the problem, 0 for a view the
 * problem holds (fixed, or outside the window), NaN for a view that is not in the problem. pair_var[t] = u' Sigma u for
 * (pairs[2t], pairs[2t+1]): 0 when both are held, NaN when either is absent. */
int irotavg_viewgraph_rotation_variance(irotavg_viewgraph *vg, int win_size, double *var, int64_t npairs,
                                        const int32_t *pairs, double *pair_var, irotavg_uncertainty_info *info /* may be NULL */);
/* edges of that problem (0 where rot_avg would skip), or a negative error */
int64_t irotavg_viewgraph_num_connections(irotavg_viewgraph *vg, int win_size);
/* conn: 2*cap view ids (i, j) of the problem's edges in problem order, edge_var / leverage / chi2: cap each; any may be
 * NULL. Returns the number of edges, or a negative error (cap too small: IROTAVG_ERR_BAD_ARG). */
int64_t irotavg_viewgraph_edge_diagnostics(irotavg_viewgraph *vg, int win_size, int64_t cap, int32_t *conn,
                                           double *edge_var, double *leverage, double *chi2,
                                           irotavg_uncertainty_info *info /* may be NULL */);
/* The statistical gate in front of irotavg_viewgraph_connect: each candidate (pairs[2c], pairs[2c+1], Rij + 9c, as connect
 * takes them; i != j) is a new, independent measurement, also when the pair is connected already; nothing is added to
 * the graph. angle[c] = |r_c|, K1's residual of the candidate at the current poses (rad); pair_var[c] as above;
 * chi2[c] = |r_c|^2 / (s^2 (pair_var[c] + sigma^4)), approximately chi-square with 3 degrees of freedom (sigma^4 = 1 / d0^2,
 * d0 = 1 / sigma^2 the weight a zero-residual measurement gets); NaN when s^2 is NaN or a view is not in the problem.
 * ncand entries each, or NULL. */
int irotavg_viewgraph_gate_connections(irotavg_viewgraph *vg, int win_size, int64_t ncand, const int32_t *pairs,
                                       const double *Rij, double *angle, double *pair_var, double *chi2,
                                       irotavg_uncertainty_info *info /* may be NULL */);

/* rmat2quat (src/ViewGraph.cpp:1175-1203) / q.normalized().toRotationMatrix() (:1426-1433);
 * row-major R, q = [x y z w] */
void irotavg_rmat2quat(const double R[9], double q[4]);
void irotavg_quat2rmat(const double q[4], double R[9]);
/* replaces ViewGraph::savePoses (src/ViewGraph.hpp:64, src/ViewGraph.cpp:1206-1231): lines
 * `id \t qw \t qx \t qy \t qz \t tx \t ty \t tz`; t = 3 doubles per view or NULL (zeros) */
int irotavg_viewgraph_save_poses(const irotavg_viewgraph *vg, const char *filename, const double *t);

/* The single-kernel window pipeline on caller data (layout as irotavg_l1ra / irotavg_irls):
 * l1ra(l1_iters) then irls(cost, sigma, irls_iters), change_th for both, in one launch.
 * IROTAVG_ERR_BAD_ARG if the problem does not fit the kernel's limits. */
int irotavg_window_solve(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ,
                         int64_t ldqq, double *Q, int64_t ldq, int cost, double sigma, int l1_iters,
                         int irls_iters, double change_th, double *weights, int *l1_out, int *irls_out);
/* Same with an explicit kernel choice: 0 = automatic (what irotavg_window_solve and rot_avg do),
 * 1 = the general LDS kernel (<= 64 free views, <= 640 edges, <= 320 views), 2 = the wave-resident
 * kernel for the usual rotAvg(10) size (<= 16 free views, <= 64 edges; BAD_ARG beyond). */
int irotavg_window_solve_kernel(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ,
                                int64_t ldqq, double *Q, int64_t ldq, int cost, double sigma,
                                int l1_iters, int irls_iters, double change_th, double *weights,
                                int *l1_out, int *irls_out, int kernel);

/* The uncertainty of one window-size problem on caller data (layout as irotavg_window_solve; host pointers), no handle:
 * one kernel launch (irotavg_amd/csrc/wincov.hip, docs/window_uncertainty_batch.md). Sigma = (A' diag(d^2) A)^-1 with
 *   weights != NULL  d_k = weights[k], as irotavg_irls / irotavg_window_solve return them (sigma unused);
 *   weights == NULL  d_k = 1 / (|r_k|^2 + sigma^2), the Geman-McClure weight of the poses Q at a zero step: what the
 *                    view-graph queries use.
 * Residuals r_k are K1's at Q either way (scale and chi2 need them). Outputs, each optional:
 *   var       n_total entries, 0 for the fixed views, as irotavg_graph_rotation_variance
 *   pair_var  npairs entries, u' Sigma u of (pairs[2t], pairs[2t+1]) (view ids of the problem): 0 when i == j or both
 *             are fixed
 *   edge_var / leverage / chi2  m entries each, scale: as irotavg_graph_edge_diagnostics defines them
 * IROTAVG_ERR_BAD_ARG before any device work: a problem beyond the limits of irotavg_window_solve, f outside
 * [0, n_total), an edge or pair id outside [0, n_total), npairs < 0, npairs > 0 without both pair arrays, or nothing
 * asked for (no output pointer and no pairs). IROTAVG_ERR_SOLVER: A' diag(d^2) A is singular. In both cases no output
 * is written. Results are deterministic: two identical calls are bitwise equal. */
int irotavg_window_uncertainty(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq,
                               const double *Q, int64_t ldq, const double *weights /* m or NULL */, double sigma,
                               double *var /* n_total or NULL */, int64_t npairs, const int32_t *pairs, double *pair_var,
                               double *edge_var, double *leverage, double *chi2 /* m each or NULL */, double *scale);

/* The closure gate of one window-size problem on caller data (layout and weights as irotavg_window_uncertainty; host
 * pointers), no handle (docs/window_gate_batch.md). A candidate is a row one could append to I / QQ: view ids (i, j) =
 * (cand_I[2c], cand_I[2c+1]) of the problem and the quaternion [x y z w] in row c of cand_QQ (column-major, leading
 * dimension ldcq), read exactly as an edge row is read. It is a new, independent measurement, also when the pair has an
 * edge already; nothing is added to the problem.
 *   angle[c]     |r_c|, r_c = K1's residual of the candidate at Q
 *   pair_var[c]  u' Sigma u, u = e_j - e_i; a fixed view (< f) contributes no coefficient, both fixed: 0
 *   chi2[c]      |r_c|^2 / (s^2 (pair_var[c] + sigma^4)), s^2 the scale of irotavg_window_uncertainty, sigma the argument in
 *                both weight modes; NaN when s^2 is NaN (angle and pair_var are still given)
 * ncand entries each, or NULL; scale: one double or NULL. IROTAVG_ERR_BAD_ARG before any device work: what
 * irotavg_window_uncertainty refuses of the problem, ncand < 0, ncand > 0 without cand_I / cand_QQ (or ldcq < ncand), a
 * candidate id outside [0, n_total) or i == j, or nothing asked for (no candidates and no scale, or no output pointer at
 * all). IROTAVG_ERR_SOLVER: A' diag(d^2) A is singular. In both cases no output is written. More than 256 candidates take
 * further launches of the same kernel; the candidates are staged on the host first (96 bytes each), so a count that memory
 * cannot hold ends as IROTAVG_ERR_NOMEM. Two identical calls are bitwise equal. */
int irotavg_window_gate(int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq, const double *Q,
                        int64_t ldq, const double *weights /* m or NULL */, double sigma, int64_t ncand,
                        const int32_t *cand_I, const double *cand_QQ, int64_t ldcq, double *angle, double *pair_var,
                        double *chi2 /* ncand each or NULL */, double *scale);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: the IRLS solve sharded by contiguous ranges of free views; one
 * process per GPU, RCCL over xGMI for the halo exchanges and the scalar all-reduces. Every
 * process passes the SAME global graph; each keeps its shard. Bootstrap: rank 0 calls
 * irotavg_dist_unique_id and broadcasts the 128 bytes (e.g. with torch.distributed), then every
 * rank calls irotavg_dist_create(world, rank, id, ...). With unique_id128 == NULL the handle holds
 * ALL `world` shards in this process on the current GPU and exchanges through an in-process
 * loopback (no RCCL): the sharded algebra can then be checked on a single GPU.
 * ------------------------------------------------------------------------------------------ */
typedef struct irotavg_dist irotavg_dist;
/* A host-staged wire for the sharded solve: the library stages device data through host buffers and
 * calls back into the application, which moves the bytes with whatever it has (e.g.
 * torch.distributed over gloo). One process = one shard, as with RCCL. Used where RCCL cannot run
 * (two ranks on ONE GPU in the multi-process test, tests/test_gpu_dist_mp.py) -- the control flow of
 * the sharded path is the same, only the wire differs. Both callbacks return 0 on success. */
typedef struct irotavg_transport {
    void *ctx;
    /* in-place reduction of n doubles over all ranks; op: 0 sum, 1 min, 2 max */
    int (*allreduce)(void *ctx, double *buf, int n, int op);
    /* one point-to-point round: for q < npeers send send_cnt[q] doubles from send + send_off[q] to rank
     * peers[q] and receive recv_cnt[q] doubles from it into recv + recv_off[q] */
    int (*exchange)(void *ctx, int npeers, const int *peers, const double *send, const int64_t *send_off,
                    const int64_t *send_cnt, double *recv, const int64_t *recv_off, const int64_t *recv_cnt);
} irotavg_transport;
int irotavg_dist_unique_id(void *out128);
int irotavg_dist_create(irotavg_dist **d, int world, int rank, const void *unique_id128, int64_t m,
                        int64_t n_total, int f, const int32_t *I, const double *QQ, int64_t ldqq,
                        const irotavg_options *opt);
int irotavg_dist_create_hosted(irotavg_dist **d, int world, int rank, const irotavg_transport *transport,
                               int64_t m, int64_t n_total, int f, const int32_t *I, const double *QQ,
                               int64_t ldqq, const irotavg_options *opt);
void irotavg_dist_destroy(irotavg_dist *d);
int irotavg_dist_set_rotations(irotavg_dist *d, const double *Q, int64_t ldq); /* GLOBAL n_total x 4 */
int irotavg_dist_get_rotations(irotavg_dist *d, double *Q, int64_t ldq); /* writes the rows this process owns */
/* device-side snapshot / restore of the local shards' rotations (as irotavg_graph_snapshot_rotations) */
int irotavg_dist_snapshot_rotations(irotavg_dist *d);
int irotavg_dist_restore_rotations(irotavg_dist *d);
int irotavg_dist_get_weights(irotavg_dist *d, double *weights);          /* writes its local edges */
int irotavg_dist_irls(irotavg_dist *d, int cost, double sigma, int max_iters, double change_th,
                      int *iters, double *runtime, double *score_trace);
/* replaces irotavg::l1ra (ral/l1_irls.hpp:100-102) on the sharded graph: the callers run l1ra THEN
 * irls (src/ViewGraph.cpp:1400-1417, ral/test.cpp:295-301) */
int irotavg_dist_l1ra(irotavg_dist *d, int max_iters, double change_th, int *iters, double *runtime,
                      double *score_trace);
int irotavg_dist_get_stats(irotavg_dist *d, irotavg_stats *out);
/* What the sharded handle actually runs on, so that a scaling run can be checked: info[0] = wire
 * (0 loopback: all shards in this process, 1 RCCL, 2 the caller's host-staged transport) + 16 when the halo of a
 * closure-free sharded sequence travels as ONE all-gather of a fixed boundary record per rank instead of point-to-point
 * messages between neighbours (round 6; RCCL and loopback), info[1] = ranks of
 * the RCCL communicator as RCCL reports them (ncclCommCount; 0 without one), info[2] = shards held by this
 * process, info[3] = world size the graph is partitioned for, info[4] = ghost views of this process's
 * shards (halo rows received per exchange), info[5] = peers of shard 0, info[6] = block size of the sharded direct
 * solver (a view sequence, also with up to 2048 loop closures: every rank reduces its range of the banded operator to
 * its last block, one gather, the `world` separators solved by every rank; 0: the sharded PCG), info[7] = the loop
 * closures that solver carries (Woodbury correction across the ranks: besides the gather the ranks SUM one buffer of
 * r x world x B + r^2 + 4 r doubles per linear solve). */
int irotavg_dist_info(irotavg_dist *d, int64_t info[8]);
/* Diagnostic of a first multi-GPU run -- where an IRLS iteration of the sharded handle spends its time. enable != 0:
 * clear the counters and switch the phase clock ON for the following irotavg_dist_irls calls (the stream is drained at
 * every phase boundary: such calls are slower than undisturbed ones, never time them); enable == 0: switch it off. Either
 * way the means collected so far are returned first: us_per_iteration[0] local edge kernels + assembly, [1] local
 * reductions (closures' forward eliminations; the whole solve on the sharded PCG), [2] gather of the separators, [3] sum
 * of the closures' buffer, [4] separator system + corrections + ways back, [5] halo of the step, [6] weights + rotation
 * update, [7] score all-reduce; *iterations = IRLS iterations they are means over. Either pointer may be NULL. */
int irotavg_dist_timing(irotavg_dist *d, int enable, double us_per_iteration[8], int64_t *iterations);
int irotavg_dist_plan(irotavg_dist *d, int local_index, int64_t counts[6], int *peers, int *send_cnt,
                      int *recv_cnt, int cap);
/* host-only partition plan of one rank (no GPU): see irotavg_amd/csrc/dist.hip */
int irotavg_dist_plan_host(int world, int rank, int64_t m, int64_t n_total, int f, const int32_t *I,
                           int64_t counts[6], int32_t *ghosts_out, int64_t ghosts_cap,
                           int32_t *send_out, int64_t send_cap, int32_t *edges_out, int64_t edges_cap,
                           int *peers, int *send_cnt, int *recv_cnt, int peers_cap);

/* library / device info */
const char *irotavg_version(void);
int irotavg_device_count(void);
/* Handles draw their device buffers from a per-device cache so that create/destroy cycles (the
 * one-shot calls, rot_avg's global re-solves) do not pay hipMalloc/hipFree each time. This returns
 * the cached blocks to the driver; result = bytes released. IROTAVG_POOL_LIMIT_MB (environment)
 * bounds the cache (default 16384; 0 = no caching). */
int64_t irotavg_trim_memory(void);
const char *irotavg_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif /* IROTAVG_HIP_H */
