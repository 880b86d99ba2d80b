// marginals.hpp -- what the two uncertainty queries share (owner: marginals.hip; the other user: edgediag.hip).
#pragma once
#include <vector>

#include "graph.hpp"

namespace irh {

// s^2 of the handle's current rotations and weights (docs/rotation_variance.md); the residual planes it is formed from
// are the query's own (the handle's stay as they are) and are handed to the caller when er_keep is given
double residual_scale(Graph &g, double *num_out, double *cnt_out, DevBuf<double> *er_keep = nullptr);
int read_dead(Graph &g, const DevBuf<int> &dead);
// dense_invert_spd on a buffer of the query's own; the handle's dead-pivot scale of its live inverse is kept
void invert_own(Graph &g, double *A, int npad);

// The band factor of A_b with its selected inverse.
struct BandFactor {
    int B = 0, nb = 0, n = 0;
    DevBuf<double> D, U, Dinv, Ga, Gc, orig;  // D / U become SD / SU (Sigma blocks) in the downward sweep

    void factor(Graph &g, int *dead);
    void select(Graph &g);
    // Y (nb B rows x ld columns) <- A_b^-1 Y
    void solve(Graph &g, double *Y, int ld);
};

// The loop closures of non-zero weight behind the Woodbury correction: Z = A_b^-1 V (nrowsZ x ldZ, the rows past
// nrows zero), S^-1 (ldZ x ldZ, padding = identity), their rows (dcp: +1, dcq: -1).
struct BandClosures {
    int k = 0, ldZ = 64, nrows = 0, nrowsZ = 0;
    DevBuf<double> Z, S;
    DevBuf<int> dcp, dcq;
};
// F of the handle's band operator under its current weights + the closure set-up. IROTAVG_ERR_SOLVER: a dead pivot
// (band part or Woodbury system).
int band_setup(Graph &g, BandFactor &F, BandClosures &C, DevBuf<int> &dead);
// pv[t] = u' Sigma u, u = e_pi[t] - e_pj[t] (-1: no entry), 1024 columns per multi right-hand-side solve
void band_pairs(Graph &g, BandFactor &F, const BandClosures &C, const std::vector<int> &pi, const std::vector<int> &pj,
                std::vector<double> &pv);

// nu <= 2048: Sigma = diag(sc) M diag(sc), M (npad x npad) the inverse of the Jacobi-scaled operator; dvar = diag(Sigma)
struct DenseInverse {
    int n = 0, npad = 0;
    DevBuf<double> M, sc, dvar;
};
int dense_inverse(Graph &g, DenseInverse &Dn, DevBuf<int> &dead);

// edgediag.hip: irotavg_graph_edge_diagnostics (arguments checked by the caller; outputs written only on success).
// dev_out: the three arrays are DEVICE pointers (irotavg_graph_edge_diagnostics_dev); scale stays a host pointer
int edge_diagnostics(Graph &g, double *edge_var, double *leverage, double *chi2, double *scale, bool dev_out = false);

}  // namespace irh
