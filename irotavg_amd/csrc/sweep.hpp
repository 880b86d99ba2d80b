// sweep.hpp -- Weiszfeld sweeps over the sorted half-edges of the cycle tools (irotavg_weiszfeld, docs/local_sweeps.md):
// the prediction a neighbour makes for a view, one term of the view's sums (the residual, its length, the coefficient, the
// leave-out rule), the step, and a one-thread host form that runs the kernel's order. Plain C++ with no HIP type in it,
// as cemp.hpp: tools/sweep_host_check.cpp runs all of it under sanitizers on a machine without a device. k_sweep
// (sweep.hip) takes every piece from here, so there is one copy of each.
//
// One sweep is a Jacobi step. For a free view v the terms are the entries i of its row [b0, b1) of the sorted half-edges,
// in row order; entry i is the half-edge v -> u of edge k, its prediction is P = q(k, u -> v) (x) Q[u]. From y = Q[v],
// `inner` times: r_i = log(y* (x) P_i) wrapped into [-pi, pi) (edge_log), c_i = w[k] / max(|r_i|, floor) (L1) or w[k] (L2),
// x = sum c r / sum c, y <- y (x) exp(x) (step_quat, right-multiplied). The sums are added in ONE order for every group
// width G: lane l adds the terms l, l + G, ... in that order, and the lanes' sums go through the xor tree of sweep_tree.
#pragma once
#include "cycles.hpp"

namespace irh {

constexpr int SWEEP_MAX_SWEEPS = 1024;
constexpr int SWEEP_MAX_INNER = 16;
constexpr double SWEEP_EPS = 2.2204e-16;  // IRH_EPS (kernels.hpp)

IRH_CYC_HD bool sweep_finite(double v) { return fabs(v) <= std::numeric_limits<double>::max(); }  // (NaN: false)

// q(k, u -> v) (x) Q[u] for the row entry v -> u: the entry runs against u -> v, so the stored quaternion is turned when
// the entry runs ALONG the stored direction
IRH_CYC_HD CycQ sweep_prediction(const CycQ qq_k, bool entry_against, const CycQ qu) {
    return cyc_qmul(cyc_directed(qq_k, !entry_against), qu);
}
// entry i of a row: its prediction from the tables (loadqq(k): QQ_k, loadq(u): Q^t[u])
template <class LoadQQ, class LoadQ>
IRH_CYC_HD CycQ sweep_form(const uint64_t *keys, const uint32_t *vals, long long i, const LoadQQ &loadqq, const LoadQ &loadq) {
    const uint32_t val = vals[i];
    return sweep_prediction(loadqq(cyc_val_edge(val)), cyc_val_against(val), loadq(cyc_key_to(keys[i])));
}
IRH_CYC_HD double sweep_weight(const uint32_t *vals, long long i, const double *w) { return w ? w[cyc_val_edge(vals[i])] : 1.0; }

// edge_log (kernels.hpp) restated on the prediction: the log of y* (x) P, wrapped into [-pi, pi), zero when s < EPS
IRH_CYC_HD void sweep_residual(CycQ y, const CycQ P, double r[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    y.w = -y.w;
    const CycQ d = cyc_qmul(y, P);
    const double s = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    double th = 2.0 * atan2(s, d.w);
    if (th < -CYC_PI)
        th += 2.0 * CYC_PI;
    else if (th >= CYC_PI)
        th -= 2.0 * CYC_PI;
    const double aux = th / s;
    r[0] = d.x * aux;
    r[1] = d.y * aux;
    r[2] = d.z * aux;
    if (s < SWEEP_EPS) r[0] = r[1] = r[2] = 0.0;
}

struct SweepSum {
    double x, y, z, c;  // sum c r (three components), sum c
};
IRH_CYC_HD SweepSum sweep_zero() { return SweepSum{0.0, 0.0, 0.0, 0.0}; }
IRH_CYC_HD SweepSum sweep_add(const SweepSum a, const SweepSum b) { return SweepSum{a.x + b.x, a.y + b.y, a.z + b.z, a.c + b.c}; }
// One term. Left out of both sums: a residual with a component that is not finite, a weight that is not finite or <= 0.
IRH_CYC_HD void sweep_term(SweepSum &a, const CycQ y, const CycQ P, double wk, bool l1, double floor) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double r[3];
    sweep_residual(y, P, r);
    if (!sweep_finite(r[0]) || !sweep_finite(r[1]) || !sweep_finite(r[2]) || !sweep_finite(wk) || !(wk > 0.0)) return;
    double c = wk;
    if (l1) {
        const double rho = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        c = wk / (rho > floor ? rho : floor);
    }
    a.x += c * r[0];
    a.y += c * r[1];
    a.z += c * r[2];
    a.c += c;
}
// x = sum c r / sum c, zero when no term is left; returns |x|
IRH_CYC_HD double sweep_mean(const SweepSum a, double x[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool any = a.c > 0.0 || a.c != a.c;  // (every term that is kept adds c > 0; a NaN sum is not "no term")
    x[0] = any ? a.x / a.c : 0.0;
    x[1] = any ? a.y / a.c : 0.0;
    x[2] = any ? a.z / a.c : 0.0;
    return sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
}
// step_quat and step_apply (kernels.hpp) restated: y (x) exp(x), th = |x|; a step that is not finite leaves y alone
IRH_CYC_HD CycQ sweep_step(const CycQ y, const double x[3], double th) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double sn = sin(th / 2.0), cs = cos(th / 2.0), coef = sn / th;
    CycQ e{x[0] * coef, x[1] * coef, x[2] * coef, cs};
    if (!sweep_finite(e.x)) e.x = 0.0;
    if (!sweep_finite(e.y)) e.y = 0.0;
    if (!sweep_finite(e.z)) e.z = 0.0;
    if (!sweep_finite(e.w)) e.w = 0.0;
    const CycQ q = cyc_qmul(y, e);
    return sweep_finite(th) ? q : y;
}
// the running maximum of |x_0|; a NaN is ignored: the comparison is false
IRH_CYC_HD void sweep_max(double &mx, double th) {
    if (th > mx) mx = th;
}

// ---- the host form ----------------------------------------------------------------------------------------------------------
struct SweepResult {
    std::vector<double> step;    // sweeps
    long long info[2] = {0, 0};  // half-edges in rows of free views; free views with an empty row
};

// the kernel's shuffle tree over the lanes of a group: every lane <- v + v of lane ^ o, o = G/2 .. 1 (all lanes end equal)
inline SweepSum sweep_tree(std::vector<SweepSum> v) {
    for (size_t o = v.size() / 2; o > 0; o >>= 1) {
        const std::vector<SweepSum> u = v;
        for (size_t l = 0; l < v.size(); l++) v[l] = sweep_add(u[l], u[l ^ o]);
    }
    return v[0];
}

// The kernel's way on one thread: emit, sort, the row of every free view, then `sweeps` Jacobi steps; per view `group`
// lanes that each add every group-th term, the first `stage_cap` predictions of a row kept between the inner iterations
// (inner > 1), the others formed again. group: 1 or a power of two. I: m pairs, qq: m rows and Q: n_total rows [x y z w]
// (Q in and out), w: m doubles or nullptr.
inline int sweep_sorted(int64_t m, int64_t n_total, int f, const int32_t *I, const double *qq, double *Q, const double *w, bool l1,
                        int sweeps, int inner, double floor, int group, int stage_cap, SweepResult &R) {
    for (int64_t k = 0; k < m; k++)
        if (!cyc_id_ok(I[2 * k], n_total) || !cyc_id_ok(I[2 * k + 1], n_total)) return CYC_BAD_ID;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    cyc_sorted_halves(m, n_total, I, keys, vals);
    const long long n2 = (long long)keys.size();
    const size_t G = (size_t)group;
    R.step.assign((size_t)sweeps, 0.0);
    R.info[0] = R.info[1] = 0;
    std::vector<long long> b0((size_t)n_total, 0), b1((size_t)n_total, 0);
    for (int64_t v = f; v < n_total; v++) {
        cyc_row(keys.data(), n2, (uint32_t)v, b0[(size_t)v], b1[(size_t)v]);
        R.info[0] += b1[(size_t)v] - b0[(size_t)v];
        R.info[1] += b1[(size_t)v] == b0[(size_t)v];
    }
    std::vector<double> plane[2] = {std::vector<double>(Q, Q + 4 * n_total), std::vector<double>(Q, Q + 4 * n_total)};
    const CycAosLoad loadqq{qq};
    for (int t = 0; t < sweeps; t++) {
        const CycAosLoad loadq{plane[t & 1].data()};
        double *out = plane[(t + 1) & 1].data();
        for (int64_t v = f; v < n_total; v++) {
            const long long beg = b0[(size_t)v], len = b1[(size_t)v] - beg;
            CycQ y = loadq((uint32_t)v);
            std::vector<CycQ> slab((size_t)std::max(stage_cap, 1));
            for (int j = 0; j < inner; j++) {
                std::vector<SweepSum> lanes(G, sweep_zero());
                for (size_t lane = 0; lane < G; lane++)
                    for (long long idx = (long long)lane; idx < len; idx += group) {
                        const bool staged = inner > 1 && idx < stage_cap;
                        const CycQ P = staged && j > 0 ? slab[(size_t)idx] : sweep_form(keys.data(), vals.data(), beg + idx, loadqq, loadq);
                        if (staged && j == 0) slab[(size_t)idx] = P;
                        sweep_term(lanes[lane], y, P, sweep_weight(vals.data(), beg + idx, w), l1, floor);
                    }
                double x[3];
                const double th = sweep_mean(sweep_tree(lanes), x);
                if (j == 0) sweep_max(R.step[(size_t)t], th);
                y = sweep_step(y, x, th);
            }
            out[4 * v] = y.x, out[4 * v + 1] = y.y, out[4 * v + 2] = y.z, out[4 * v + 3] = y.w;
        }
    }
    for (int64_t v = f; v < n_total && sweeps > 0; v++)
        for (int c = 0; c < 4; c++) Q[4 * v + c] = plane[sweeps & 1][(size_t)(4 * v + c)];
    return CYC_OK;
}

}  // namespace irh
