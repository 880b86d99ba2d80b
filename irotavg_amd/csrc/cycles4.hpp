// cycles4.hpp -- the four-cycle test of relative rotations (irotavg_cycle_check4, docs/cycle_check.md "Four-cycles"): the
// quadrilateral error, the table of row bounds, the staged and the unstaged view of the searched row, the walk one lane
// does, and two host forms to hold the kernels against. Plain C++ with no HIP type in it, as cycles.hpp, on whose
// half-edge layout it stands: tools/cycles4_host_check.cpp runs all of it under sanitizers on a machine without a device.
// k_cyc_rows and k_cyc_quads (cycles4.hip) take every piece from here, so there is one copy of each.
//
// A quadrilateral of edge k = (a, b) is (k1, k2, k3): k1 joins b and c, k2 joins c and d, k3 joins d and a; a, b, c, d
// pairwise distinct. Rows hold no self loop, so c != d comes with k2; c and d outside {a, b} is tested. The wave of one
// edge walks the shorter of rows a and b (x) entry by entry, walks the row of every such entry, and looks each of its
// neighbours up in the other row (y):
//   x == b: entry b -> c is k1, row c gives k2 as c -> d, the hit in row a gives k3 as a -> d (turned);
//   x == a: entry a -> d is k3 (turned), row d gives k2 as d -> c (turned), the hit in row b gives k1 as b -> c.
#pragma once
#include "cycles.hpp"

namespace irh {

constexpr int CYC4_STAGE = 1024;  // entries of the searched row that one wave stages (8 bytes each)
constexpr int CYC4_WAVE = 64;

// D = q3 (x) (q2 (x) p), p = q(k1, b -> c) (x) q(k, a -> b): the one evaluation of a quadrilateral's error, whichever row
// a path walks and whether it keeps p in registers or not
IRH_CYC_HD double cyc_quad_error_from(const CycQ p, const CycQ q2, const CycQ q3) {
    return cyc_angle_error(cyc_qmul(q3, cyc_qmul(q2, p)));
}
// q0 = q(k, a -> b), q1 = q(k1, b -> c), q2 = q(k2, c -> d), q3 = q(k3, d -> a)
IRH_CYC_HD double cyc_quad_error(const CycQ q0, const CycQ q1, const CycQ q2, const CycQ q3) {
    return cyc_quad_error_from(cyc_qmul(q1, q0), q2, q3);
}

// the row of the TARGET view of sorted half-edge i, as positions among the n2 sorted keys (n2 < 2^31)
struct alignas(8) CycSpan {
    int32_t beg, end;
};
IRH_CYC_HD CycSpan cyc_target_row(const uint64_t *keys, long long n2, long long i) {
    CycSpan s;
    s.beg = s.end = 0;
    if (keys[i] == CYC_KEY_NONE) return s;  // a self loop: in no row, and no walk comes by
    long long beg, end;
    cyc_row(keys, n2, cyc_key_to(keys[i]), beg, end);
    s.beg = (int32_t)beg;
    s.end = (int32_t)end;
    return s;
}

// the searched row y, neighbours ascending: a copy of (neighbour, value) pairs, or the sorted half-edges themselves
struct CycRowStaged {
    const uint32_t *ent;  // 2 len words
    int len;
    IRH_CYC_HD uint32_t to(int t) const { return ent[2 * t]; }
    IRH_CYC_HD uint32_t val(int t) const { return ent[2 * t + 1]; }
};
struct CycRowGlobal {
    const uint64_t *keys;
    const uint32_t *vals;
    long long beg;
    int len;
    IRH_CYC_HD uint32_t to(int t) const { return cyc_key_to(keys[beg + t]); }
    IRH_CYC_HD uint32_t val(int t) const { return vals[beg + t]; }
};
// the first entry of y whose neighbour is not below w (len if none); 32 rounds end it whatever the row holds
template <class Row>
IRH_CYC_HD int cyc4_find(const Row &y, uint32_t w) {
    int lo = 0, hi = y.len;
    for (int round = 0; round < 32 && lo < hi; round++) {
        const int mid = lo + (hi - lo) / 2;
        if (y.to(mid) < w)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// What the four-cycle test does with a quadrilateral: the sums of one lane. The walk below hands every quadrilateral it
// closes to a sink as (d, k1, k2, k3); the message passing (cemp4.hpp) counts and stores them instead.
struct Cyc4Sums {
    CycAcc &acc;
    double threshold;
    IRH_CYC_HD void operator()(double d, uint32_t, uint32_t, uint32_t) { cyc_acc_add(acc, d, threshold); }
};

// Entry i of the walked row x: false when it is edge k itself or one parallel to it. Otherwise kx is its edge and qx the
// partial product: x == b: b -> c as k1 needs it, multiplied onto q0 once for the whole row of c; x == a: a -> d, and k3
// needs d -> a.
template <class Load>
IRH_CYC_HD bool cyc4_walked(const uint64_t *keys, const uint32_t *vals, long long i, uint32_t a, uint32_t b, bool x_is_b,
                            const CycQ q0, const Load &load, uint32_t &kx, CycQ &qx) {
    const uint32_t c = cyc_key_to(keys[i]);
    if (c == a || c == b) return false;
    const uint32_t vi = vals[i];
    kx = cyc_val_edge(vi);
    const CycQ qi = load(kx);
    qx = x_is_b ? cyc_qmul(cyc_directed(qi, cyc_val_against(vi)), q0) : cyc_directed(qi, !cyc_val_against(vi));
    return true;
}

// Entry j of the row of an x-entry (edge kx): its neighbour w (d when x == b, c when x == a) is looked up in y, and every
// entry of the run of equals there closes a quadrilateral, handed to sink(d, k1, k2, k3) in run order. qx: cyc4_walked's.
template <class Row, class Load, class Sink>
IRH_CYC_HD void cyc4_entry(const uint64_t *keys, const uint32_t *vals, long long j, uint32_t a, uint32_t b, bool x_is_b,
                           const Row &y, const CycQ q0, uint32_t kx, const CycQ qx, const Load &load, Sink &sink) {
    const uint32_t w = cyc_key_to(keys[j]);
    if (w == a || w == b) return;
    int t = cyc4_find(y, w);
    if (t >= y.len || y.to(t) != w) return;
    const uint32_t vj = vals[j], kj = cyc_val_edge(vj);
    // x == b: the entry runs c -> d as k2 needs it; x == a: it runs d -> c
    const CycQ q2 = cyc_directed(load(kj), x_is_b ? cyc_val_against(vj) : !cyc_val_against(vj));
    for (; t < y.len && y.to(t) == w; t++) {
        const uint32_t vy = y.val(t), ky = cyc_val_edge(vy);
        // x == b: the hit runs a -> d and k3 needs d -> a; x == a: it runs b -> c as k1 needs it
        const CycQ qy = cyc_directed(load(ky), x_is_b ? !cyc_val_against(vy) : cyc_val_against(vy));
        sink(x_is_b ? cyc_quad_error_from(qx, q2, qy) : cyc_quad_error(q0, qy, q2, qx), x_is_b ? kx : ky, kj, x_is_b ? ky : kx);
    }
}

// What lane `sl` of sub-group `sub` does for edge (a, b): of the walked row [x0, x1) the entries sub, sub + nsub, ...,
// and of each entry's row (rows: cyc_target_row of every sorted half-edge) the entries sl, sl + S, ...
template <class Row, class Load, class Sink>
IRH_CYC_HD void cyc4_lane(const uint64_t *keys, const uint32_t *vals, const CycSpan *rows, long long x0, long long x1, int sub,
                          int nsub, int sl, int S, uint32_t a, uint32_t b, bool x_is_b, const Row &y, const CycQ q0,
                          const Load &load, Sink &sink) {
    for (long long i = x0 + sub; i < x1; i += nsub) {
        uint32_t kx;
        CycQ qx;
        if (!cyc4_walked(keys, vals, i, a, b, x_is_b, q0, load, kx, qx)) continue;
        const CycSpan r = rows[i];
        for (long long j = (long long)r.beg + sl; j < r.end; j += S) cyc4_entry(keys, vals, j, a, b, x_is_b, y, q0, kx, qx, load, sink);
    }
}

// ---- host forms -------------------------------------------------------------------------------------------------------------
// entry t of the result belongs to edges[t] (edges == nullptr: all m edges in order, ne == m)
inline int cyc4_begin(int64_t m, int64_t n_total, const int32_t *I, int64_t ne, const int32_t *edges, CycResult &R) {
    for (int64_t k = 0; k < m; k++)
        if (!cyc_id_ok(I[2 * k], n_total) || !cyc_id_ok(I[2 * k + 1], n_total)) return CYC_BAD_ID;
    if (!edges && ne != m) return CYC_BAD_ID;
    for (int64_t t = 0; edges && t < ne; t++)
        if (edges[t] < 0 || edges[t] >= m) return CYC_BAD_ID;
    R.count.assign((size_t)ne, 0);
    R.ok.assign((size_t)ne, 0);
    R.mn.assign((size_t)ne, std::numeric_limits<double>::infinity());
    for (long long &s : R.summary) s = 0;
    return CYC_OK;
}

// The kernels' way on one thread: emit, sort, the table of row bounds, and per tested edge the two rows, the longer one
// staged unless it has more than stage_cap entries, the walk dealt to 64 / group sub-groups of `group` lanes (one
// sub-group when group >= 64) that each keep their own sums, merged at the end. I: m pairs, qq: m rows [x y z w].
inline int quads_sorted(int64_t m, int64_t n_total, const int32_t *I, const double *qq, double threshold, int64_t ne,
                        const int32_t *edges, int group, int stage_cap, CycResult &R) {
    if (cyc4_begin(m, n_total, I, ne, edges, R) != CYC_OK) return CYC_BAD_ID;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    cyc_sorted_halves(m, n_total, I, keys, vals);
    const long long n2 = (long long)keys.size();
    std::vector<CycSpan> rows(keys.size());
    for (long long i = 0; i < n2; i++) rows[(size_t)i] = cyc_target_row(keys.data(), n2, i);
    const CycAosLoad load{qq};
    const int nsub = group >= CYC4_WAVE ? 1 : CYC4_WAVE / group;
    std::vector<uint32_t> slab;
    for (int64_t t = 0; t < ne; t++) {
        const int64_t k = edges ? edges[t] : t;
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        CycAcc total = cyc_acc_zero();
        if (a != b) {
            long long a0, a1, b0, b1;
            cyc_row(keys.data(), n2, (uint32_t)a, a0, a1);
            cyc_row(keys.data(), n2, (uint32_t)b, b0, b1);
            const bool x_is_b = b1 - b0 <= a1 - a0;
            const long long x0 = x_is_b ? b0 : a0, x1 = x_is_b ? b1 : a1, y0 = x_is_b ? a0 : b0, y1 = x_is_b ? a1 : b1;
            const int ylen = (int)(y1 - y0);
            const CycQ q0 = load((uint32_t)k);
            const bool staged = ylen <= stage_cap;
            slab.clear();
            for (int p = 0; staged && p < ylen; p++) slab.push_back(cyc_key_to(keys[(size_t)(y0 + p)])), slab.push_back(vals[(size_t)(y0 + p)]);
            const CycRowStaged ys{slab.data(), ylen};
            const CycRowGlobal yg{keys.data(), vals.data(), y0, ylen};
            for (int sub = 0; sub < nsub; sub++)
                for (int sl = 0; sl < group; sl++) {
                    CycAcc acc = cyc_acc_zero();
                    Cyc4Sums sums{acc, threshold};
                    if (staged)
                        cyc4_lane(keys.data(), vals.data(), rows.data(), x0, x1, sub, nsub, sl, group, (uint32_t)a, (uint32_t)b,
                                  x_is_b, ys, q0, load, sums);
                    else
                        cyc4_lane(keys.data(), vals.data(), rows.data(), x0, x1, sub, nsub, sl, group, (uint32_t)a, (uint32_t)b,
                                  x_is_b, yg, q0, load, sums);
                    cyc_acc_merge(total, acc.count, acc.ok, acc.mn);
                }
        }
        cyc_store(R, (size_t)t, total);
    }
    return CYC_OK;
}

// The definition, literally and in sequence: for edge k = (a, b), every half-edge b -> c with c outside {a, b}, every
// half-edge c -> d with d outside {a, b, c}, and for each of them every edge that joins d and a.
inline int quads_reference(int64_t m, int64_t n_total, const int32_t *I, const double *qq, double threshold, int64_t ne,
                           const int32_t *edges, CycResult &R) {
    if (cyc4_begin(m, n_total, I, ne, edges, R) != CYC_OK) return CYC_BAD_ID;
    typedef std::pair<uint32_t, bool> Half;                           // edge, against its stored direction
    std::map<int32_t, std::vector<std::pair<int32_t, Half>>> out;      // view -> (neighbour, half-edge)
    std::map<std::pair<int32_t, int32_t>, std::vector<Half>> between;  // (u, v) -> the half-edges u -> v
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        if (a == b) continue;
        out[a].push_back({b, Half((uint32_t)k, false)});
        out[b].push_back({a, Half((uint32_t)k, true)});
        between[{a, b}].push_back(Half((uint32_t)k, false));
        between[{b, a}].push_back(Half((uint32_t)k, true));
    }
    const CycAosLoad load{qq};
    for (int64_t t = 0; t < ne; t++) {
        const int64_t k = edges ? edges[t] : t;
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        CycAcc acc = cyc_acc_zero();
        if (a != b)
            for (const std::pair<int32_t, Half> &e1 : out[b]) {
                const int32_t c = e1.first;
                if (c == a || c == b) continue;
                for (const std::pair<int32_t, Half> &e2 : out[c]) {
                    const int32_t d = e2.first;
                    if (d == a || d == b || d == c) continue;
                    const auto it = between.find({d, a});
                    if (it == between.end()) continue;
                    for (const Half &e3 : it->second)
                        cyc_acc_add(acc, cyc_quad_error(load((uint32_t)k), cyc_directed(load(e1.second.first), e1.second.second),
                                                        cyc_directed(load(e2.second.first), e2.second.second),
                                                        cyc_directed(load(e3.first), e3.second)), threshold);
                }
            }
        cyc_store(R, (size_t)t, acc);
    }
    return CYC_OK;
}

}  // namespace irh
