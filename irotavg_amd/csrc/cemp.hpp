// cemp.hpp -- cycle-edge message passing over the triangles of the triangle test (irotavg_cycle_cemp,
// docs/cycle_check.md, "Corruption estimates"): the record of the triangle table, the walk of one entry of the shorter row
// that counts or stores the used triangles, the slot rule of one round, one term of the iteration, and a one-thread host
// form that runs the kernels' way. Plain C++ with no HIP type in it, as cycles.hpp: tools/cemp_host_check.cpp runs all of it
// under sanitizers on a machine without a device. k_cemp_walk and k_cemp_iter (cemp.hip) take every piece from here.
//
// Table: the used (finite) triangles of edge k are one contiguous segment of 16-byte records, in the order in which
// cycles_sorted visits them on ONE lane: ascending entry of the walked row, then ascending position in the run of equals.
#pragma once
#include "cycles.hpp"

namespace irh {

constexpr int CEMP_MAX_ITERS = 64;

struct alignas(16) CempRec {
    double d;         // the triangle error, finite
    uint32_t k1, k2;  // the two other edges: b -> c and c -> a
};

IRH_CYC_HD bool cemp_finite(double d) { return fabs(d) <= std::numeric_limits<double>::max(); }  // (NaN: false)

// What a lane keeps of one entry: how many used triangles it closes, and the first of them (a run of equals longer than
// one is rare: the others are stored by a second walk of the entry with CempStore).
struct CempHits {
    int n;
    CempRec first;
    IRH_CYC_HD void operator()(const CempRec &r) {
        if (n == 0) first = r;
        n++;
    }
};
// stores the records of one entry from `at` on, never at or behind `end`, and adds their errors to `sum` in that order
struct CempStore {
    CempRec *at;
    const CempRec *end;
    double sum;
    IRH_CYC_HD void operator()(const CempRec &r) {
        if (at < end) *at = r;
        at++;
        sum += r.d;
    }
};

// cyc_entry with a sink in place of the sums: every used triangle of entry i goes to sink(record), in run order
template <class Load, class Sink>
IRH_CYC_HD void cemp_entry(const uint64_t *keys, const uint32_t *vals, long long i, uint32_t y, bool x_is_b, long long l0,
                           long long l1, const CycQ q0, const Load &load, Sink &sink) {
    const uint32_t c = cyc_key_to(keys[i]);
    if (c == y) return;
    const uint64_t target = cyc_key(y, c);
    long long j = cyc_lower_bound(keys, l0, l1, target);
    if (j >= l1 || keys[j] != target) return;
    const uint32_t vx = vals[i], kx = cyc_val_edge(vx);
    const CycQ qx = cyc_directed(load(kx), x_is_b ? cyc_val_against(vx) : !cyc_val_against(vx));
    for (; j < l1 && keys[j] == target; j++) {
        const uint32_t vy = vals[j], ky = cyc_val_edge(vy);
        const CycQ qy = cyc_directed(load(ky), x_is_b ? !cyc_val_against(vy) : cyc_val_against(vy));
        const double d = x_is_b ? cyc_triangle_error(q0, qx, qy) : cyc_triangle_error(q0, qy, qx);
        if (cemp_finite(d)) sink(CempRec{d, x_is_b ? kx : ky, x_is_b ? ky : kx});
    }
}

// The slot rule of one round (the group's lanes hold G consecutive entries): a lane's records start behind the segment
// start, the records of the rounds done and those of the lower lanes of this round.
IRH_CYC_HD long long cemp_slot(long long seg, long long done, long long before) { return seg + done + before; }

// ---- one iteration ----------------------------------------------------------------------------------------------------------
IRH_CYC_HD double cemp_e(double s1, double s2) { return s1 + s2; }
IRH_CYC_HD void cemp_min(double &mu, double e) {  // a NaN is ignored: the comparison is false
    if (e < mu) mu = e;
}
struct CempSum {
    double num, den;
};
// w = exp(-beta (e - mu)); a NaN weight (a NaN estimate of either edge, or no finite e at all) leaves the term out
IRH_CYC_HD void cemp_term(CempSum &a, double d, double e, double beta, double mu) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double w = exp(-beta * (e - mu));
    if (w == w) {
        a.num += w * d;
        a.den += w;
    }
}
IRH_CYC_HD double cemp_quotient(const CempSum a) { return a.den > 0.0 ? a.num / a.den : std::numeric_limits<double>::quiet_NaN(); }
IRH_CYC_HD double cemp_mean(double sum, long long count) {
    return count > 0 ? sum / (double)count : std::numeric_limits<double>::quiet_NaN();
}

// ---- the host form ----------------------------------------------------------------------------------------------------------
struct CempResult {
    std::vector<CempRec> table;
    std::vector<long long> off;  // m + 1
    std::vector<double> s;
    std::vector<int32_t> used;
    long long summary[2] = {0, 0};
};

// the kernels' shuffle tree over the lanes of a group: lane 0 of v <- op(v, v of lane ^ o), o = G/2 .. 1
template <class T, class Op>
inline T cemp_tree(std::vector<T> v, const Op &op) {
    for (size_t o = v.size() / 2; o > 0; o >>= 1) {
        const std::vector<T> w = v;
        for (size_t l = 0; l < v.size(); l++) v[l] = op(w[l], w[l ^ o]);
    }
    return v[0];
}

// The kernels' way on one thread: emit, sort; per edge the shorter row in rounds of `group` entries, the records placed by
// the slot rule, the start vector from the lanes' sums; then `iters` Jacobi iterations, each lane over every group-th
// record of the segment. group: 1 or a power of two. I: m pairs, qq: m rows [x y z w], beta: iters doubles.
inline int cemp_sorted(int64_t m, int64_t n_total, const int32_t *I, const double *qq, int iters, const double *beta, int group,
                       CempResult &R) {
    for (int64_t k = 0; k < m; k++)
        if (!cyc_id_ok(I[2 * k], n_total) || !cyc_id_ok(I[2 * k + 1], n_total)) return CYC_BAD_ID;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    cyc_sorted_halves(m, n_total, I, keys, vals);
    const long long n2 = (long long)keys.size();
    const CycAosLoad load{qq};
    const size_t G = (size_t)group;
    const auto add = [](double a, double b) { return a + b; };
    R.table.clear();
    R.off.assign((size_t)m + 1, 0);
    R.s.assign((size_t)m, 0.0);
    R.used.assign((size_t)m, 0);
    R.summary[0] = R.summary[1] = 0;
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        std::vector<CempRec> seg;
        std::vector<double> lsum(G, 0.0);
        if (a != b) {
            long long a0, a1, b0, b1;
            cyc_row(keys.data(), n2, (uint32_t)a, a0, a1);
            cyc_row(keys.data(), n2, (uint32_t)b, b0, b1);
            const bool x_is_b = b1 - b0 <= a1 - a0;
            const long long s0 = x_is_b ? b0 : a0, s1 = x_is_b ? b1 : a1, l0 = x_is_b ? a0 : b0, l1 = x_is_b ? a1 : b1;
            const uint32_t y = (uint32_t)(x_is_b ? a : b);
            const CycQ q0 = load((uint32_t)k);
            long long done = 0;
            for (long long base = s0; base < s1; base += group) {
                std::vector<CempHits> h(G, CempHits{0, CempRec{0.0, 0u, 0u}});
                long long total = 0;
                for (size_t lane = 0; lane < G; lane++)
                    if (base + (long long)lane < s1) {
                        cemp_entry(keys.data(), vals.data(), base + (long long)lane, y, x_is_b, l0, l1, q0, load, h[lane]);
                        total += h[lane].n;
                    }
                seg.resize((size_t)(done + total), CempRec{0.0, 0u, 0u});
                long long before = 0;
                for (size_t lane = 0; lane < G; lane++) {
                    CempRec *const at = seg.data() + cemp_slot(0, done, before);
                    if (h[lane].n == 1) {
                        *at = h[lane].first;
                        lsum[lane] += h[lane].first.d;
                    } else if (h[lane].n > 1) {
                        CempStore w{at, seg.data() + seg.size(), lsum[lane]};
                        cemp_entry(keys.data(), vals.data(), base + (long long)lane, y, x_is_b, l0, l1, q0, load, w);
                        lsum[lane] = w.sum;
                    }
                    before += h[lane].n;
                }
                done += total;
            }
        }
        const long long count = (long long)seg.size();
        R.off[(size_t)k + 1] = R.off[(size_t)k] + count;
        R.table.insert(R.table.end(), seg.begin(), seg.end());
        R.s[(size_t)k] = cemp_mean(cemp_tree(lsum, add), count);
        R.used[(size_t)k] = cyc_stored_count(count);
        R.summary[0] += count;
        R.summary[1] += count == 0;
    }
    std::vector<double> next((size_t)m);
    for (int t = 0; t < iters; t++) {
        for (int64_t k = 0; k < m; k++) {
            const long long beg = R.off[(size_t)k], end = R.off[(size_t)k + 1];
            std::vector<double> mu(G, std::numeric_limits<double>::infinity());
            for (size_t lane = 0; lane < G; lane++)
                for (long long r = beg + (long long)lane; r < end; r += group)
                    cemp_min(mu[lane], cemp_e(R.s[R.table[(size_t)r].k1], R.s[R.table[(size_t)r].k2]));
            const double shift = cemp_tree(mu, [](double p, double q) { return q < p ? q : p; });
            std::vector<double> num(G), den(G);
            for (size_t lane = 0; lane < G; lane++) {
                CempSum acc{0.0, 0.0};
                for (long long r = beg + (long long)lane; r < end; r += group) {
                    const CempRec &rec = R.table[(size_t)r];
                    cemp_term(acc, rec.d, cemp_e(R.s[rec.k1], R.s[rec.k2]), beta[t], shift);
                }
                num[lane] = acc.num, den[lane] = acc.den;
            }
            next[(size_t)k] = cemp_quotient(CempSum{cemp_tree(num, add), cemp_tree(den, add)});
        }
        R.s.swap(next);
    }
    return CYC_OK;
}

}  // namespace irh
