// cemp4.hpp -- cycle-edge message passing over the quadrilaterals of the edges listed (irotavg_cycle_cemp4,
// docs/cycle_check.md, "Corruption estimates over four-cycles"): the record of the quadrilateral table, the sinks that
// count and store the used quadrilaterals of one entry of the four-cycle walk (cycles4.hpp), the slot rule of one round of
// a wave, and a one-thread host form that runs the kernels' way. The shift, the NaN rule, the term and the quotient of an
// iteration are cemp.hpp's: there is one copy of them. Plain C++ with no HIP type in it: tools/cemp4_host_check.cpp runs
// all of it under sanitizers on a machine without a device. k_cemp4_walk and k_cemp4_iter (cemp4.hip) take every piece
// from here.
//
// Table: the used (finite) quadrilaterals of listed position t are one contiguous segment of 32-byte records. The wave of
// a position walks row x in outer rounds of `nsub` entries (sub-group `sub` takes entry x0 + round * nsub + sub) and the
// rows of those entries in inner rounds of S entries each (lane `sl` of the sub-group takes entry beg + inner * S + sl),
// as many inner rounds as the longest of the nsub rows needs. The records of a segment are ordered by outer round, then
// inner round, then lane of the wave (sub * S + sl), then position in the run of equals.
#pragma once
#include "cemp.hpp"
#include "cycles4.hpp"

namespace irh {

// 20 bytes in a slot of 32, aligned to 32: a record never straddles a cache line and moves as aligned 16-byte pieces
struct alignas(32) Cemp4Rec {
    double d;             // the quadrilateral error, finite
    uint32_t k1, k2, k3;  // the three other edges: b -> c, c -> d, d -> a
};

// What a lane keeps of one entry: how many used quadrilaterals it closes, and the first of them (a run of equals longer
// than one is rare: the others are stored by a second walk of the entry with Cemp4Store).
struct Cemp4Hits {
    int n;
    Cemp4Rec first;
    IRH_CYC_HD void operator()(double d, uint32_t k1, uint32_t k2, uint32_t k3) {
        if (!cemp_finite(d)) return;
        if (n == 0) first = Cemp4Rec{d, k1, k2, k3};
        n++;
    }
};
// count mode: the used quadrilaterals of a lane
struct Cemp4Count {
    long long n;
    IRH_CYC_HD void operator()(double d, uint32_t, uint32_t, uint32_t) { n += cemp_finite(d) ? 1 : 0; }
};
// stores the records of one entry from `at` on, never at or behind `end`, and adds their errors to `sum` in that order
struct Cemp4Store {
    Cemp4Rec *at;
    const Cemp4Rec *end;
    double sum;
    IRH_CYC_HD void operator()(double d, uint32_t k1, uint32_t k2, uint32_t k3) {
        if (!cemp_finite(d)) return;
        if (at < end) *at = Cemp4Rec{d, k1, k2, k3};
        at++;
        sum += d;
    }
};

// The slot rule of one inner round: a lane's records start behind the segment start, the records of the rounds done and
// those of the lower lanes of the wave in this round.
IRH_CYC_HD long long cemp4_slot(long long seg, long long done, long long before) { return seg + done + before; }

IRH_CYC_HD double cemp4_e(double s1, double s2, double s3) { return s1 + s2 + s3; }

// ---- the host form ----------------------------------------------------------------------------------------------------------
struct Cemp4Result {
    std::vector<Cemp4Rec> table;
    std::vector<long long> off;  // ne + 1
    std::vector<double> s4;      // ne
    std::vector<int32_t> used;   // ne
    long long summary[2] = {0, 0};
};

// The kernels' way on one thread: emit, sort, the table of row bounds; per listed position the two rows, the longer one
// staged unless it has more than stage_cap entries, the walk in rounds of a wave of 64 / group sub-groups of `group` lanes
// (one sub-group when group >= 64), the records placed by the slot rule, the start vector from the lanes' sums; then
// `iters` Jacobi iterations over the state (s_in with the listed entries replaced), each of `igroup` lanes over every
// igroup-th record of the segment. I: m pairs, qq: m rows [x y z w], s_in: m (nullptr with edges == nullptr), beta: iters.
inline int cemp4_sorted(int64_t m, int64_t n_total, const int32_t *I, const double *qq, const double *s_in, int64_t ne,
                        const int32_t *edges, int iters, const double *beta, int group, int stage_cap, int igroup,
                        Cemp4Result &R) {
    CycResult ids;
    if (cyc4_begin(m, n_total, I, ne, edges, ids) != CYC_OK) return CYC_BAD_ID;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    cyc_sorted_halves(m, n_total, I, keys, vals);
    const long long n2 = (long long)keys.size();
    std::vector<CycSpan> rows(keys.size());
    for (long long i = 0; i < n2; i++) rows[(size_t)i] = cyc_target_row(keys.data(), n2, i);
    const CycAosLoad load{qq};
    const int S = group >= CYC4_WAVE ? CYC4_WAVE : group, nsub = CYC4_WAVE / S;
    const auto add = [](double p, double q) { return p + q; };
    R.table.clear();
    R.off.assign((size_t)ne + 1, 0);
    R.s4.assign((size_t)ne, 0.0);
    R.used.assign((size_t)ne, 0);
    R.summary[0] = R.summary[1] = 0;
    std::vector<uint32_t> slab;
    for (int64_t t = 0; t < ne; t++) {
        const int64_t k = edges ? edges[t] : t;
        const uint32_t a = (uint32_t)I[2 * k], b = (uint32_t)I[2 * k + 1];
        std::vector<Cemp4Rec> seg;
        std::vector<double> lsum(CYC4_WAVE, 0.0);
        if (a != b) {
            long long a0, a1, b0, b1;
            cyc_row(keys.data(), n2, a, a0, a1);
            cyc_row(keys.data(), n2, b, b0, b1);
            const bool x_is_b = b1 - b0 <= a1 - a0;
            const long long x0 = x_is_b ? b0 : a0, x1 = x_is_b ? b1 : a1, y0 = x_is_b ? a0 : b0, y1 = x_is_b ? a1 : b1;
            const int ylen = (int)(y1 - y0);
            const CycQ q0 = load((uint32_t)k);
            const bool staged = ylen <= stage_cap;
            slab.clear();
            for (int p = 0; staged && p < ylen; p++) slab.push_back(cyc_key_to(keys[(size_t)(y0 + p)])), slab.push_back(vals[(size_t)(y0 + p)]);
            const CycRowStaged ys{slab.data(), ylen};
            const CycRowGlobal yg{keys.data(), vals.data(), y0, ylen};
            const auto entry = [&](long long j, uint32_t kx, const CycQ qx, auto &sink) {
                if (staged)
                    cyc4_entry(keys.data(), vals.data(), j, a, b, x_is_b, ys, q0, kx, qx, load, sink);
                else
                    cyc4_entry(keys.data(), vals.data(), j, a, b, x_is_b, yg, q0, kx, qx, load, sink);
            };
            long long done = 0;
            for (long long outer = x0; outer < x1; outer += nsub) {
                std::vector<uint32_t> kx((size_t)nsub, 0u);
                std::vector<CycQ> qx((size_t)nsub, CycQ{0, 0, 0, 0});
                std::vector<CycSpan> r((size_t)nsub, CycSpan{0, 0});
                int longest = 0;
                for (int sub = 0; sub < nsub; sub++)
                    if (outer + sub < x1 && cyc4_walked(keys.data(), vals.data(), outer + sub, a, b, x_is_b, q0, load, kx[(size_t)sub], qx[(size_t)sub])) {
                        r[(size_t)sub] = rows[(size_t)(outer + sub)];
                        longest = std::max(longest, r[(size_t)sub].end - r[(size_t)sub].beg);
                    }
                for (int inner = 0; inner < longest; inner += S) {
                    std::vector<Cemp4Hits> h(CYC4_WAVE, Cemp4Hits{0, Cemp4Rec{0.0, 0u, 0u, 0u}});
                    long long total = 0;
                    for (int lane = 0; lane < CYC4_WAVE; lane++) {
                        const int sub = lane / S;
                        const long long j = (long long)r[(size_t)sub].beg + inner + lane % S;
                        if (j < r[(size_t)sub].end) entry(j, kx[(size_t)sub], qx[(size_t)sub], h[(size_t)lane]);
                        total += h[(size_t)lane].n;
                    }
                    seg.resize((size_t)(done + total), Cemp4Rec{0.0, 0u, 0u, 0u});
                    long long before = 0;
                    for (int lane = 0; lane < CYC4_WAVE; lane++) {
                        const int sub = lane / S;
                        Cemp4Rec *const at = seg.data() + cemp4_slot(0, done, before);
                        if (h[(size_t)lane].n == 1) {
                            *at = h[(size_t)lane].first;
                            lsum[(size_t)lane] += h[(size_t)lane].first.d;
                        } else if (h[(size_t)lane].n > 1) {
                            Cemp4Store w{at, seg.data() + seg.size(), lsum[(size_t)lane]};
                            entry((long long)r[(size_t)sub].beg + inner + lane % S, kx[(size_t)sub], qx[(size_t)sub], w);
                            lsum[(size_t)lane] = w.sum;
                        }
                        before += h[(size_t)lane].n;
                    }
                    done += total;
                }
            }
        }
        const long long count = (long long)seg.size();
        R.off[(size_t)t + 1] = R.off[(size_t)t] + count;
        R.table.insert(R.table.end(), seg.begin(), seg.end());
        R.s4[(size_t)t] = cemp_mean(cemp_tree(lsum, add), count);
        R.used[(size_t)t] = cyc_stored_count(count);
        R.summary[0] += count;
        R.summary[1] += count == 0;
    }
    if (iters == 0) return CYC_OK;
    // the state: s_in, the listed entries replaced (duplicates hold equal values)
    std::vector<double> cur((size_t)m, 0.0), next;
    for (int64_t k = 0; k < m && s_in; k++) cur[(size_t)k] = s_in[k];
    for (int64_t t = 0; t < ne; t++) cur[(size_t)(edges ? edges[t] : t)] = R.s4[(size_t)t];
    next = cur;
    const size_t G = (size_t)igroup;
    for (int it = 0; it < iters; it++) {
        for (int64_t t = 0; t < ne; t++) {
            const long long beg = R.off[(size_t)t], end = R.off[(size_t)t + 1];
            const auto e_of = [&](long long r) {
                const Cemp4Rec &rec = R.table[(size_t)r];
                return cemp4_e(cur[rec.k1], cur[rec.k2], cur[rec.k3]);
            };
            std::vector<double> mu(G, std::numeric_limits<double>::infinity());
            for (size_t lane = 0; lane < G; lane++)
                for (long long r = beg + (long long)lane; r < end; r += igroup) cemp_min(mu[lane], e_of(r));
            const double shift = cemp_tree(mu, [](double p, double q) { return q < p ? q : p; });
            std::vector<double> num(G), den(G);
            for (size_t lane = 0; lane < G; lane++) {
                CempSum acc{0.0, 0.0};
                for (long long r = beg + (long long)lane; r < end; r += igroup) cemp_term(acc, R.table[(size_t)r].d, e_of(r), beta[it], shift);
                num[lane] = acc.num, den[lane] = acc.den;
            }
            R.s4[(size_t)t] = cemp_quotient(CempSum{cemp_tree(num, add), cemp_tree(den, add)});
            next[(size_t)(edges ? edges[t] : t)] = R.s4[(size_t)t];
        }
        cur = next;
    }
    return CYC_OK;
}

}  // namespace irh
