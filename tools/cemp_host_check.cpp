// cemp_host_check.cpp -- the pieces k_cemp_walk and k_cemp_iter run (irotavg_amd/csrc/cemp.hpp: the walk of one entry, the
// slot rule, one term of the iteration, cemp_sorted) held against the definition written out in sequence, as a stand-alone
// program that needs no device, meant to be built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/cemp_host_check.cpp -o cemp_host_check && ./cemp_host_check
// Exit status 0 and "cemp host check ok" when every expectation holds.
#include <cstdio>
#include <cstring>
#include <random>

#include "cemp.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                \
    do {                                                         \
        if (!(c)) {                                              \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            failures++;                                          \
        }                                                        \
    } while (0)

// The definition in sequence: the rows by a linear scan of the sorted half-edges, every entry of the shorter row against
// every entry of the longer one, one running sum, the global smallest e as the shift.
static void literal(int64_t m, int64_t n_total, const std::vector<int32_t> &I, const std::vector<double> &qq, int iters,
                    const std::vector<double> &beta, CempResult &R) {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    cyc_sorted_halves(m, n_total, I.data(), keys, vals);
    const CycAosLoad load{qq.data()};
    R = CempResult();
    R.off.assign(1, 0);
    for (int64_t k = 0; k < m; k++) {
        const uint32_t a = (uint32_t)I[2 * k], b = (uint32_t)I[2 * k + 1];
        std::vector<size_t> ra, rb;
        for (size_t t = 0; t < keys.size() && a != b; t++) {
            if (keys[t] >> 32 == a) ra.push_back(t);
            if (keys[t] >> 32 == b) rb.push_back(t);
        }
        const bool x_is_b = rb.size() <= ra.size();
        double sum = 0.0;
        long long count = 0;
        for (size_t i : x_is_b ? rb : ra)
            for (size_t j : x_is_b ? ra : rb) {
                const uint32_t c = (uint32_t)keys[i];
                if (c == a || c == b || (uint32_t)keys[j] != c) continue;
                const size_t i1 = x_is_b ? i : j, i2 = x_is_b ? j : i;  // b -> c, and a -> c to be turned
                const uint32_t k1 = vals[i1] >> 1, k2 = vals[i2] >> 1;
                const double d = cyc_triangle_error(load((uint32_t)k), cyc_directed(load(k1), vals[i1] & 1u),
                                                    cyc_directed(load(k2), !(vals[i2] & 1u)));
                if (!std::isfinite(d)) continue;
                R.table.push_back(CempRec{d, k1, k2});
                sum += d;
                count++;
            }
        R.off.push_back(R.off.back() + count);
        R.s.push_back(count ? sum / (double)count : NAN);
        R.used.push_back((int32_t)count);
        R.summary[0] += count;
        R.summary[1] += count == 0;
    }
    for (int t = 0; t < iters; t++) {
        std::vector<double> next((size_t)m, NAN);
        for (int64_t k = 0; k < m; k++) {
            double mu = INFINITY, num = 0.0, den = 0.0;
            for (long long r = R.off[(size_t)k]; r < R.off[(size_t)k + 1]; r++)
                mu = std::fmin(mu, R.s[R.table[(size_t)r].k1] + R.s[R.table[(size_t)r].k2]);  // (fmin ignores a NaN)
            for (long long r = R.off[(size_t)k]; r < R.off[(size_t)k + 1]; r++) {
                const CempRec &c = R.table[(size_t)r];
                const double w = std::exp(-beta[(size_t)t] * (R.s[c.k1] + R.s[c.k2] - mu));
                if (!std::isnan(w)) num += w * c.d, den += w;
            }
            if (den > 0.0) next[(size_t)k] = num / den;
        }
        R.s = next;
    }
}

static bool same_table(const CempResult &A, const CempResult &B) {
    return A.off == B.off && A.used == B.used && A.summary[0] == B.summary[0] && A.summary[1] == B.summary[1] &&
           A.table.size() == B.table.size() &&
           (A.table.empty() || std::memcmp(A.table.data(), B.table.data(), A.table.size() * sizeof(CempRec)) == 0);
}
static double max_diff(const std::vector<double> &a, const std::vector<double> &b) {
    double worst = a.size() == b.size() ? 0.0 : INFINITY;
    for (size_t k = 0; k < a.size() && k < b.size(); k++) {
        if (std::isnan(a[k]) != std::isnan(b[k])) return INFINITY;
        if (!std::isnan(a[k])) worst = std::fmax(worst, std::fabs(a[k] - b[k]));
    }
    return worst;
}

static CycQ unit(std::mt19937 &rng) {
    std::normal_distribution<double> N(0.0, 1.0);
    const CycQ q{N(rng), N(rng), N(rng), N(rng)};
    const double s = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return CycQ{q.x / s, q.y / s, q.z / s, q.w / s};
}

// The book of tests/test_gpu_cycle_cemp.py: spine (0, 1), p pages; every third page has its hub-0 edge doubled, every
// fifth its hub-1 edge doubled the other way round, so the runs of equals vary across the lanes of a round; a self loop;
// one NaN row, whose triangles vanish from all three edges. Measurements: consistent, then turned by up to 0.3 rad.
static void book(int p, std::mt19937 &rng, int64_t &n_total, std::vector<int32_t> &I, std::vector<double> &qq) {
    I = {0, 1};
    for (int c = 0; c < p; c++) {
        const int v = 2 + c;
        I.insert(I.end(), {0, v});
        if (c % 2) I.insert(I.end(), {v, 1}); else I.insert(I.end(), {1, v});
        if (c % 3 == 0) I.insert(I.end(), {0, v});
        if (c % 5 == 0) { if (c % 2) I.insert(I.end(), {1, v}); else I.insert(I.end(), {v, 1}); }
    }
    I.insert(I.end(), {2, 2});
    n_total = 2 + p;
    std::vector<CycQ> Q;
    for (int v = 0; v < n_total; v++) Q.push_back(unit(rng));
    std::uniform_real_distribution<double> U(0.0, 0.3);
    qq.clear();
    for (size_t k = 0; k < I.size() / 2; k++) {
        const double t = U(rng);
        const CycQ q = cyc_qmul(CycQ{std::sin(t / 2), 0.0, 0.0, std::cos(t / 2)},
                                cyc_qmul(Q[(size_t)I[2 * k + 1]], cyc_directed(Q[(size_t)I[2 * k]], true)));
        qq.insert(qq.end(), {q.x, q.y, q.z, q.w});
    }
    qq[4 * 2 + 1] = NAN;  // the hub-1 edge of page 0
}

int main() {
    std::mt19937 rng(20241126);
    EXPECT(sizeof(CempRec) == 16 && cemp_slot(100, 7, 3) == 110);
    EXPECT(cemp_finite(0.0) && cemp_finite(3.2) && !cemp_finite(NAN) && !cemp_finite(INFINITY));
    {
        CempSum a{0.0, 0.0};
        cemp_term(a, 0.25, 1.0, 1e300, 1.0);  // the smallest e: weight exactly 1 whatever beta is
        EXPECT(a.num == 0.25 && a.den == 1.0);
        cemp_term(a, 0.5, NAN, 2.0, 1.0);  // a NaN estimate: left out of both sums
        cemp_term(a, 0.5, 2.0, 1e300, 1.0);  // weight 0
        EXPECT(a.num == 0.25 && a.den == 1.0 && cemp_quotient(a) == 0.25 && std::isnan(cemp_quotient(CempSum{0.0, 0.0})));
        double mu = INFINITY;
        cemp_min(mu, NAN), cemp_min(mu, 2.0), cemp_min(mu, NAN), cemp_min(mu, 3.0);
        EXPECT(mu == 2.0 && std::isnan(cemp_mean(0.0, 0)) && cemp_mean(3.0, 2) == 1.5);
    }
    const std::vector<double> beta = {8 / CYC_PI, 16 / CYC_PI, 32 / CYC_PI};
    long long records = 0;
    for (int p : {1, 7, 8, 9, 15, 16, 17, 33, 65}) {
        int64_t n_total;
        std::vector<int32_t> I;
        std::vector<double> qq;
        book(p, rng, n_total, I, qq);
        const int64_t m = (int64_t)I.size() / 2;
        for (int iters : {0, 3}) {
            CempResult L, S[3];
            literal(m, n_total, I, qq, iters, beta, L);
            const int widths[3] = {1, 8, 16};
            for (int w = 0; w < 3; w++) {
                EXPECT(cemp_sorted(m, n_total, I.data(), qq.data(), iters, beta.data(), widths[w], S[w]) == CYC_OK);
                EXPECT(same_table(S[w], L));                                             // records and their order, bitwise
                EXPECT(max_diff(S[w].s, L.s) <= 1e-13 && max_diff(S[w].s, S[0].s) <= 1e-13);
            }
            // the NaN row and the self loop close no used triangle
            EXPECT(L.used[2] == 0 && std::isnan(L.s[2]) && L.used[(size_t)m - 1] == 0 && L.summary[1] >= 2);
            records += L.summary[0];
        }
        I[3] = (int32_t)n_total;
        CempResult R;
        EXPECT(cemp_sorted(m, n_total, I.data(), qq.data(), 0, nullptr, 8, R) == CYC_BAD_ID);
    }
    EXPECT(records > 1000);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("cemp host check ok (%lld records)\n", records);
    return 0;
}
