// cemp4_host_check.cpp -- the pieces k_cemp4_walk and k_cemp4_iter run (irotavg_amd/csrc/cemp4.hpp: the sinks of the
// four-cycle walk, the slot rule, cemp4_sorted) held against the definition written out from maps in long double, as a
// stand-alone program that needs no device, meant to be built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/cemp4_host_check.cpp -o cemp4_host_check && ./cemp4_host_check
// Exit status 0 and "cemp4 host check ok" when every expectation holds.
#include <array>
#include <cstdio>
#include <random>

#include "cemp4.hpp"

using namespace irh;
typedef long double LD;
typedef std::array<LD, 4> QL;  // x y z w

static int failures = 0;
#define EXPECT(c)                                                \
    do {                                                         \
        if (!(c)) {                                              \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            failures++;                                          \
        }                                                        \
    } while (0)

static QL mul(const QL &a, const QL &b) {
    return QL{a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
              a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
}

struct Literal {
    std::vector<LD> s4;
    std::vector<int32_t> used;
    long long summary[2] = {0, 0};
};

// The definition in sequence: for a listed edge k = (a, b) every half-edge b -> c, every half-edge c -> d and every edge
// that joins d and a, from maps; one running sum per edge; the global smallest e as the shift.
static void literal(int64_t m, const std::vector<int32_t> &I, const std::vector<double> &qq, const std::vector<double> &s_in,
                    const std::vector<int32_t> &edges, int iters, const std::vector<double> &beta, Literal &R) {
    typedef std::pair<uint32_t, bool> Half;  // edge, against its stored direction
    std::map<int32_t, std::vector<std::pair<int32_t, Half>>> out;
    std::map<std::pair<int32_t, int32_t>, std::vector<Half>> between;
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        if (a == b) continue;
        out[a].push_back({b, Half((uint32_t)k, false)});
        out[b].push_back({a, Half((uint32_t)k, true)});
        between[{a, b}].push_back(Half((uint32_t)k, false));
        between[{b, a}].push_back(Half((uint32_t)k, true));
    }
    const auto q = [&](const Half &h) {
        return QL{qq[4 * h.first], qq[4 * h.first + 1], qq[4 * h.first + 2], h.second ? -(LD)qq[4 * h.first + 3] : (LD)qq[4 * h.first + 3]};
    };
    const LD pi = 4 * std::atan((LD)1);
    struct Quad {
        LD d;
        uint32_t k1, k2, k3;
    };
    const size_t ne = edges.size();
    std::vector<std::vector<Quad>> U(ne);
    std::vector<LD> S(s_in.begin(), s_in.end());
    R = Literal();
    R.s4.assign(ne, NAN);
    for (size_t t = 0; t < ne; t++) {
        const int32_t k = edges[t], a = I[2 * k], b = I[2 * k + 1];
        if (a != b)
            for (const auto &e1 : out[b]) {
                const int32_t c = e1.first;
                if (c == a || c == b) continue;
                for (const auto &e2 : out[c]) {
                    const int32_t d = e2.first;
                    const auto it = between.find({d, a});
                    if (d == a || d == b || d == c || it == between.end()) continue;
                    for (const Half &e3 : it->second) {
                        const QL D = mul(q(e3), mul(q(e2.second), mul(q(e1.second), q(Half((uint32_t)k, false)))));
                        LD th = 2 * std::atan2(std::sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]), D[3]);
                        if (th >= pi) th -= 2 * pi;
                        if (std::isfinite(th)) U[t].push_back(Quad{std::fabs(th), e1.second.first, e2.second.first, e3.first});
                    }
                }
            }
        LD sum = 0;
        for (const Quad &u : U[t]) sum += u.d;
        if (!U[t].empty()) R.s4[t] = sum / (LD)U[t].size();
        R.used.push_back((int32_t)U[t].size());
        R.summary[0] += (long long)U[t].size();
        R.summary[1] += U[t].empty();
    }
    for (size_t t = 0; t < ne; t++) S[(size_t)edges[t]] = R.s4[t];
    for (int it = 0; it < iters; it++) {
        for (size_t t = 0; t < ne; t++) {
            LD mu = INFINITY, num = 0, den = 0;
            for (const Quad &u : U[t]) mu = std::fmin(mu, S[u.k1] + S[u.k2] + S[u.k3]);  // (fmin ignores a NaN)
            for (const Quad &u : U[t]) {
                const LD w = std::exp(-(LD)beta[(size_t)it] * (S[u.k1] + S[u.k2] + S[u.k3] - mu));
                if (!std::isnan(w)) num += w * u.d, den += w;
            }
            R.s4[t] = den > 0 ? num / den : (LD)NAN;
        }
        for (size_t t = 0; t < ne; t++) S[(size_t)edges[t]] = R.s4[t];
    }
}

static CycQ unit(std::mt19937 &rng) {
    std::normal_distribution<double> N(0.0, 1.0);
    const CycQ q{N(rng), N(rng), N(rng), N(rng)};
    const double s = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return CycQ{q.x / s, q.y / s, q.z / s, q.w / s};
}

// measurements Q_b (x) inverse(Q_a) of random poses, each turned by `turn` rad about x (noise) or by a large angle (bad)
static void measure(int64_t n_total, const std::vector<int32_t> &I, std::mt19937 &rng, double turn, double p_bad, std::vector<double> &qq) {
    std::vector<CycQ> Q;
    for (int v = 0; v < n_total; v++) Q.push_back(unit(rng));
    std::uniform_real_distribution<double> U(0.0, 1.0);
    qq.clear();
    for (size_t k = 0; k < I.size() / 2; k++) {
        const double t = U(rng) < p_bad ? 0.5 + 2.5 * U(rng) : turn * U(rng);
        const CycQ q = cyc_qmul(CycQ{std::sin(t / 2), 0.0, 0.0, std::cos(t / 2)},
                                cyc_qmul(Q[(size_t)I[2 * k + 1]], cyc_directed(Q[(size_t)I[2 * k]], true)));
        qq.insert(qq.end(), {q.x, q.y, q.z, q.w});
    }
}

// The ladder of tests/test_gpu_cycle_cemp4.py: tested edge (0, 1), p rungs 1 - c - d - 0; every third rung has its middle
// edge doubled, every fifth its edge at view 0 doubled the other way round; a self loop; one NaN row.
static void ladder(int p, std::mt19937 &rng, int64_t &n_total, std::vector<int32_t> &I, std::vector<double> &qq) {
    I = {0, 1};
    for (int r = 0; r < p; r++) {
        const int c = 2 + 2 * r, d = c + 1;
        I.insert(I.end(), {1, c, d, c, d, 0});
        if (r % 3 == 0) I.insert(I.end(), {c, d});
        if (r % 5 == 0) I.insert(I.end(), {0, d});
    }
    I.insert(I.end(), {2, 2});
    n_total = 2 + 2 * p;
    measure(n_total, I, rng, 0.3, 0.0, qq);
    qq[4 * 2 + 1] = NAN;  // the middle edge of rung 0
}

// the 64-view graph: every pair at distance <= 4, and sixteen closures in four clusters; some measurements bad
static void closures(std::mt19937 &rng, int64_t &n_total, std::vector<int32_t> &I, std::vector<double> &qq) {
    I.clear();
    for (int a = 0; a < 64; a++)
        for (int b = a + 1; b < std::min(64, a + 5); b++) I.insert(I.end(), {a, b});
    const int ab[4][2] = {{2, 30}, {10, 50}, {20, 58}, {36, 60}};
    for (const auto &c : ab)
        for (int j = 0; j < 4; j++) I.insert(I.end(), {c[0] + j, c[1] + j});
    n_total = 64;
    measure(n_total, I, rng, 0.02, 0.1, qq);
}

static void hold(int64_t m, int64_t n_total, const std::vector<int32_t> &I, const std::vector<double> &qq, const std::vector<double> &s_in,
                 const std::vector<int32_t> &edges, int iters, const std::vector<double> &beta, long long &records) {
    Literal L;
    literal(m, I, qq, s_in, edges, iters, beta, L);
    const int64_t ne = (int64_t)edges.size();
    Cemp4Result first;
    for (int group : {1, 8, 64})
        for (int cap : {2, CYC4_STAGE}) {
            Cemp4Result R;
            EXPECT(cemp4_sorted(m, n_total, I.data(), qq.data(), s_in.data(), ne, edges.data(), iters, beta.data(), group, cap, 8, R) == CYC_OK);
            EXPECT(R.used == L.used && R.summary[0] == L.summary[0] && R.summary[1] == L.summary[1]);
            EXPECT(R.off.back() == (long long)R.table.size() && R.summary[0] == R.off.back());
            for (int64_t t = 0; t < ne; t++) {
                EXPECT(std::isnan(R.s4[(size_t)t]) == std::isnan(L.s4[(size_t)t]));
                if (!std::isnan(R.s4[(size_t)t])) EXPECT(std::fabs((LD)R.s4[(size_t)t] - L.s4[(size_t)t]) <= 1e-13L);
            }
            // the staging cap decides where a row is searched, never what is found: the same records in the same order
            if (cap == 2) first = R;
            for (size_t r = 0; cap != 2 && r < R.table.size(); r++)
                EXPECT(first.off == R.off && first.table[r].d == R.table[r].d && first.table[r].k1 == R.table[r].k1 &&
                       first.table[r].k2 == R.table[r].k2 && first.table[r].k3 == R.table[r].k3);
        }
    records += L.summary[0];
}

int main() {
    std::mt19937 rng(20261126);
    EXPECT(sizeof(Cemp4Rec) == 32 && alignof(Cemp4Rec) == 32 && cemp4_slot(100, 7, 3) == 110);
    const std::vector<double> beta = {8 / CYC_PI, 16 / CYC_PI, 32 / CYC_PI, 64 / CYC_PI, 128 / CYC_PI, 256 / CYC_PI};
    long long records = 0;
    int64_t n_total;
    std::vector<int32_t> I;
    std::vector<double> qq;
    for (int p : {1, 7, 8, 9, 17, 65, 1030}) {
        ladder(p, rng, n_total, I, qq);
        const int64_t m = (int64_t)I.size() / 2;
        std::vector<int32_t> all((size_t)m);
        for (int64_t k = 0; k < m; k++) all[(size_t)k] = (int32_t)k;
        std::vector<double> s_in((size_t)m, 0.05);
        s_in[5] = NAN;
        for (int iters : {0, 3}) {
            if (p > 100 && iters == 0) continue;  // (the long rows once)
            hold(m, n_total, I, qq, s_in, all, iters, beta, records);
            hold(m, n_total, I, qq, s_in, {0}, iters, beta, records);
        }
        Cemp4Result R;
        const int32_t bad[2] = {0, (int32_t)m};
        EXPECT(cemp4_sorted(m, n_total, I.data(), qq.data(), s_in.data(), 2, bad, 0, nullptr, 8, CYC4_STAGE, 8, R) == CYC_BAD_ID);
    }
    {
        closures(rng, n_total, I, qq);
        const int64_t m = (int64_t)I.size() / 2;
        CempResult T;  // the triangle estimates: NaN exactly at the sixteen closures
        EXPECT(cemp_sorted(m, n_total, I.data(), qq.data(), 6, beta.data(), 8, T) == CYC_OK);
        std::vector<int32_t> listed;
        for (int64_t k = 0; k < m; k++)
            if (std::isnan(T.s[(size_t)k])) listed.push_back((int32_t)k);
        EXPECT(listed.size() == 16 && listed.front() == (int32_t)m - 16);
        listed.push_back(listed[3]);  // a duplicate
        hold(m, n_total, I, qq, T.s, listed, 0, beta, records);
        hold(m, n_total, I, qq, T.s, listed, 6, beta, records);
    }
    EXPECT(records > 1000);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("cemp4 host check ok (%lld records)\n", records);
    return 0;
}
