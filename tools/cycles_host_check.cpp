// cycles_host_check.cpp -- the pieces of the triangle test that k_cyc_emit and k_cyc_triangles run
// (irotavg_amd/csrc/cycles.hpp: the half-edge key, the row lookup in the sorted half-edges, the walk of the shorter row
// against the longer one, and the literal sequential reference) held against a brute-force loop over all edge triples, as
// a stand-alone program that needs no device, meant to be built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/cycles_host_check.cpp -o cycles_host_check && ./cycles_host_check
// Exit status 0 and "cycles host check ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "cycles.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
            failures++;                                                  \
        }                                                                \
    } while (0)

typedef std::vector<int32_t> Edges;   // pairs
typedef std::vector<double> Quats;    // rows [x y z w]
static const double INF = std::numeric_limits<double>::infinity();

// the definition over all ordered pairs (k1, k2), nothing sorted and nothing looked up
static void brute(const Edges &I, const Quats &qq, double threshold, CycResult &R) {
    const size_t m = I.size() / 2;
    R.count.assign(m, 0);
    R.ok.assign(m, 0);
    R.mn.assign(m, INF);
    for (long long &s : R.summary) s = 0;
    const CycAosLoad load{qq.data()};
    for (size_t k = 0; k < m; k++) {
        const int32_t a = I[2 * k], b = I[2 * k + 1];
        CycAcc acc = cyc_acc_zero();
        for (size_t k1 = 0; k1 < m && a != b; k1++) {
            const int32_t u1 = I[2 * k1], v1 = I[2 * k1 + 1];
            if (u1 == v1 || (u1 != b && v1 != b)) continue;
            const int32_t c = u1 == b ? v1 : u1;
            if (c == a || c == b) continue;
            for (size_t k2 = 0; k2 < m; k2++) {
                const int32_t u2 = I[2 * k2], v2 = I[2 * k2 + 1];
                if (!((u2 == c && v2 == a) || (u2 == a && v2 == c))) continue;
                const CycQ q1 = cyc_directed(load((uint32_t)k1), u1 != b), q2 = cyc_directed(load((uint32_t)k2), u2 != c);
                cyc_acc_add(acc, cyc_triangle_error(load((uint32_t)k), q1, q2), threshold);
            }
        }
        cyc_store(R, k, acc);
    }
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}
static bool same(const CycResult &A, const CycResult &B) {
    return A.count == B.count && A.ok == B.ok && same_bits(A.mn, B.mn) && std::memcmp(A.summary, B.summary, sizeof(A.summary)) == 0;
}

// every form against the brute force; returns the brute-force result
static CycResult check_graph(int64_t n_total, const Edges &I, const Quats &qq, double threshold) {
    const int64_t m = (int64_t)I.size() / 2;
    CycResult B, R, S;
    brute(I, qq, threshold, B);
    EXPECT(cycles_reference(m, n_total, I.data(), qq.data(), threshold, R) == CYC_OK);
    EXPECT(same(R, B));
    for (int group : {1, 8, 16, 32, 64}) {
        EXPECT(cycles_sorted(m, n_total, I.data(), qq.data(), threshold, group, S) == CYC_OK);
        EXPECT(same(S, B));
    }
    EXPECT(B.summary[1] + B.summary[2] + B.summary[3] == m);
    long long total = 0;
    for (int64_t k = 0; k < m; k++) {
        total += B.count[(size_t)k];
        EXPECT(B.ok[(size_t)k] <= B.count[(size_t)k]);
        if (B.count[(size_t)k] == 0) EXPECT(B.mn[(size_t)k] == INF);
    }
    EXPECT(total == B.summary[0]);
    return B;
}

static CycQ unit(std::mt19937 &rng) {
    std::normal_distribution<double> N(0.0, 1.0);
    CycQ q{N(rng), N(rng), N(rng), N(rng)};
    const double s = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return CycQ{q.x / s, q.y / s, q.z / s, q.w / s};
}
static CycQ turn(double angle) { return CycQ{std::sin(angle / 2), 0.0, 0.0, std::cos(angle / 2)}; }
static void put(Quats &qq, const CycQ q) {
    qq.push_back(q.x), qq.push_back(q.y), qq.push_back(q.z), qq.push_back(q.w);
}
// the measurement of edge (a, b) from absolute rotations: Q_b (x) inverse(Q_a)
static CycQ relative(const std::vector<CycQ> &Q, int a, int b) { return cyc_qmul(Q[(size_t)b], cyc_directed(Q[(size_t)a], true)); }
static Quats consistent(const std::vector<CycQ> &Q, const Edges &I) {
    Quats qq;
    for (size_t k = 0; k < I.size() / 2; k++) put(qq, relative(Q, I[2 * k], I[2 * k + 1]));
    return qq;
}
static std::vector<CycQ> views(int n, std::mt19937 &rng) {
    std::vector<CycQ> Q;
    for (int v = 0; v < n; v++) Q.push_back(unit(rng));
    return Q;
}
// hubs 0 and 1 joined, d common neighbours 2 .. d + 1, `extra` private neighbours of hub 0 on both sides of them in id order
static Edges book(int d, int extra) {
    Edges I = {0, 1};
    for (int c = 0; c < d; c++) {
        const int v = 2 + extra / 2 + c;
        I.insert(I.end(), {0, v, v, 1});
    }
    for (int p = 0; p < extra; p++) I.insert(I.end(), {0, p < extra / 2 ? 2 + p : 2 + d + p});
    return I;
}

int main() {
    std::mt19937 rng(20240917);
    // ---- the encoding
    EXPECT(cyc_key(3, 5) == ((3ull << 32) | 5ull) && cyc_key_to(cyc_key(3, 5)) == 5);
    EXPECT(cyc_val_edge(cyc_val(0x3ffffffeu, true)) == 0x3ffffffeu && cyc_val_against(cyc_val(0x3ffffffeu, true)));
    EXPECT(!cyc_val_against(cyc_val(7, false)) && cyc_val(0x3fffffffu - 1, true) == 0x7ffffffdu);
    EXPECT(cyc_key_bits(1) == 33 && cyc_key_bits(2) == 33 && cyc_key_bits(3) == 34 && cyc_key_bits(4) == 34);
    EXPECT(cyc_key_bits(5) == 35 && cyc_key_bits(0x7fffffff) == 63 && cyc_key_bits(0x40000000) == 62);
    for (int64_t n : {1ll, 2ll, 3ll, 4ll, 1000ll, 0x40000000ll, 0x40000001ll, 0x7fffffffll}) {
        const uint64_t mask = ((uint64_t)1 << cyc_key_bits(n)) - 1, top = cyc_key((uint32_t)(n - 1), (uint32_t)(n - 1));
        EXPECT((top & mask) == top && (CYC_KEY_NONE & mask) > top);  // every id within the bits, a self loop behind them all
    }
    EXPECT(cyc_id_ok(0, 1) && !cyc_id_ok(1, 1) && !cyc_id_ok(-1, 5) && cyc_id_ok(0x7ffffffe, 0x7fffffff) && !cyc_id_ok(0x7fffffff, 0x7fffffff));
    EXPECT(cyc_stored_count(5) == 5 && cyc_stored_count(0x7fffffffLL) == 0x7fffffff && cyc_stored_count(0x80000000LL) == 0x7fffffff);
    {
        const uint64_t keys[6] = {1, 3, 3, 3, 7, CYC_KEY_NONE};
        EXPECT(cyc_lower_bound(keys, 0, 6, 0) == 0 && cyc_lower_bound(keys, 0, 6, 3) == 1 && cyc_lower_bound(keys, 0, 6, 4) == 4);
        EXPECT(cyc_lower_bound(keys, 0, 6, 8) == 5 && cyc_lower_bound(keys, 0, 5, 8) == 5 && cyc_lower_bound(keys, 2, 2, 0) == 2);
    }
    // ---- the error: zero on a consistent triangle, the planted angle on a turned one, the same under q -> -q
    {
        const std::vector<CycQ> Q = views(3, rng);
        const CycQ q0 = relative(Q, 0, 1), q1 = relative(Q, 1, 2), q2 = relative(Q, 2, 0);
        EXPECT(cyc_triangle_error(q0, q1, q2) <= 4e-16);
        const CycQ t = cyc_qmul(turn(0.3), q1), neg{-q2.x, -q2.y, -q2.z, -q2.w};
        EXPECT(std::fabs(cyc_triangle_error(q0, t, q2) - 0.3) <= 4e-16);
        EXPECT(std::fabs(cyc_triangle_error(q0, t, neg) - 0.3) <= 4e-16);
        EXPECT(std::isnan(cyc_triangle_error(q0, CycQ{NAN, 0, 0, 1}, q2)));
        EXPECT(cyc_triangle_error(cyc_directed(q0, true), cyc_directed(q2, true), cyc_directed(q1, true)) <= 4e-16);  // the other way round
    }
    // ---- the named shapes of tests/test_gpu_cycle_check.py
    {
        const std::vector<CycQ> Q = views(8, rng);
        Edges I = {0, 1, 1, 2, 2, 0};
        CycResult B = check_graph(3, I, consistent(Q, I), 0.1);
        EXPECT(B.count == std::vector<int32_t>({1, 1, 1}) && B.ok == B.count && B.mn[0] <= 4e-16 && B.mn[1] <= 4e-16);
        // one edge stored as (b, a), another multiplied by -1, one turned by 0.3 rad
        I = {0, 1, 2, 1, 2, 0};
        Quats qq = consistent(Q, I);
        for (int c = 0; c < 4; c++) qq[8 + (size_t)c] = -qq[8 + (size_t)c];
        const CycQ t = cyc_qmul(turn(0.3), CycQ{qq[0], qq[1], qq[2], qq[3]});
        qq[0] = t.x, qq[1] = t.y, qq[2] = t.z, qq[3] = t.w;
        B = check_graph(3, I, qq, 0.1);
        EXPECT(B.count == std::vector<int32_t>({1, 1, 1}) && B.ok == std::vector<int32_t>({0, 0, 0}));
        for (double e : B.mn) EXPECT(std::fabs(e - 0.3) <= 4e-16);
        EXPECT(B.summary[0] == 3 && B.summary[1] == 0 && B.summary[2] == 3 && B.summary[3] == 0);
        // self loops, parallel edges with and without reversal, an unused id
        I = {0, 1, 1, 2, 2, 0, 1, 1, 0, 1, 1, 0, 5, 5};
        B = check_graph(7, I, consistent(Q, I), 0.1);
        EXPECT(B.count == std::vector<int32_t>({1, 3, 3, 0, 1, 1, 0}) && B.mn[3] == INF && B.mn[6] == INF && B.summary[3] == 2);
        I = {0, 1, 1, 2, 2, 3, 3, 4};  // a path
        B = check_graph(5, I, consistent(Q, I), 0.1);
        EXPECT(B.summary[0] == 0 && B.summary[3] == 4);
        I = {0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3};  // K4
        B = check_graph(4, I, consistent(Q, I), 0.1);
        EXPECT(B.count == std::vector<int32_t>(6, 2) && B.ok == B.count && B.summary[1] == 6);
        // a NaN row: counted, never ok, the minimum left alone
        I = {0, 1, 1, 2, 2, 0, 2, 3, 3, 0};
        qq = consistent(Q, I);
        qq[4] = NAN;
        B = check_graph(4, I, qq, INF);
        EXPECT(B.count == std::vector<int32_t>({1, 1, 2, 1, 1}) && B.ok == std::vector<int32_t>({0, 0, 1, 1, 1}));
        EXPECT(B.mn[0] == INF && B.mn[1] == INF && B.mn[2] <= 4e-16);
        // ids at the top of the range: nothing grows with n_total
        const int32_t big[5] = {0, 1, 1 << 30, 0x7fffffff - 2, 0x7fffffff - 1};
        I = {big[0], big[4], big[4], big[3], big[3], big[0], big[2], big[4], big[3], big[2], big[1], big[2]};
        qq.clear();
        for (int k = 0; k < 6; k++) put(qq, unit(rng));
        B = check_graph(0x7fffffff, I, qq, 1.0);
        EXPECT(B.count == std::vector<int32_t>({1, 2, 1, 1, 1, 0}));
        CycResult R;
        EXPECT(cycles_sorted(6, 0x7fffffff - 1, I.data(), qq.data(), 1.0, 16, R) == CYC_BAD_ID);
        EXPECT(cycles_reference(6, 0x7fffffff - 1, I.data(), qq.data(), 1.0, R) == CYC_BAD_ID);
        I[3] = -1;
        EXPECT(cycles_sorted(6, 0x7fffffff, I.data(), qq.data(), 1.0, 16, R) == CYC_BAD_ID);
    }
    // ---- book graphs: the shorter / longer choice, search misses at both ends of a row, runs across the group width
    for (int d : {7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129})
        for (int extra : {0, d}) {
            const Edges I = book(d, extra);
            const int n = 2 + d + extra;
            const std::vector<CycQ> Q = views(n, rng);
            const CycResult B = check_graph(n, I, consistent(Q, I), 1e-9);
            EXPECT(B.count[0] == d && B.ok[0] == d);
            for (int c = 0; c < 2 * d; c++) EXPECT(B.count[1 + (size_t)c] == 1);
            for (int p = 0; p < extra; p++) EXPECT(B.count[1 + 2 * (size_t)d + (size_t)p] == 0);
        }
    // ---- seeded random multigraphs: self loops, duplicates, reversed duplicates, unused ids, noise around a threshold
    long long triangles = 0, contradicted = 0, untested = 0;
    for (int it = 0; it < 2000; it++) {
        const int n = 2 + (int)(rng() % 39), m = 1 + (int)(rng() % 120), spread = 1 + (int)(rng() % 3);
        const std::vector<CycQ> Q = views(n * spread, rng);
        Edges I;
        for (int k = 0; k < m; k++) {
            const unsigned kind = rng() % 10;
            int a, b;
            if (kind == 0 && k > 0) {  // a duplicate, every other one reversed
                const size_t j = rng() % (unsigned)k;
                a = I[2 * j], b = I[2 * j + 1];
                if (rng() & 1) std::swap(a, b);
            } else {
                a = (int)(rng() % (unsigned)n) * spread;  // (spread > 1: ids that no edge uses)
                b = kind == 1 ? a : (int)(rng() % (unsigned)n) * spread;
            }
            I.push_back(a), I.push_back(b);
        }
        Quats qq;
        std::uniform_real_distribution<double> U(0.0, 0.2);
        for (int k = 0; k < m; k++) {
            CycQ q = relative(Q, I[2 * (size_t)k], I[2 * (size_t)k + 1]);
            if (rng() % 4 == 0) q = cyc_qmul(turn(U(rng)), q);
            if (rng() % 7 == 0) q = CycQ{-q.x, -q.y, -q.z, -q.w};
            if (rng() % 97 == 0) q.y = NAN;
            put(qq, q);
        }
        const CycResult B = check_graph((int64_t)n * spread + (int64_t)(rng() % 3), I, qq, it % 5 == 0 ? INF : U(rng));
        triangles += B.summary[0], contradicted += B.summary[2], untested += B.summary[3];
    }
    EXPECT(triangles > 100000 && contradicted > 1000 && untested > 1000);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("cycles host check ok (%lld triangles, %lld contradicted and %lld untested edges in the random graphs)\n", triangles,
                contradicted, untested);
    return 0;
}
