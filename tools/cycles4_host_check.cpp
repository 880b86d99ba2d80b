// cycles4_host_check.cpp -- the pieces of the four-cycle test that k_cyc_rows and k_cyc_quads run
// (irotavg_amd/csrc/cycles4.hpp: the table of row bounds, the staged and the unstaged searched row, the walk of one lane)
// held against the literal reference from maps, as a stand-alone program that needs no device, meant to be built with a
// sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/cycles4_host_check.cpp -o cycles4_host_check && ./cycles4_host_check
// Exit status 0 and "cycles4 host check ok" when every expectation holds.
#include <cstdio>
#include <cstring>
#include <random>

#include "cycles4.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
            failures++;                                                  \
        }                                                                \
    } while (0)

typedef std::vector<int32_t> Edges;  // pairs
typedef std::vector<double> Quats;   // rows [x y z w]
typedef std::vector<int32_t> Counts;
static const double INF = std::numeric_limits<double>::infinity();

static bool same(const CycResult &A, const CycResult &B) {
    return A.count == B.count && A.ok == B.ok && A.mn.size() == B.mn.size() &&
           (A.mn.empty() || std::memcmp(A.mn.data(), B.mn.data(), A.mn.size() * sizeof(double)) == 0) &&
           std::memcmp(A.summary, B.summary, sizeof(A.summary)) == 0;
}

// quads_sorted at every group width and at a staging cap that no row of more than two entries fits, against the reference
static CycResult check_graph(int64_t n_total, const Edges &I, const Quats &qq, double threshold, const Edges *subset = nullptr) {
    const int64_t m = (int64_t)I.size() / 2, ne = subset ? (int64_t)subset->size() : m;
    const int32_t *edges = subset ? subset->data() : nullptr;
    CycResult R, S;
    EXPECT(quads_reference(m, n_total, I.data(), qq.data(), threshold, ne, edges, R) == CYC_OK);
    for (int group : {1, 8, 16, 64})
        for (int cap : {2, CYC4_STAGE}) {
            EXPECT(quads_sorted(m, n_total, I.data(), qq.data(), threshold, ne, edges, group, cap, S) == CYC_OK);
            EXPECT(same(S, R));
        }
    EXPECT(R.summary[1] + R.summary[2] + R.summary[3] == ne);
    for (int64_t t = 0; t < ne; t++) {
        EXPECT(R.ok[(size_t)t] <= R.count[(size_t)t]);
        if (R.count[(size_t)t] == 0) EXPECT(R.mn[(size_t)t] == INF);
    }
    return R;
}

static CycQ unit(std::mt19937 &rng) {
    std::normal_distribution<double> N(0.0, 1.0);
    CycQ q{N(rng), N(rng), N(rng), N(rng)};
    const double s = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return CycQ{q.x / s, q.y / s, q.z / s, q.w / s};
}
static CycQ turn(double angle) { return CycQ{std::sin(angle / 2), 0.0, 0.0, std::cos(angle / 2)}; }
static void put(Quats &qq, const CycQ q) { qq.insert(qq.end(), {q.x, q.y, q.z, q.w}); }
static std::vector<CycQ> views(int n, std::mt19937 &rng) {
    std::vector<CycQ> Q;
    for (int v = 0; v < n; v++) Q.push_back(unit(rng));
    return Q;
}
// the measurements of consistent rotations: Q_b (x) inverse(Q_a) for every edge
static Quats consistent(const std::vector<CycQ> &Q, const Edges &I) {
    Quats qq;
    for (size_t k = 0; k < I.size() / 2; k++) put(qq, cyc_qmul(Q[(size_t)I[2 * k + 1]], cyc_directed(Q[(size_t)I[2 * k]], true)));
    return qq;
}
// edge 0 = (0, 1); ra further neighbours of view 0, rb of view 1, each of the former joined to each of the latter
static Edges bipartite(int ra, int rb) {
    Edges I = {0, 1};
    for (int i = 0; i < ra; i++) I.insert(I.end(), {0, 2 + i});
    for (int j = 0; j < rb; j++) I.insert(I.end(), {2 + ra + j, 1});
    for (int i = 0; i < ra; i++)
        for (int j = 0; j < rb; j++) I.insert(I.end(), {2 + i, 2 + ra + j});
    return I;
}

int main() {
    std::mt19937 rng(20241126);
    // ---- the error with the partial product kept has the bits of the error formed in one go
    {
        const CycQ q0 = unit(rng), q1 = unit(rng), q2 = unit(rng), q3 = unit(rng);
        const double e = cyc_quad_error(q0, q1, q2, q3), ep = cyc_quad_error_from(cyc_qmul(q1, q0), q2, q3);
        EXPECT(std::memcmp(&e, &ep, sizeof e) == 0);
    }
    // ---- the named shapes of tests/test_gpu_cycle_check4.py
    {
        const std::vector<CycQ> Q = views(8, rng);
        Edges I = {0, 1, 1, 2, 2, 3, 3, 0};
        CycResult R = check_graph(4, I, consistent(Q, I), 0.1);
        EXPECT(R.count == Counts({1, 1, 1, 1}) && R.ok == R.count);
        // one edge stored as (b, a), one multiplied by -1, one turned by 0.3 rad: every edge reports 0.3
        I = {0, 1, 2, 1, 2, 3, 3, 0};
        Quats qq = consistent(Q, I);
        for (int c = 0; c < 4; c++) qq[8 + (size_t)c] = -qq[8 + (size_t)c];
        const CycQ t = cyc_qmul(turn(0.3), CycQ{qq[0], qq[1], qq[2], qq[3]});
        qq[0] = t.x, qq[1] = t.y, qq[2] = t.z, qq[3] = t.w;
        R = check_graph(4, I, qq, 0.1);
        EXPECT(R.count == Counts({1, 1, 1, 1}) && R.ok == Counts({0, 0, 0, 0}) && R.summary[2] == 4);
        for (double e : R.mn) EXPECT(std::fabs(e - 0.3) <= 6e-16);
        I = {0, 1, 1, 2, 2, 0};  // a lone triangle is no quadrilateral
        R = check_graph(3, I, consistent(Q, I), 0.1);
        EXPECT(R.summary[0] == 0 && R.summary[3] == 3);
        I = {0, 1, 1, 2, 2, 3, 3, 0, 0, 2};  // a square with a diagonal: the diagonal closes triangles only
        R = check_graph(4, I, consistent(Q, I), 0.1);
        EXPECT(R.count == Counts({1, 1, 1, 1, 0}));
        I = {0, 1, 1, 2, 2, 3, 3, 0, 1, 1, 5, 5};  // self loops
        R = check_graph(7, I, consistent(Q, I), 0.1);
        EXPECT(R.count == Counts({1, 1, 1, 1, 0, 0}) && R.mn[4] == INF);
        // a parallel and a reversed duplicate of k = edge 0, and a duplicate of k1 = edge 1: the counts multiply
        I = {0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 0, 1, 2};
        R = check_graph(4, I, consistent(Q, I), 0.1);
        EXPECT(R.count == Counts({2, 3, 6, 6, 2, 2, 3}) && R.ok == R.count);
        I = {0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3};  // K4
        R = check_graph(4, I, consistent(Q, I), 0.1);
        EXPECT(R.count == Counts(6, 2) && R.ok == R.count);
        qq = consistent(Q, I);
        qq[4 * 3] = NAN;  // edge (1, 2): counted, never ok, the minimum left alone
        R = check_graph(4, I, qq, INF);
        EXPECT(R.count == Counts(6, 2) && R.ok[3] == 0 && R.mn[3] == INF && R.ok[0] == 1 && R.mn[0] <= 6e-16);
        EXPECT(R.ok[2] == 0 && R.mn[2] == INF);  // (0, 3) lies opposite: both of its quadrilaterals pass the NaN edge
        // a subset out of order with a duplicate and a self loop; bad edge ids
        I = {0, 1, 1, 2, 2, 3, 3, 0, 4, 4};
        Edges sub = {3, 4, 0, 3};
        R = check_graph(5, I, consistent(Q, I), 0.1, &sub);
        EXPECT(R.count == Counts({1, 0, 1, 1}) && R.summary[0] == 3 && R.summary[3] == 1);
        for (int32_t bad : {-1, 5}) {
            sub[1] = bad;
            EXPECT(quads_sorted(5, 5, I.data(), consistent(Q, I).data(), 0.1, 4, sub.data(), 16, 2, R) == CYC_BAD_ID);
            EXPECT(quads_reference(5, 5, I.data(), consistent(Q, I).data(), 0.1, 4, sub.data(), R) == CYC_BAD_ID);
        }
        EXPECT(quads_sorted(5, 4, I.data(), consistent(Q, I).data(), 0.1, 5, nullptr, 16, 2, R) == CYC_BAD_ID);
    }
    // ---- complete bipartite neighbourhoods: both orientations of the shorter / longer choice, across the widths
    for (int r : {7, 8, 9, 15, 16, 17, 63, 64, 65})
        for (int swap = 0; swap < 2; swap++) {
            const int ra = r + swap, rb = r + 1 - swap, n = 2 + ra + rb;
            const Edges I = bipartite(ra, rb);
            const Edges sub = {0, 1, ra + 1, (int32_t)(I.size() / 2) - 1};  // the edge, a spoke of either end, a cross edge
            const CycResult R = check_graph(n, I, consistent(views(n, rng), I), 1e-9, &sub);
            EXPECT(R.count == Counts(4, ra * rb) && R.ok == R.count);  // (the three others pass view 0 or 1 once more)
        }
    // ---- seeded random multigraphs: self loops, duplicates, reversed duplicates, NaN rows, noise around a threshold
    long long quads = 0, contradicted = 0, untested = 0;
    for (int it = 0; it < 600; it++) {
        const int n = 2 + (int)(rng() % 29), m = 1 + (int)(rng() % 90);
        const std::vector<CycQ> Q = views(n, rng);
        Edges I;
        for (int k = 0; k < m; k++) {
            const unsigned kind = rng() % 10;
            int a, b;
            if (kind == 0 && k > 0) {  // a duplicate, every other one reversed
                const size_t j = rng() % (unsigned)k;
                a = I[2 * j], b = I[2 * j + 1];
                if (rng() & 1) std::swap(a, b);
            } else {
                a = (int)(rng() % (unsigned)n);
                b = kind == 1 ? a : (int)(rng() % (unsigned)n);
            }
            I.push_back(a), I.push_back(b);
        }
        Quats qq = consistent(Q, I);
        std::uniform_real_distribution<double> U(0.0, 0.2);
        for (int k = 0; k < m; k++) {
            CycQ q{qq[4 * (size_t)k], qq[4 * (size_t)k + 1], qq[4 * (size_t)k + 2], qq[4 * (size_t)k + 3]};
            if (rng() % 4 == 0) q = cyc_qmul(turn(U(rng)), q);
            if (rng() % 7 == 0) q = CycQ{-q.x, -q.y, -q.z, -q.w};
            if (rng() % 97 == 0) q.y = NAN;
            qq[4 * (size_t)k] = q.x, qq[4 * (size_t)k + 1] = q.y, qq[4 * (size_t)k + 2] = q.z, qq[4 * (size_t)k + 3] = q.w;
        }
        Edges sub;
        for (int t = 0; t < (int)(rng() % 7); t++) sub.push_back((int32_t)(rng() % (unsigned)m));
        const CycResult R = check_graph(n, I, qq, it % 5 == 0 ? INF : U(rng), it % 3 == 0 && !sub.empty() ? &sub : nullptr);
        quads += R.summary[0], contradicted += R.summary[2], untested += R.summary[3];
    }
    EXPECT(quads > 100000 && contradicted > 500 && untested > 500);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("cycles4 host check ok (%lld quadrilaterals, %lld contradicted and %lld untested edges in the random graphs)\n",
                quads, contradicted, untested);
    return 0;
}
