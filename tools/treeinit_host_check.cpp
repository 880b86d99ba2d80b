// treeinit_host_check.cpp -- the pieces the kernels of the spanning-tree initialiser run (irotavg_amd/csrc/treeinit.hpp:
// the key, the offer, the hook with its mutual pick, the pointer jumping over two copies of the state, the finishing
// product) as tree_rounds, held against tree_reference (Kruskal over the sorted keys and a long-double propagation from
// view 0), as a stand-alone program that needs no device, meant to be built with a sanitizer:
//   g++ -std=c++17 -g -O2 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/treeinit_host_check.cpp -o treeinit_host_check && ./treeinit_host_check
// Exit status 0 and "treeinit host check ok" when every expectation holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>

#include "treeinit.hpp"

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
typedef std::vector<int32_t> Ranks;

static std::mt19937_64 rng(20240917);
static double uniform() { return std::uniform_real_distribution<double>(-1.0, 1.0)(rng); }
static void push_unit(Quats &q) {
    double v[4], s = 0;
    do {
        s = 0;
        for (double &c : v) c = uniform(), s += c * c;
    } while (s < 0.01 || s > 1.0);
    for (double c : v) q.push_back(c / std::sqrt(s));
}
static Quats random_quats(size_t m) {
    Quats q;
    for (size_t k = 0; k < m; k++) push_unit(q);
    return q;
}

// the angular distance 2 acos |<p, q>| in the form that keeps its precision near 0: the angle of p (x) q^-1
static double angle(const TreeQ p, const TreeQ q) {
    const long double w = (long double)p.w * q.w + (long double)p.x * q.x + (long double)p.y * q.y + (long double)p.z * q.z;
    const long double x = (long double)p.x * q.w - (long double)p.w * q.x - (long double)p.y * q.z + (long double)p.z * q.y;
    const long double y = (long double)p.y * q.w - (long double)p.w * q.y - (long double)p.z * q.x + (long double)p.x * q.z;
    const long double z = (long double)p.z * q.w - (long double)p.w * q.z - (long double)p.x * q.y + (long double)p.y * q.x;
    return (double)(2 * atan2l(sqrtl(x * x + y * y + z * z), fabsl(w)));
}

struct Outcome {
    int status;
    TreeResult rounds, ref;
    double worst;
};
// tree_rounds against tree_reference: the same status, in_tree, info, and rows within 64 n_total 2.2e-16 rad
static Outcome check_graph(int64_t n_total, int f, const Edges &I, const Quats &qq, const Ranks *rank) {
    const int64_t m = (int64_t)I.size() / 2;
    Outcome o;
    const TreeQ q0{0.5, -0.5, 0.5, 0.5};
    const int32_t *rk = rank ? rank->data() : nullptr;
    o.status = tree_rounds(m, n_total, f, I.data(), qq.data(), rk, q0, o.rounds);
    const int ref = tree_reference(m, n_total, f, I.data(), qq.data(), rk, q0, o.ref);
    o.worst = 0;
    EXPECT(o.status == ref);
    EXPECT(o.status != TREE_INTERNAL);
    if (o.status == TREE_OK || o.status == TREE_NOT_SPANNING) EXPECT(std::memcmp(o.rounds.info, o.ref.info, sizeof(o.ref.info)) == 0);
    if (o.status != TREE_OK || ref != TREE_OK) return o;
    EXPECT(o.rounds.in_tree == o.ref.in_tree);
    EXPECT(std::accumulate(o.rounds.in_tree.begin(), o.rounds.in_tree.end(), 0LL) == n_total - 1);
    EXPECT(o.rounds.info[1] == 1);
    const double tol = 64.0 * (double)n_total * 2.2e-16;
    for (int64_t v = f; v < n_total; v++) o.worst = std::max(o.worst, angle(o.rounds.T[(size_t)v], o.ref.T[(size_t)v]));
    EXPECT(o.worst <= tol);
    return o;
}

static Edges path_edges(int n) {
    Edges I;
    for (int i = 0; i + 1 < n; i++) I.push_back(i), I.push_back(i + 1);
    return I;
}
// the edges (i, i + 1) of a path listed by the ruler function of i + 1 (the number of times 2 divides it), then by i
static Edges ruler_path(int n) {
    std::vector<std::pair<int, int>> order;
    for (int i = 0; i + 1 < n; i++) {
        int level = 0;
        while (((i + 1) >> level & 1) == 0) level++;
        order.push_back({level, i});
    }
    std::sort(order.begin(), order.end());
    Edges I;
    for (const auto &p : order) I.push_back(p.second), I.push_back(p.second + 1);
    return I;
}
static Edges reversed(const Edges &I) {
    Edges R;
    for (size_t k = I.size() / 2; k-- > 0;) R.push_back(I[2 * k]), R.push_back(I[2 * k + 1]);
    return R;
}
static Quats reversed_rows(const Quats &q) {
    Quats R;
    for (size_t k = q.size() / 4; k-- > 0;) R.insert(R.end(), q.begin() + 4 * (long)k, q.begin() + 4 * (long)k + 4);
    return R;
}

static void named_shapes() {
    {  // two views, one edge, forward and backward; the mutual pick at n_total = 2
        const Quats q = random_quats(1);
        Outcome a = check_graph(2, 1, Edges{0, 1}, q, nullptr), b = check_graph(2, 1, Edges{1, 0}, q, nullptr);
        EXPECT(a.status == TREE_OK && b.status == TREE_OK && a.rounds.info[0] == 1 && b.rounds.info[0] == 1);
        EXPECT(angle(a.rounds.T[1], b.rounds.T[1]) > 1e-3);  // (the direction matters)
    }
    {  // a 5-chain in order and reversed: the same tree and the same rows
        const Edges I = path_edges(5);
        const Quats q = random_quats(4);
        Outcome a = check_graph(5, 1, I, q, nullptr), b = check_graph(5, 1, reversed(I), reversed_rows(q), nullptr);
        EXPECT(a.status == TREE_OK && b.status == TREE_OK);
        for (size_t v = 1; v < 5; v++) EXPECT(angle(a.rounds.T[v], b.rounds.T[v]) <= 64.0 * 5 * 2.2e-16);
    }
    {  // the mutual pick inside a 4-path; the final representative is not view 0
        Outcome a = check_graph(4, 1, Edges{1, 2, 0, 1, 2, 3}, random_quats(3), nullptr);
        EXPECT(a.status == TREE_OK && a.rounds.info[0] == 1);
        Outcome b = check_graph(3, 1, Edges{1, 2, 0, 1}, random_quats(2), nullptr);
        EXPECT(b.status == TREE_OK);
    }
    {  // a path of 300 in order: one round, a hook chain of 299, nine passes that move; by the ruler function: pairs
        Outcome a = check_graph(300, 1, path_edges(300), random_quats(299), nullptr);
        EXPECT(a.status == TREE_OK && a.rounds.info[0] == 1 && a.rounds.jumps_max <= 9 && a.rounds.jumps_max >= 8);
        Outcome b = check_graph(300, 1, ruler_path(300), random_quats(299), nullptr);
        // 300 -> 150 -> 75 -> 37 -> 18 -> 9 -> 4 -> 2 -> 1: components at least halve, so eight rounds are the most 300
        // views can take (an odd one out has an edge that leaves it, and joins in the same round)
        EXPECT(b.status == TREE_OK && b.rounds.info[0] == 8);
    }
    {  // rank: a triangle whose lowest-index edge has rank 2 is avoided; as a bridge it is used; with rank -1 it is not
        const Edges tri{0, 1, 1, 2, 2, 0};
        const Ranks r2{2, 0, 0};
        Outcome a = check_graph(3, 1, tri, random_quats(3), &r2);
        EXPECT(a.status == TREE_OK && a.rounds.info[2] == 0 && a.rounds.info[3] == 0 && a.rounds.in_tree == Ranks({0, 1, 1}));
        const Edges bridge{0, 1, 1, 2, 2, 0, 3, 4, 4, 5, 5, 3, 2, 3};
        Ranks rb{0, 0, 0, 0, 0, 0, 2};
        Outcome b = check_graph(6, 1, bridge, random_quats(7), &rb);
        EXPECT(b.status == TREE_OK && b.rounds.info[2] == 1 && b.rounds.info[3] == 2 && b.rounds.in_tree[6] == 1);
        rb[6] = -1;
        Outcome c = check_graph(6, 1, bridge, random_quats(7), &rb);
        EXPECT(c.status == TREE_NOT_SPANNING && c.rounds.info[1] == 2);
    }
    {  // self loops, parallel edges, reversed duplicates, an edge between fixed views, a free view behind a fixed one
        const Edges I{1, 1, 0, 1, 0, 1, 1, 0, 1, 2, 2, 3, 3, 2, 0, 2, 4, 4};
        Outcome a = check_graph(4, 3, I, random_quats(9), nullptr);
        EXPECT(a.status == TREE_BAD_ID);  // (view 4 of the last self loop is outside 4 views)
        Outcome b = check_graph(5, 3, I, random_quats(9), nullptr);
        EXPECT(b.status == TREE_NOT_SPANNING && b.rounds.info[1] == 2);  // view 4 has a self loop alone: isolated
        Edges J(I.begin(), I.end() - 2);
        Outcome c = check_graph(4, 3, J, random_quats(8), nullptr);
        EXPECT(c.status == TREE_OK && c.rounds.in_tree == Ranks({0, 1, 0, 0, 1, 1, 0, 0}));
    }
    for (int n : {255, 256, 257, 1023, 1024, 1025}) {  // around one workgroup pass: a random tree and some chords
        Edges I;
        for (int v = 1; v < n; v++) I.push_back((int32_t)(rng() % (uint64_t)v)), I.push_back(v);
        while ((int)I.size() / 2 < n) I.push_back((int32_t)(rng() % (uint64_t)n)), I.push_back((int32_t)(rng() % (uint64_t)n));
        Outcome a = check_graph(n, 1, I, random_quats(I.size() / 2), nullptr);
        EXPECT(a.status == TREE_OK);
    }
}

static void random_multigraphs(int count) {
    int spanning = 0, not_spanning = 0;
    double worst = 0;
    for (int t = 0; t < count; t++) {
        // enough edges per view that the ranks of -1 and the self loops rarely cut a graph by themselves
        const int m = 1 + (int)(rng() % 1500), n = 2 + (int)(rng() % (uint64_t)std::min(299, std::max(1, m / 5)));
        const bool cut = rng() % 5 == 0;  // about a fifth: no edge crosses between the views below `half` and the others
        const int half = 1 + (int)(rng() % (uint64_t)(n - 1));
        Edges I;
        Ranks rank;
        auto side = [&](bool low) { return low ? (int32_t)(rng() % (uint64_t)half) : (int32_t)(half + rng() % (uint64_t)(n - half)); };
        for (int k = 0; k < m; k++) {
            int32_t a, b;
            const unsigned kind = (unsigned)(rng() % 16);
            if (k > 0 && kind == 0) a = I[2 * (size_t)(k - 1)], b = I[2 * (size_t)(k - 1) + 1];       // a duplicate
            else if (k > 0 && kind == 1) a = I[2 * (size_t)(k - 1) + 1], b = I[2 * (size_t)(k - 1)];  // a reversed duplicate
            else if (kind == 2) a = b = (int32_t)(rng() % (uint64_t)n);                              // a self loop
            else if (cut) {
                const bool low = rng() % 2 == 0;
                a = side(low), b = side(low);
            } else
                a = (int32_t)(rng() % (uint64_t)n), b = (int32_t)(rng() % (uint64_t)n);
            I.push_back(a), I.push_back(b);
            rank.push_back((int32_t)(rng() % 5) - 1);  // -1 .. 3
        }
        Outcome o = check_graph(n, 1 + (int)(rng() % 3) % n, I, random_quats((size_t)m), t % 7 == 0 ? nullptr : &rank);
        EXPECT(o.status == TREE_OK || o.status == TREE_NOT_SPANNING);
        (o.status == TREE_OK ? spanning : not_spanning)++;
        worst = std::max(worst, o.worst);
    }
    std::printf("random multigraphs: %d spanning, %d not, largest deviation %.3g rad\n", spanning, not_spanning, worst);
    EXPECT(spanning > count / 4 && not_spanning > count / 10);
}

int main() {
    EXPECT(tree_key(0, 5) < tree_key(1, 0) && tree_key(3, 0x7fffffffu) < TREE_KEY_NONE && tree_key(0x7fffffff, 0x7fffffffu) < TREE_KEY_NONE);
    EXPECT(tree_key_edge(tree_key(2, 77)) == 77 && tree_key_rank(tree_key(2, 77)) == 2);
    EXPECT(tree_jump_passes(1) == 1 && tree_jump_passes(2) == 2 && tree_jump_passes(300) == 10 && tree_jump_passes(0x7fffffff) == 32);
    named_shapes();
    random_multigraphs(4000);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("treeinit host check ok\n");
    return 0;
}
