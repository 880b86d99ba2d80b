// wintree_host_check.cpp -- the one-thread form of k_window_tree (irotavg_amd/csrc/wintree.hpp: nodes, keys, hooks, pointer
// jumping, the round and pass counts, the LDS layout) held against a literal Kruskal on the contracted graph and the path
// products in long double, as a stand-alone program that needs no device, meant to be built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/wintree_host_check.cpp -o wintree_host_check && ./wintree_host_check
// Exit status 0 and "wintree host check ok" when every expectation holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "winbatch.hpp"
#include "wintree.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
            failures++;                                                  \
        }                                                                \
    } while (0)

struct Problem {
    int nv, f;
    std::vector<int32_t> I, rank;  // pairs; one rank per edge
    std::vector<double> qq, Q;     // rows [x y z w]
};
struct LQ {
    long double x, y, z, w;
};
static LQ lmul(const LQ &a, const LQ &b) {
    return LQ{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
              a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}

static void unit_rows(std::mt19937 &rng, size_t rows, std::vector<double> &out) {
    std::normal_distribution<double> g;
    out.resize(4 * rows);
    for (size_t r = 0; r < rows; r++) {
        double n = 0;
        for (int c = 0; c < 4; c++) out[4 * r + c] = g(rng), n += out[4 * r + c] * out[4 * r + c];
        for (int c = 0; c < 4; c++) out[4 * r + c] /= std::sqrt(n);
    }
}

// The definition, literally: the usable edges sorted by key, a union-find over the nodes, then the rotations from the
// fixed rows along the tree. Returns the free views left outside the root's component.
static int kruskal(const Problem &P, std::vector<int32_t> &in_tree, int &rank_pos, int &rank_max, std::vector<LQ> &T) {
    const int ne = (int)P.rank.size(), nn = P.nv - P.f + 1;
    std::vector<uint64_t> keys;
    for (int k = 0; k < ne; k++)
        if (P.rank[(size_t)k] >= 0 && wt_node(P.I[2 * (size_t)k], P.f) != wt_node(P.I[2 * (size_t)k + 1], P.f))
            keys.push_back(((uint64_t)(uint32_t)P.rank[(size_t)k] << 32) | (uint32_t)k);
    std::sort(keys.begin(), keys.end());
    std::vector<int> parent((size_t)nn);
    for (int v = 0; v < nn; v++) parent[(size_t)v] = v;
    auto find = [&parent](int v) {
        while (parent[(size_t)v] != v) v = parent[(size_t)v] = parent[(size_t)parent[(size_t)v]];
        return v;
    };
    in_tree.assign((size_t)ne, 0);
    rank_pos = rank_max = 0;
    std::vector<std::vector<int>> adj((size_t)P.nv);
    for (const uint64_t key : keys) {
        const int k = (int)(uint32_t)key, a = P.I[2 * (size_t)k], b = P.I[2 * (size_t)k + 1];
        const int ra = find(wt_node(a, P.f)), rb = find(wt_node(b, P.f));
        if (ra == rb) continue;
        parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);
        in_tree[(size_t)k] = 1;
        rank_pos += (key >> 32) > 0;
        rank_max = std::max(rank_max, (int)(key >> 32));
        adj[(size_t)a].push_back(k);
        adj[(size_t)b].push_back(k);
    }
    int left = 0;
    for (int v = 1; v < nn; v++) left += find(v) != 0;
    T.assign((size_t)P.nv, LQ{0, 0, 0, 1});
    std::vector<char> seen((size_t)P.nv, 0);
    std::vector<int> queue;
    for (int u = 0; u < P.f; u++) {
        T[(size_t)u] = LQ{P.Q[4 * (size_t)u], P.Q[4 * (size_t)u + 1], P.Q[4 * (size_t)u + 2], P.Q[4 * (size_t)u + 3]};
        seen[(size_t)u] = 1;
        queue.push_back(u);
    }
    for (size_t head = 0; head < queue.size(); head++) {
        const int u = queue[head];
        for (const int k : adj[(size_t)u]) {
            const int a = P.I[2 * (size_t)k], b = P.I[2 * (size_t)k + 1], v = a == u ? b : a;
            if (seen[(size_t)v]) continue;
            LQ e{P.qq[4 * (size_t)k], P.qq[4 * (size_t)k + 1], P.qq[4 * (size_t)k + 2], P.qq[4 * (size_t)k + 3]};
            if (v == a) e.w = -e.w;  // walked from b: the inverse
            T[(size_t)v] = lmul(e, T[(size_t)u]);
            seen[(size_t)v] = 1;
            queue.push_back(v);
        }
    }
    return left;
}

static int check(const Problem &P) {
    const int ne = (int)P.rank.size();
    WinTreeHost R;
    const int rc = wintree_rounds(P.nv, P.f, ne, P.I.data(), P.rank.data(), P.qq.data(), P.Q.data(), R);
    std::vector<int32_t> in_tree;
    std::vector<LQ> T;
    int rank_pos, rank_max;
    const int left = kruskal(P, in_tree, rank_pos, rank_max, T);
    EXPECT(rc == (left ? WT_NOT_SPANNING : WT_OK));
    EXPECT(R.left == left);
    EXPECT(R.rounds <= wt_rounds(P.nv - P.f) && R.rounds <= WT_MAX_ROUNDS);  // the round bound
    EXPECT(R.flat);                                                          // the pass bound
    if (rc != WT_OK) return rc;
    EXPECT(R.in_tree == in_tree);
    EXPECT(std::count(in_tree.begin(), in_tree.end(), 1) == P.nv - P.f);
    EXPECT(R.rank_pos == rank_pos && R.rank_max == rank_max);
    for (int v = P.f; v < P.nv; v++) {  // unit measurements and unit fixed rows: |<a, b>| = cos of half the angle
        const TreeQ &g = R.T[(size_t)v];
        const LQ &w = T[(size_t)v];
        const long double dot = std::fabs(g.x * w.x + g.y * w.y + g.z * w.z + g.w * w.w);
        EXPECT(std::fabs(1.0L - dot) < 1e-12L);
    }
    if (P.rank == std::vector<int32_t>((size_t)ne, 0)) {  // rank NULL is rank 0
        WinTreeHost Z;
        EXPECT(wintree_rounds(P.nv, P.f, ne, P.I.data(), nullptr, P.qq.data(), P.Q.data(), Z) == WT_OK && Z.in_tree == R.in_tree);
    }
    return rc;
}

static Problem make(int nv, int f, const std::vector<int32_t> &I, const std::vector<int32_t> &rank, unsigned seed) {
    std::mt19937 rng(seed);
    Problem P{nv, f, I, rank, {}, {}};
    if (P.rank.empty()) P.rank.assign(I.size() / 2, 0);
    unit_rows(rng, I.size() / 2, P.qq);
    unit_rows(rng, (size_t)nv, P.Q);
    for (size_t i = 4 * (size_t)f; i < P.Q.size(); i++) P.Q[i] = std::nan("");  // free rows are never read
    return P;
}

int main() {
    // ---- the key, the ends, the counts, the layout
    EXPECT(tree_key_rank(tree_key(0x7fffffff, 639)) == 0x7fffffff && tree_key_edge(tree_key(0x7fffffff, 639)) == 639);
    EXPECT(tree_key(0x7fffffff, 639) != TREE_KEY_NONE && tree_key(0, 639) < tree_key(1, 0) && tree_key(2, 5) < tree_key(2, 6));
    EXPECT(wt_end_a(wt_ends(319, 0)) == 319 && wt_end_b(wt_ends(319, 0)) == 0 && wt_end_b(wt_ends(0, 319) | WT_IN_TREE) == 319 &&
           wt_end_a(wt_ends(0, 319) | WT_IN_TREE) == 0);
    EXPECT(wt_node(0, 3) == 0 && wt_node(2, 3) == 0 && wt_node(3, 3) == 1 && wt_view(1, 3) == 3 && wt_node(319, 256) == 64);
    EXPECT(!wt_usable(0, 2, 3, 0) && !wt_usable(4, 4, 3, 0) && !wt_usable(0, 4, 3, -1) && wt_usable(4, 0, 3, 0x7fffffff));
    EXPECT(wt_rounds(1) == 1 && wt_rounds(2) == 2 && wt_rounds(63) == 6 && wt_rounds(64) == 7);
    EXPECT(wt_passes(64, 0) == 7 && wt_passes(64, 6) == 1 && wt_passes(1, 0) == 1 && wt_passes(3, 0) == 2);
    const WinTreeLds L = wintree_lds(WT_MAX_NODES, WIN_MAX_NE);
    EXPECT(L.oRel == 0 && L.oBest == 2 * 32 * 65 && L.oVia == L.oBest + 8 * 65 && L.oComp == L.oVia + 8 * 65 &&
           L.oEnds == L.oComp + 2 * 4 * 65 && L.bytes == L.oEnds + 4 * 640 && L.bytes <= 9 * 1024);
    EXPECT(L.oBest % 8 == 0 && L.oVia % 8 == 0 && L.oComp % 4 == 0 && L.oEnds % 4 == 0 && wintree_lds(2, 1).oBest % 8 == 0);
    EXPECT(sizeof(WinTreeResult) % 8 == 0);

    // ---- named shapes
    typedef std::vector<int32_t> V;
    EXPECT(check(make(2, 1, V{0, 1}, V{}, 1)) == WT_OK);
    EXPECT(check(make(2, 1, V{1, 0}, V{}, 2)) == WT_OK);
    EXPECT(check(make(4, 3, V{0, 3, 3, 1, 2, 3, 3, 2}, V{2, 1, 1, 0}, 3)) == WT_OK);               // one free view, the ranks decide
    EXPECT(check(make(5, 2, V{0, 1, 1, 0, 2, 2, 0, 2, 2, 3, 3, 4, 4, 2}, V{0, 0, 0, 1, 0, 0, 0}, 4)) == WT_OK);  // fixed-fixed, a self loop
    EXPECT(check(make(4, 2, V{0, 2, 2, 3}, V{0, -1}, 5)) == WT_NOT_SPANNING);                        // the cut
    EXPECT(check(make(4, 2, V{0, 2, 2, 3, 3, 2}, V{0, -1, 0x7fffffff}, 6)) == WT_OK);                // ... and the next key
    EXPECT(check(make(5, 3, V{2, 4, 0, 3}, V{}, 7)) == WT_OK);                                      // fixed view 1 is isolated
    {
        V chain, star, own;  // 64 free views: a chain listed backwards, a star, one fixed view each
        for (int v = 64; v >= 1; v--) chain.push_back(v - 1), chain.push_back(v);
        for (int v = 1; v <= 64; v++) star.push_back(v), star.push_back(0);
        for (int v = 0; v < 64; v++) own.push_back(256 + v), own.push_back(v);
        EXPECT(check(make(65, 1, chain, V{}, 8)) == WT_OK);
        EXPECT(check(make(65, 1, star, V{}, 9)) == WT_OK);
        EXPECT(check(make(320, 256, own, V{}, 10)) == WT_OK);
        V up(64);  // the chain again, ranks rising towards the root: every node's own smallest key points away from it
        for (int k = 0; k < 64; k++) up[(size_t)k] = k;
        EXPECT(check(make(65, 1, chain, up, 11)) == WT_OK);
    }

    // ---- seeded random multigraphs up to the limits: self loops, duplicates, negative ranks, some not spanning
    std::mt19937 rng(20240607);
    int spanning = 0, cut = 0;
    for (int it = 0; it < 4000; it++) {
        const int nu = it % 7 == 0 ? WIN_MAX_NU : 1 + (int)(rng() % WIN_MAX_NU);
        const int f = it % 5 == 0 ? 1 : 1 + (int)(rng() % (unsigned)(WIN_MAX_NV - nu)), nv = nu + f;
        const int ne = it % 11 == 0 ? WIN_MAX_NE : nu + (int)(rng() % (unsigned)(WIN_MAX_NE - nu + 1));
        V I, rank;
        for (int k = 0; k < ne; k++) {
            int a = (int)(rng() % (unsigned)nv), b = (int)(rng() % (unsigned)nv);
            if (k < nu && it % 3 != 0) a = f + k, b = k == 0 ? 0 : f + (int)(rng() % (unsigned)k);  // (mostly: a spanning backbone)
            if (rng() % 16 == 0) b = a;
            if (k > 0 && rng() % 8 == 0) a = I[2 * (size_t)(k - 1) + 1], b = I[2 * (size_t)(k - 1)];  // the edge before, reversed
            I.push_back(a);
            I.push_back(b);
            rank.push_back(rng() % 4 == 0 ? (it % 2 ? -1 : 3) : (int32_t)(rng() % 3));
        }
        (check(make(nv, f, I, rank, 100u + (unsigned)it)) == WT_OK ? spanning : cut)++;
    }
    EXPECT(spanning > 1000 && cut > 100);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("wintree host check ok (%d spanning, %d cut)\n", spanning, cut);
    return 0;
}
