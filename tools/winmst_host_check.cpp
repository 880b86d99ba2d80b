// winmst_host_check.cpp -- the restatement of irotavg_init_mst that k_window_mst_user runs (irotavg_amd/csrc/winmst.hpp:
// arrival labels, the first visit of an edge after a label, the relaxation to the least fixed point) held against a
// literal transcription of the sequential sweep, as a stand-alone program that needs no device, meant to be built with a
// sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/winmst_host_check.cpp -o winmst_host_check && ./winmst_host_check
// Exit status 0 and "winmst host check ok" when every expectation holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "winbatch.hpp"
#include "winmst.hpp"

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

// the fixed point again, relaxing the edges in the order `order` gives them (any order must reach the same labels)
static std::vector<uint32_t> relax_in_order(int nv, const Edges &I, const std::vector<int> &order) {
    std::vector<uint32_t> L((size_t)nv, MST_INF);
    L[0] = MST_ROOT;
    for (int r = 0; r < nv + 1; r++) {
        bool changed = false;
        for (int k : order) {
            const int a = I[2 * (size_t)k], b = I[2 * (size_t)k + 1];
            if (a == b) continue;
            const uint32_t lb = mst_first_visit(L[(size_t)b], (uint32_t)k);  // (the other direction first)
            if (lb < L[(size_t)a]) L[(size_t)a] = lb, changed = true;
            const uint32_t la = mst_first_visit(L[(size_t)a], (uint32_t)k);
            if (la < L[(size_t)b]) L[(size_t)b] = la, changed = true;
        }
        if (!changed) break;
    }
    return L;
}

// relaxation against the sweep: the same verdict, and on success the same parent edge and direction for every view
static int check_graph(int nv, const Edges &I, std::mt19937 *rng = nullptr) {
    const int ne = (int)I.size() / 2;
    MstTree R, S;
    const int rr = mst_relax(nv, ne, I.data(), R), rs = mst_sequential(nv, ne, I.data(), S);
    EXPECT(rr == rs);
    EXPECT(R.rounds <= nv + 1);
    if (rr != MST_OK || rs != MST_OK) return rs;
    EXPECT(R.edge == S.edge);
    EXPECT(R.forward == S.forward);
    EXPECT(R.label[0] == MST_ROOT);
    for (int v = 1; v < nv; v++) {
        const uint32_t L = R.label[(size_t)v];
        EXPECT(L >= 1 && L <= mst_label((uint32_t)S.rounds - 1, (uint32_t)ne - 1));  // a visit of one of the sweeps that ran
        EXPECT(mst_edge_of(L) < (uint32_t)ne);
        const int k = R.edge[(size_t)v], u = R.forward[(size_t)v] ? I[2 * (size_t)k] : I[2 * (size_t)k + 1];
        EXPECT((R.forward[(size_t)v] ? I[2 * (size_t)k + 1] : I[2 * (size_t)k]) == v && u != v);
        EXPECT(R.label[(size_t)u] < L);                                        // the parent arrived first
        EXPECT(mst_first_visit(R.label[(size_t)u], (uint32_t)k) == L);
    }
    std::vector<int> order((size_t)ne);
    for (int k = 0; k < ne; k++) order[(size_t)k] = ne - 1 - k;
    EXPECT(relax_in_order(nv, I, order) == R.label);
    if (rng) {
        std::shuffle(order.begin(), order.end(), *rng);
        EXPECT(relax_in_order(nv, I, order) == R.label);
    }
    return rs;
}

// a chain 0 - 1 - ... - (nv - 1), its edges listed from the far end (reversed: one view per sweep) or from view 0 (one
// sweep), padded to m edges with duplicates of its farthest edge placed in front of them: they are of use in the last
// sweep alone, where the first of them wins over the chain's own copy
static Edges chain(int nv, bool reversed, int m = 0) {
    Edges T, I;
    for (int v = 0; v + 1 < nv; v++) {
        const int a = reversed ? nv - 2 - v : v;
        T.push_back(a);
        T.push_back(a + 1);
    }
    const int pad = std::max(0, m - (nv - 1));
    for (int k = 0; k < pad; k++) {
        I.push_back(k & 1 ? nv - 1 : nv - 2);  // every other duplicate turned round
        I.push_back(k & 1 ? nv - 2 : nv - 1);
    }
    I.insert(I.end(), T.begin(), T.end());
    return I;
}

int main() {
    // ---- the encoding
    EXPECT(mst_first_visit(MST_ROOT, 0) == 1 && mst_first_visit(MST_ROOT, 6) == 7);
    EXPECT(mst_first_visit(MST_INF, 3) == MST_INF);
    EXPECT(mst_first_visit(mst_label(0, 2), 3) == mst_label(0, 3));  // later in the same sweep
    EXPECT(mst_first_visit(mst_label(0, 2), 2) == mst_label(1, 2));  // strictly after: the next sweep
    EXPECT(mst_first_visit(mst_label(4, 6), 0) == mst_label(5, 0));
    EXPECT(mst_edge_of(mst_label(4, 6)) == 6 && mst_edge_of(mst_label(0, 0)) == 0 && mst_edge_of(mst_label(318, 639)) == 639);
    EXPECT((MST_STRIDE & (MST_STRIDE - 1)) == 0 && MST_STRIDE >= (uint32_t)WIN_MAX_NE);
    EXPECT(mst_label(WIN_MAX_NV - 1, WIN_MAX_NE - 1) < (1u << 31));   // a sweep past the last one any window can need
    for (uint32_t s = 0; s < 320; s += 29)
        for (uint32_t ku = 0; ku < 640; ku += 71)
            for (uint32_t k = 0; k < 640; k += 53) {
                const uint32_t L = mst_label(s, ku), F = mst_first_visit(L, k);
                EXPECT(F > L && F - L <= MST_STRIDE && mst_edge_of(F) == k);  // the very next visit of k
                EXPECT(F == mst_label(k > ku ? s : s + 1, k));
            }
    // ---- the named shapes of tests/test_gpu_window_init_batch.py
    EXPECT(check_graph(2, {0, 1}) == MST_OK);
    EXPECT(check_graph(2, {1, 0}) == MST_OK);
    {
        MstTree S;
        const Edges rev = chain(6, true), fwd = chain(6, false);
        EXPECT(check_graph(6, rev) == MST_OK && mst_sequential(6, 5, rev.data(), S) == MST_OK && S.rounds == 5);
        EXPECT(check_graph(6, fwd) == MST_OK && mst_sequential(6, 5, fwd.data(), S) == MST_OK && S.rounds == 1);
    }
    {  // the ordering trap: view 3 takes the later duplicate in sweep 0, not the earlier one in sweep 1
        const Edges I = {2, 3, 0, 1, 1, 2, 2, 3};
        MstTree R;
        EXPECT(check_graph(4, I) == MST_OK && mst_relax(4, 4, I.data(), R) == MST_OK && R.edge[3] == 3 && R.label[3] == 4);
    }
    EXPECT(check_graph(4, {1, 1, 0, 1, 2, 1, 1, 2, 0, 1, 3, 2}) == MST_OK);         // self-loop, opposite directions, duplicate
    EXPECT(check_graph(5, {1, 2, 0, 1, 2, 0, 3, 2, 2, 4}) == MST_OK);               // an edge between two fixed views (f = 3)
    EXPECT(check_graph(4, {0, 2, 2, 3}) == MST_NOT_SPANNING);                       // view 1 isolated
    EXPECT(check_graph(3, {0, 1, 1, 3}) == MST_BAD_ID);
    EXPECT(check_graph(3, {0, 1, -1, 2}) == MST_BAD_ID);
    for (int m : {63, 64, 65, 255, 256, 257, 640})
        for (int nv : {64, 65, 320})
            if (m >= nv - 1) {
                EXPECT(check_graph(nv, chain(nv, false, m)) == MST_OK);
                EXPECT(check_graph(nv, chain(nv, true, m)) == MST_OK);
            }
    // ---- the limits: a reversed chain over 320 views padded to 640 edges takes 319 sweeps and gives the largest label
    {
        const Edges I = chain(WIN_MAX_NV, true, WIN_MAX_NE);
        MstTree R, S;
        EXPECT((int)I.size() == 2 * WIN_MAX_NE);
        EXPECT(mst_relax(WIN_MAX_NV, WIN_MAX_NE, I.data(), R) == MST_OK);
        EXPECT(mst_sequential(WIN_MAX_NV, WIN_MAX_NE, I.data(), S) == MST_OK && S.rounds == WIN_MAX_NV - 1);
        EXPECT(R.edge == S.edge && R.forward == S.forward);
        EXPECT(R.peak == mst_label(WIN_MAX_NV - 2, 0) && R.edge[WIN_MAX_NV - 1] == 0);  // the first duplicate
        EXPECT(R.peak < (1u << 31) && (uint64_t)WIN_MAX_NV * MST_STRIDE + 1 < (1ull << 31));  // no label can pass 2^31
        EXPECT(R.rounds <= WIN_MAX_NV + 1);
        WinBatchPlan P;
        const int32_t sizes[3] = {WIN_MAX_NV, WIN_MAX_NV - WIN_MAX_NU, WIN_MAX_NE};
        EXPECT(winbatch_plan(1, sizes, 1, P) && P.desc[0].nv == WIN_MAX_NV);
        EXPECT(winmst_lds_bytes(WIN_MAX_NV, WIN_MAX_NE) < 20 * 1024);
    }
    // ---- seeded random graphs up to the window limits: duplicates, self-loops, both directions; about a fifth do not span
    std::mt19937 rng(20240611);
    int spanning = 0, not_spanning = 0, most_rounds = 0;
    for (int it = 0; it < 4000; it++) {
        const bool small = it % 4 != 0;
        const int nv = 2 + (int)(rng() % (small ? 38 : WIN_MAX_NV - 1));
        const int ne = 1 + (int)(rng() % (small ? 129 : WIN_MAX_NE));
        Edges I;
        const int kind = (int)(rng() % 5);
        if (kind != 0 && ne >= nv - 1) {  // around a random spanning tree, its edges anywhere in the list
            std::vector<int> slot((size_t)ne);
            for (int k = 0; k < ne; k++) slot[(size_t)k] = k;
            std::shuffle(slot.begin(), slot.end(), rng);
            I.assign(2 * (size_t)ne, 0);
            for (int k = 0; k < ne; k++) {
                int a, b;
                if (k < nv - 1) {
                    a = (int)(rng() % (unsigned)(k + 1));
                    b = k + 1;
                } else {
                    a = (int)(rng() % (unsigned)nv);
                    b = (int)(rng() % (unsigned)nv);  // (a == b: a self-loop)
                }
                if (rng() & 1) std::swap(a, b);
                I[2 * (size_t)slot[(size_t)k]] = a;
                I[2 * (size_t)slot[(size_t)k] + 1] = b;
            }
            if (kind == 1) {  // relabel all but view 0 so that tree order and id order differ
                std::vector<int> p((size_t)nv);
                for (int v = 0; v < nv; v++) p[(size_t)v] = v;
                std::shuffle(p.begin() + 1, p.end(), rng);
                for (int32_t &x : I) x = p[(size_t)x];
            }
        } else {
            for (int k = 0; k < 2 * ne; k++) I.push_back((int32_t)(rng() % (unsigned)nv));
        }
        const int rc = check_graph(nv, I, &rng);
        EXPECT(rc == MST_OK || rc == MST_NOT_SPANNING);
        (rc == MST_OK ? spanning : not_spanning)++;
        MstTree R;
        (void)mst_relax(nv, ne, I.data(), R);
        most_rounds = std::max(most_rounds, R.rounds);
    }
    EXPECT(spanning > 2000 && not_spanning > 300);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("winmst host check ok (%d spanning, %d not spanning, at most %d rounds)\n", spanning, not_spanning, most_rounds);
    return 0;
}
