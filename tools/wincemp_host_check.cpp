// wincemp_host_check.cpp -- the index math of k_window_cemp (irotavg_amd/csrc/wincemp.hpp: the packed half-edge word, the
// sorting network, the row-start table, the walk of the lanes of a group) run on one thread and held against a literal
// triple loop over the edges, as a stand-alone program that needs no device, meant to be built with a sanitizer:
//   g++ -std=c++17 -g -O2 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/wincemp_host_check.cpp -o wincemp_host_check && ./wincemp_host_check
// Exit status 0 and "wincemp host check ok" when every expectation holds. The floating-point value of s is not this
// program's matter (tests/test_gpu_window_cemp_batch.py).
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "winbatch.hpp"
#include "wincemp.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
            failures++;                                                  \
        }                                                                \
    } while (0)

typedef std::vector<int32_t> Edges;                // pairs
typedef std::array<uint32_t, 5> Triple;            // k, k1, k1 against, k2, k2 against
struct Collect {
    uint32_t k;
    std::vector<Triple> *out;
    void operator()(uint32_t k1, bool g1, uint32_t k2, bool g2) { out->push_back(Triple{k, k1, g1, k2, g2}); }
};

// the kernel's way: emit, pad, the network stage by stage, the row starts, every edge on its eight lanes
static std::vector<Triple> kernel_way(int nv, const Edges &I) {
    const int ne = (int)I.size() / 2, n2 = 2 * ne, N = wc_sort_len(n2);
    std::vector<uint32_t> w((size_t)N, WC_NONE), sorted;
    for (int k = 0; k < ne; k++) wc_emit((uint32_t)k, (uint32_t)I[2 * (size_t)k], (uint32_t)I[2 * (size_t)k + 1], &w[2 * (size_t)k]);
    sorted = w;
    std::sort(sorted.begin(), sorted.end());
    int stages = 0;
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1, stages++)
            for (int i = N - 1; i >= 0; i--) wc_bitonic(w.data(), i, j, k);  // (any order of the positions of a stage)
    EXPECT(w == sorted);
    EXPECT(N >= n2 && N < 2 * std::max(n2, 2) && stages <= 66);
    std::vector<int> start((size_t)nv + 1);
    for (int u = 0; u <= nv; u++) start[(size_t)u] = wc_row_start(w.data(), n2, (uint32_t)u);
    for (int u = 0; u < nv; u++)
        for (int i = start[(size_t)u]; i < start[(size_t)u + 1]; i++) EXPECT(wc_from(w[(size_t)i]) == (uint32_t)u);
    EXPECT(start[0] == 0 && (start[(size_t)nv] == n2 || w[(size_t)start[(size_t)nv]] == WC_NONE));
    std::vector<Triple> out;
    for (int k = 0; k < ne; k++) {
        const uint32_t a = (uint32_t)I[2 * (size_t)k], b = (uint32_t)I[2 * (size_t)k + 1];
        EXPECT(wc_end_a(wc_ends(a, b)) == a && wc_end_b(wc_ends(a, b)) == b);
        if (a == b) continue;
        const WcRows r = wc_rows(start.data(), a, b);
        EXPECT(r.x1 - r.x0 <= r.l1 - r.l0);
        Collect sink{(uint32_t)k, &out};
        for (int lane = 0; lane < WC_GROUP; lane++) wc_lane(w.data(), r, lane, sink);
    }
    std::sort(out.begin(), out.end());
    return out;
}

// the definition: every ordered pair (k1, k2), k1 joining b and c, k2 joining c and a, c outside {a, b}, no self loop
static std::vector<Triple> literal(const Edges &I) {
    const int ne = (int)I.size() / 2;
    std::vector<Triple> out;
    for (int k = 0; k < ne; k++) {
        const int a = I[2 * (size_t)k], b = I[2 * (size_t)k + 1];
        if (a == b) continue;
        for (int k1 = 0; k1 < ne; k1++) {
            const int p = I[2 * (size_t)k1], q = I[2 * (size_t)k1 + 1];
            if (p == q || (p != b && q != b)) continue;
            const int c = p == b ? q : p;
            if (c == a || c == b) continue;
            for (int k2 = 0; k2 < ne; k2++) {
                const int u = I[2 * (size_t)k2], v = I[2 * (size_t)k2 + 1];
                if (!((u == c && v == a) || (u == a && v == c))) continue;
                out.push_back(Triple{(uint32_t)k, (uint32_t)k1, (uint32_t)(p != b), (uint32_t)k2, (uint32_t)(u != c)});
            }
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}

static size_t check_graph(int nv, const Edges &I) {
    const std::vector<Triple> got = kernel_way(nv, I), want = literal(I);
    EXPECT(got == want);
    return want.size();
}

static Edges book(int pages) {  // hub edge (0, 1), a page per view 2 .. pages + 1; some hub and page edges doubled, a self loop
    Edges I{0, 1, 1, 0, 0, 1};
    for (int c = 2; c < pages + 2; c++) {
        I.insert(I.end(), {1, c, c, 0});
        if (c % 3 == 0) I.insert(I.end(), {c, 1});
        if (c % 5 == 0) I.insert(I.end(), {0, c, 0, c});
    }
    I.insert(I.end(), {1, 1});
    return I;
}
static Edges band(int m) {  // three predecessors per view, cut at m edges
    Edges I;
    for (int v = 1; (int)I.size() < 2 * m; v++)
        for (int p = 1; p <= 3 && p <= v && (int)I.size() < 2 * m; p++) I.insert(I.end(), {v - p, v});
    return I;
}
static int views_of(const Edges &I) { return *std::max_element(I.begin(), I.end()) + 1; }

int main() {
    {  // the word at the limits
        const uint32_t w = wc_pack(WIN_MAX_NV - 1, WIN_MAX_NV - 1, 2 * WIN_MAX_NE - 1);
        EXPECT(wc_from(w) == 319 && wc_to(w) == 319 && wc_val(w) == 1279 && wc_val_edge(wc_val(w)) == 639 && wc_val_against(wc_val(w)));
        EXPECT(w < WC_NONE && wc_from(WC_NONE) >= (uint32_t)WIN_MAX_NV);
        EXPECT(wc_pack(1, 0, 0) > wc_pack(0, 319, 1279) && wc_pack(0, 1, 0) > wc_pack(0, 0, 1279));
        EXPECT(wc_sort_len(1280) == 2048 && wc_sort_len(1024) == 1024 && wc_sort_len(2) == 2);
    }
    {  // the LDS layout
        constexpr WinCempLds L = wincemp_lds(WIN_MAX_NV, WIN_MAX_NE);
        EXPECT(L.bytes <= WINCEMP_LDS_BUDGET && 3 * L.bytes <= WIN_MAX_LDS);
        EXPECT(L.oQQ % 32 == 0 && L.oS % 8 == 0 && L.oW % 4 == 0 && L.oStart % 4 == 0 && L.oEnds % 4 == 0 && L.oUsed % 4 == 0);
        EXPECT(L.oUsed + 4 * (size_t)WIN_MAX_NE <= L.bytes);
        EXPECT(wincemp_lds(2, 1).bytes >= 32 + 16 + 8 + 12 + 8);
    }
    size_t triangles = 0;
    int graphs = 0;
    // the named shapes of the GPU test
    triangles += check_graph(3, Edges{0, 1, 1, 2, 2, 0}), graphs++;
    triangles += check_graph(5, Edges{0, 1, 1, 2, 2, 3, 3, 4}), graphs++;
    for (int p : {1, 7, 8, 9, 17, 65}) triangles += check_graph(p + 2, book(p)), graphs++;
    for (int m : {31, 32, 33, 255, 256, 257, 511, 512, 513, 640}) triangles += check_graph(views_of(band(m)), band(m)), graphs++;
    triangles += check_graph(WIN_MAX_NV, band(100)), graphs++;  // the upper views isolated
    {  // a 36-clique: 630 edges, every row 35 long
        Edges I;
        for (int a = 0; a < 36; a++)
            for (int b = a + 1; b < 36; b++) I.insert(I.end(), {(a + b) % 2 ? a : b, (a + b) % 2 ? b : a});
        triangles += check_graph(36, I), graphs++;
    }
    // seeded random multigraphs with self loops, parallel and reversed edges; every twentieth near the limits
    std::mt19937 rng(20240607u);
    for (int g = 0; g < 400; g++) {
        const bool big = g % 20 == 19;
        const int nv = big ? 200 + (int)(rng() % 121) : 2 + (int)(rng() % 39);
        const int ne = big ? 500 + (int)(rng() % 141) : 1 + (int)(rng() % 120);
        const int span = 1 + (int)(rng() % (big ? 12 : nv));  // small: dense neighbourhoods and many parallel edges
        Edges I;
        for (int k = 0; k < ne; k++) {
            const int a = (int)(rng() % (unsigned)nv);
            int b = (a + (int)(rng() % (unsigned)(span + 1))) % nv;
            if (rng() % 16 == 0) b = a;
            if (rng() % 2) I.insert(I.end(), {a, b});
            else I.insert(I.end(), {b, a});
        }
        triangles += check_graph(nv, I), graphs++;
    }
    EXPECT(triangles > 100000);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("wincemp host check ok (%d graphs, %zu triangles)\n", graphs, triangles);
    return 0;
}
