// wincemp.hpp -- the index math of k_window_cemp (wincemp.hip: irotavg_window_cemp_batch_dev, docs/window_cemp_batch.md):
// cycle-edge message passing over the triangles of ONE window-size problem whose half-edges, measurements and estimates
// all live in LDS. The packed half-edge word, one compare-exchange of the sorting network, the row-start table, the walk
// of one lane of a group over the shorter row of an edge, the LDS layout and the result record. Plain C++ with no HIP
// type in it, as cycles.hpp and winmst.hpp: tools/wincemp_host_check.cpp runs all of it on one thread under sanitizers on
// a machine without a device, and the kernel takes every piece from here, so there is one copy of each.
//
// Layout: edge k = (a, b) gives two half-edges, the words (a:9 | b:9 | 2k:11) and (b:9 | a:9 | 2k+1:11), the source in
// the highest of the 29 bits. The low bit of the value says that the half-edge runs against the stored direction. A word
// is unique, so ascending order is total and no result depends on how the sort reaches it: the half-edges that leave
// view u are one contiguous row, neighbours ascending, parallel edges next to each other by ascending value. A self loop
// and the padding of the network are the word of all ones, which sorts behind every row (a source is below 2^9).
#pragma once
#include <cstddef>
#include <cstdint>

#include "winbatch.hpp"  // the size limits

#if defined(__HIPCC__)
#define IRH_WC_HD __host__ __device__ __forceinline__
#else
#define IRH_WC_HD inline
#endif

namespace irh {

constexpr int WC_THREADS = 256;
constexpr int WC_GROUP = 8;                       // lanes of one edge
constexpr int WC_GROUPS = WC_THREADS / WC_GROUP;  // edges of one pass: group g takes edges g, g + 32, ...
constexpr int WC_ID_BITS = 9, WC_VAL_BITS = 11;
constexpr uint32_t WC_NONE = ~0u;
static_assert(WIN_MAX_NV <= (1 << WC_ID_BITS) && 2 * WIN_MAX_NE <= (1 << WC_VAL_BITS), "a half-edge is one 32-bit word");

IRH_WC_HD uint32_t wc_pack(uint32_t from, uint32_t to, uint32_t val) {
    return (from << (WC_ID_BITS + WC_VAL_BITS)) | (to << WC_VAL_BITS) | val;
}
IRH_WC_HD uint32_t wc_from(uint32_t w) { return w >> (WC_ID_BITS + WC_VAL_BITS); }
IRH_WC_HD uint32_t wc_to(uint32_t w) { return (w >> WC_VAL_BITS) & ((1u << WC_ID_BITS) - 1u); }
IRH_WC_HD uint32_t wc_val(uint32_t w) { return w & ((1u << WC_VAL_BITS) - 1u); }
IRH_WC_HD uint32_t wc_pair(uint32_t w) { return w >> WC_VAL_BITS; }  // (from, to): what a run of equals shares
IRH_WC_HD uint32_t wc_val_edge(uint32_t val) { return val >> 1; }
IRH_WC_HD bool wc_val_against(uint32_t val) { return (val & 1u) != 0; }
// the two half-edges of edge k (ids already inside [0, nv)); a self loop has no row
IRH_WC_HD void wc_emit(uint32_t k, uint32_t a, uint32_t b, uint32_t word[2]) {
    word[0] = a == b ? WC_NONE : wc_pack(a, b, 2u * k);
    word[1] = a == b ? WC_NONE : wc_pack(b, a, 2u * k + 1u);
}

// the length of the sorting network over n2 half-edges: the next power of two (at least 2)
constexpr int wc_sort_len(int n2) {
    int n = 2;
    while (n < n2) n <<= 1;
    return n;
}
// One compare-exchange of the bitonic network: position i of stage (k, j), k = 2, 4, .. n the sorted span and
// j = k/2 .. 1 the distance; the lower position of a pair does the work, so the positions of one stage touch disjoint
// words. The stages of one network are counted by the two loops around it: log2(n) (log2(n) + 1) / 2 of them.
IRH_WC_HD void wc_bitonic(uint32_t *w, int i, int j, int k) {
    const int l = i ^ j;
    if (l <= i) return;
    const uint32_t p = w[i], q = w[l];
    if ((p > q) == ((i & k) == 0)) {
        w[i] = q;
        w[l] = p;
    }
}

// the first position in [lo, hi) whose word is not below `target` (hi if none). hi - lo <= 2 WIN_MAX_NE < 2^11 and the
// span halves every round: 12 rounds end it whatever the words hold.
IRH_WC_HD int wc_lower_bound(const uint32_t *w, int lo, int hi, uint32_t target) {
    for (int round = 0; round < 12 && lo < hi; round++) {
        const int mid = lo + (hi - lo) / 2;
        if (w[mid] < target)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// entry u of the row-start table, u = 0 .. nv: the first of the n2 sorted words whose source is not below u. Row u is
// [start[u], start[u + 1]); start[nv] is where the words of all ones begin.
IRH_WC_HD int wc_row_start(const uint32_t *w, int n2, uint32_t u) { return wc_lower_bound(w, 0, n2, wc_pack(u, 0u, 0u)); }

// What a group knows of its edge k = (a, b), a != b: the walked (shorter) row [x0, x1) of x, the searched row [l0, l1)
// of the other end y. Ties go to b's row, as cemp_sorted decides.
struct WcRows {
    int x0, x1, l0, l1;
    uint32_t y;
    bool x_is_b;
};
IRH_WC_HD WcRows wc_rows(const int *start, uint32_t a, uint32_t b) {
    const int a0 = start[a], a1 = start[a + 1], b0 = start[b], b1 = start[b + 1];
    WcRows r;
    r.x_is_b = b1 - b0 <= a1 - a0;
    r.x0 = r.x_is_b ? b0 : a0;
    r.x1 = r.x_is_b ? b1 : a1;
    r.l0 = r.x_is_b ? a0 : b0;
    r.l1 = r.x_is_b ? a1 : b1;
    r.y = r.x_is_b ? a : b;
    return r;
}
// Entry i of the walked row against the searched one: its neighbour c is looked up there, and every half-edge y -> c of
// the run of equals closes a triangle with it. x is b: the entry is k1 (b -> c) and the run holds k2 as a -> c, to be
// turned; x is a: the entry is k2 as a -> c, to be turned, and the run holds k1 (b -> c). The sink gets, for k1 and k2,
// the edge and whether its measurement is taken against the stored direction: q(k1, b -> c), q(k2, c -> a).
template <class Sink>
IRH_WC_HD void wc_entry(const uint32_t *w, int i, const WcRows &r, Sink &sink) {
    const uint32_t wx = w[i], c = wc_to(wx);
    if (c == r.y) return;  // edge k itself or one parallel to it (c == x does not occur: self loops have no row)
    const uint32_t target = wc_pack(r.y, c, 0u);
    const uint32_t vx = wc_val(wx);
    for (int j = wc_lower_bound(w, r.l0, r.l1, target); j < r.l1 && wc_pair(w[j]) == wc_pair(target); j++) {
        const uint32_t vy = wc_val(w[j]);
        if (r.x_is_b)
            sink(wc_val_edge(vx), wc_val_against(vx), wc_val_edge(vy), !wc_val_against(vy));
        else
            sink(wc_val_edge(vy), wc_val_against(vy), wc_val_edge(vx), !wc_val_against(vx));
    }
}
// One lane of the group: entries lane, lane + G, ... of the walked row, one per round, in ascending order. This is the
// visit order of the lane: every floating-point sum of the kernel adds in it.
template <class Sink>
IRH_WC_HD void wc_lane(const uint32_t *w, const WcRows &r, int lane, Sink &sink) {
    for (int i = r.x0 + lane; i < r.x1; i += WC_GROUP) wc_entry(w, i, r, sink);
}

// the two ends of an edge as the kernel keeps them once the guard has passed them: one word, a in its low half
IRH_WC_HD uint32_t wc_ends(uint32_t a, uint32_t b) { return a | (b << 16); }
IRH_WC_HD uint32_t wc_end_a(uint32_t ends) { return ends & 0xffffu; }
IRH_WC_HD uint32_t wc_end_b(uint32_t ends) { return ends >> 16; }

// Dynamic LDS of one workgroup, in bytes from its base: the measurements (32 ne), the two planes of estimates (16 ne),
// the network's words, the row-start table (nv + 1), the ends (ne) and the used triangles (ne) of every edge.
struct WinCempLds {
    size_t oQQ, oS, oW, oStart, oEnds, oUsed, bytes;
};
constexpr WinCempLds wincemp_lds(int nv, int ne) {
    const size_t oS = 32 * (size_t)ne, oW = oS + 16 * (size_t)ne, oStart = oW + 4 * (size_t)wc_sort_len(2 * ne);
    const size_t oEnds = oStart + 4 * ((size_t)nv + 1), oUsed = oEnds + 4 * (size_t)ne, end = oUsed + 4 * (size_t)ne;
    return WinCempLds{0, oS, oW, oStart, oEnds, oUsed, (end + 31) & ~(size_t)31};
}
constexpr size_t WINCEMP_LDS_BUDGET = 48 * 1024;
static_assert(3 * WINCEMP_LDS_BUDGET <= WIN_MAX_LDS && wincemp_lds(WIN_MAX_NV, WIN_MAX_NE).bytes <= WINCEMP_LDS_BUDGET,
              "every term grows with its size: three problems at the limits share a compute unit");

// what a workgroup leaves: the sequence number last (hostwait.hpp)
struct WinCempResult {
    int status, seq;
    int used, untested;  // sum of |U(k)|, edges with no used triangle
};
static_assert((long long)WIN_MAX_NE * WIN_MAX_NE * WIN_MAX_NE <= 0x7fffffffLL, "a triangle is a triple of edges: the sum is an int");

}  // namespace irh
