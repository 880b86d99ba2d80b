// winmst.hpp -- the spanning-tree initialisation of a window-size problem (irotavg_init_mst, capi.cpp) restated so that
// it parallelises (docs/window_init_batch.md): arrival labels, the first visit of an edge after a label, a relaxation to
// the least fixed point and a literal transcription of the sequential sweep to hold it against. Plain C++ with no HIP
// type in it, as winbatch.hpp: tools/winmst_host_check.cpp runs all of it under sanitizers on a machine without a device.
// k_window_mst_user (winmst.hip) takes the encoding, the first-visit function and the product from here, so there is one
// copy of each.
//
// The sweep: view 0 is seen; the edge list is walked in order, again and again; edge k = (a, b) with exactly one end seen
// marks the other end seen. The arrival time of a view is T(v) = (sweep, edge index), view 0 before everything, and
//     T(v) = min over the edges k = (u, v), u != v, of the first visit of edge k strictly after T(u),
// where the first visit of k after (s, k_u) is (s, k) if k > k_u and (s + 1, k) otherwise. The cost grows strictly along
// an edge, so the least fixed point of "relax every edge in both directions with a minimum" is unique and any order of
// relaxations reaches it. The edge that gives a view its minimum is the edge the sweep reaches it by, in its direction.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define IRH_MST_HD __host__ __device__ __forceinline__
#else
#define IRH_MST_HD inline
#endif

namespace irh {

// ---- labels: 0 the root (before every visit), sweep * MST_STRIDE + k + 1 the visit of edge k in that sweep, all ones:
// never. MST_STRIDE is a power of two not below the edge limit of a window (640), so that sweep and edge come apart by
// a shift and a mask, not by two divisions by the problem's own edge count per edge and pass. A view arrives
// in sweep n_total - 2 at the latest (one view per sweep); at the window limits (320 views) no label passes 326 272.
constexpr uint32_t MST_ROOT = 0u;
constexpr uint32_t MST_INF = 0xffffffffu;
constexpr uint32_t MST_STRIDE = 1024u;
IRH_MST_HD uint32_t mst_label(uint32_t sweep, uint32_t k) { return sweep * MST_STRIDE + k + 1u; }
IRH_MST_HD uint32_t mst_edge_of(uint32_t label) { return (label - 1u) % MST_STRIDE; }  // label: neither root nor never
// the first visit of edge k strictly after `label` (never stays never)
IRH_MST_HD uint32_t mst_first_visit(uint32_t label, uint32_t k) {
    if (label == MST_INF) return MST_INF;
    if (label == MST_ROOT) return k + 1u;
    const uint32_t sweep = (label - 1u) / MST_STRIDE, ku = (label - 1u) % MST_STRIDE;
    return mst_label(k > ku ? sweep : sweep + 1u, k);
}

// ---- the product, [x y z w], operand by operand as h_qmul (capi.cpp) and qmul (kernels.hpp) form it. The
// products stay products: no contraction into fma, which a device build would choose and the x86 build of h_qmul has not.
IRH_MST_HD void mst_qmul(const double a[4], const double b[4], double o[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[0] = x;
    o[1] = y;
    o[2] = z;
    o[3] = w;
}

// dynamic LDS of one workgroup of k_window_mst_user: the rotations (32 nv), the endpoints (8 ne), the labels and the
// round a view was evaluated in (4 nv each)
constexpr size_t winmst_lds_bytes(int nv, int ne) { return 32 * (size_t)nv + 8 * (size_t)ne + 8 * (size_t)nv; }

// what a workgroup of k_window_mst_user leaves: the sequence number last (hostwait.hpp)
struct WinMstResult {
    int status, seq;
};

// ---- host forms: the tree as (parent edge, direction) per view; view 0 has edge -1
enum { MST_OK = 0, MST_NOT_SPANNING = 1, MST_BAD_ID = 2 };
struct MstTree {
    std::vector<int> edge;        // the edge a view is reached by
    std::vector<char> forward;    // 1: the view is the edge's second end (Q_b = QQ_k (x) Q_a), 0: its first
    std::vector<uint32_t> label;  // arrival labels (mst_relax alone fills them)
    int rounds = 0;               // relaxation rounds, the one that changes nothing included
    uint32_t peak = 0;            // largest finite label
};

// The relaxation as the kernel runs it, one thread: rounds over the edges, both directions, until nothing changes; at most
// nv + 1 rounds (a view of tree depth d is final after round d).
inline int mst_relax(int nv, int ne, const int32_t *I, MstTree &out) {
    out.edge.assign((size_t)nv, -1);
    out.forward.assign((size_t)nv, 0);
    out.label.assign((size_t)nv, MST_INF);
    out.rounds = 0;
    out.peak = 0;
    if ((uint32_t)ne > MST_STRIDE) return MST_BAD_ID;  // (past the window limits: the labels have no room for it)
    for (int k = 0; k < ne; k++)
        if ((uint32_t)I[2 * k] >= (uint32_t)nv || (uint32_t)I[2 * k + 1] >= (uint32_t)nv) return MST_BAD_ID;
    std::vector<uint32_t> &L = out.label;
    L[0] = MST_ROOT;
    for (int r = 0; r < nv + 1; r++) {
        bool changed = false;
        out.rounds++;
        for (int k = 0; k < ne; k++) {
            const int a = I[2 * k], b = I[2 * k + 1];
            if (a == b) continue;
            const uint32_t la = mst_first_visit(L[(size_t)a], (uint32_t)k);
            if (la < L[(size_t)b]) {
                L[(size_t)b] = la;
                changed = true;
            }
            const uint32_t lb = mst_first_visit(L[(size_t)b], (uint32_t)k);
            if (lb < L[(size_t)a]) {
                L[(size_t)a] = lb;
                changed = true;
            }
        }
        if (!changed) break;
    }
    for (int v = 0; v < nv; v++) {
        if (L[(size_t)v] == MST_INF) return MST_NOT_SPANNING;
        if (L[(size_t)v] > out.peak) out.peak = L[(size_t)v];
        if (v == 0) continue;
        const int k = (int)mst_edge_of(L[(size_t)v]);
        out.edge[(size_t)v] = k;
        out.forward[(size_t)v] = I[2 * k + 1] == v ? 1 : 0;
    }
    return MST_OK;
}

// The sweep of irotavg_init_mst, literally (its products left out): the reference of the relaxation above.
inline int mst_sequential(int nv, int ne, const int32_t *I, MstTree &out) {
    out.edge.assign((size_t)nv, -1);
    out.forward.assign((size_t)nv, 0);
    out.label.clear();
    out.rounds = 0;
    out.peak = 0;
    std::vector<char> seen((size_t)nv, 0);
    seen[0] = 1;
    int count = 1;
    while (count < nv) {
        bool grew = false;
        out.rounds++;
        for (int k = 0; k < ne; k++) {
            const int a = I[2 * k], b = I[2 * k + 1];
            if (a < 0 || b < 0 || a >= nv || b >= nv) return MST_BAD_ID;
            if (seen[(size_t)a] && !seen[(size_t)b]) {
                out.edge[(size_t)b] = k;
                out.forward[(size_t)b] = 1;
                seen[(size_t)b] = 1;
                count++;
                grew = true;
            } else if (!seen[(size_t)a] && seen[(size_t)b]) {
                out.edge[(size_t)a] = k;
                out.forward[(size_t)a] = 0;
                seen[(size_t)a] = 1;
                count++;
                grew = true;
            }
        }
        if (!grew && count < nv) return MST_NOT_SPANNING;
    }
    return MST_OK;
}

}  // namespace irh
