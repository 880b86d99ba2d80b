// wintree.hpp -- the rank-aware tree initialisation of a window-size problem (irotavg_window_init_tree_batch_dev;
// docs/window_init_tree_batch.md): the node map of the contracted graph, the usable-edge rule, the packed ends of an
// edge, the hook and the jump of one node, the round and pass counts, the LDS layout of k_window_tree and a one-thread
// form of the whole algorithm. Plain C++ with no HIP type in it, as winmst.hpp and treeinit.hpp:
// tools/wintree_host_check.cpp runs all of it under sanitizers on a machine without a device. k_window_tree
// (wintree.hip) takes every piece from here, and the key, the quaternion product and the label algebra from
// treeinit.hpp, so there is one copy of each.
//
// Definition: the fixed views [0, f) together are one root; an edge is usable when its rank is not negative and its ends
// are two different nodes; the tree is the minimum spanning forest of {root} + free views under the keys (rank[k], k),
// which are distinct, so it is unique. T(u) = Q[u] for a fixed u, T(b) = QQ_k (x) T(a) along a tree edge k = (a, b) walked
// from a, T(a) = QQ_k* (x) T(b) walked from b; a free view v gets +-T(v) up to rounding.
//
// State per node: comp[v], the representative of its component, and rel[v] with T(v) = rel[v] (x) T(comp[v]); the root's
// own rotation is the identity, so the label of a node of the root's component is its row. A round: every usable edge
// between two components offers its key to both representatives (a minimum); a representative other than the root hooks
// under the other end's representative (of a mutual pair the smaller id stays); pointer jumping makes comp flat again.
// Every step reads the state of before it and writes the other copy.
#pragma once
#include "treeinit.hpp"  // tree_key, TreeQ, tree_qmul, tree_directed, tree_hook_label, tree_jump_label
#include "winbatch.hpp"  // WIN_MAX_NU, WIN_MAX_NV, WIN_MAX_NE

namespace irh {

constexpr int WT_MAX_NODES = WIN_MAX_NU + 1;  // the root and the free views
IRH_TREE_HD int wt_node(int v, int f) { return v < f ? 0 : v - f + 1; }
IRH_TREE_HD int wt_view(int node, int f) { return f + node - 1; }  // node >= 1
// rank < 0: never used; self loops and edges between two fixed views: never used
IRH_TREE_HD bool wt_usable(int a, int b, int f, int32_t rank) { return rank >= 0 && wt_node(a, f) != wt_node(b, f); }

// the ends of an edge as one word of LDS: a in bits 0..14, b in bits 16..30 (ids are below WIN_MAX_NV); bit 15 is set
// at the very end on a tree edge
constexpr uint32_t WT_IN_TREE = 0x8000u;
static_assert(WIN_MAX_NV <= 0x8000, "an id has 15 bits");
IRH_TREE_HD uint32_t wt_ends(int a, int b) { return (uint32_t)a | ((uint32_t)b << 16); }
IRH_TREE_HD int wt_end_a(uint32_t e) { return (int)(e & 0x7fffu); }
IRH_TREE_HD int wt_end_b(uint32_t e) { return (int)(e >> 16); }

// ---- rounds and passes ----------------------------------------------------------------------------------------------------
// A representative other than the root that has an offer either hooks or is the smaller one of a mutual pair whose other
// one hooks, so such representatives at least halve per round: at most nu >> r of them enter round r, and after
// floor(log2(nu)) + 1 rounds there is none left. In round r a chain of hooks is at most nu >> r long and a node that is
// no representative hangs one further down; j passes of pointer jumping cover 2^j pointers.
constexpr int wt_ceil_log2(int x) {  // the smallest j with 2^j >= x
    int j = 0;
    while ((1 << j) < x) j++;
    return j;
}
constexpr int wt_rounds(int nu) {
    int r = 0;
    while ((nu >> r) > 0) r++;
    return r;
}
constexpr int wt_passes(int nu, int round) { return wt_ceil_log2((nu >> round) + 1); }
constexpr int WT_MAX_ROUNDS = 7, WT_MAX_PASSES = 8;
static_assert(wt_rounds(WIN_MAX_NU) <= WT_MAX_ROUNDS && wt_passes(WIN_MAX_NU, 0) <= WT_MAX_PASSES,
              "the loops of k_window_tree are bounded by these");

// ---- the LDS of one workgroup of k_window_tree, in bytes from its base: two copies of the labels (32 nn each), the best
// key and the key a node hooked by (8 nn each), two copies of comp (4 nn each), the ends of the edges (4 ne)
struct WinTreeLds {
    size_t oRel, oBest, oVia, oComp, oEnds, bytes;
};
constexpr WinTreeLds wintree_lds(int nn, int ne) {
    const size_t n = (size_t)nn, oBest = 64 * n, oVia = oBest + 8 * n, oComp = oVia + 8 * n, oEnds = oComp + 8 * n;
    return WinTreeLds{0, oBest, oVia, oComp, oEnds, oEnds + 4 * (size_t)ne};
}
static_assert(wintree_lds(WT_MAX_NODES, WIN_MAX_NE).bytes <= 9 * 1024, "half of k_window_mst_user's: many problems share a compute unit");

// what a workgroup of k_window_tree leaves: the sequence number last (hostwait.hpp)
struct WinTreeResult {
    int status, seq;
    int left, rank_pos, rank_max, pad;
};

// ---- the steps of one node --------------------------------------------------------------------------------------------------
// Hook: node v of the state (comp, rel, best) of before the round -> its state after the hooks (comp_new, rel_new). true:
// it hooked, by the edge of `key`. ends: wt_ends of every edge; qq(k): QQ_k, q(u): the caller's row of the fixed view u.
template <class LoadQQ, class LoadQ>
IRH_TREE_HD bool wt_hook(int v, int f, const int32_t *comp, const TreeQ *rel, const uint64_t *best, const uint32_t *ends,
                         const LoadQQ &qq, const LoadQ &q, int32_t &comp_new, TreeQ &rel_new, uint64_t &key) {
    comp_new = comp[v];
    rel_new = rel[v];
    key = best[v];
    if (v == 0 || comp_new != v || key == TREE_KEY_NONE) return false;  // the root never hooks
    const uint32_t k = tree_key_edge(key), e = ends[k];
    const int a = wt_end_a(e), b = wt_end_b(e), na = wt_node(a, f), nb = wt_node(b, f);
    const int32_t ca = comp[na], cb = comp[nb];
    if ((ca == v) == (cb == v)) return false;  // (does not occur: an offer reaches the representatives of its two ends)
    const bool mine_is_b = cb == v;
    const int mine = mine_is_b ? nb : na, other = mine_is_b ? na : nb;
    const int32_t lo = mine_is_b ? ca : cb;
    // the mutual pick: the smaller id stays (treeinit.hpp: no other cycle can arise, the keys fall strictly along a chain
    // of picks; leaving the root's own pick out removes an edge of the round and adds none)
    if (best[lo] == key && v < lo) return false;
    // T(other) = rel[other] (x) T(lo); a fixed view's is the caller's row and T(root) the identity
    const TreeQ rel_other = other == 0 ? q(mine_is_b ? a : b) : rel[other];
    comp_new = lo;
    rel_new = tree_hook_label(rel[mine], tree_directed(qq(k), !mine_is_b), rel_other);
    return true;
}
// Jump: node v one doubling further. Behind a representative nothing moves and no product is formed, so a pass more
// than needed changes no bit.
IRH_TREE_HD void wt_jump(int v, const int32_t *comp, const TreeQ *rel, int32_t &comp_new, TreeQ &rel_new) {
    const int32_t p = comp[v], pp = comp[p];
    comp_new = pp;
    rel_new = pp == p ? rel[v] : tree_jump_label(rel[v], rel[p]);
}

// ---- the whole algorithm on one thread, step by step as the kernel runs it -----------------------------------------------------
enum { WT_OK = 0, WT_BAD_ID = 1, WT_NOT_SPANNING = 2 };
struct WinTreeHost {
    std::vector<TreeQ> T;          // nv rows; rows >= f meaningful on success
    std::vector<int32_t> in_tree;  // ne, on success
    int left = 0, rank_pos = 0, rank_max = 0;
    int rounds = 0;    // rounds that hooked something
    bool flat = true;  // comp was flat after the passes of every round
};
// I: ne pairs, rank: ne or nullptr, qq: ne rows [x y z w], Q: nv rows [x y z w] (rows < f are read)
inline int wintree_rounds(int nv, int f, int ne, const int32_t *I, const int32_t *rank, const double *qq, const double *Q,
                          WinTreeHost &R) {
    R = WinTreeHost();
    for (int k = 0; k < ne; k++)
        if (!tree_id_ok(I[2 * k], nv) || !tree_id_ok(I[2 * k + 1], nv)) return WT_BAD_ID;
    const int nu = nv - f, nn = nu + 1;
    std::vector<int32_t> comp[2] = {std::vector<int32_t>((size_t)nn), std::vector<int32_t>((size_t)nn)};
    std::vector<TreeQ> rel[2] = {std::vector<TreeQ>((size_t)nn, tree_identity()), std::vector<TreeQ>((size_t)nn, tree_identity())};
    std::vector<uint64_t> best((size_t)nn), via((size_t)nn, TREE_KEY_NONE), key((size_t)ne, TREE_KEY_NONE);
    std::vector<uint32_t> ends((size_t)ne);
    for (int v = 0; v < nn; v++) comp[0][(size_t)v] = v;
    for (int k = 0; k < ne; k++) {
        const int a = I[2 * k], b = I[2 * k + 1];
        const int32_t rk = rank ? rank[k] : 0;
        ends[(size_t)k] = wt_ends(a, b);
        if (wt_usable(a, b, f, rk)) key[(size_t)k] = tree_key(rk, (uint32_t)k);
    }
    const TreeAosLoad lqq{qq}, lq{Q};
    int cur = 0;
    for (int round = 0; round < wt_rounds(nu); round++) {
        std::fill(best.begin(), best.end(), TREE_KEY_NONE);
        for (int k = 0; k < ne; k++) {
            if (key[(size_t)k] == TREE_KEY_NONE) continue;
            const int32_t ca = comp[cur][(size_t)wt_node(I[2 * k], f)], cb = comp[cur][(size_t)wt_node(I[2 * k + 1], f)];
            if (ca == cb) continue;
            best[(size_t)ca] = std::min(best[(size_t)ca], key[(size_t)k]);
            best[(size_t)cb] = std::min(best[(size_t)cb], key[(size_t)k]);
        }
        int hooks = 0;
        for (int v = 0; v < nn; v++) {
            uint64_t by;
            if (!wt_hook(v, f, comp[cur].data(), rel[cur].data(), best.data(), ends.data(), lqq, lq, comp[cur ^ 1][(size_t)v],
                         rel[cur ^ 1][(size_t)v], by))
                continue;
            via[(size_t)v] = by;
            hooks++;
        }
        cur ^= 1;
        if (hooks == 0) break;
        R.rounds++;
        const int passes = wt_passes(nu, round);
        for (int j = 0; j < passes; j++, cur ^= 1)
            for (int v = 0; v < nn; v++)
                wt_jump(v, comp[cur].data(), rel[cur].data(), comp[cur ^ 1][(size_t)v], rel[cur ^ 1][(size_t)v]);
        for (int v = 0; v < nn; v++) R.flat = R.flat && comp[cur][(size_t)comp[cur][(size_t)v]] == comp[cur][(size_t)v];
    }
    for (int v = 1; v < nn; v++) R.left += comp[cur][(size_t)v] != 0;
    if (R.left) return WT_NOT_SPANNING;
    R.T.assign((size_t)nv, tree_identity());
    R.in_tree.assign((size_t)ne, 0);
    for (int v = 1; v < nn; v++) {
        R.T[(size_t)wt_view(v, f)] = rel[cur][(size_t)v];
        R.in_tree[tree_key_edge(via[(size_t)v])] = 1;
        R.rank_pos += tree_key_rank(via[(size_t)v]) > 0;
        R.rank_max = std::max(R.rank_max, (int)tree_key_rank(via[(size_t)v]));
    }
    return WT_OK;
}

}  // namespace irh
