// bcr_route_host_check.cpp -- the route decision of the banded direct solver (irotavg_amd/csrc/bcr_route.hpp: which launches
// a solve is made of, as which instantiation of k_bcr_reduce) as a stand-alone program that needs no device, meant to be
// built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/bcr_route_host_check.cpp -o bcr_route_host_check && ./bcr_route_host_check
// It walks the whole input space -- block sizes 8 ... 32, one to six levels from view counts on both sides of a sixteen-block
// top and of 256 level-1 chunks, closures, shard, ghosts, guard, every only / phase / open_top, the unit-weight requests with
// and without a valid store, the debug words, each switch, a granted and a refused reservation -- and checks at every point
// what bcr.hip relies on without saying so; then a dozen literal rows: the routes of the shapes of tests/band_cases.py and
// tests/closure_cases.py, written down from what the solver did for them before the decision had a place of its own.
// Exit status 0 and "bcr route host check ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bcr_route.hpp"

using namespace irh;

static long failures = 0, points = 0;
#define EXPECT(c)                                                                   \
    do {                                                                            \
        if (!(c)) {                                                                 \
            if (failures < 20) std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            failures++;                                                             \
        }                                                                           \
    } while (0)

// the levels bcr_alloc gives nb0 level-0 blocks (no mixed level 1: that only moves blocks between levels 0 and 1)
static BcrShape shape_of(int B, int nb0, int nfar, bool shard, bool no_top16) {
    BcrShape s;
    s.B = B;
    s.nfar = nfar;
    s.shard = shard;
    s.asm_windowed = true;
    s.top16 = B <= 24 && nfar == 0 && !shard && !no_top16;
    int nb = nb0;
    for (int l = 0;; l++) {
        const int topmax = s.top16 ? 16 : 8;
        s.nl = l + 1;
        s.nch[l] = (nb + 7) / 8;
        if (nb <= topmax && !shard && l > 0 && s.top16) break;
        if (nb <= 8 && !shard) {
            s.top16 = false;
            break;
        }
        if (nb <= 8) break;
        nb = s.nch[l];
    }
    return s;
}

static bool same_launch(const BcrLaunch &a, const BcrLaunch &b) {
    return a.l0 == b.l0 && a.top == b.top && a.wide == b.wide && a.assemble == b.assemble && a.uf == b.uf;
}

// the instantiations of k_bcr_reduce that exist (bcr_launch_reduce, bcr.hip)
static bool instantiated(int B, const BcrLaunch &k) {
    if (k.wide && B > 24) return false;                                                      // NW == 8 only for B <= 24
    if (k.uf != 0 && !(k.assemble && !k.top && (B == 8 || B == 16 || B == 24))) return false;
    if (k.uf < 0 || k.uf > 2) return false;
    if (k.assemble && !(k.l0 && (8 * B) % 64 == 0)) return false;
    return true;
}

static void check_point(const BcrShape &s, const BcrRequest &q, bool reserved) {
    points++;
    const BcrRoute r = bcr_route(s, q, reserved);
    const int nl = s.nl, dbg = bcr_dbg(s, q);
    const bool whole = q.only < 0 && q.phase == 0 && !r.uf_up_only;
    EXPECT(dbg == (q.dbg >= 0 ? q.dbg : s.dbg));
    // fused_up
    EXPECT(r.fused_up == (reserved && bcr_wants_up(s, q)));
    if (r.fused_up) {
        EXPECT(s.B <= 24 && nl >= 3 && nl - 1 <= kUpLevels && s.nfar == 0 && s.nch[1] <= 256 && !(dbg & 64));
        EXPECT(!s.shard && !s.no_fused_up && q.only < 0 && q.phase == 0 && !q.open_top);
    }
    // the unit-weight factor
    EXPECT(r.uf >= 0 && r.uf <= 2);
    if (r.uf != 0) {
        EXPECT(r.fused_up && s.top16 && (s.B == 8 || s.B == 16 || s.B == 24) && dbg == 0 && !s.guard && !q.out);
        EXPECT(!s.no_unit_factor && q.unit != 0 && (r.asm0 || q.unit == 3));
        EXPECT((r.uf == 2) == s.unit_valid);
        EXPECT(r.uf != 1 || q.unit == 1);
    }
    EXPECT(!r.uf_up_only || (r.uf == 2 && q.unit == 3));
    // level 0 assembling
    if (r.asm0) {
        EXPECT((8 * s.B) % 64 == 0 && s.nfar == 0 && !s.shard && q.only < 0 && q.phase == 0 && !q.open_top && q.assemble);
        EXPECT(r.red[0] == kRedOwn && r.own[0].assemble);
    }
    BcrRequest plain;
    plain.assemble = bcr_can_assemble(s);
    if (plain.assemble) EXPECT(bcr_route(s, plain, reserved).asm0);          // what ls_solve relies on
    if (bcr_can_assemble(s)) EXPECT(s.ng == 0 && !s.no_fused_asm && !s.no_fused_up && s.asm_windowed);
    // the step inside the ways back
    EXPECT(r.apply_slots == (r.apply ? bcr_apply_slots(s) : 0));
    if (r.apply) {
        EXPECT(q.apply && bcr_apply_slots(s) > 0 && whole && !q.out && s.ng == 0 && nl >= 2);
        EXPECT(r.back[0] == kBackOwn);                                       // level 0's chunks: k_bcr_back applies
        EXPECT(r.back[1] == kBackTop || (r.back[1] == kBackWithRed && nl == 2));  // a mixed level 1's rows: k_bcr_back_top
        EXPECT(bcr_apply_slots(s) == s.nch[0] + (r.back[1] == kBackTop ? s.nch[1] : 0));
    }
    if (bcr_apply_slots(s) > 0) EXPECT(bcr_apply_slots(s) <= kBcrApplySlotsMax && s.nfar == 0 && !s.shard && s.ng == 0);
    // the launches
    bool top_alone = false;
    for (int l = 0; l < kBcrMaxLevels; l++) {
        if (l >= nl) {
            EXPECT(r.red[l] == kRedNone && r.back[l] == kBackNone);
            continue;
        }
        if (q.phase == 2 || (q.only >= 0 && q.only != l)) EXPECT(r.red[l] == kRedNone);
        if (q.phase == 1 || (q.only >= 0 && q.only < 100)) EXPECT(r.back[l] == kBackNone || r.back[l] == kBackWithRed);
        switch (r.red[l]) {
        case kRedNone: break;
        case kRedOwn:
            EXPECT(instantiated(s.B, r.own[l]));
            EXPECT(r.own[l].l0 == (l == 0) && r.own[l].top == (l == nl - 1 && !q.open_top));
            EXPECT(r.own[l].wide == (s.B <= 24 && s.nch[l] <= 256));
            EXPECT(r.own[l].assemble == (l == 0 && r.asm0) && r.own[l].uf == (l == 0 ? r.uf : 0));
            EXPECT(!(s.top16 && l == nl - 1));
            break;
        case kRedUp: EXPECT(r.fused_up && l >= 1); break;
        case kRedTopAlone:
            EXPECT(s.top16 && l == nl - 1 && !r.fused_up && s.B <= 24 && nl >= 2);
            top_alone = true;
            break;
        default: EXPECT(false);
        }
        switch (r.back[l]) {
        case kBackNone: break;
        case kBackOwn: EXPECT(l == 0 || !r.fused_back); break;
        case kBackTop: EXPECT(r.fused_back && l >= 1 && l <= (s.top16 ? nl - 2 : nl - 1)); break;
        case kBackWithRed: EXPECT(s.top16 && l == nl - 1 && r.red[l] != kRedNone && r.red[l] != kRedOwn); break;
        default: EXPECT(false);
        }
        if (whole) EXPECT(r.red[l] != kRedNone && r.back[l] != kBackNone);   // once each: a level has one entry of each kind
        if (r.uf_up_only) EXPECT(r.red[l] == (l == 0 ? kRedNone : kRedUp) && (r.back[l] == kBackNone || l == nl - 1));
    }
    EXPECT(r.top_alone == top_alone);
    EXPECT(r.fused_back == ((s.top16 ? nl - 2 : nl - 1) >= 1 && !s.shard && !q.open_top));
    // the reductions (phase 1) and the ways back (phase 2) are the whole solve's launches: every level covered once by the
    // pair; the KINDS are compared only where the whole solve takes neither the upper launch nor the assembling one (a
    // split solve never does: both need phase 0)
    if (q.only < 0 && q.phase == 0) {
        BcrRequest q1 = q, q2 = q;
        q1.phase = 1;
        q2.phase = 2;
        const BcrRoute r1 = bcr_route(s, q1, reserved), r2 = bcr_route(s, q2, reserved);
        EXPECT(!r1.fused_up && !r2.fused_up && !r1.asm0 && !r2.asm0 && !r1.uf && !r2.uf && !r1.apply && !r2.apply);
        for (int l = 0; l < nl; l++) {
            EXPECT(r1.red[l] != kRedNone && r2.red[l] == kRedNone);
            EXPECT((r1.back[l] != kBackNone) + (r2.back[l] != kBackNone) == 1);
            if (!r.fused_up && !r.asm0) {
                EXPECT(r1.red[l] == r.red[l] && (r.red[l] != kRedOwn || same_launch(r1.own[l], r.own[l])));
                EXPECT((r1.back[l] != kBackNone ? r1.back[l] : r2.back[l]) == r.back[l]);
            }
        }
    }
}

static void enumerate() {
    const int nb0s[] = {5, 9, 16, 17, 129, 1025, 16384, 16385, 131073};
    const int dbgs[] = {0, 64, 128};
    int most_levels = 0, fewest_levels = 99;
    for (int B = 8; B <= 32; B += 4)
        for (int nb0 : nb0s)
            for (int no_top16 = 0; no_top16 < (B <= 24 ? 2 : 1); no_top16++)
                for (int nfar = 0; nfar <= 5; nfar += 5)
                    for (int shard = 0; shard < 2; shard++)
                        for (int ng = 0; ng <= 3; ng += 3)
                            for (int guard = 0; guard < (ng ? 1 : 2); guard++)
                                for (int sw = 0; sw < 5; sw++) {  // no switch, each of the three, the classic assembly
                                    BcrShape s = shape_of(B, nb0, nfar, shard != 0, no_top16 != 0);
                                    s.ng = ng;
                                    s.guard = guard != 0;
                                    s.no_fused_asm = sw == 1;
                                    s.no_unit_factor = sw == 2;
                                    s.no_fused_up = sw == 3;
                                    s.asm_windowed = sw != 4;
                                    most_levels = std::max(most_levels, s.nl);
                                    fewest_levels = std::min(fewest_levels, s.nl);
                                    std::vector<int> onlys = {-1, 0, 100};
                                    if (s.nl > 1) onlys.insert(onlys.end(), {1, 101});
                                    if (s.nl > 2) onlys.insert(onlys.end(), {s.nl - 1, 100 + s.nl - 1});
                                    static char sink;
                                    for (int only : onlys)
                                        for (int phase = 0; phase < 3; phase++)
                                            for (int open_top = 0; open_top < 2; open_top++)
                                                for (int assemble = 0; assemble < 2; assemble++)
                                                    for (int unit = 0; unit < 4; unit++)
                                                        for (int valid = 0; valid < (unit ? 2 : 1); valid++)
                                                            for (int apply = 0; apply < 2; apply++)
                                                                for (int out = 0; out < 2; out++)
                                                                    for (int dbg : dbgs)
                                                                        for (int reserved = 0; reserved < 2; reserved++) {
                                                                            BcrRequest q;
                                                                            q.only = only;
                                                                            q.phase = phase;
                                                                            q.open_top = open_top != 0;
                                                                            q.assemble = assemble != 0;
                                                                            q.unit = unit;
                                                                            q.apply = apply != 0;
                                                                            q.out = out ? &sink : nullptr;
                                                                            q.dbg = dbg && assemble ? dbg : -1;  // the request's word or
                                                                            s.dbg = assemble ? 0 : dbg;          // the handle's switch
                                                                            s.unit_valid = valid != 0;
                                                                            check_point(s, q, reserved != 0);
                                                                        }
                                }
    EXPECT(fewest_levels == 1 && most_levels == 6);
}

// ---- literal rows ----
struct Row {
    const char *name;
    BcrShape s;
    BcrRequest q;
    bool reserved;
    // expected
    bool fused_up;
    int uf;
    bool asm0, top_alone, fused_back, apply;
    int apply_slots;
    std::vector<int> red, back;           // per level
    std::vector<BcrLaunch> own;           // per level with red == kRedOwn, in level order
};

static BcrLaunch launch(bool l0, bool top, bool wide, bool assemble, int uf) {
    BcrLaunch k;
    k.l0 = l0;
    k.top = top;
    k.wide = wide;
    k.assemble = assemble;
    k.uf = uf;
    return k;
}

static void check_row(const Row &w, const std::vector<int> &nch) {
    const BcrRoute r = bcr_route(w.s, w.q, w.reserved);
    bool ok = (int)nch.size() == w.s.nl && r.fused_up == w.fused_up && r.uf == w.uf && r.asm0 == w.asm0 &&
              r.top_alone == w.top_alone && r.fused_back == w.fused_back && r.apply == w.apply &&
              r.apply_slots == w.apply_slots && !r.uf_up_only && (int)w.red.size() == w.s.nl && (int)w.back.size() == w.s.nl;
    size_t k = 0;
    for (int l = 0; ok && l < w.s.nl; l++) {
        ok = w.s.nch[l] == nch[(size_t)l] && r.red[l] == w.red[(size_t)l] && r.back[l] == w.back[(size_t)l];
        if (ok && r.red[l] == kRedOwn) ok = k < w.own.size() && same_launch(r.own[l], w.own[k++]);
    }
    ok = ok && k == w.own.size();
    if (!ok) {
        std::fprintf(stderr, "row %s: the route is not the expected one\n", w.name);
        failures++;
    }
}

static void rows() {
    BcrRequest first;  // run_irls's first solve of a call through ls_solve on a handle that can assemble
    first.assemble = true;
    first.apply = true;
    first.unit = 1;
    BcrRequest later = first;
    later.unit = 0;
    BcrRequest no_asm = first;  // ... on a handle that cannot
    no_asm.assemble = false;
    const int O = kRedOwn, U = kRedUp, T = kRedTopAlone, bO = kBackOwn, bT = kBackTop, bW = kBackWithRed, bN = kBackNone;

    // band_cases up-b8-nb129-s: blocks [129, 17, 3], the top a single workgroup
    BcrShape up8 = shape_of(8, 129, 0, false, false);
    EXPECT(up8.top16 && bcr_can_assemble(up8) && bcr_apply_slots(up8) == 20);
    check_row({"plain, the filling solve", up8, first, true, true, 1, true, false, true, true, 20, {O, U, U}, {bO, bT, bW},
               {launch(true, false, true, true, 1)}}, {17, 3, 1});
    BcrShape up8v = up8;
    up8v.unit_valid = true;
    check_row({"plain, served from the store", up8v, first, true, true, 2, true, false, true, true, 20, {O, U, U}, {bO, bT, bW},
               {launch(true, false, true, true, 2)}}, {17, 3, 1});
    check_row({"plain, a later iteration", up8v, later, true, true, 0, true, false, true, true, 20, {O, U, U}, {bO, bT, bW},
               {launch(true, false, true, true, 0)}}, {17, 3, 1});
    // IROTAVG_BCR_NO_FUSED_ASM: K3 in a launch of its own, and no store without the assembling launch
    BcrShape nofa = up8;
    nofa.no_fused_asm = true;
    EXPECT(!bcr_can_assemble(nofa));
    check_row({"NO_FUSED_ASM", nofa, no_asm, true, true, 0, false, false, true, true, 20, {O, U, U}, {bO, bT, bW},
               {launch(true, false, true, false, 0)}}, {17, 3, 1});
    // IROTAVG_BCR_UP_CAP=0, or any refused reservation: level by level, the top in a launch of its own
    check_row({"a refused reservation", up8, first, false, false, 0, true, true, true, true, 20, {O, O, T}, {bO, bT, bW},
               {launch(true, false, true, true, 0), launch(false, false, true, false, 0)}}, {17, 3, 1});
    // IROTAVG_BCR_NO_TOP16: a chunk-form top of three blocks inside the upper launch, its way back in k_bcr_back_top
    BcrShape not16 = shape_of(8, 129, 0, false, true);
    EXPECT(!not16.top16);
    check_row({"NO_TOP16", not16, first, true, true, 0, true, false, true, true, 20, {O, U, U}, {bO, bT, bT},
               {launch(true, false, true, true, 0)}}, {17, 3, 1});
    // the thresholds. Level 1 of exactly 256 chunks still takes the upper launch (blocks [16384, 2048, 256, 32, 4]) ...
    BcrShape c256 = shape_of(8, 16384, 0, false, false);
    EXPECT(c256.top16 && bcr_apply_slots(c256) == 0);  // (2048 + 256 slots: more than the pinned block holds)
    check_row({"256 level-1 chunks", c256, first, true, true, 1, true, false, true, false, 0, {O, U, U, U, U},
               {bO, bT, bT, bT, bW}, {launch(true, false, false, true, 1)}}, {2048, 256, 32, 4, 1});
    // ... 257 do not ([16385, 2049, 257, 33, 5]): level by level, eight waves from level 2 on, the top alone
    BcrShape c257 = shape_of(8, 16385, 0, false, false);
    check_row({"257 level-1 chunks", c257, first, true, false, 0, true, true, true, false, 0, {O, O, O, O, T},
               {bO, bT, bT, bT, bW},
               {launch(true, false, false, true, 0), launch(false, false, false, false, 0), launch(false, false, true, false, 0),
                launch(false, false, true, false, 0)}}, {2049, 257, 33, 5, 1});
    // a level of 16 blocks is a single-workgroup top ([128, 16]); 17 blocks are a level of chunks ([129, 17, 3], above)
    BcrShape t16 = shape_of(8, 128, 0, false, false);
    check_row({"a top of 16 blocks", t16, first, true, false, 0, true, true, false, true, 16, {O, T}, {bO, bW},
               {launch(true, false, true, true, 0)}}, {16, 2});
    // a level 0 of 256 chunks gets eight waves, one of 257 four ([2048, 256, 32, 4] / [2049, 257, 33, 5])
    check_row({"256 level-0 chunks", shape_of(8, 2048, 0, false, false), later, true, true, 0, true, false, true, true, 288,
               {O, U, U, U}, {bO, bT, bT, bW}, {launch(true, false, true, true, 0)}}, {256, 32, 4, 1});
    check_row({"257 level-0 chunks", shape_of(8, 2049, 0, false, false), later, true, true, 0, true, false, true, true, 290,
               {O, U, U, U}, {bO, bT, bT, bW}, {launch(true, false, false, true, 0)}}, {257, 33, 5, 1});
    // band_cases mixed-b8 on 256 compute units: blocks [4109, 525, 66, 9], 512 chunks at level 0
    BcrShape mixed = shape_of(8, 4109, 0, false, false);
    mixed.nch[0] = 512;
    mixed.nch[1] = 66;
    EXPECT(mixed.nl == 4 && mixed.top16 && bcr_apply_slots(mixed) == 578);
    check_row({"mixed", mixed, first, true, true, 1, true, false, true, true, 578, {O, U, U, U}, {bO, bT, bT, bW},
               {launch(true, false, false, true, 1)}}, {512, 66, 9, 2});
    // band_cases top16-b12-nb128: blocks [128, 16]; twelve rows are no whole slices
    BcrShape b12 = shape_of(12, 128, 0, false, false);
    EXPECT(!bcr_can_assemble(b12) && b12.top16);
    check_row({"blocks of 12, two levels", b12, no_asm, true, false, 0, false, true, false, true, 16, {O, T}, {bO, bW},
               {launch(true, false, true, false, 0)}}, {16, 2});
    // band_cases sep-b32-nb65: blocks [65, 9, 2], four waves, every level a launch of its own
    BcrShape b32 = shape_of(32, 65, 0, false, false);
    EXPECT(bcr_can_assemble(b32) && !b32.top16);
    check_row({"blocks of 32, three levels", b32, first, true, false, 0, true, false, true, true, 11, {O, O, O}, {bO, bT, bT},
               {launch(true, false, false, true, 0), launch(false, false, false, false, 0), launch(false, true, false, false, 0)}},
              {9, 2, 1});
    // band_cases one-b8-63-u: level 0 is the top
    BcrShape one = shape_of(8, 8, 0, false, false);
    check_row({"one level", one, later, true, false, 0, true, false, false, false, 0, {O}, {bO},
               {launch(true, true, true, true, 0)}}, {1});
    // closure_cases up-b8-nb129: the reductions, the closures' work in between, the ways back
    BcrShape cl = shape_of(8, 129, 27, false, false);
    EXPECT(!cl.top16 && !bcr_can_assemble(cl) && bcr_apply_slots(cl) == 0);
    BcrRequest p1, p2;
    p1.phase = 1;
    p2.phase = 2;
    check_row({"closures, the reductions", cl, p1, true, false, 0, false, false, true, false, 0, {O, O, O}, {bN, bN, bN},
               {launch(true, false, true, false, 0), launch(false, false, true, false, 0), launch(false, true, true, false, 0)}},
              {17, 3, 1});
    check_row({"closures, the ways back", cl, p2, true, false, 0, false, false, true, false, 0, {kRedNone, kRedNone, kRedNone},
               {bO, bT, bT}, {}}, {17, 3, 1});
    // a shard of blocks [129, 17, 3]: an open top, every way back a launch of its own
    BcrShape sh = shape_of(8, 129, 0, true, false);
    p1.open_top = p2.open_top = true;
    check_row({"a shard, the reductions", sh, p1, true, false, 0, false, false, false, false, 0, {O, O, O}, {bN, bN, bN},
               {launch(true, false, true, false, 0), launch(false, false, true, false, 0), launch(false, false, true, false, 0)}},
              {17, 3, 1});
    check_row({"a shard, the ways back", sh, p2, true, false, 0, false, false, false, false, 0, {kRedNone, kRedNone, kRedNone},
               {bO, bO, bO}, {}}, {17, 3, 1});
}

int main() {
    enumerate();
    rows();
    if (failures) {
        std::fprintf(stderr, "%ld expectation(s) failed over %ld points\n", failures, points);
        return 1;
    }
    std::printf("bcr route host check ok (%ld points)\n", points);
    return 0;
}
