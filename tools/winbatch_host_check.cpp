// winbatch_host_check.cpp -- the host arithmetic of irotavg_window_solve_batch_dev (irotavg_amd/csrc/winbatch.hpp: size
// checks, packing offsets, descriptors, the stride rule, the span of a strided matrix and the 16-byte row rule) and of
// irotavg_window_uncertainty_batch_dev / irotavg_window_gate_batch_dev (pair and candidate offsets, the LDS layout with its
// chunk of candidate measurements, the "nothing asked for" rules) as a stand-alone program that needs no device, meant to
// be built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/winbatch_host_check.cpp -o winbatch_host_check && ./winbatch_host_check
// Exit status 0 and "winbatch host check ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "winbatch.hpp"

using namespace irh;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
            failures++;                                                  \
        }                                                                \
    } while (0)

static void check_plan(const std::vector<int32_t> &sizes, int kernel) {
    const int64_t nb = (int64_t)sizes.size() / 3;
    WinBatchPlan P;
    EXPECT(winbatch_plan(nb, sizes.data(), kernel, P));
    EXPECT((int64_t)P.desc.size() == nb);
    std::vector<char> seen((size_t)nb, 0);
    std::vector<int64_t> eoff((size_t)nb), voff((size_t)nb);
    int64_t e = 0, v = 0;
    for (int64_t b = 0; b < nb; b++) {
        eoff[(size_t)b] = e;
        voff[(size_t)b] = v;
        v += sizes[3 * b];
        e += sizes[3 * b + 2];
    }
    EXPECT(P.sum_m == e && P.sum_n == v);
    size_t lds = 0;
    int last_w = -1, last_g = -1;
    for (int64_t i = 0; i < nb; i++) {
        const WinDesc &d = P.desc[(size_t)i];
        EXPECT(d.idx >= 0 && d.idx < nb && !seen[(size_t)d.idx]);
        seen[(size_t)d.idx] = 1;
        EXPECT(d.nv == sizes[3 * d.idx] && d.f == sizes[3 * d.idx + 1] && d.ne == sizes[3 * d.idx + 2]);
        EXPECT(d.eoff == eoff[(size_t)d.idx] && d.voff == voff[(size_t)d.idx]);
        const bool wave = i < P.nwave;
        if (wave) {
            EXPECT(win_fits_wave(d.nv, d.f, d.ne) && kernel != 1);
            EXPECT(d.idx > last_w);  // each list in the caller's order
            last_w = d.idx;
        } else {
            EXPECT(kernel == 1 || !win_fits_wave(d.nv, d.f, d.ne));
            EXPECT(d.idx > last_g);
            last_g = d.idx;
            const size_t l = win_lds_bytes_user(d.nv, d.ne, d.nv - d.f);
            EXPECT(l <= WIN_MAX_LDS);
            if (l > lds) lds = l;
        }
    }
    EXPECT(P.lds == lds);
}

int main() {
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
    const int64_t lmax = std::numeric_limits<int64_t>::max(), lmin = std::numeric_limits<int64_t>::min();
    WinBatchPlan P;
    // counts and kernels
    const int32_t one[3] = {12, 2, 40};
    EXPECT(!winbatch_plan(0, one, 0, P) && !winbatch_plan(-1, one, 0, P) && !winbatch_plan(lmin, one, 0, P));
    EXPECT(!winbatch_plan(WIN_BATCH_MAX + 1, one, 0, P) && !winbatch_plan(lmax, one, 0, P));
    EXPECT(!winbatch_plan(1, nullptr, 0, P) && !winbatch_plan(1, one, 3, P) && !winbatch_plan(1, one, -1, P));
    EXPECT(winbatch_plan(1, one, 0, P) && P.nwave == 1 && P.lds == 0);
    EXPECT(winbatch_plan(1, one, 1, P) && P.nwave == 0 && P.lds == win_lds_bytes_user(12, 40, 10));
    // sizes at and past the limits, and values that overflow int32 arithmetic when subtracted or summed
    const int32_t bad[][3] = {{66, 1, 100}, {321, 300, 100}, {70, 6, 641}, {20, 20, 30}, {20, 1, 0}, {20, -1, 30},
                              {0, 0, 5}, {-3, 0, 5}, {20, 21, 30}, {imax, imax - 1, 5}, {imax, 0, imax}, {imin, 0, 5},
                              {5, imin, 5}, {imin, imax, imin}, {imax, imin, imax}, {5, 1, imin}, {5, 1, imax}};
    for (const auto &b : bad) {
        const int32_t s[9] = {12, 2, 40, b[0], b[1], b[2], 2, 1, 1};
        EXPECT(!winbatch_plan(3, s, 0, P));
        EXPECT(!winbatch_plan(3, s, 1, P));
        EXPECT(!winbatch_plan(1, b, 2, P));
    }
    EXPECT(!win_fits(imax, imin, 1) && !win_fits_wave(imax, imin, 1) && !win_fits(imin, imax, 1));
    const int32_t w17[3] = {18, 1, 40}, e65[3] = {12, 2, 65};
    EXPECT(!winbatch_plan(1, w17, 2, P) && !winbatch_plan(1, e65, 2, P));
    EXPECT(winbatch_plan(1, w17, 0, P) && P.nwave == 0);
    // mixed plans, every kernel choice
    {
        std::vector<int32_t> s;
        unsigned r = 12345u;
        auto rnd = [&](int lo, int hi) {
            r = r * 1664525u + 1013904223u;
            return lo + (int)((r >> 8) % (unsigned)(hi - lo + 1));
        };
        for (int b = 0; b < 5000; b++) {
            const int nu = rnd(1, 64), f = rnd(0, 320 - nu);
            int ne = rnd(1, 640);
            while (!win_fits(nu + f, f, ne)) ne--;
            s.insert(s.end(), {nu + f, f, ne});
        }
        check_plan(s, 0);
        check_plan(s, 1);
        std::vector<int32_t> w;
        for (size_t b = 0; b < s.size() / 3; b++)
            if (win_fits_wave(s[3 * b], s[3 * b + 1], s[3 * b + 2])) w.insert(w.end(), {s[3 * b], s[3 * b + 1], s[3 * b + 2]});
        EXPECT(!w.empty());
        check_plan(w, 2);
        check_plan(w, 0);
    }
    // nb at the cap, every problem at the limits: a BYTE offset (32 per row) in int32 would overflow
    {
        std::vector<int32_t> s;
        s.reserve(3 * (size_t)WIN_BATCH_MAX);
        for (int64_t b = 0; b < WIN_BATCH_MAX; b++) s.insert(s.end(), {320, 256, 640});
        check_plan(s, 0);
        EXPECT(winbatch_plan(WIN_BATCH_MAX, s.data(), 1, P));
        EXPECT(P.sum_m == WIN_BATCH_MAX * 640 && P.sum_n == WIN_BATCH_MAX * 320 && 32 * P.sum_m > (int64_t)imax);
        EXPECT(P.desc.back().eoff == (WIN_BATCH_MAX - 1) * 640 && P.desc.back().voff == (WIN_BATCH_MAX - 1) * 320);
        int64_t lo, hi;
        EXPECT(strides_ok(P.sum_m, 4, 4, 1) && strides_ok(P.sum_m, 4, (int64_t)1 << 31, 1));
        matrix_span(P.sum_m, 4, (int64_t)1 << 31, -1, lo, hi);
        EXPECT(lo == -3 && hi == (P.sum_m - 1) * ((int64_t)1 << 31));
        EXPECT(!strides_ok(P.sum_m, 4, 1, P.sum_m - 1) && strides_ok(P.sum_m, 4, 1, P.sum_m) &&
               strides_ok(P.sum_m, 4, -1, -P.sum_m));
    }
    // the stride rule at its edges
    const int64_t L = (int64_t)1 << 31;
    EXPECT(strides_ok(100, 4, 4, 1) && strides_ok(100, 4, -4, 1) && strides_ok(100, 4, 4, -1) && strides_ok(100, 4, 1, 100));
    EXPECT(strides_ok(100, 4, 1, -100) && strides_ok(100, 4, 3, 300) && strides_ok(100, 4, 6, 1) && strides_ok(1, 4, 1, 1));
    EXPECT(!strides_ok(100, 4, 3, 1) && !strides_ok(100, 4, 1, 99) && !strides_ok(100, 4, 2, 1) && !strides_ok(100, 4, 1, 1));
    EXPECT(!strides_ok(100, 4, 0, 1) && !strides_ok(100, 4, 4, 0) && !strides_ok(0, 4, 4, 1) && !strides_ok(-5, 4, 4, 1));
    EXPECT(strides_ok(100, 4, L, 1) && strides_ok(100, 4, -L, 1) && strides_ok(100, 4, 1, L) && strides_ok(L, 4, L, 1));
    EXPECT(strides_ok(L, 4, 1, L) && !strides_ok(L, 4, 1, L - 1) && !strides_ok(L + 1, 4, 4, 1));
    EXPECT(!strides_ok(100, 4, L + 1, 1) && !strides_ok(100, 4, 1, -L - 1) && !strides_ok(100, 4, lmax, 1));
    EXPECT(!strides_ok(100, 4, lmin, 1) && !strides_ok(100, 4, 1, lmin) && !strides_ok(100, 4, lmin, lmin) &&
           !strides_ok(lmax, 4, 4, 1) && !strides_ok(lmin, 4, 4, 1));
    {
        int64_t lo, hi;
        matrix_span(100, 4, 4, 1, lo, hi);
        EXPECT(lo == 0 && hi == 399);
        matrix_span(100, 4, -4, 1, lo, hi);
        EXPECT(lo == -396 && hi == 3);
        matrix_span(100, 4, 1, -128, lo, hi);
        EXPECT(lo == -384 && hi == 99);
        matrix_span(L, 4, -L, -L, lo, hi);  // the largest accepted magnitudes: no overflow
        EXPECT(lo == -(L - 1) * L - 3 * L && hi == 0);
        matrix_span(1, 1, 1, 1, lo, hi);
        EXPECT(lo == 0 && hi == 0);
    }
    // 16-byte row accesses: contiguous rows behind a 16-byte aligned pointer, nothing else
    EXPECT(rows16(0x1000, 4, 1) && rows16(0x1010, 4, 1) && !rows16(0x1008, 4, 1) && !rows16(0x1004, 4, 1));
    EXPECT(!rows16(0x1000, 1, 4) && !rows16(0x1000, 8, 1) && !rows16(0x1000, 4, 2) && !rows16(0x1000, -4, 1) &&
           !rows16(0x1000, 4, -1) && !rows16(0x1000, 1, 1000) && !rows16(0x1000, lmin, 1) && !rows16(0x1000, 4, lmax));
    EXPECT(rows16(~(uintptr_t)15, 4, 1) && !rows16(~(uintptr_t)7, 4, 1));
    // ---- the uncertainty batch (irotavg_window_uncertainty_batch_dev): pair offsets, LDS, the "nothing asked for" rule
    {
        WinCovPlan C;
        const int32_t np1[1] = {5}, neg[1] = {-1};
        EXPECT(!wincov_plan(0, one, nullptr, nullptr, C) && !wincov_plan(-1, one, np1, nullptr, C) && !wincov_plan(WIN_BATCH_MAX + 1, one, nullptr, nullptr, C));
        EXPECT(!wincov_plan(1, nullptr, np1, nullptr, C) && !wincov_plan(1, one, neg, nullptr, C));
        EXPECT(wincov_plan(1, one, nullptr, nullptr, C) && C.sum_p == 0 && C.desc[0].np == 0 && C.desc[0].poff == 0);
        EXPECT(wincov_plan(1, one, np1, nullptr, C) && C.sum_p == 5 && C.desc[0].np == 5 && C.sum_m == 40 && C.sum_n == 12);
        EXPECT(C.lds == wincov_lds(12, 40, 10, true).bytes);
        for (const auto &b : bad) {
            const int32_t s[9] = {12, 2, 40, b[0], b[1], b[2], 2, 1, 1}, c[3] = {0, 1, 2};
            EXPECT(!wincov_plan(3, s, c, nullptr, C) && !wincov_plan(3, s, nullptr, nullptr, C));
        }
        const int32_t s3[9] = {12, 2, 40, 320, 256, 640, 2, 1, 1}, c3[3] = {7, 0, imax}, cneg[3] = {7, imin, 3};
        EXPECT(!wincov_plan(3, s3, cneg, nullptr, C));
        EXPECT(wincov_plan(3, s3, c3, nullptr, C) && C.sum_p == 7 + (int64_t)imax && C.sum_m == 681 && C.sum_n == 334);
        EXPECT(C.desc[0].poff == 0 && C.desc[1].poff == 7 && C.desc[2].poff == 7 && C.desc[2].np == imax);
        EXPECT(C.lds == wincov_lds(320, 640, 64, true).bytes && C.lds <= WIN_MAX_LDS);
        // random batches: descriptors in the caller's order, offsets the 64-bit cumulative sums
        std::vector<int32_t> s, c;
        unsigned r = 777u;
        auto rnd = [&](int lo, int hi) {
            r = r * 1664525u + 1013904223u;
            return lo + (int)((r >> 8) % (unsigned)(hi - lo + 1));
        };
        for (int b = 0; b < 3000; b++) {
            const int nu = rnd(1, 64), f = rnd(0, 320 - nu);
            int ne = rnd(1, 640);
            while (!win_fits(nu + f, f, ne)) ne--;
            s.insert(s.end(), {nu + f, f, ne});
            c.push_back(b % 3 == 0 ? 0 : rnd(0, 4000000));
        }
        EXPECT(wincov_plan(3000, s.data(), c.data(), nullptr, C) && C.desc.size() == 3000);
        int64_t e = 0, v = 0, p = 0;
        size_t lds = 0;
        for (int b = 0; b < 3000; b++) {
            const WinCovDesc &d = C.desc[(size_t)b];
            EXPECT(d.d.idx == b && d.d.nv == s[3 * b] && d.d.f == s[3 * b + 1] && d.d.ne == s[3 * b + 2] && d.np == c[(size_t)b]);
            EXPECT(d.d.eoff == e && d.d.voff == v && d.poff == p);
            const WinCovLds L = wincov_lds(d.d.nv, d.d.ne, d.d.nv - d.d.f, true);
            // the arrays follow each other without overlap; double4 rows on 32 bytes, doubles and id pairs on 8
            EXPECT(L.oQ == 0 && L.oQQ == 32 * (size_t)d.d.nv && L.oR == L.oQQ + 32 * (size_t)d.d.ne && L.oM == L.oR + 32 * (size_t)d.d.ne);
            EXPECT(L.oI == L.oM + 8 * (size_t)(d.d.nv - d.d.f) * WINCOV_LD && L.oSc == L.oI + 8 * (size_t)d.d.ne);
            EXPECT(L.oM % 32 == 0 && L.oI % 8 == 0 && L.oRed % 8 == 0 && L.bytes == L.oRed + 16 * WINCOV_THREADS && L.bytes <= WIN_MAX_LDS);
            if (L.bytes > lds) lds = L.bytes;
            e += d.d.ne;
            v += d.d.nv;
            p += d.np;
        }
        EXPECT(C.sum_m == e && C.sum_n == v && C.sum_p == p && C.lds == lds && p > (int64_t)imax);
        // the staged kernel's layout: no copy of the measurements, laid out for the limits
        const WinCovLds O = wincov_lds(WIN_MAX_NV, WIN_MAX_NE, WIN_MAX_NU, false);
        EXPECT(O.oQQ == O.oR && O.oR == 10240 && O.oM == 30720 && O.oI == 64000 && O.bytes == 74752);
        // asked for: any one output is enough; pairs need a positive count AND both arrays
        EXPECT(!wincov_asked(false, 0, false, false, false, false, false) && !wincov_asked(false, 0, true, false, false, false, false));
        EXPECT(wincov_asked(true, 0, false, false, false, false, false) && wincov_asked(false, 0, false, true, false, false, false));
        EXPECT(wincov_asked(false, 0, false, false, true, false, false) && wincov_asked(false, 0, false, false, false, true, false));
        EXPECT(wincov_asked(false, 0, false, false, false, false, true) && wincov_asked(false, 3, true, false, false, false, false));
        EXPECT(!wincov_asked(true, 3, false, true, true, true, true) && !wincov_asked(true, -1, true, true, true, true, true));
        EXPECT(!wincov_asked(true, lmin, true, true, true, true, true) && wincov_asked(false, lmax, true, false, false, false, false));
    }
    // ---- the gate batch (irotavg_window_gate_batch_dev): candidate offsets and counts, the LDS chunk, its "asked for" rule
    {
        WinCovPlan C;
        const int32_t nc1[1] = {5}, neg[1] = {-1}, np1[1] = {3};
        EXPECT(!wincov_plan(0, one, nullptr, nc1, C) && !wincov_plan(1, nullptr, nullptr, nc1, C) && !wincov_plan(1, one, nullptr, neg, C));
        EXPECT(!wincov_plan(1, one, neg, nc1, C) && !wincov_plan(1, one, np1, neg, C));
        EXPECT(wincov_plan(1, one, nullptr, nullptr, C) && C.sum_c == 0 && C.desc[0].nc == 0 && C.desc[0].coff == 0);
        EXPECT(wincov_plan(1, one, np1, nc1, C) && C.sum_c == 5 && C.sum_p == 3 && C.desc[0].nc == 5 && C.desc[0].np == 3);
        EXPECT(C.lds == wincov_lds(12, 40, 10, true, 5).bytes && C.lds == wincov_lds(12, 40, 10, true, 5).oC + 5 * 32);
        for (const auto &b : bad) {
            const int32_t s[9] = {12, 2, 40, b[0], b[1], b[2], 2, 1, 1}, c[3] = {0, 1, 2};
            EXPECT(!wincov_plan(3, s, nullptr, c, C));
        }
        const int32_t s3[9] = {12, 2, 40, 320, 256, 640, 2, 1, 1}, c3[3] = {7, imax, imax}, cneg[3] = {7, imin, 3};
        EXPECT(!wincov_plan(3, s3, nullptr, cneg, C));
        EXPECT(wincov_plan(3, s3, nullptr, c3, C) && C.sum_c == 7 + 2 * (int64_t)imax && C.sum_p == 0);
        EXPECT(C.desc[0].coff == 0 && C.desc[1].coff == 7 && C.desc[2].coff == 7 + (int64_t)imax && C.desc[2].nc == imax);
        // the chunk never grows past WINCOV_CAND_CHUNK rows: the largest problem with any number of candidates fits
        EXPECT(C.lds == wincov_lds(320, 640, 64, true, imax).bytes && C.lds == wincov_lds(320, 640, 64, true).oC + 32 * WINCOV_CAND_CHUNK);
        EXPECT(C.lds <= WIN_MAX_LDS && WINCOV_CAND_CHUNK == 256);
        EXPECT(wincov_lds(12, 40, 10, true, -4).bytes == wincov_lds(12, 40, 10, true).bytes);
        EXPECT(wincov_lds(12, 40, 10, true, 256).bytes == wincov_lds(12, 40, 10, true, 257).bytes);
        // random batches: offsets the 64-bit cumulative sums of both counts, the chunk behind the reduction scratch
        std::vector<int32_t> s, c, pc;
        unsigned r = 4242u;
        auto rnd = [&](int lo, int hi) {
            r = r * 1664525u + 1013904223u;
            return lo + (int)((r >> 8) % (unsigned)(hi - lo + 1));
        };
        for (int b = 0; b < 3000; b++) {
            const int nu = rnd(1, 64), f = rnd(0, 320 - nu);
            int ne = rnd(1, 640);
            while (!win_fits(nu + f, f, ne)) ne--;
            s.insert(s.end(), {nu + f, f, ne});
            c.push_back(b % 4 == 0 ? 0 : (b % 4 == 1 ? rnd(1, 300) : rnd(0, 4000000)));
            pc.push_back(rnd(0, 9));
        }
        EXPECT(wincov_plan(3000, s.data(), pc.data(), c.data(), C) && C.desc.size() == 3000);
        int64_t p = 0, q = 0;
        size_t lds = 0;
        for (int b = 0; b < 3000; b++) {
            const WinCovDesc &d = C.desc[(size_t)b];
            EXPECT(d.d.idx == b && d.nc == c[(size_t)b] && d.np == pc[(size_t)b] && d.coff == q && d.poff == p);
            const WinCovLds L = wincov_lds(d.d.nv, d.d.ne, d.d.nv - d.d.f, true, d.nc), L0 = wincov_lds(d.d.nv, d.d.ne, d.d.nv - d.d.f, true);
            // double4 rows on 32 bytes behind everything the plain layout holds; without candidates nothing is added
            EXPECT(L.oC >= L0.bytes && L.oC < L0.bytes + 32 && L.oC % 32 == 0 && L.oRed == L0.oRed && L.oM == L0.oM);
            EXPECT(L0.bytes == L0.oRed + 16 * WINCOV_THREADS && L.bytes <= WIN_MAX_LDS);
            EXPECT(L.bytes == (d.nc ? L.oC + 32 * (size_t)(d.nc < WINCOV_CAND_CHUNK ? d.nc : WINCOV_CAND_CHUNK) : L0.bytes));
            if (L.bytes > lds) lds = L.bytes;
            p += d.np;
            q += d.nc;
        }
        EXPECT(C.sum_c == q && C.sum_p == p && C.lds == lds && q > (int64_t)imax);
        // asked for: an output needs candidates to fill it; the scale alone is a request; a count needs both arrays
        EXPECT(!wingate_asked(0, false, false, false, false, false) && !wingate_asked(0, true, true, true, true, false));
        EXPECT(wingate_asked(0, false, false, false, false, true) && wingate_asked(0, false, true, true, true, true));
        EXPECT(wingate_asked(4, true, true, false, false, false) && wingate_asked(4, true, false, true, false, false));
        EXPECT(wingate_asked(4, true, false, false, true, false) && wingate_asked(4, true, false, false, false, true));
        EXPECT(!wingate_asked(4, true, false, false, false, false) && !wingate_asked(4, false, true, true, true, true));
        EXPECT(!wingate_asked(-1, true, true, true, true, true) && !wingate_asked(lmin, true, true, true, true, true));
        EXPECT(wingate_asked(lmax, true, true, false, false, false));
    }
    // ---- the pinned block of a batched call (batchdev.hpp): records, then descriptors on 8 bytes; what reserve is asked for
    {
        const size_t recs[3] = {sizeof(WinResult), sizeof(WinCovResult), 8}, descs[2] = {sizeof(WinDesc), sizeof(WinCovDesc)};
        for (size_t rec : recs)
            for (size_t desc : descs)
                for (size_t nb : {(size_t)1, (size_t)3, (size_t)70, (size_t)WIN_BATCH_MAX}) {
                    const BatchBlock L = batch_block(rec, desc, nb);
                    EXPECT(L.oD == rec * nb && L.oD % 8 == 0 && L.bytes == L.oD + desc * nb && L.headroom == L.bytes / 2);
                    // the next size the block serves without growing again
                    EXPECT(batch_block(rec, desc, nb + nb / 2).bytes <= L.bytes + L.headroom);
                }
    }
    // ---- the coverage rule of the `_dev` argument checks (span_covered): a made-up address space of three allocations,
    // B directly behind A, then a gap, then C
    {
        struct Alloc {
            uintptr_t base;
            size_t size;
        };
        const Alloc A{0x10000, 0x1000}, B{0x11000, 0x800}, C{0x20000, 0x4000}, top{~(uintptr_t)0xfff, 0x1000};
        int asked = 0;
        auto range = [&](uintptr_t at, uintptr_t &base, size_t &size) {
            asked++;
            for (const Alloc &a : {A, B, C, top})
                if (at >= a.base && at - a.base < a.size) {
                    base = a.base;
                    size = a.size;
                    return true;
                }
            return false;
        };
        EXPECT(span_covered(0x10000, 0x11000, range) == 1 && asked == 1);  // all of A: one question
        EXPECT(span_covered(0x10ff8, 0x11000, range) == 1 && span_covered(0x10010, 0x10018, range) == 1);
        EXPECT(span_covered(0x10000, 0x11001, range) == 1);   // one byte into B, which follows A without a gap
        EXPECT(span_covered(0x10800, 0x11800, range) == 1);   // up to the end of B
        EXPECT(span_covered(0x10800, 0x11801, range) == 0);   // one byte past it: the gap
        EXPECT(span_covered(0x10000, 0x20008, range) == 0);   // claimed to end inside C: both ends are somebody's, the gap is not
        EXPECT(span_covered(0x11000, 0x24000, range) == 0 && span_covered(0x20000, 0x24000, range) == 1);
        EXPECT(span_covered(0x20000, 0x24001, range) == 0);
        EXPECT(span_covered(0x18000, 0x18008, range) == -1 && span_covered(0x8, 0x10, range) == -1);  // the first byte is nobody's
        EXPECT(span_covered(0x10010, 0x10010, range) == 0 && span_covered(0x10010, 0x10008, range) == 0);  // empty, wrapped
        EXPECT(span_covered(0x10010, 0x8, range) == 0);
        EXPECT(span_covered(~(uintptr_t)0xfff, ~(uintptr_t)0, range) == 1);  // at the top of the address space: no overflow
        auto liar = [](uintptr_t at, uintptr_t &base, size_t &size) {  // an allocation that does not contain the address asked about
            base = at + 8;
            size = 64;
            return true;
        };
        auto empty = [](uintptr_t at, uintptr_t &base, size_t &size) {
            base = at;
            size = 0;
            return true;
        };
        EXPECT(span_covered(0x1000, 0x1010, liar) == -1 && span_covered(0x1000, 0x1010, empty) == -1);
        auto crumbs = [](uintptr_t at, uintptr_t &base, size_t &size) {  // 8-byte pieces without end: the walk is bounded
            base = at;
            size = 8;
            return true;
        };
        EXPECT(span_covered(0x1000, 0x1000 + 8 * 64, crumbs) == 1 && span_covered(0x1000, 0x1000 + 8 * 64 + 1, crumbs) == 0);
    }
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("winbatch host check ok\n");
    return 0;
}
