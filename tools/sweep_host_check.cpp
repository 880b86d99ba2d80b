// sweep_host_check.cpp -- the pieces k_sweep runs (irotavg_amd/csrc/sweep.hpp: the prediction, one term, the step,
// sweep_sorted) held against the definition written out in sequence, as a stand-alone program that needs no device, meant
// to be built with a sanitizer:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iirotavg_amd/csrc
//       tools/sweep_host_check.cpp -o sweep_host_check && ./sweep_host_check
// Exit status 0 and "sweep host check ok" when every expectation holds.
#include <cstdio>

#include "sweep.hpp"

using namespace irh;
typedef long double LD;

static int failures = 0;
#define EXPECT(c)                                                \
    do {                                                         \
        if (!(c)) {                                              \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
            failures++;                                          \
        }                                                        \
    } while (0)

struct QL {
    LD x, y, z, w;
};
static QL mul(QL a, QL b) {
    return QL{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
              a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
static LD angle_between(QL a, QL b) {
    a.w = -a.w;
    const QL d = mul(a, b);
    return 2 * std::atan2(std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z), std::fabs(d.w));
}

struct Problem {
    int64_t n_total;
    int f;
    std::vector<int32_t> I;
    std::vector<double> qq, Q, w;  // rows [x y z w]; w empty: all ones
};

// The definition in sequence, in long double: the neighbours of a view from a list per view in edge order, sorted by
// neighbour alone (stable), one running sum per view.
static std::vector<QL> literal(const Problem &p, bool l1, int sweeps, int inner, double floor, std::vector<LD> &step) {
    const LD pi = 4 * std::atan((LD)1);
    struct Half {
        int32_t u;
        uint32_t k;
        bool along;  // the half-edge v -> u runs along the stored direction: q(k, u -> v) has w negated
    };
    const int64_t m = (int64_t)p.I.size() / 2;
    std::vector<std::vector<Half>> nb((size_t)p.n_total);
    for (int64_t k = 0; k < m; k++) {
        const int32_t a = p.I[2 * k], b = p.I[2 * k + 1];
        if (a == b) continue;
        nb[(size_t)a].push_back(Half{b, (uint32_t)k, true});
        nb[(size_t)b].push_back(Half{a, (uint32_t)k, false});
    }
    for (auto &row : nb) std::stable_sort(row.begin(), row.end(), [](const Half &s, const Half &t) { return s.u < t.u; });
    std::vector<QL> Q((size_t)p.n_total);
    for (int64_t v = 0; v < p.n_total; v++) Q[(size_t)v] = QL{p.Q[4 * v], p.Q[4 * v + 1], p.Q[4 * v + 2], p.Q[4 * v + 3]};
    step.assign((size_t)sweeps, 0);
    for (int t = 0; t < sweeps; t++) {
        std::vector<QL> next = Q;
        for (int64_t v = p.f; v < p.n_total; v++) {
            QL y = Q[(size_t)v];
            for (int j = 0; j < inner; j++) {
                LD sx = 0, sy = 0, sz = 0, sc = 0;
                for (const Half &h : nb[(size_t)v]) {
                    QL q{p.qq[4 * h.k], p.qq[4 * h.k + 1], p.qq[4 * h.k + 2], p.qq[4 * h.k + 3]};
                    if (h.along) q.w = -q.w;
                    QL yi = y;
                    yi.w = -yi.w;
                    const QL d = mul(yi, mul(q, Q[(size_t)h.u]));
                    const LD s = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
                    LD th = 2 * std::atan2(s, d.w);
                    if (th >= pi) th -= 2 * pi;
                    LD r[3] = {d.x * th / s, d.y * th / s, d.z * th / s};
                    if (s < (LD)SWEEP_EPS) r[0] = r[1] = r[2] = 0;
                    const LD wk = p.w.empty() ? (LD)1 : (LD)p.w[h.k];
                    if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]) || !std::isfinite(wk) || !(wk > 0)) continue;
                    const LD rho = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
                    const LD c = l1 ? wk / std::max(rho, (LD)floor) : wk;
                    sx += c * r[0], sy += c * r[1], sz += c * r[2], sc += c;
                }
                const LD x[3] = {sc > 0 ? sx / sc : 0, sc > 0 ? sy / sc : 0, sc > 0 ? sz / sc : 0};
                const LD th = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
                if (j == 0 && th > step[(size_t)t]) step[(size_t)t] = th;
                const LD coef = th > 0 ? std::sin(th / 2) / th : 0;
                y = mul(y, QL{x[0] * coef, x[1] * coef, x[2] * coef, std::cos(th / 2)});
            }
            next[(size_t)v] = y;
        }
        Q.swap(next);
    }
    return Q;
}

// rotations of a few tenths of a radian from a closed form: every residual stays far from the wrap at pi
static void quat(double s, double out[4]) {
    const double v[4] = {std::sin(s + 1.0), std::cos(2.0 * s), std::sin(3.0 * s + 0.5), 4.0};
    const double nrm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    for (int c = 0; c < 4; c++) out[c] = v[c] / nrm;
}
// edges typed in; measurements Q_b (x) Q_a* of the closed-form truth, each turned a little; the start is another closed form
static Problem problem(int64_t n_total, int f, const std::vector<int32_t> &I) {
    Problem p{n_total, f, I, {}, {}, {}};
    const size_t m = I.size() / 2;
    p.qq.resize(4 * m);
    p.Q.resize(4 * (size_t)n_total);
    for (size_t k = 0; k < m; k++) {
        double a[4], b[4], e[4];
        quat(0.7 * I[2 * k], a);
        quat(0.7 * I[2 * k + 1], b);
        quat(100.0 + 1.3 * (double)k, e);
        const CycQ q = cyc_qmul(CycQ{e[0] * 0.1, e[1] * 0.1, e[2] * 0.1, 1.0}, cyc_qmul(CycQ{b[0], b[1], b[2], b[3]}, CycQ{a[0], a[1], a[2], -a[3]}));
        p.qq[4 * k] = -q.x, p.qq[4 * k + 1] = -q.y, p.qq[4 * k + 2] = -q.z, p.qq[4 * k + 3] = -q.w;  // (b (x) [a, -w]: minus b a*)
    }
    for (int64_t v = 0; v < n_total; v++) quat(0.7 * (double)v + 0.2 * std::sin(5.0 * (double)v), &p.Q[4 * (size_t)v]);
    return p;
}
// a star: view 0 fixed, the leaves 1 .. d, the centre d + 1, and one self loop at the centre (degree 0: nothing else)
static Problem star(int d) {
    std::vector<int32_t> I;
    for (int l = 1; l <= d; l++) I.insert(I.end(), {l % 2 ? l : d + 1, l % 2 ? d + 1 : l});
    I.insert(I.end(), {d + 1, d + 1});
    if (d > 0) I.insert(I.end(), {0, 1});
    return problem(d + 2, 1, I);
}

static void run(const Problem &p, const char *name) {
    const int64_t m = (int64_t)p.I.size() / 2;
    const int widths[3] = {1, 8, 16}, caps[2] = {2, 48};
    for (int l1 = 0; l1 < 2; l1++)
        for (int inner = 1; inner <= 3; inner += 2) {
            const int sweeps = 3;
            std::vector<LD> step;
            const std::vector<QL> want = literal(p, l1 != 0, sweeps, inner, 1e-6, step);
            LD worst = 0;
            for (int wi = 0; wi < 3; wi++)
                for (int ci = 0; ci < 2; ci++) {
                    std::vector<double> Q = p.Q;
                    SweepResult R;
                    EXPECT(sweep_sorted(m, p.n_total, p.f, p.I.data(), p.qq.data(), Q.data(), p.w.empty() ? nullptr : p.w.data(), l1 != 0,
                                        sweeps, inner, 1e-6, widths[wi], caps[ci], R) == CYC_OK);
                    for (int64_t v = 0; v < p.n_total; v++) {
                        const QL got{Q[4 * v], Q[4 * v + 1], Q[4 * v + 2], Q[4 * v + 3]};
                        worst = std::max(worst, angle_between(got, want[(size_t)v]));
                        if (v < p.f) EXPECT(Q[4 * v] == p.Q[4 * v] && Q[4 * v + 3] == p.Q[4 * v + 3]);
                    }
                    for (int t = 0; t < sweeps; t++) worst = std::max(worst, std::fabs((LD)R.step[(size_t)t] - step[(size_t)t]));
                }
            // every width and cap lies within 1e-13 of the definition: within 2e-13 of each other, which the bound below halves
            if (!(worst <= 5e-14L)) std::fprintf(stderr, "%s, l1 %d, inner %d: %.3Le rad\n", name, l1, inner, worst);
            EXPECT(worst <= 5e-14L);
        }
}

int main() {
    {  // the pieces: a prediction along and against the stored direction, the leave-out rule, the floor, the step
        const CycQ qq{0.1, 0.2, 0.3, 0.9}, qu{0.0, 0.0, 0.0, 1.0};
        EXPECT(sweep_prediction(qq, true, qu).w == 0.9 && sweep_prediction(qq, false, qu).w == -0.9);
        const CycQ y{0.0, 0.0, 0.0, 1.0}, P{std::sin(0.25), 0.0, 0.0, std::cos(0.25)};
        double r[3];
        sweep_residual(y, P, r);
        EXPECT(std::fabs(std::fabs(r[0]) - 0.5) < 1e-15 && r[1] == 0.0 && r[2] == 0.0);
        sweep_residual(y, y, r);
        EXPECT(r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0);  // s < EPS
        SweepSum a = sweep_zero();
        sweep_term(a, y, P, 0.0, true, 1e-6), sweep_term(a, y, P, -1.0, true, 1e-6), sweep_term(a, y, P, NAN, true, 1e-6);
        sweep_term(a, y, P, INFINITY, false, 1e-6), sweep_term(a, y, CycQ{NAN, 0.0, 0.0, 1.0}, 1.0, false, 1e-6);
        EXPECT(a.c == 0.0 && a.x == 0.0);
        double x[3];
        EXPECT(sweep_mean(a, x) == 0.0 && x[0] == 0.0);
        sweep_term(a, y, P, 2.0, true, 1.0);  // below the floor: c = w / floor
        EXPECT(a.c == 2.0);
        sweep_term(a, y, P, 2.0, true, 1e-6);
        EXPECT(std::fabs(a.c - 6.0) < 1e-14);
        const double big[3] = {INFINITY, 0.0, 0.0}, none[3] = {0.0, 0.0, 0.0};
        EXPECT(sweep_step(P, big, INFINITY).x == P.x && sweep_step(P, none, 0.0).x == P.x && sweep_step(P, none, 0.0).w == P.w);
        double mx = 0.0;
        sweep_max(mx, NAN), sweep_max(mx, 2.0), sweep_max(mx, NAN);
        EXPECT(mx == 2.0);
    }
    const int degrees[9] = {0, 1, 7, 8, 9, 47, 48, 49, 99};  // G - 1, G, G + 1, kStage - 1, kStage, kStage + 1, 2 kStage + 3
    for (int d : degrees) run(star(d), "star");
    {  // a ring of seven with chords, a parallel and a reversed duplicate edge, a self loop, a NaN row, f = 3, weights
        Problem p = problem(7, 3, {0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 0, 0, 3, 1, 4, 2, 5, 3, 4, 4, 3, 5, 5, 6, 2, 3, 6});
        run(p, "ring");
        p.qq[4 * 9 + 1] = NAN;                                                    // edge 9 = (2, 5)
        p.w = {1.0, 2.0, 0.5, 1.0, 0.0, 3.0, -1.0, 1.0, 1.5, 1.0, NAN, 2.0, 1.0, 0.0, 0.25};  // view 6 keeps the terms of (5, 6) and (3, 6)
        run(p, "ring, weighted");
        p.w[5] = 0.0, p.w[14] = INFINITY;                                         // ... and now none: its row empties
        run(p, "ring, view 6 without a term");
        std::vector<double> Q = p.Q;
        SweepResult R;
        EXPECT(sweep_sorted(15, 7, 3, p.I.data(), p.qq.data(), Q.data(), p.w.data(), true, 2, 3, 1e-6, 8, 2, R) == CYC_OK);
        EXPECT(R.info[0] == 18&& R.info[1] == 0 && Q[24] == p.Q[24] && Q[27] == p.Q[27]);
        p.I[3] = 7;
        EXPECT(sweep_sorted(15, 7, 3, p.I.data(), p.qq.data(), Q.data(), nullptr, true, 1, 1, 1e-6, 8, 48, R) == CYC_BAD_ID);
    }
    if (failures) return 1;
    std::printf("sweep host check ok\n");
    return 0;
}
