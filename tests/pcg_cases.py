"""Cases and a NumPy reference for the FIRST iterates of the multigrid-preconditioned CG (irotavg_amd/csrc/solver.hip,
cgcg.hip, dense.hip), shared by the CPU test of the reference itself (test_pcg_cases_cpu.py) and the GPU test
(test_gpu_pcg_iterates.py). A plain module: building a case and its reference needs no device.

Operator. L0 = A' diag(w^2) A and b = A' diag(w^2) r, A = oracle.make_A (an edge whose second view is fixed has no row,
one whose first view is fixed keeps a single coefficient), r = log_map(delta_rel(I, QQ, Q0)), three columns.

Hierarchy (k_coarse_level / k_coarse_vals / k_coarse_diag). P_l is piecewise constant over agg_l
consecutive rows, the last aggregate may be short; L_{l+1} = P_l' L_l P_l; the inverse diagonal is 0 where the diagonal
is <= 0 (an isolated view: a dead row). The last level is multiplied by its explicit inverse (a dead pivot's row and
column are zero: dense.hip) times dense_scale = 1 on a fresh handle -- or, when the level cap ended the hierarchy above
mg_dense_max, it is the Jacobi sweep omega D^-1 b alone.

Cycle from level l on b_l (cycle_from, down_row, up_row):   x_l = omega D_l^-1 b_l;   b_{l+1} = P_l' (b_l - L_l x_l);
y_{l+1} = cycle(l + 1);   x' = x_l + kc P_l y_{l+1};   y_l = x' + omega D_l^-1 (b_l - L_l x').
Top level. Multiplicative: z = cycle(0) on r. Additive: z = omega D_0^-1 r + kc P_0 cycle(1) on P_0' r.

Iteration. Textbook PCG from x0 = 0, the three columns independently; beta = 0 in the first iteration or after r.z = 0,
alpha = 0 where p.Lp = 0 (the kernels' guards). The scalar r.z lives in two slots that alternate by the parity of the
iteration, as SC_RZ0 / SC_RZ1 do.

Two precisions: Reference(..., dtype=np.float64) inverts the last level with numpy.linalg.inv, dtype=np.longdouble with a
long-double Cholesky + refinement (dense_cases.chol_solve_ld); everything else is dense mat-vecs in the dtype.
e_ref(k) = max|x_k^f64 - x_k^ld| / max|x_k^ld|, and the comparison of any iterate X with the reference is

    ratio = (max|X - x_k^ld| / max|x_k^ld|) / max(e_ref(k), nu 2^-52)          bar: BAR = 16

(the device sums rows in SELL-lane order, aggregates through seg_sum trees and dot products through per-workgroup
partials: a reordering of about as many terms as the float64 reference's own; a CG step adds two quotients of dot
products on top of what the dense-inverse tests allow 8 for).

`mutant=` names a defect applied to the reference alone (test_pcg_cases_cpu.py: what the bar can see).
"""
import functools

import numpy as np

from dense_cases import chol_solve_ld
from irotavg_amd import synth
from oracle import oracle as O

LD = np.longdouble
EPS = 2.0 ** -52
BAR = 16.0
OMEGA = 0.7          # irotavg_default_options: mg_omega (the GPU test passes it on explicitly)

MUTANTS = ("kc", "post_omega", "short_aggregate", "coarse_value", "coarse_excess", "dead_idg_one", "dead_idg_unclamped",
           "beta_zero", "parity", "bottom_rz")


# ---- graphs ---------------------------------------------------------------------------------------------------------
def make_case(name, route, nu, f, bw, opts, aggs, *, dense=True, closures=0, p_loop=0.0, isolated=None, spread=False,
              seed=0):
    """A view sequence of nu free views behind f fixed ones, edges spanning up to bw views, `closures` (or a fraction
    p_loop of the band's edges) long-range edges between free views, optionally one isolated free view (row `isolated`).
    opts: the handle's options; aggs: the aggregation factor of every level but the last, as those options fix them."""
    rng = np.random.default_rng([105, nu, f, bw, seed])
    n = nu + f
    I = []
    for j in range(1, n):
        for dd in range(1, bw + 1):
            if j - dd >= 0 and (dd == 1 or dd == bw or rng.random() < 0.7):
                I.append((j - dd, j))
    I = np.array(I, dtype=np.int64)
    nloop = closures if closures else int(round(p_loop * len(I)))
    if nloop:
        gap = min(400, nu // 2)
        a = rng.integers(f, n - gap, size=nloop)
        b = a + gap + (rng.integers(0, n, size=nloop) % (n - a - gap))
        I = np.concatenate([I, np.stack([a, b], 1)])
    if isolated is not None:
        v = f + isolated
        I = I[(I[:, 0] != v) & (I[:, 1] != v)]
        if f <= v - 1 and v + 1 < n:
            I = np.concatenate([I, [[v - 1, v + 1]]])          # the sequence stays in one piece around it
    I = I.astype(np.int32)
    m = len(I)
    w = 10.0 ** rng.uniform(-3.0, 3.0, size=m) if spread else rng.uniform(0.1, 5.0, size=m)
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(m, 3))), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(n, 3))), Qgt)
    Q0[:f] = Qgt[:f]
    levels = [nu]
    for a_ in aggs:
        levels.append((levels[-1] + a_ - 1) // a_)
    return dict(name=name, route=route, nu=nu, n=n, f=f, bw=bw, I=I, QQ=QQ, Q0=Q0, w=w, opts=dict(opts), aggs=list(aggs),
                levels=levels, dense=dense, far=nloop > 0, kc=1.6 if nloop > 0 else 2.0,
                additive=opts.get("mg_multiplicative_top", 0) != 1, isolated=isolated, spread=spread)


def _small(dense_max, agg0=8, agg=8, **kw):
    return dict(band_direct=-1, mg_dense_max=dense_max, mg_agg0=agg0, mg_agg=agg, **kw)


def _cases():
    C = []

    def add(*a, **k):
        C.append(make_case(*a, **k))
    mult = dict(mg_multiplicative_top=1)
    # multiplicative top: two and three levels
    add("mult2-255", "mult", 255, 1, 8, _small(64, **mult), [8])                       # last aggregate of 7, one tile
    add("mult2-256", "mult", 256, 3, 32, _small(64, **mult), [8])                      # exactly one tile, 32 full aggregates
    add("mult2-257-a16", "mult", 257, 3, 32, _small(64, agg0=16, **mult), [16], isolated=256)   # dead row = last aggregate
    add("mult3-519", "mult", 519, 3, 32, _small(32, **mult), [8, 8])                   # 65 -> 9, last aggregate of 7
    add("mult3-1025", "mult", 1025, 1, 16, _small(32, **mult), [8, 8], isolated=300)   # dead row inside tile 1
    # additive, two levels, one loop closure: few enough far entries that the p-update and the SpMV are one launch
    add("add2far-1025", "add2far", 1025, 1, 32, _small(200), [8], closures=1)          # 129 coarse rows
    add("add2far-1537", "add2far", 1537, 3, 32, _small(200), [8], closures=1)          # 193 coarse rows
    add("add2far-1025-a16", "add2far", 1025, 3, 32, _small(80, agg0=16), [16], closures=1)      # 65 coarse rows
    # the same system through the separate p-update and SpMV
    add("add2sep-1537", "add2sep", 1537, 3, 32, _small(200, no_fused_pspmv=1), [8], closures=1)
    # additive, two levels, many loop edges
    add("add2loop-256-a16", "add2loop", 256, 1, 16, _small(64, agg0=16), [16], p_loop=0.05)     # one tile, 16 coarse rows
    add("add2loop-505", "add2loop", 505, 1, 16, _small(64), [8], p_loop=0.05)          # 64 coarse rows
    add("add2loop-513", "add2loop", 513, 3, 16, _small(80), [8], p_loop=0.05)          # 65 coarse rows
    add("add2loop-1537", "add2loop", 1537, 1, 16, _small(200), [8], p_loop=0.05)
    add("add2loop-1025-spread", "add2loop", 1025, 1, 8, _small(200), [8], p_loop=0.05, spread=True)
    # additive, three levels, band graph: classic launches with the level-1 down-sweep in the update
    for tag, route, extra in (("l1f", "l1fused", dict(pcg_classic=1)), ("cg2", "cg2", dict(pcg_classic=0))):
        add(tag + "-520", route, 520, 1, 32, _small(32, **extra), [8, 8])                  # 65 -> 9, level 0's aggregates all full
        add(tag + "-577", route, 577, 3, 16, _small(32, **extra), [8, 8], isolated=576)    # 73 -> 10, dead last aggregate
        add(tag + "-1025", route, 1025, 3, 32, _small(32, **extra), [8, 8])               # 129 -> 17, level 1 over two slices
        add(tag + "-1537-spread", route, 1537, 1, 8, _small(64, **extra), [8, 8], spread=True)   # 193 -> 25
    add("cg2-1537-4lev", "cg2", 1537, 3, 32, _small(8, pcg_classic=0), [8, 8, 8])      # 193 -> 25 -> 4: cycle_levels(g, 2)
    # level cap without a dense level: Jacobi at the bottom
    add("cap-mult2-519", "cap", 519, 1, 16, _small(16, mg_levels_max=2, **mult), [8], dense=False)
    add("cap-add2-513", "cap", 513, 3, 32, _small(16, mg_levels_max=2), [8], dense=False)
    add("cap-add2-1025-far", "cap", 1025, 1, 16, _small(16, mg_levels_max=2), [8], dense=False, closures=3)
    add("cap-add3-1025", "cap", 1025, 1, 16, _small(8, mg_levels_max=3, pcg_classic=1), [8, 8], dense=False)
    # every mg_* option left to the build: a loop closure caps the dense level at 1100 rows, aggregates of 2, kc = 1.6
    add("default-1537", "default", 1537, 1, 16, dict(band_direct=-1), [2], closures=1)
    return C


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


# ---- the operator ---------------------------------------------------------------------------------------------------
def residuals(case):
    return O.log_map(O.delta_rel(case["I"], case["QQ"], case["Q0"]))[:, :3]


def operator(case, dtype):
    """(L0, b, excess, first): L0 and b accumulated in `dtype` from the fp64 weights and residuals; excess = the part of
    the diagonal owed to fixed views (row sums of L0, by construction); first = (row, w^2) of one such edge."""
    A = O.make_A(case["n"], case["f"], case["I"]).tocsr()
    A.sort_indices()
    nu = case["nu"]
    w2 = np.asarray(case["w"], dtype=dtype) ** 2
    r = np.asarray(residuals(case), dtype=dtype)
    cnt = np.diff(A.indptr)
    assert cnt.max() <= 2
    L = np.zeros((nu, nu), dtype=dtype)
    b = np.zeros((nu, 3), dtype=dtype)
    ex = np.zeros(nu, dtype=dtype)
    e1 = np.nonzero(cnt == 1)[0]
    c1 = A.indices[A.indptr[e1]]
    a1 = np.asarray(A.data[A.indptr[e1]], dtype=dtype)
    np.add.at(L, (c1, c1), a1 * a1 * w2[e1])
    np.add.at(ex, c1, a1 * a1 * w2[e1])
    np.add.at(b, c1, (a1 * w2[e1])[:, None] * r[e1])
    e2 = np.nonzero(cnt == 2)[0]
    p, q = A.indices[A.indptr[e2]], A.indices[A.indptr[e2] + 1]
    ap, aq = np.asarray(A.data[A.indptr[e2]], dtype=dtype), np.asarray(A.data[A.indptr[e2] + 1], dtype=dtype)
    for (u, au), (v, av) in (((p, ap), (p, ap)), ((q, aq), (q, aq)), ((p, ap), (q, aq)), ((q, aq), (p, ap))):
        np.add.at(L, (u, v), au * av * w2[e2])
    np.add.at(b, p, (ap * w2[e2])[:, None] * r[e2])
    np.add.at(b, q, (aq * w2[e2])[:, None] * r[e2])
    first = (int(c1[0]), w2[e1[0]]) if len(e1) else None
    return L, b, ex, first


# ---- the reference --------------------------------------------------------------------------------------------------
def spd_inverse(sub, dtype):
    """The explicit inverse of a live last level (also of stale_cases.py): numpy.linalg.inv in float64, a long-double
    Cholesky + refinement in long double."""
    if dtype is not LD:
        return np.linalg.inv(sub)
    if len(sub) <= 200:
        return chol_solve_ld(sub, np.eye(len(sub)))
    # (only the family that leaves mg_dense_max to the build has a last level this large, where the Cholesky's Python
    # loops take ten seconds) one Newton step on LAPACK's inverse: the residual I - C X is squared
    inv = np.asarray(np.linalg.inv(np.asarray(sub, dtype=np.float64)), dtype=LD)
    R = np.eye(len(sub), dtype=LD) - sub @ inv
    assert np.abs(R).max() < 1e-9
    return inv + inv @ R


class Reference:
    def __init__(self, case, dtype, levels=None, kc=None, omega=OMEGA, additive=None, mutant=None):
        """levels / kc / additive: what the handle reports (default: what the case's options are expected to give)."""
        assert mutant is None or mutant in MUTANTS
        self.dtype, self.mutant, self.nu = dtype, mutant, case["nu"]
        levels = list(case["levels"] if levels is None else levels)
        assert levels[0] == case["nu"]
        self.omega = dtype(omega)
        self.kc = dtype(case["kc"] if kc is None else kc)
        if mutant == "kc":
            self.kc = self.kc * dtype(1 + 1e-6)
        self.additive = case["additive"] if additive is None else additive
        self.dense = case["dense"]
        L, self.b, ex, first = operator(case, dtype)
        self.L, self.idg, self.agg, self.start, self.member = [L], [], [], [], []
        for l in range(len(levels) - 1):
            n_f, n_c = levels[l], levels[l + 1]
            agg = case["aggs"][l]
            assert (n_f + agg - 1) // agg == n_c, (levels, case["aggs"])       # not the hierarchy the case states
            start = np.arange(0, n_f, agg)
            self.agg.append(agg)
            self.start.append(start)
            self.member.append(np.arange(n_f) // agg)
            C = np.add.reduceat(np.add.reduceat(self.L[l], start, axis=0), start, axis=1)
            if l == 0 and mutant == "coarse_value":
                off = np.abs(C - np.diag(np.diag(C)))
                i, j = np.unravel_index(np.argmax(off), off.shape)
                C[i, j] += dtype(1e-9) * np.abs(C).max()       # (the largest entry of the level: a diagonal one)
            if l == 0 and mutant == "coarse_excess":
                C[first[0] // agg, first[0] // agg] -= first[1]
            self.L.append(C)
        for l, Ll in enumerate(self.L):
            d = np.diag(Ll).copy()
            dead = ~(d > 0)
            with np.errstate(divide="ignore"):
                idg = np.where(dead, dtype(0), dtype(1) / np.where(dead, dtype(1), d))
                if mutant == "dead_idg_one":
                    idg = np.where(dead, dtype(1), idg)
                if mutant == "dead_idg_unclamped":
                    idg = dtype(1) / d
            self.idg.append(idg)
        self.dead_rows = np.nonzero(~(np.diag(L) > 0))[0]
        self.S = None
        if self.dense:
            C = self.L[-1]
            live = np.nonzero(np.diag(C) > 0)[0]
            self.S = np.zeros_like(C)
            self.S[np.ix_(live, live)] = spd_inverse(C[np.ix_(live, live)], dtype)

    # -- the cycle
    def restrict(self, l, v):
        out = np.add.reduceat(v, self.start[l], axis=0)
        if self.mutant == "short_aggregate" and len(v) % self.agg[l]:
            out[-1] = 0
        return out

    def cycle(self, l, b):
        w = (self.omega * self.idg[l])[:, None]
        x = w * b
        if l == len(self.L) - 1:
            return self.S @ b if self.dense else x
        L = self.L[l]
        yc = self.cycle(l + 1, self.restrict(l, b - L @ x))
        xp = x + self.kc * yc[self.member[l]]
        wp = self.idg[l][:, None] if self.mutant == "post_omega" else w
        return xp + wp * (b - L @ xp)

    def has_post_smoothing(self):
        return len(self.L) > (2 if self.additive else 1)

    def has_short_aggregate(self):
        return any(len(self.L[l]) % a for l, a in enumerate(self.agg))

    def precondition(self, r):
        if len(self.L) == 1:
            return self.idg[0][:, None] * r
        if not self.additive:
            return self.cycle(0, r)
        y1 = self.cycle(1, self.restrict(0, r))
        return (self.omega * self.idg[0])[:, None] * r + self.kc * y1[self.member[0]]

    def matrix(self):
        """M^-1: the preconditioner applied to every unit vector."""
        return self.precondition(np.eye(self.nu, dtype=self.dtype))

    # -- the iteration
    def pcg(self, k=None, rtol=None, maxit=2000):
        """(iterates x_1 ... , relres per iterate): k iterations, or until every column's ||r|| <= rtol ||b||."""
        dt, L = self.dtype, self.L[0]
        x, r = np.zeros_like(self.b), self.b.copy()
        p = np.zeros_like(r)
        bb = (r * r).sum(0)
        rz = [np.zeros(3, dtype=dt), np.zeros(3, dtype=dt)]      # the two parity slots
        X, res = [], []
        it = 0
        while it < (k if k is not None else maxit):
            par = it & 1
            if self.mutant == "parity" and it >= 1:
                par ^= 1
            z = self.precondition(r)
            rzn = (r * z).sum(0)
            if self.mutant == "bottom_rz" and self.additive and len(self.L) == 2 and not self.dense:
                rzn = (r * (self.omega * self.idg[0])[:, None] * r).sum(0)     # r.z without the coarse part kc b1.y1
            rzo = rz[par]
            ok = (rzo > 0) & (it > 0) & (self.mutant != "beta_zero")
            beta = np.where(ok, rzn / np.where(ok, rzo, dt(1)), dt(0))
            rz[par ^ 1] = rzn
            p = z + beta * p
            q = L @ p
            pq = (p * q).sum(0)
            alpha = np.where(pq > 0, rz[par ^ 1] / np.where(pq > 0, pq, dt(1)), dt(0))
            x = x + alpha * p
            r = r - alpha * q
            it += 1
            X.append(x.copy())
            res.append(np.sqrt(np.where(bb > 0, (r * r).sum(0) / np.where(bb > 0, bb, dt(1)), dt(0))))
            if rtol is not None and np.all(res[-1] <= rtol):
                break
        return X, res


@functools.lru_cache(maxsize=4)
def _reference_pair(name, levels, kc_x1000, additive):
    case = CASE[name]
    kw = dict(levels=list(levels), kc=kc_x1000 / 1000.0, additive=additive)
    r64, rld = Reference(case, np.float64, **kw), Reference(case, LD, **kw)
    X64, _ = r64.pcg(3)
    Xld, res = rld.pcg(3)
    scale = [float(np.abs(x).max()) for x in Xld]
    e_ref = [float(np.abs(np.asarray(a, dtype=LD) - b).max()) / s for a, b, s in zip(X64, Xld, scale)]
    return dict(r64=r64, rld=rld, X64=X64, Xld=Xld, res=res, scale=scale, e_ref=e_ref)


def reference_pair(case, levels=None, kc=None, additive=None):
    """The fp64 and the long-double reference of a case and their first three iterates (computed once per case)."""
    levels = tuple(case["levels"] if levels is None else levels)
    kc = case["kc"] if kc is None else kc
    return _reference_pair(case["name"], levels, int(round(kc * 1000)), case["additive"] if additive is None else additive)


def ratio(case, pair, k, X):
    """The comparison of the module docstring for an iterate X claimed to be x_k."""
    err = float(np.abs(np.asarray(X, dtype=LD) - pair["Xld"][k - 1]).max()) / pair["scale"][k - 1]
    return err / max(pair["e_ref"][k - 1], case["nu"] * EPS)
