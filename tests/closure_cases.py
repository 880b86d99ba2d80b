"""Cases and references for ONE linear solve of the banded direct solver WITH LOOP CLOSURES (irotavg_amd/csrc/bcr.hip,
bcr_solve_t: the Sherman-Morrison-Woodbury correction around the block cyclic reduction), shared by the CPU test of the
references themselves (test_closure_cases_cpu.py) and the GPU test (test_gpu_closure_solve.py). The closure-free half of the
solver is band_cases.py's; this module reuses its graphs, its restatement of the reduction, its measure and its bar. A plain
module: building a case and its references needs no device.

A case is a band_cases.make_case sequence (band edges of span <= bw, the span-1 edge always, three dropped edges onto fixed
views) plus an explicit list of EXTRA edges, given as operator rows (i, j) (view = row + f) with explicit or drawn weights;
their measurements are drawn from the same ground truth, with the same noise, as make_case draws the band's. The module
classifies the extra edges by the solver's rule (bcr_plan): with B = block_size(widest span <= 32),

    closure  <=>  |i - j| > 32  and  |i // B - j // B| >= 2;

an extra edge of more than 32 views between NEIGHBOURING blocks (block sizes 20 ... 32, spans 33 ... 2 B - 1) is a WIDE
IN-BAND edge: it stays in the block tridiagonal operator. With closures the handle has no sixteen-block top, no
single-launch upper levels and no fused level-0 assembly: the expected level shape is expected_levels(nu, B, no_top16=True).

Operator. L = A_b + V C V' and b, exactly what pcg_cases.operator builds from the whole edge list; A_b is BUILT from the
edges that are not closures (never formed as L minus the closures: the subtraction leaves rounding residue), column q of
V = e_j - e_i for closure q = (i, j), C = diag(w_q^2) over the closures of weight > 0 (a closure of weight exactly zero
is dead: cl_alive).

References of a case (references()):
* x_ld    -- long double. Up to DENSE_MAX rows: dense_cases.chol_solve_ld on the dense L. Above: the Woodbury formula in long
             double (band_cases.band_chol on A_b with [b | V], a dense long-double solve of S), refined against the FULL
             operator until the correction is below 2^-60 max|x| -- at most three steps, asserted (two measured). The
             refinement's residual is formed at twice the precision (residual_twofold: error-free transformations); on a
             residual in plain long double the correction stalls at eps cond |x|, above that limit. The CPU test holds
             the solve to chol_solve_ld on small cases and the residual to exact rational arithmetic;
* x_lu64  -- numpy.linalg.solve on the dense float64 L (up to DENSE64 rows), LAPACK banded + the formula above;
* x_wb64  -- the Woodbury formula in float64 as bcr.hip's comment states it: Y = A_b^-1 b and Z = A_b^-1 V, BOTH from
             band_cases.bcr_solve64 at the handle's level shape, S = C^-1 + V' Z, lambda = S^-1 V' Y, x = Y - Z lambda.
             (Y and Z must come from ONE factorisation, as they do on the device: Y is up to 300 x the solution on these
             sequences -- the band part is anchored at its first views only -- and the errors of two different
             factorisations do not cancel in Y - Z lambda. With Z from LAPACK's banded Cholesky instead, e_wb64 measured
             2e-10 on `spread`, 5e-10 on `mixed-b8` and 4e-7 on `cancel` where this form gives 4e-12, 3e-12 and 2e-9: a
             bar up to 150 x looser, owed to the reference alone.)

    e_ref    = max( max|x_lu64 - x_ld| , max|x_wb64 - x_ld| ) / max|x_ld|
    ratio(X) = ( max|X - x_ld| / max|x_ld| ) / max( e_ref , nu 2^-52 )                    bar: band_cases.BAR = 16

`mutant=` names a defect applied to x_wb64 alone (MUTANTS; test_closure_cases_cpu.py: what the bar can see).
"""
import functools

import numpy as np

import band_cases as BC
import pcg_cases as PC
from band_cases import BAR, EPS, LD, ratio  # noqa: F401  (the measure and the bar are band_cases')
from dense_cases import chol_solve_ld
from irotavg_amd import synth

DENSE_MAX = BC.DENSE_MAX     # rows up to which the long-double reference is one dense Cholesky
DENSE64 = 2100               # rows up to which the float64 LU reference is dense
FAR_MAX = 1024               # bcr_plan_block: closures a graph of fewer than 8192 free views keeps (kBcrMaxFar / 2)

MUTANTS = ("lambda_sign", "cinv_dropped", "dead_as_unit", "endpoint_off_by_one", "dup_once", "wide_dropped", "wide_as_far_only")


# ---- graphs ---------------------------------------------------------------------------------------------------------
def classify(rows, B):
    """The solver's rule on extra edges given as rows: a boolean per edge, True = closure."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    return (np.abs(rows[:, 0] - rows[:, 1]) > 32) & (np.abs(rows[:, 0] // B - rows[:, 1] // B) >= 2)


def make_case(name, route, nu, f, bw, fam, extra, wx=None, *, closures, weak=None, weak_w=None, anchor_late=False, env=None,
              system=None, seed=0):
    """band_cases.make_case(nu, f, bw, fam) + the extra edges `extra` (rows) of weights `wx` (None: drawn from the family).
    closures: how many of them the case EXPECTS to be closures (the CPU test holds it to classify()). weak / weak_w:
    band_cases' weak link with the link's weight set to weak_w. anchor_late: every edge from a fixed view into the first free
    view removed, (f, 0) -- which make_A drops -- and (f - 1, f + 1) added. env / system: as in band_cases."""
    base = BC.make_case(name, route, nu, f, bw, fam, weak=weak, seed=seed)
    rng = np.random.default_rng([109, nu, f, bw, seed])
    I, w, QQ, Qgt = base["I"], base["w"].copy(), base["QQ"], base["Qgt"]
    if weak_w is not None:
        w[(I[:, 0] == f + weak - 1) & (I[:, 1] == f + weak)] = weak_w
    extra = np.asarray(extra, dtype=np.int64).reshape(-1, 2)
    assert extra.min(initial=0) >= 0 and extra.max(initial=0) < nu and np.all(np.abs(extra[:, 0] - extra[:, 1]) > 32)
    new = extra + f
    draw = len(new)
    if anchor_late:
        keep = ~((I[:, 0] < f) & (I[:, 1] == f))
        I, w, QQ = I[keep], w[keep], QQ[keep]
        new = np.concatenate([[[f, 0], [f - 1, f + 1]], new])
    wn = 10.0 ** rng.uniform(-3.0, 3.0, size=len(new)) if fam == "s" else rng.uniform(0.1, 5.0, size=len(new))
    if wx is not None:
        wn[len(new) - draw:] = wx
    QQn = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(len(new), 3))),
                     synth.qmul(Qgt[new[:, 1]], synth.qconj(Qgt[new[:, 0]])))
    ext0 = len(I) + len(new) - draw                            # the edge id of the first extra edge
    I = np.concatenate([I, new]).astype(np.int32)
    w, QQ = np.concatenate([w, wn]), np.concatenate([QQ, QQn])
    B = base["B"]
    far = classify(extra, B)
    assert np.all(np.abs(extra[~far, 0] // B - extra[~far, 1] // B) == 1)      # a wide in-band edge: neighbouring blocks
    ncl = int(far.sum())
    direct = len(extra) <= FAR_MAX                             # (the plan's first scan counts every span > 32)
    env = dict(env or {})
    if ncl:
        levels, top16 = BC.expected_levels(nu, B, no_top16=True)
    else:
        levels, top16 = base["levels"], base["top16"]
    ij = I.astype(np.int64) - f
    free = (ij[:ext0, 0] >= 0) & (ij[:ext0, 1] >= 0)
    bwb = int(max(np.abs(ij[:ext0, 0] - ij[:ext0, 1])[free].max(), np.abs(extra[~far, 0] - extra[~far, 1]).max(initial=0)))
    return dict(name=name, route=route, nu=nu, n=nu + f, f=f, bw=base["bw"], bwb=bwb, I=I, QQ=QQ, Q0=base["Q0"], w=w, fam=fam,
                env=env, system=system or name, B=B, levels=levels, top16=top16, extra=extra, far=far, ext0=ext0,
                closures=closures, direct=direct, fused=1 if ncl == 0 and B % 8 == 0 else 0, anchor_late=anchor_late)


def random_closures(rng, nu, B, r, taken=()):
    """r closures at distinct pairs of rows (distinct from `taken` too), every second one listed reversed at random."""
    gap = max(33, 2 * B)
    seen, out = {frozenset(t) for t in taken}, []
    while len(out) < r:
        i = int(rng.integers(0, nu - gap))
        j = int(rng.integers(i + gap, nu))
        if frozenset((i, j)) in seen:
            continue
        seen.add(frozenset((i, j)))
        out.append((j, i) if rng.random() < 0.5 else (i, j))
    return out


def placed_up(B, nb0):
    """The six placed closures of an `up` case of nb0 blocks (chunks of eight blocks; the last block holds B - 3 rows)."""
    nu = nb0 * B - 3
    return [(16 * B + 1, 21 * B + 2),            # both endpoints in chunk 2
            (32 * B + 3, 26 * B + 1),            # block 0 of chunk 4 (spills into the separator before it) and chunk 3
            (2 * B + 1, 30 * B + 5),             # an endpoint in chunk 0: no separator before it
            (23 * B + 3, 40 * B),                # an endpoint in block 7 of chunk 2
            (5 * B + 4, (nb0 - 1) * B + 2),      # an endpoint in the last chunk: one real block
            (0, nu - 1)]


def _cases():
    C = []

    def add(name, route, nu, bw, fam, extra, wx=None, **k):
        k.setdefault("closures", len(extra))
        C.append(make_case(name, route, nu, (1, 3)[len(C) % 2], bw, fam, extra, wx, **k))

    def rng_of(*key):
        return np.random.default_rng([111] + list(key))
    # 1. level shapes and endpoint positions
    add("one-b8", "shape", 64, 8, "u", [(3, 44), (60, 10), (0, 63)])
    add("one-b8-61", "shape", 61, 8, "u", [(60, 5), (3, 44), (20, 58)])
    for B in (8, 16, 24, 32):
        nu = 9 * B - 3
        placed = [(8 * B + 1, 2 * B), (7 * B + 2, B + 1), (3, 5 * B + 3), (0, nu - 1)]
        add("two-b%d-nb9" % B, "shape", nu, B, "u", placed + random_closures(rng_of(1, B), nu, B, 3, placed))
    for B in (8, 12, 16, 20, 24, 28, 32):
        nb0 = 129 if B == 8 else 65
        nu, placed = nb0 * B - 3, placed_up(B, nb0)
        add("up-b%d-nb%d" % (B, nb0), "shape", nu, B, "u", random_closures(rng_of(2, B), nu, B, 24, placed) + placed)
    nu = 512 * 64 + 13 * 8 - 3
    add("mixed-b8", "mixed", nu, 8, "u", [(32768, 32808), (32790, 32850), (32800, 20000), (32720, 17), (0, nu - 1),
                                         (32868, 32700)])
    # 2. closure counts at every switch of kernel: one list of distinct pairs, its first r
    nu = 1029
    rng = rng_of(3)
    pairs, wp = random_closures(rng, nu, 8, 1025), rng.uniform(0.1, 5.0, size=1025)
    for r in (8, 96, 97, 192, 193, 400, 401, 1024, 1025):
        add("count-r%d" % r, "count", nu, 8, "u", pairs[:r], wp[:r])
    nu = 35 * 32 - 3
    rng = rng_of(4)
    pairs32, wp32 = random_closures(rng, nu, 32, 257), rng.uniform(0.1, 5.0, size=257)
    for r in (256, 257):
        add("count-b32-r%d" % r, "count", nu, 32, "u", pairs32[:r], wp32[:r])
    # 3. the switch: the tile kernel at every closure count
    by = {c["name"]: c for c in C}
    for base in ("count-r8", "up-b8-nb129", "count-r96"):
        b = by[base]
        C.append(make_case("tiles-" + base, "switch", b["nu"], b["f"], 8, "u", b["extra"], b["w"][b["ext0"]:],
                           closures=b["closures"], env={"IROTAVG_BCR_S_TILES": "1"}, system=base))
    # 4. weights and multiplicity (the geometry of up-b8-nb129)
    nu = 1029
    rng = rng_of(5)
    live = random_closures(rng, nu, 8, 11)
    wl = rng.uniform(0.1, 5.0, size=12)
    wl[[2, 5, 9, 11]] = 0.0                                    # four dead closures; the last one duplicates the live pair 0
    add("dead", "weights", nu, 8, "u", live + [live[0][::-1]], wl)
    others = random_closures(rng, nu, 8, 5, [(200, 700)])
    add("dup", "weights", nu, 8, "u", [(200, 700)] + others[:2] + [(700, 200)] + others[2:] + [(200, 700)],
        [1.5, 1.0, 2.0, 0.7, 3.0, 0.5, 1.2, 2.5])
    hub = 517
    spokes = [int(v) for v in rng.permutation(np.r_[0:hub - 40, hub + 40:nu])[:16]]
    add("star", "weights", nu, 8, "u", [(hub, v) if k % 2 else (v, hub) for k, v in enumerate(spokes)])
    add("spread", "weights", nu, 8, "s", random_closures(rng, nu, 8, 30))
    nu = 65 * 24 - 3
    placed = placed_up(24, 65)
    add("b24-s", "weights", nu, 24, "s", random_closures(rng, nu, 24, 24, placed) + placed)
    # 5. cancellation: the band part alone hangs on a weak link, two closures hold the halves together
    add("cancel", "cancel", 1025, 8, "u", [(100, 900), (590, 640)], [1.0, 2.0], weak=600, weak_w=1e-3)
    # 6. wide in-band edges
    add("wide-b32", "wide", 541, 32, "u", [(40, 90), (100, 150), (33, 95)], closures=0)
    add("wide-b32-cl", "wide", 541, 32, "u", [(40, 90), (100, 150), (33, 95), (10, 120)], closures=1)
    add("wide-b24-cl", "wide", 405, 24, "u", [(30, 70), (100, 140), (10, 120)], closures=1)
    # the device plan's anchoring rule: the first free view is tied through LATER views only
    b = {c["name"]: c for c in C}["up-b8-nb129"]
    C.append(make_case("anchor-late", "anchor", b["nu"], b["f"], 8, "u", b["extra"], closures=30, anchor_late=True))
    return C


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)
SOLVED = [c["name"] for c in CASES if c["direct"]]            # (count-r1025 is left to the iterative solver: no references)


# ---- the operator ---------------------------------------------------------------------------------------------------
def closure_rows(case, dtype=np.float64):
    """(edge ids, i, j, w^2 formed in `dtype`) of the case's closures, in edge order."""
    e = case["ext0"] + np.nonzero(case["far"])[0]
    ij = case["I"][e].astype(np.int64) - case["f"]
    return e, ij[:, 0], ij[:, 1], np.asarray(case["w"][e], dtype=dtype) ** 2


def incidence(nu, ci, cj, dtype):
    V = np.zeros((nu, len(ci)), dtype=dtype)
    q = np.arange(len(ci))
    np.add.at(V, (cj, q), 1)
    np.add.at(V, (ci, q), -1)
    return V


def band_part(case):
    """The case without its closures: what A_b is built from."""
    keep = np.ones(len(case["I"]), dtype=bool)
    keep[closure_rows(case)[0]] = False
    return dict(case, I=case["I"][keep], QQ=case["QQ"][keep], w=case["w"][keep], bw=case["bwb"])


@functools.lru_cache(maxsize=2)
def _parts(system, ld):
    """(S_b in band storage, b, the dense L or None) accumulated in the dtype from the fp64 weights and residuals."""
    case, dtype = CASE[system], (LD if ld else np.float64)
    nu, bwb = case["nu"], case["bwb"]
    band = band_part(case)
    if nu <= (DENSE_MAX if ld else DENSE64):
        Lb = PC.operator(band, dtype)[0]
        assert not np.any(np.triu(Lb, bwb + 1))
        L, b, _, _ = PC.operator(case, dtype)
        return BC.band_from_dense(Lb, bwb), b, L
    S, b = BC.band_operator(band, dtype)
    e, ci, cj, w2 = closure_rows(case, dtype)
    t = w2[:, None] * np.asarray(PC.residuals(case)[e], dtype=dtype)
    b = b.copy()
    np.add.at(b, cj, t)
    np.add.at(b, ci, -t)
    return S, b, None


def parts(case, dtype):
    return _parts(case["system"], dtype is LD)


def full_matvec(case, X):
    """L X in long double, L the FULL operator."""
    S, _, L = parts(case, LD)
    X = np.asarray(X, dtype=LD)
    if L is not None:
        return L @ X
    _, ci, cj, w2 = closure_rows(case, LD)
    V = incidence(case["nu"], ci, cj, LD)
    return BC.band_matvec(S, X) + V @ (w2[:, None] * (V.T @ X))


def residual_ld(case, X):
    """max over the three columns of ||b - L X|| / ||b||, formed in long double."""
    b = parts(case, LD)[1]
    with np.errstate(all="ignore"):
        r = b - full_matvec(case, X)
        return float(np.sqrt((r * r).sum(0) / (b * b).sum(0)).max())


# ---- the Woodbury formula -------------------------------------------------------------------------------------------
def _formula(Y, Z, V, w2, mutant=None):
    S = V.T @ Z
    if mutant != "cinv_dropped":
        S = S + np.diag(1 / w2)
    lam = np.linalg.solve(S, V.T @ Y) if S.dtype == np.float64 else chol_solve_ld(S, V.T @ Y)
    return Y + Z @ lam if mutant == "lambda_sign" else Y - Z @ lam


_SPLIT = LD(2.0 ** 32 + 1)         # Dekker's splitter for a 64-bit significand


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _two_prod(a, b):
    def split(v):
        t = _SPLIT * v
        h = t - (t - v)
        return h, v - h
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def residual_twofold(case, x):
    """b - L x of the long-double FULL operator (band storage + closures) with every product and sum carried as an unevaluated
    pair (error-free transformations): as if formed at twice the precision. A residual formed in plain long double stalls
    the refinement at eps cond |x| -- 6e-18 at 1300 rows, 1e-15 at 32869."""
    S, b, _ = parts(case, LD)
    nu, bw = len(S), S.shape[1] // 2
    Xp = np.zeros((nu + 2 * bw, 3), dtype=LD)
    Xp[bw:bw + nu] = x
    s, c = b.copy(), np.zeros_like(b)
    for d in range(2 * bw + 1):
        p, e = _two_prod(-S[:, d, None], Xp[d:d + nu])
        s, q = _two_sum(s, p)
        c += q + e
    for i, j, wq in zip(*closure_rows(case, LD)[1:]):
        h, l = _two_sum(x[j], -x[i])
        p, e = _two_prod(wq, h)
        lo = e + wq * l
        s[j], q = _two_sum(s[j], -p)
        c[j] += q - lo
        s[i], q = _two_sum(s[i], p)
        c[i] += q + lo
    return s + c


def woodbury_ld(case):
    """(x, refinement steps): the formula in long double, refined against the full operator."""
    S, b, _ = parts(case, LD)
    _, ci, cj, w2 = closure_rows(case, LD)
    al = w2 > 0
    V, w2 = incidence(case["nu"], ci[al], cj[al], LD), w2[al]
    solve = BC.band_chol(S)
    Z = solve(V)

    def apply(R):
        return _formula(solve(R), Z, V, w2)
    x, steps = apply(b), 0
    while True:
        d = apply(residual_twofold(case, x))
        x, steps = x + d, steps + 1
        if np.abs(d).max() < 2.0 ** -60 * np.abs(x).max():
            return x, steps
        assert steps < 3, "the long-double Woodbury reference did not settle in three refinement steps"


def woodbury64(case, B=None, levels=None, top16=None, mutant=None, info=None):
    """x_wb64 of the module docstring at a level shape (default: the one the case is named for), with a mutant."""
    assert mutant is None or mutant in MUTANTS
    S, b, _ = parts(case, np.float64)
    nu, bwb = case["nu"], case["bwb"]
    _, ci, cj, w2 = closure_rows(case)
    if mutant in ("wide_dropped", "wide_as_far_only"):
        # the first wide in-band edge: its two off-diagonal entries missing from A_b (an assembly window that cuts it), or
        # the whole edge taken out of A_b as a closure's would be -- and never re-entered
        k = int(np.nonzero(~case["far"])[0][0])
        i, j = (int(v) for v in case["extra"][k])
        wk = case["w"][case["ext0"] + k] ** 2
        S = S.copy()
        S[i, bwb + j - i] += wk
        S[j, bwb + i - j] += wk
        if mutant == "wide_as_far_only":
            S[i, bwb] -= wk
            S[j, bwb] -= wk
    if mutant == "dead_as_unit":
        w2 = np.where(w2 > 0, w2, 1.0)
    if mutant == "endpoint_off_by_one" and len(ci):
        ci = ci.copy()
        ci[0] += 1 if ci[0] + 1 < nu else -1
    if mutant == "dup_once":
        key = [frozenset((int(a), int(c))) for a, c in zip(ci, cj)]
        first = np.array([key.index(k) == q for q, k in enumerate(key)], dtype=bool)
        ci, cj, w2 = ci[first], cj[first], w2[first]
    al = w2 > 0
    ci, cj, w2 = ci[al], cj[al], w2[al]
    shape = (case["B"] if B is None else B, case["levels"] if levels is None else levels,
             case["top16"] if top16 is None else top16)
    Y = BC.bcr_solve64(S, b, *shape, info=info)
    if not len(ci):
        return Y
    V = incidence(nu, ci, cj, np.float64)
    Vp = np.concatenate([V, np.zeros((nu, -len(ci) % 3))], 1)                 # (bcr_solve64 takes three columns at a time)
    Z = np.concatenate([BC.bcr_solve64(S, Vp[:, k:k + 3], *shape) for k in range(0, Vp.shape[1], 3)], 1)[:, :len(ci)]
    return _formula(Y, Z, V, w2, mutant)


def lu64(case):
    from scipy.linalg import solveh_banded
    S, b, L = parts(case, np.float64)
    if L is not None:
        return np.linalg.solve(L, b)
    _, ci, cj, w2 = closure_rows(case)
    al = w2 > 0
    V = incidence(case["nu"], ci[al], cj[al], np.float64)
    YZ = solveh_banded(np.ascontiguousarray(S[:, case["bwb"]:].T), np.concatenate([b, V], 1), lower=True)
    return _formula(YZ[:, :3], YZ[:, 3:], V, w2[al])


# ---- references -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _references(system, B, levels, top16):
    case = CASE[system]
    nu = case["nu"]
    info = {}
    x_wb = woodbury64(case, B, levels, top16, info=info)
    x_lu = lu64(case)
    _, bld, Lld = parts(case, LD)
    steps = 0
    if Lld is not None:
        x_ld = chol_solve_ld(Lld, bld)
    else:
        x_ld, steps = woodbury_ld(case)
    scale = float(np.abs(x_ld).max())
    e_lu = float(np.abs(x_lu - x_ld).max()) / scale
    e_wb = float(np.abs(x_wb - x_ld).max()) / scale
    return dict(x_ld=x_ld, x_lu64=x_lu, x_wb64=x_wb, scale=scale, e_lu=e_lu, e_wb=e_wb, e_ref=max(e_lu, e_wb), floor=nu * EPS,
                ndead=info["dead"], steps=steps, res_lu64=residual_ld(case, x_lu), res_wb64=residual_ld(case, x_wb))


def references(case, block=None, levels=None, top16=None):
    """The three references of a case (computed once per system and level shape); block / levels / top16: what the handle
    reports (default: what the case is named for)."""
    assert case["direct"]
    levels = case["levels"] if levels is None else levels
    return _references(case["system"], case["B"] if block is None else block, tuple(tuple(int(v) for v in lv) for lv in levels),
                       case["top16"] if top16 is None else top16)
