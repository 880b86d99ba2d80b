"""Cases and a NumPy reference for the first PCG iterates of a solve on a RE-USED or REPAIRED coarse inverse
(irotavg_amd/csrc/dense.hip: dense_is_stale, dense_lowrank_repair; read by the dense apply and by k_cg_apply of cgcg.hip),
shared by test_stale_cases_cpu.py and test_gpu_stale_inverse.py. A plain module on top of pcg_cases: no device needed.

What the handle does. When the weights of a handle move between two solves, assemble() asks dense_is_stale() what the
last level of the multigrid cycle multiplies by from now on. With E_ref the coarse operator the explicit inverse belongs
to and E_now the one just assembled (`stale_step` restates the rules from the code):

* lo, hi = min, max of now / ref over the diagonal and every off-diagonal entry that is non-zero in both; an entry that is
  non-zero in only one of them (or a ratio <= 0) makes hi = inf.
* "scale": hi <= 1.1 lo. The inverse is kept and multiplied by dense_scale = 1 / sqrt(lo hi). E_ref stays.
* otherwise lod, hid over the diagonal alone, c = sqrt(lod hid). If hid <= 1.1 lod and fewer than twelve repairs were
  made since the last inversion, the off-diagonal entries with q = now / (c ref) outside [1 / 1.1, 1.1] are collected,
  each pair once (column > row), delta = now - c ref, sorted by (row, column). A structural change, a q outside
  (1e-4, 1e4), no pair or more than 64 pairs: "invert". Else "repair": with Z = rows i_k - j_k of the inverse,
  S = c G^-1 + V'Z (G = diag(-delta)), W = S^-1 Z the inverse becomes (Minv - Z'W) / c, dense_scale = 1, and E_ref becomes
  c E_ref with the deviating entries replaced by E_now's and c diag_i - delta, c diag_j - delta for every listed pair.
* "invert": everything else. E_ref = E_now, dense_scale = 1.

The chained reference (`run_chain`). Given a case and weight vectors w_0, w_1, ... it follows the verdicts from solve to
solve and produces the last-level matrix of every solve twice:
* exact (long double): the exact inverse of "the operator the inverse belongs to" times the scale -- what a repair is
  meant to compute;
* formula (float64): numpy.linalg.inv at an inversion, then the update formula above applied to that matrix from repair
  to repair, as the device does. Its cancellation (Minv - Z'W) is part of e_ref, the yardstick.
Both inverses are pcg_cases.spd_inverse, as in the reference of a fresh handle. e_ref depends on the host's LAPACK (a
factor two between machines at 769 rows); test_stale_cases_cpu.py holds it below BAR x nu 2^-52 wherever it runs.
The iterates are those of pcg_cases.Reference.pcg with Reference.S replaced by that matrix.

    ratio = (max|X - x_k^ld| / max|x_k^ld|) / max(e_ref(k), nu 2^-52)          bar: pcg_cases.BAR = 16

Which iterate the handle returns (`stopping`). A solve on a non-fresh handle cannot be cut at k iterations with
pcg_max_iters: ERR_NOT_CONVERGED on a re-used inverse makes ls_solve re-invert and solve again. It is cut by the
tolerance instead: pcg_check ends the solve at the first iterate whose three column residuals are all <= pcg_rtol ||b||.
With rho_j the largest column residual of the long-double iterate j (rho_0 = 1), pcg_rtol = sqrt(rho_k min_{j<k} rho_j)
stops at k when both lie a factor MARGIN = 1.25 from it; a (case, solve, k) where they do not is not used.

`mutant=` names a defect applied to the float64 formula chain alone (test_stale_cases_cpu.py: what the bar can see).
"""
import functools

import numpy as np

import pcg_cases as PC
from irotavg_amd import synth

LD = PC.LD
EPS = PC.EPS
BAR = PC.BAR
SPREAD = 1.1            # graph.hpp: stale_spread
WB_MAX = 64             # dense.hip: kWbMax
WB_REPAIRS_MAX = 12     # dense.hip: kWbRepairsMax
Q_MIN, Q_MAX = 1e-4, 1e4
MARGIN = 1.25
W_CLOSURE = 0.05

MUTANTS = ("no_repair", "delta_sign", "c_all", "ref_kept", "inband_now", "scale_lo", "both_triangles", "slice0")


# ---- dense_is_stale / dense_lowrank_repair, on dense operators ----------------------------------------------------------
def stale_step(E_ref, E_now, repairs_in_a_row, mutant=None):
    """dict(verdict, factor, pairs, E_after): verdict "scale" / "repair" / "invert"; factor = the scale, c, or 1;
    pairs = the sorted list (i, j, delta) of a repair; E_after = the operator the inverse belongs to afterwards."""
    assert mutant is None or mutant in MUTANTS
    dt = E_now.dtype.type
    n = len(E_now)
    dr, dn = np.diag(E_ref).copy(), np.diag(E_now).copy()
    assert (dr > 0).all() and (dn > 0).all()                   # (no case of this module has a dead row)
    off = ~np.eye(n, dtype=bool)
    both = off & (E_ref != 0) & (E_now != 0)
    structural = bool((off & ((E_ref != 0) != (E_now != 0))).any())
    invert = dict(verdict="invert", factor=dt(1), pairs=[], E_after=E_now.copy())
    qd = dn / dr
    qo = E_now[both] / E_ref[both]
    qa = np.concatenate([qd, qo])
    lo = qa[qa > 0].min()
    hi = dt(np.inf) if structural or (qa <= 0).any() else qa.max()
    if hi <= dt(SPREAD) * lo:
        scale = dt(1) / lo if mutant == "scale_lo" else dt(1) / np.sqrt(lo * hi)
        return dict(verdict="scale", factor=scale, pairs=[], E_after=E_ref.copy())
    lod, hid = qd.min(), qd.max()
    if not (hid <= dt(SPREAD) * lod and both.any() and repairs_in_a_row < WB_REPAIRS_MAX):
        return invert
    c = np.sqrt(lod * hid)
    if mutant == "c_all" and np.isfinite(hi):
        c = np.sqrt(lo * hi)
    if structural:
        return invert
    band = dt(SPREAD)
    rows, cols = np.nonzero(both)
    q = E_now[rows, cols] / (c * E_ref[rows, cols])
    dev = ~((q <= band) & (q * band >= 1))
    if (dev & ~((q < Q_MAX) & (q > Q_MIN))).any():
        return invert
    rows, cols = rows[dev], cols[dev]
    delta = E_now[rows, cols] - c * E_ref[rows, cols]
    if mutant == "slice0":                                     # sell_row_of without the walk over the slices
        rows = rows % 64
    if mutant == "both_triangles":
        listed = [(min(i, j), max(i, j), d) for i, j, d in zip(rows, cols, delta)]
    else:
        listed = [(i, j, d) for i, j, d in zip(rows, cols, delta) if j > i]
    pairs = sorted(((int(i), int(j), d) for i, j, d in listed), key=lambda p: p[:2])
    if not 0 < len(pairs) <= WB_MAX or any(not (d != 0) or not np.isfinite(d) for _, _, d in pairs):
        return invert
    E_after = c * E_ref
    dmask = np.zeros((n, n), dtype=bool)
    r0, c0 = np.nonzero(both)
    dmask[r0[dev], c0[dev]] = True
    E_after[dmask] = E_now[dmask]
    da = c * dr
    for i, j, d in pairs:                                      # k_wb_ref_diag: sequential over the sorted list
        da[i] -= d
        da[j] -= d
    E_after[np.arange(n), np.arange(n)] = da
    return dict(verdict="repair", factor=c, pairs=pairs, E_after=E_after)


def woodbury(Minv, c, pairs, flip=False):
    """(Minv - Z' S^-1 Z) / c as k_wb_z, k_wb_s, the host's LU, k_wb_w and k_wb_apply form it."""
    i = np.array([p[0] for p in pairs])
    j = np.array([p[1] for p in pairs])
    d = np.array([p[2] for p in pairs], dtype=Minv.dtype)
    Z = Minv[i] - Minv[j]
    S = (Z[:, i] - Z[:, j]).T.copy()
    S[np.arange(len(i)), np.arange(len(i))] += c / (d if flip else -d)
    W = np.linalg.inv(np.asarray(S, dtype=np.float64)).astype(Minv.dtype) @ Z
    return (Minv - Z.T @ W) * (Minv.dtype.type(1) / c)


def run_chain(sc, dtype, exact, hier=None, mutant=None, solves=None):
    """Follows the verdicts over sc["weights"]. A list, per solve, of dict(verdict, factor, pairs, inversions, repairs,
    X, res): X / res the first three iterates and their column residuals, for the solves in `solves` (default: the
    case's tested ones), None elsewhere. exact: the last level is the exact inverse of the operator the inverse belongs
    to; else the update formula chained from solve to solve (and `mutant` applied)."""
    assert not (exact and mutant)
    case = sc["case"]
    solves = sc["tested"] if solves is None else solves
    out = []
    E_ref = Minv = None
    scale, in_row, inversions, repairs = dtype(1), 0, 0, 0
    for t, w in enumerate(sc["weights"]):
        R = PC.Reference(dict(case, w=w, dense=False), dtype, **(hier or {}))
        R.dense = True
        E = R.L[-1]
        step = stale_step(E_ref, E, in_row, mutant) if t else dict(verdict="invert", factor=dtype(1), pairs=[], E_after=E)
        v = step["verdict"]
        if v == "repair" and mutant == "inband_now":
            E_ref, Minv, scale, in_row, repairs = E.copy(), PC.spd_inverse(E, dtype), dtype(1), in_row + 1, repairs + 1
        elif v == "repair" and mutant == "no_repair":
            scale, repairs = dtype(1) / step["factor"], repairs + 1
        elif v == "repair":
            if not exact:
                Minv = woodbury(Minv, step["factor"], step["pairs"], flip=mutant == "delta_sign")
            else:
                Minv = None
            if mutant != "ref_kept":
                E_ref = step["E_after"]
            scale, in_row, repairs = dtype(1), in_row + 1, repairs + 1
        elif v == "scale":
            scale = step["factor"]
        else:
            E_ref, scale, in_row, inversions = E.copy(), dtype(1), 0, inversions + 1
            Minv = None if exact else PC.spd_inverse(E, dtype)
        X = res = None
        if t in solves:
            if exact and Minv is None:
                Minv = PC.spd_inverse(E_ref, dtype)
            R.S = Minv * scale
            X, res = R.pcg(3)
        out.append(dict(verdict=v, factor=step["factor"], pairs=[(i, j) for i, j, _ in step["pairs"]],
                        inversions=inversions, repairs=repairs, X=X, res=res))
    return out


def stopping(res, k):
    """(pcg_rtol, holds): the tolerance that ends the solve at iterate k, and whether both residuals clear MARGIN."""
    rho = [1.0] + [float(np.max(r)) for r in res]
    prev, cur = min(rho[:k]), rho[k]
    rtol = float(np.sqrt(prev * cur))
    return rtol, cur * MARGIN <= rtol and rtol * MARGIN <= prev


@functools.lru_cache(maxsize=4)
def _reference(name, levels, kc_x1000, additive):
    sc = CASE[name]
    hier = dict(levels=list(levels), kc=kc_x1000 / 1000.0, additive=additive)
    c64 = run_chain(sc, np.float64, False, hier)
    cld = run_chain(sc, LD, True, hier)
    for a, b in zip(c64, cld):                                 # both precisions follow the same chain
        assert (a["verdict"], a["pairs"], a["inversions"], a["repairs"]) == \
               (b["verdict"], b["pairs"], b["inversions"], b["repairs"]), (name, a["verdict"], b["verdict"])
    ref = dict(chain=cld, chain64=c64, solve={})
    for t in sc["tested"]:
        Xld, X64 = cld[t]["X"], c64[t]["X"]
        scale = [float(np.abs(x).max()) for x in Xld]
        e_ref = [float(np.abs(np.asarray(a, dtype=LD) - b).max()) / s for a, b, s in zip(X64, Xld, scale)]
        stop = [stopping(cld[t]["res"], k) for k in (1, 2, 3)]
        ref["solve"][t] = dict(Xld=Xld, X64=X64, res=cld[t]["res"], scale=scale, e_ref=e_ref, stop=stop)
    return ref


def reference(sc, levels=None, kc=None, additive=None):
    """The two chains of a case and, per tested solve, the iterates, e_ref and the stopping tolerances (computed once)."""
    case = sc["case"]
    levels = tuple(case["levels"] if levels is None else levels)
    kc = case["kc"] if kc is None else kc
    return _reference(sc["name"], levels, int(round(kc * 1000)), case["additive"] if additive is None else additive)


def ratio(sc, ref, t, k, X):
    """The comparison of the module docstring for an iterate X claimed to be x_k of solve t."""
    s = ref["solve"][t]
    err = float(np.abs(np.asarray(X, dtype=LD) - s["Xld"][k - 1]).max()) / s["scale"][k - 1]
    return err / max(s["e_ref"][k - 1], sc["case"]["nu"] * EPS)


# ---- cases --------------------------------------------------------------------------------------------------------------
def with_closures(case, coarse_pairs):
    """The case with one loop closure of weight W_CLOSURE per coarse pair (p, q): between the middle views of the level-0
    aggregates p and q, so the closures own exactly those coarse entries."""
    agg, f, nu = case["aggs"][0], case["f"], case["nu"]
    assert len(set(coarse_pairs)) == len(coarse_pairs) and all(p < q for p, q in coarse_pairs)
    rng = np.random.default_rng([106, nu, len(coarse_pairs)])
    a = np.array([f + min(agg * p + agg // 2, nu - 1) for p, _ in coarse_pairs])
    b = np.array([f + min(agg * q + agg // 2, nu - 1) for _, q in coarse_pairs])
    Q0 = case["Q0"]
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(len(a), 3))), synth.qmul(Q0[b], synth.qconj(Q0[a])))
    out = dict(case)
    out["I"] = np.concatenate([case["I"], np.stack([a, b], 1).astype(np.int32)])
    out["QQ"] = np.concatenate([case["QQ"], QQ])
    out["w"] = np.concatenate([case["w"], np.full(len(a), W_CLOSURE)])
    out.update(far=True, kc=1.6)
    return out


def _weights(case, ncl, steps, seed):
    """w_0 = the case's weights; w_t = s w_0 (1 + jitter u_t), the last ncl (the closures) times g instead of the jitter.
    steps: (s, jitter, g) per solve after the first; g a number, a vector, or None for the closures' jitter-free s."""
    rng = np.random.default_rng([107, len(case["w"]), seed])
    w0 = case["w"]
    W = [w0.copy()]
    for s, jitter, g in steps:
        w = s * w0 * (1 + jitter * rng.uniform(-1, 1, size=len(w0)))
        if ncl:
            w[-ncl:] = s * w0[-ncl:] * (1.0 if g is None else g)
        W.append(w)
    return W


def _stale_case(name, case, weights, verdicts, tested, pairs=0, ks=(1, 2, 3)):
    """tested: the solves whose iterates are pinned; ks: the iterates whose stopping tolerance clears MARGIN."""
    assert len(weights) == len(verdicts) and verdicts[0] == "invert" and len(ks) >= 2
    return dict(name=name, case=dict(case, name=name), weights=weights, verdicts=list(verdicts),
                tested={t: tuple(ks) for t in tested}, pairs=pairs)


def _cases():
    C = []
    mult = dict(mg_multiplicative_top=1)
    small = PC._small

    # -- scale re-use, one case per way the scale is consumed: the exactly uniform step w_1 = 3 w_0, then a near-uniform one
    # (per-edge factors within 1 +- 0.02: the operator's entries within 1.083 < 1.1, lo != hi)
    bases = [("mult2-513", PC.make_case("", "mult", 513, 1, 16, small(80, **mult), [8])),          # 65 coarse rows
             ("mult3-519", PC.CASE["mult3-519"]), ("add2far-1025", PC.CASE["add2far-1025"]),
             ("add2loop-513", PC.CASE["add2loop-513"]), ("l1f-1025", PC.CASE["l1f-1025"]),
             ("cg2-1025", PC.CASE["cg2-1025"]), ("cg2-1537-4lev", PC.CASE["cg2-1537-4lev"])]
    for tag, base in bases:
        W = _weights(base, 0, [(3.0, 0.0, None), (5.1, 0.02, None)], 1)
        # (four levels: the residuals of x_2 and x_3 are 0.106 and 0.084, too close for a tolerance between them)
        ks = (1, 2) if tag == "cg2-1537-4lev" else (1, 2, 3)
        C.append(_stale_case("scale-" + tag, base, W, ["invert", "scale", "scale"], [1, 2], ks=ks))

    # -- repairs. Closures of weight 0.05 among band weights in (0.1, 5), re-weighted by x20 .. x30 (or back) per step while
    # every other weight moves by a common factor times 1 +- 0.01
    def up(r, seed):
        return 20.0 + 10.0 * np.random.default_rng([108, r, seed]).uniform(size=r)

    def repair(name, base, pairs, seed):
        c = with_closures(base, pairs)
        r = len(pairs)
        W = _weights(c, r, [(1.3, 0.01, up(r, seed))], seed)
        C.append(_stale_case(name, c, W, ["invert", "repair" if r <= WB_MAX else "invert"], [1], pairs=r))

    b65 = PC.make_case("", "add2far", 1025, 3, 32, small(80, agg0=16), [16])                       # 65 rows, ndense_pad 128
    b129 = PC.make_case("", "add2far", 1025, 1, 32, small(200), [8])                               # 129 rows
    b193 = PC.make_case("", "add2far", 1537, 3, 32, small(200), [8])                               # 193 rows: four slices
    b769 = PC.make_case("", "default", 1537, 1, 16, dict(band_direct=-1), [2])                     # 769 rows, pad 832
    repair("repair-65-r1", b65, [(10, 50)], 2)
    repair("repair-129-r3-shared-row", b129, [(20, 70), (20, 95), (20, 120)], 3)
    # rows in SELL slices 1 and 2, columns in slices 2 and 3 (row 192 is the short last aggregate)
    repair("repair-193-r17", b193, [(64 + 3 * k, 140 + 3 * k) for k in range(16)] + [(70, 192)], 4)
    repair("repair-193-r64", b193, [(2 * k, 128 + k) for k in range(64)], 5)
    repair("repair-769-r3", b769, [(100, 300), (100, 500), (650, 760)], 6)
    repair("repair-769-r17", b769, [(40 * k + 5, 40 * k + 45 + k) for k in range(17)], 7)

    # a mild step: one closure entry moves by x1.3, one by x0.85 against the common factor, every other weight within
    # 1 +- 0.002. Both deviate from c (the diagonal's factor); a c taken over all entries, sqrt(0.85 x 1.3) = 1.051 c,
    # still leaves every other entry in the band and both closures outside it: the repair survives with the wrong c
    c = with_closures(b129, [(25, 80), (45, 115)])
    W = _weights(c, 2, [(1.3, 0.002, np.sqrt([1.3, 0.85]))], 14)
    C.append(_stale_case("repair-129-r2-mild", c, W, ["invert", "repair"], [1], pairs=2))

    # -- a chain on one handle: invert, scale, repair (closures up), scale, repair (closures down)
    c = with_closures(b129, [(15, 60), (40, 110)])
    g = up(2, 8)
    W = _weights(c, 2, [(3.0, 0.0, None), (3.9, 0.01, g), (7.8, 0.01, g), (6.0, 0.01, None)], 8)
    C.append(_stale_case("chain-129", c, W, ["invert", "scale", "repair", "scale", "repair"], [1, 2, 3, 4], pairs=2))

    # -- the cap: twelve repairs in a row (closures up and down in turn), the thirteenth step inverts
    c = with_closures(b129, [(30, 90), (50, 125)])
    g = up(2, 9)
    steps = [(1.0 + 0.1 * t, 0.01, g if t % 2 == 0 else None) for t in range(13)]
    W = _weights(c, 2, steps, 9)
    C.append(_stale_case("cap-129", c, W, ["invert"] + ["repair"] * 12 + ["invert"], [12, 13], pairs=2))

    # -- re-inversion verdicts, each on a handle of its own
    repair("invert-193-65-pairs", b193, [(2 * k, 128 + k % 64) if k < 64 else (1, 190) for k in range(65)], 10)
    c = with_closures(b129, [(20, 70)])
    C.append(_stale_case("invert-129-vanished", c, _weights(c, 1, [(1.3, 0.01, 0.0)], 11), ["invert", "invert"], [1]))
    C.append(_stale_case("invert-129-x200", c, _weights(c, 1, [(1.0, 0.01, 200.0)], 12), ["invert", "invert"], [1]))
    W = _weights(c, 1, [(1.0, 0.01, None)], 13)
    late = np.minimum(c["I"][:, 0], c["I"][:, 1]) >= c["n"] // 2                                 # the later half of the views
    W[1] = np.where(late, 1.5 * W[1], W[1])
    C.append(_stale_case("invert-129-diagonal-spread", c, W, ["invert", "invert"], [1]))
    return C


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)

# the stopping mechanism itself, on a fresh handle: one pcg_cases case per kernel family (classic with the fused
# p-update + SpMV, classic with the separate ones, the level-1 down-sweep in the update, the two-launch iteration)
MECHANISM_CASES = ("add2far-1025", "add2sep-1537", "l1f-1025", "cg2-1025")

# the cases each mutant is tried on (test_stale_cases_cpu.py). Every mutant but ref_kept leaves the chain of verdicts as
# it is (asserted there): it acts inside the repair or the scale, not through another verdict. ref_kept compares the
# next step with the operator of before the repair, so the verdicts after the first repair change with it.
MUTANT_CASES = {
    "no_repair": ("repair-65-r1", "repair-129-r3-shared-row", "repair-193-r17", "repair-193-r64", "repair-769-r3"),
    "delta_sign": ("repair-65-r1", "repair-129-r3-shared-row", "repair-193-r17", "repair-193-r64", "chain-129",
                   "cap-129"),
    "c_all": ("repair-129-r2-mild",),
    "ref_kept": ("chain-129",),
    "inband_now": ("repair-65-r1", "repair-129-r3-shared-row", "repair-193-r64", "repair-129-r2-mild"),
    "scale_lo": ("scale-mult2-513", "scale-add2far-1025", "scale-cg2-1025"),
    "both_triangles": ("repair-65-r1", "repair-129-r3-shared-row", "repair-193-r17"),
    "slice0": ("repair-193-r17",),
}
