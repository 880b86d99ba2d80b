"""Cases and references for ONE linear solve x = L^-1 b of the banded direct solver (irotavg_amd/csrc/bcr.hip: block cyclic
reduction), shared by the CPU test of the references themselves (test_band_cases_cpu.py) and the GPU test
(test_gpu_band_solve.py). A plain module: building a case and its references needs no device.

Operator. Exactly what pcg_cases.operator builds: L = A' diag(w^2) A and b = A' diag(w^2) r, A = oracle.make_A (an edge
whose second view is fixed has no row, one whose first view is fixed keeps a single coefficient), r = log_map(delta_rel(I,
QQ, Q0)), three columns. Systems of up to DENSE_MAX rows are built dense by pcg_cases.operator itself; the larger ones in
BAND STORAGE (nu x (2 bw + 1): S[i, bw + j - i] = L[i, j]) by band_operator, which test_band_cases_cpu.py holds to
pcg_cases.operator on a small case. An isolated view has an empty row and column: the references remove it (x = 0 there).

References of a case (references()):
* x_ld    -- long-double banded Cholesky with a step of refinement: dense_cases.chol_solve_ld(M, B, bw=) for the systems in
             dense storage, its band-storage twin band_chol_solve for the others (the CPU test holds the twin to
             chol_solve_ld on a small case);
* x_lu64  -- numpy.linalg.solve in float64 (dense storage) or LAPACK's float64 banded Cholesky (scipy.linalg.solveh_banded);
* x_bcr64 -- bcr_solve64: a float64 NumPy restatement of the KERNEL'S algorithm, chunk for chunk (below).

Error measure, after pcg_cases.ratio:

    e_ref    = max( max|x_lu64 - x_ld| , max|x_bcr64 - x_ld| ) / max|x_ld|
    ratio(X) = ( max|X - x_ld| / max|x_ld| ) / max( e_ref , nu 2^-52 )                    bar: BAR = 16

The bar comes from the references alone. 16 is pcg_cases' figure for the same argument (a reordering of about as many terms
as the reference's own); a plain odd-even float64 cyclic reduction measured 0.6 - 2.7 x the error of numpy.linalg.solve on
pcg_cases systems of 520 - 1537 rows, bw 8 / 16 / 32, weights uniform and over six decades, so a correct kernel has an order
of magnitude of room. The CPU test asserts the restatement's own error <= 4 x max(the LU error, the floor) on every case.

The restatement (bcr_solve64; the formulas are those of bcr.hip's header comment).
* Blocks of B rows (rows past nu: the identity), chunks of eight blocks (positions past the last block: identity blocks
  without couplings, whose eliminations change nothing). Inside a chunk the eliminations run (0 2 4 6)(1 5)(3), block 7 is
  the separator; eliminating block i between its neighbours a (left; -1: the separator of the chunk before) and c (right):
      W = D_i^-1 [P' | Q | R_i],   P = A[a, i], Q = A[i, c]
      D_c -= Q' W_Q,  R_c -= Q' W_R   (all of a round first: phase 1),   then
      D_a -= P W_P,   A[a, c] = -P W_Q,   R_a -= P W_R.
  A chunk hands on: its separator (sepD, sepR), what it subtracted from the separator before it (extD, extR) and the coupling
  of that separator to its own (extG). Block j of the next level: D = sepD[j] + extD[j + 1], R likewise, coupling to j - 1 =
  extG[j].
* D_i^-1 is an explicit inverse by a symmetric sweep without pivoting (sweep_inverse, as bcr_invert): pivot k is dead when it
  is not above kDeadTol = 1e-13 x the block's diagonal entry of that row as the sweep found it; its row and column of the
  inverse are zero.
* The level recursion is bcr_alloc's, taken as an ARGUMENT (`levels`: (blocks, chunks, reduced) per level, what
  Graph.direct_info() reports; expected_levels() restates bcr_alloc for the cases' names): a MIXED level 1 (reduced <
  blocks) whose blocks past `reduced` are level-0 blocks 8 reduced + (gb - reduced) that no chunk reduced, and -- `top16` --
  a last level of up to sixteen blocks eliminated in the order bcr_top_schedule gives (the first four even positions of the
  list of blocks still alive, round by round); otherwise the last level is one chunk whose block 7 is solved.
* The way back: x_i = W_R - W_P x_a - W_Q x_c, rounds in reverse, level by level.

`mutant=` names a defect applied to the restatement alone (MUTANTS; test_band_cases_cpu.py: what the bar can see).
"""
import functools

import numpy as np
from numpy.lib.stride_tricks import as_strided

import pcg_cases as PC
from dense_cases import chol_solve_ld
from irotavg_amd import synth

LD = np.longdouble
EPS = 2.0 ** -52
BAR = 16.0
DEAD_TOL = 1e-13     # common.hpp: kDeadTol
NCU = 256            # compute units of an MI355X: bcr_alloc sizes the mixed level by them
DENSE_MAX = 1200     # rows up to which a system is held dense (pcg_cases.operator, chol_solve_ld, numpy.linalg.solve)

MUTANTS = ("fill_dropped", "fill_scaled", "pivot_row_formula", "short_block_rhs", "seam_neighbour", "mixed_offset",
           "top_order", "dead_unclamped")

ORDER = (((0, -1, 1), (2, 1, 3), (4, 3, 5), (6, 5, 7)), ((1, -1, 3), (5, 3, 7)), ((3, -1, 7),))   # (i, a, c) per round


# ---- the level shape ------------------------------------------------------------------------------------------------
def block_size(band):
    """bcr_plan_block: the smallest multiple of four that holds the band, at least 8."""
    return 8 if band <= 8 else (band + 3) // 4 * 4


def expected_levels(nu, B, ncu=NCU, no_mixed=False, no_top16=False):
    """bcr_alloc's recursion: ([(blocks, chunks, reduced)], top16) of a plain handle (no closures, not a shard)."""
    nb0 = -(-nu // B)
    nch0 = -(-nb0 // 8)
    cap = ncu * (2 if B <= 24 else 1)
    full = nch0 // cap * cap
    rem = nch0 - full
    nraw = 0
    if full > 0 and 0 < rem <= cap // 4 and not no_mixed:
        nraw, nch0 = nb0 - 8 * full, full
    top16 = B <= 24 and not no_top16
    topmax = 16 if top16 else 8
    lev, nb, nch, l = [], nb0, nch0, 0
    while True:
        lev.append((nb, nch, nb - nraw if (l == 1 and nraw > 0) else nb))
        if nb <= topmax and l > 0 and top16:
            break
        if nb <= 8:
            top16 = False
            break
        nb = nch + (nraw if l == 0 else 0)
        nch = -(-nb // 8)
        l += 1
    return lev, top16


def top_schedule(n):
    """bcr_top_schedule: (rounds of (i, a, c), the block that is left)."""
    alive, rounds = list(range(n)), []
    while len(alive) > 1 and len(rounds) < 6:
        rnd, nxt = [], []
        for p, blk in enumerate(alive):
            if p % 2 == 0 and len(rnd) < 4:
                rnd.append((blk, alive[p - 1] if p > 0 else -1, alive[p + 1] if p + 1 < len(alive) else -1))
            else:
                nxt.append(blk)
        rounds.append(rnd)
        alive = nxt
    assert len(alive) == 1
    return rounds, alive[0]


# ---- graphs ---------------------------------------------------------------------------------------------------------
def make_case(name, route, nu, f, bw, fam, *, scale=1.0, weak=None, isolated=(), env=None, system=None, twin=None, seed=0):
    """A view sequence of nu free views behind f fixed ones whose edges span up to bw views (the spans 1 and bw always,
    the others with probability 0.7), three edges whose SECOND endpoint is fixed (make_A drops them), weights of family
    `fam` ('u': uniform(0.1, 5), 's': 10^U(-3, 3)) times `scale`. weak: row v is tied to the rows before it by the single
    edge (v - 1, v), of weight 1e-5. isolated: rows without any edge. env: the switches the handle is created under;
    system: the case whose system this one solves again; twin: the same system with unscaled weights."""
    rng = np.random.default_rng([107, nu, f, bw, seed])
    n = nu + f
    j = np.repeat(np.arange(1, n), bw)
    dd = np.tile(np.arange(1, bw + 1), n - 1)
    keep = (j - dd >= 0) & ((dd == 1) | (dd == bw) | (rng.random(len(j)) < 0.7))
    I = np.stack([j[keep] - dd[keep], j[keep]], 1)
    for row in isolated:
        v = f + row
        I = I[(I[:, 0] != v) & (I[:, 1] != v)]
        if f <= v - 1 and v + 1 < n:
            I = np.concatenate([I, [[v - 1, v + 1]]])          # the sequence stays in one piece around it
    wk = None
    if weak is not None:
        v = f + weak
        I = I[~((I[:, 0] < v) & (I[:, 1] >= v)) | ((I[:, 0] == v - 1) & (I[:, 1] == v))]
        wk = int(np.nonzero((I[:, 0] == v - 1) & (I[:, 1] == v))[0][0])
    I = np.concatenate([I, [[f + min(2, nu - 1), 0], [f + nu // 2, f - 1], [n - 1, 0]]]).astype(np.int32)
    m = len(I)
    w = (10.0 ** rng.uniform(-3.0, 3.0, size=m) if fam == "s" else rng.uniform(0.1, 5.0, size=m)) * scale
    if wk is not None:
        w[wk] = 1e-5
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(m, 3))), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(n, 3))), Qgt)
    Q0[:f] = Qgt[:f]
    env = dict(env or {})
    band = min(bw, nu - 1)                                     # the widest span between two free views
    B = block_size(band)
    levels, top16 = expected_levels(nu, B, no_mixed="IROTAVG_BCR_NO_MIXED" in env, no_top16="IROTAVG_BCR_NO_TOP16" in env)
    return dict(name=name, route=route, nu=nu, n=n, f=f, bw=band, I=I, QQ=QQ, Q0=Q0, Qgt=Qgt, w=w, fam=fam, scale=scale, weak=weak,
                isolated=tuple(isolated), env=env, system=system or name, twin=twin, B=B, levels=levels, top16=top16)


def _cases():
    C = []

    def add(name, route, nu, bw, fam, **k):
        C.append(make_case(name, route, nu, (1, 3)[len(C) % 2], bw, fam, **k))

    def nb(nb0, B):
        return nb0 * B - 3
    # one chunk, the top at level 0
    for B in range(8, 33, 4):
        for fam in ("u", "s") if B in (8, 32) else ("u",):
            for nu in (8 * B, 8 * B - 1, 5):                   # (five views: the band is 4 whatever bw, blocks of 8)
                add("one-b%d-%d-%s" % (B, nu, fam), "one", nu, B, fam)
    # two levels, a top of 2 ... 8 blocks (blocks of 28 / 32 and 65 blocks: three levels, each a launch of its own)
    for B in (8, 16, 24):
        for nb0 in (9, 16, 17, 64):
            add("two-b%d-nb%d" % (B, nb0), "two", nb(nb0, B), B, "u")
    for B in (28, 32):
        for nb0 in (9, 64, 65):
            add("%s-b%d-nb%d" % ("two" if nb0 < 65 else "sep", B, nb0), "two" if nb0 < 65 else "sep", nb(nb0, B), B, "u")
    # two levels, the single-workgroup top of 9 ... 16 blocks
    for B in (8, 12, 20, 24):
        for nb0 in (65, 72, 73, 121, 128):
            add("top16-b%d-nb%d" % (B, nb0), "top16", nb(nb0, B), B, "u")
    # three and four levels, the upper levels in one launch
    for B, nb0 in ((8, 129), (8, 1025), (24, 129)):
        for fam in ("u", "s"):
            add("up-b%d-nb%d-%s" % (B, nb0, fam), "up", nb(nb0, B), B, fam)
    # ... in separate launches (blocks of 32)
    add("sep-b32-nb513", "sep", nb(513, 32), 32, "u")
    # a mixed level 1 (sized for 256 compute units)
    add("mixed-b8", "mixed", 512 * 64 + 13 * 8 - 3, 8, "u")
    add("mixed-b32", "mixed", 256 * 8 * 32 + 5 * 32 - 1, 32, "u")
    # the switches: the same systems again
    by = {c["name"]: c for c in C}
    for tag, env in (("nofusedasm", {"IROTAVG_BCR_NO_FUSED_ASM": "1"}), ("notop16", {"IROTAVG_BCR_NO_TOP16": "1"}),
                     ("upcap0", {"IROTAVG_BCR_UP_CAP": "0"})):
        base = by["up-b8-nb129-s"]
        C.append(make_case("switch-%s" % tag, "switch", base["nu"], base["f"], 8, "s", env=env, system=base["name"]))
    base = by["mixed-b8"]
    C.append(make_case("switch-nomixed", "switch", base["nu"], base["f"], 8, "u", env={"IROTAVG_BCR_NO_MIXED": "1"},
                       system=base["name"]))
    # large pivots: all weights x 2^10 (and the unscaled twin where the list above has none)
    add("up-b16-nb129-s", "up", nb(129, 16), 16, "s")
    by = {c["name"]: c for c in C}
    for B in (8, 16, 24):
        base = by["up-b%d-nb129-s" % B]
        C.append(make_case("big-b%d-nb129-s" % B, "big", base["nu"], base["f"], B, "s", scale=1024.0, twin=base["name"]))
    # a weak link: cond 1e10 and more
    add("weak-b8-1025", "weak", 1025, 8, "u", weak=600)
    # dead pivots: row 0 of a block, the last row of a separator block, the last (short) block
    add("dead-b8-row0", "dead", 1025, 8, "u", isolated=(80,))
    add("dead-b8-sep", "dead", 1025, 8, "u", isolated=(191,))
    add("dead-b8-last", "dead", 1025, 8, "u", isolated=(1024,))
    return C


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


# ---- the operator ---------------------------------------------------------------------------------------------------
def _scatter(n, idx, val):
    """sum of val over equal idx -> (n, ...), in val's dtype (np.add.at is slow, np.bincount knows no long double)."""
    out = np.zeros((n,) + val.shape[1:], dtype=val.dtype)
    if len(idx):
        o = np.argsort(idx, kind="stable")
        idx, val = idx[o], val[o]
        first = np.nonzero(np.concatenate([[True], idx[1:] != idx[:-1]]))[0]
        out[idx[first]] = np.add.reduceat(val, first, axis=0)
    return out


def band_operator(case, dtype):
    """(S, b): L in band storage and the right-hand side, accumulated in `dtype` from the fp64 weights and residuals."""
    nu, f, bw = case["nu"], case["f"], case["bw"]
    I = case["I"].astype(np.int64)
    i, j = I[:, 0] - f, I[:, 1] - f
    assert not np.any((i == j) & (j >= 0))
    e1 = np.nonzero((j >= 0) & (i < 0))[0]
    e2 = np.nonzero((j >= 0) & (i >= 0))[0]
    w2 = np.asarray(case["w"], dtype=dtype) ** 2
    r = np.asarray(PC.residuals(case), dtype=dtype)
    W = 2 * bw + 1
    p, q = j[e2], i[e2]
    assert np.abs(p - q).max() <= bw
    flat = np.concatenate([j[e1] * W + bw, p * W + bw, q * W + bw, p * W + bw + (q - p), q * W + bw + (p - q)])
    val = np.concatenate([w2[e1], w2[e2], w2[e2], -w2[e2], -w2[e2]])
    S = _scatter(nu * W, flat, val).reshape(nu, W)
    wr1, wr2 = w2[e1][:, None] * r[e1], w2[e2][:, None] * r[e2]
    b = _scatter(nu, np.concatenate([j[e1], p, q]), np.concatenate([wr1, wr2, -wr2]))
    return S, b


def band_from_dense(L, bw):
    nu = len(L)
    S = np.zeros((nu, 2 * bw + 1), dtype=L.dtype)
    for d in range(-bw, bw + 1):
        k = np.arange(max(0, -d), min(nu, nu - d))
        S[k, bw + d] = L[k, k + d]
    return S


def dense_from_band(S):
    nu, bw = len(S), S.shape[1] // 2
    L = np.zeros((nu, nu), dtype=S.dtype)
    for d in range(-bw, bw + 1):
        k = np.arange(max(0, -d), min(nu, nu - d))
        L[k, k + d] = S[k, bw + d]
    return L


@functools.lru_cache(maxsize=4)
def _operator(system, ld):
    case, dtype = CASE[system], (LD if ld else np.float64)
    if case["nu"] <= DENSE_MAX:
        L, b, _, _ = PC.operator(case, dtype)
        assert not np.any(np.triu(L, case["bw"] + 1))
        return band_from_dense(L, case["bw"]), b
    return band_operator(case, dtype)


def operator(case, dtype):
    """(S, b) of the case's system in band storage (cached: the two most recent)."""
    return _operator(case["system"], dtype is LD)


def band_matvec(S, X):
    nu, bw = len(S), S.shape[1] // 2
    Xp = np.zeros((nu + 2 * bw,) + X.shape[1:], dtype=S.dtype)
    Xp[bw:bw + nu] = X
    out = np.zeros_like(Xp[:nu])
    for d in range(2 * bw + 1):
        out += S[:, d, None] * Xp[d:d + nu]
    return out


def _without_dead(S, b):
    """The dead rows (empty row and column) and the system with them removed: a unit diagonal and a zero right-hand side."""
    bw = S.shape[1] // 2
    dead = np.nonzero(~(S[:, bw] > 0))[0]
    if len(dead):
        S, b = S.copy(), b.copy()
        assert not np.any(S[dead])
        S[dead, bw] = 1
        b[dead] = 0
    return dead, S, b


# ---- long-double (or float64) Cholesky in band storage --------------------------------------------------------------
def band_chol(S):
    """The right-looking Cholesky factor of S on its band storage, as a function Rm -> L^-1 Rm (no refinement)."""
    nu, W = S.shape
    bw, dt = W // 2, S.dtype
    U = np.zeros((nu + bw, W), dtype=dt)
    U[:nu] = S
    U[nu:, bw] = 1
    it = U.itemsize
    for j in range(nu):
        d = np.sqrt(U[j, bw])
        U[j, bw] = d
        l = U[j, bw + 1:] / d
        U[j, bw + 1:] = l
        # rows and columns j + 1 ... j + bw: element (a, b) sits at U[j + 1 + a, bw + b - a]
        win = as_strided(U[j + 1:, bw:], shape=(bw, bw), strides=((W - 1) * it, it))
        win -= np.outer(l, l)

    def solve(Rm):
        Y = np.zeros((nu + bw,) + Rm.shape[1:], dtype=dt)
        Y[:nu] = Rm
        for j in range(nu):
            Y[j] /= U[j, bw]
            Y[j + 1:j + 1 + bw] -= np.outer(U[j, bw + 1:], Y[j])
        for j in range(nu - 1, -1, -1):
            Y[j] = (Y[j] - U[j, bw + 1:] @ Y[j + 1:j + 1 + bw]) / U[j, bw]
        return Y[:nu]
    return solve


def band_chol_solve(S, Bm, refine=1):
    """L^-1 Bm in S's dtype: right-looking Cholesky on the band storage + `refine` rounds of refinement."""
    solve = band_chol(S)
    Bm = np.asarray(Bm, dtype=S.dtype)
    X = solve(Bm)
    for _ in range(refine):
        X = X + solve(Bm - band_matvec(S, X))
    return X


# ---- the restatement ------------------------------------------------------------------------------------------------
def sweep_inverse(Dm, mutant=None, count=None):
    """Explicit inverses of the SPD blocks Dm (N x B x B) by bcr_invert's symmetric sweep, dead pivots zeroed."""
    t = np.array(Dm, dtype=np.float64)
    N, B, _ = t.shape
    dgt = DEAD_TOL * np.einsum("nii->ni", t).copy()
    with np.errstate(all="ignore"):
        for k in range(B):
            p = t[:, k, k].copy()
            alive = p > dgt[:, k]
            if mutant == "dead_unclamped":
                alive = np.ones_like(alive)
            if count is not None:
                count[0] += int((~alive).sum())
            pinv = np.where(alive, 1.0 / np.where(alive, p, 1.0), 0.0)
            rowk, colk = t[:, k, :].copy(), t[:, :, k].copy()
            if mutant == "pivot_row_formula":
                f = np.where(alive[:, None], rowk - ((p - 1.0) / np.where(alive, p, 1.0))[:, None] * rowk, 0.0)
            else:
                f = rowk * pinv[:, None]
            t -= colk[:, :, None] * f[:, None, :]
            t[:, k, :] = f
            t[:, :, k] = colk * pinv[:, None]
            t[:, k, k] = -pinv
    return -t


def level0_blocks(S, b, B, nblk):
    """(D, G, R) of the first nblk blocks of level 0: G[k] = L[block k - 1, block k]; rows past nu: the identity."""
    nu, bw = len(S), S.shape[1] // 2
    Sp = np.zeros((nblk * B, 2 * bw + 1))
    Sp[:nu] = S[:nblk * B]
    Sp[nu:, bw] = 1.0
    r, c = np.arange(B)[:, None], np.arange(B)[None, :]
    rows = (np.arange(nblk) * B)[:, None, None] + r[None]
    D = Sp[rows, np.clip(c - r + bw, 0, 2 * bw)[None]] * (np.abs(c - r) <= bw)
    G = Sp[np.maximum(rows - B, 0), np.clip(B + c - r + bw, 0, 2 * bw)[None]] * (B + c - r <= bw)
    G[0] = 0.0
    R = np.zeros((nblk * B, 3))
    R[:min(nu, nblk * B)] = b[:nblk * B]
    return D, G, R.reshape(nblk, B, 3)


def _reduce(D, G, R, inv, fill=None, norhs=None):
    """The three rounds on every chunk of a level at once. fill = (chunk, factor): the fill block of that chunk's last
    elimination times factor; norhs = (chunk, position): that block's right-hand side is not updated."""
    nch, B = len(D) // 8, D.shape[-1]
    sD, sR = D.reshape(nch, 8, B, B).copy(), R.reshape(nch, 8, B, 3).copy()
    sG = G.reshape(nch, 8, B, B).copy()               # slot 0: separator before the chunk -> block 0; slot s: s - 1 -> s
    xD, xR = np.zeros((nch, B, B)), np.zeros((nch, B, 3))
    Wk = {}

    def rhs(target, upd):
        if norhs is not None and norhs[1] == target:
            upd = upd.copy()
            upd[norhs[0]] = 0.0
        return upd
    for rnd in ORDER:
        for i, a, c in rnd:
            Di = inv(sD[:, i])
            P, Q = sG[:, a + 1], sG[:, i + 1]
            WP, WQ, WR = Di @ P.transpose(0, 2, 1), Di @ Q, Di @ sR[:, i]
            QT = Q.transpose(0, 2, 1)
            sD[:, c] -= QT @ WQ
            sR[:, c] -= rhs(c, QT @ WR)
            Wk[i] = (WP, WQ, WR)
        for i, a, c in rnd:
            WP, WQ, WR = Wk[i]
            P = sG[:, a + 1].copy()
            if a >= 0:
                sD[:, a] -= P @ WP
                sR[:, a] -= rhs(a, P @ WR)
            else:
                xD -= P @ WP
                xR -= P @ WR
            F = -(P @ WQ)
            if fill is not None and i == 3:
                F[fill[0]] *= fill[1]
            sG[:, a + 1] = F
    return dict(W=Wk, sepD=sD[:, 7].copy(), sepR=sR[:, 7].copy(), extD=xD, extR=xR, extG=sG[:, 0].copy())


def _back(Wk, x7, xext):
    nch, B, _ = x7.shape
    x = np.zeros((nch, 8, B, 3))
    x[:, 7] = x7
    for rnd in reversed(ORDER):
        for i, a, c in rnd:
            WP, WQ, WR = Wk[i]
            x[:, i] = WR - WP @ (xext if a < 0 else x[:, a]) - WQ @ x[:, c]
    return x.reshape(nch * 8, B, 3)


def _top16(D, G, R, n, inv, swap):
    """bcr_top_body: the solutions of all n blocks of the last level."""
    rounds, last = top_schedule(n)
    if swap and n >= 4:
        # every elimination a round of its own, block 1 (round 1, between nothing and 3) BEFORE block 2 (round 0): its
        # coupling to the right is still the one to block 2
        seq = [[e] for rnd in rounds for e in rnd]
        k2 = next(k for k, r in enumerate(seq) if r[0][0] == 2)
        k1 = next(k for k, r in enumerate(seq) if r[0][0] == 1)
        seq[k2], seq[k1] = seq[k1], seq[k2]
        rounds = seq
    sD, sR = D[:n].copy(), R[:n].copy()
    sG = [G[x + 1].copy() for x in range(n - 1)] + [None]      # block x -> the next block alive
    B = D.shape[-1]
    Z = np.zeros((B, B))
    Wk = {}
    for rnd in rounds:
        for i, a, c in rnd:
            Di = inv(sD[i][None])[0]
            P, Q = (sG[a] if a >= 0 else Z), (sG[i] if c >= 0 else Z)
            Wk[i] = (Di @ P.T, Di @ Q, Di @ sR[i])
            if c >= 0:
                sD[c] -= Q.T @ Wk[i][1]
                sR[c] -= Q.T @ Wk[i][2]
        for i, a, c in rnd:
            if a >= 0:
                WP, WQ, WR = Wk[i]
                P = sG[a].copy()
                sD[a] -= P @ WP
                sR[a] -= P @ WR
                sG[a] = -(P @ WQ)
    x = np.zeros((n, B, 3))
    x[last] = inv(sD[last][None])[0] @ sR[last]
    for rnd in reversed(rounds):
        for i, a, c in rnd:
            WP, WQ, WR = Wk[i]
            x[i] = WR - (WP @ x[a] if a >= 0 else 0.0) - (WQ @ x[c] if c >= 0 else 0.0)
    return x


def bcr_solve64(S, b, B, levels, top16, mutant=None, info=None):
    """x = L^-1 b the way bcr.hip computes it, in float64 (see the module docstring). S, b: the system in band storage;
    levels: [(blocks, chunks, reduced)]; top16: the last level is the single-workgroup top. info: a dict that receives
    `dead`, the dead pivots met."""
    assert mutant is None or mutant in MUTANTS
    S, b = np.asarray(S, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nu, nl = len(S), len(levels)
    levels = [tuple(int(v) for v in lv) for lv in levels]
    nb0, nch0, _ = levels[0]
    assert nb0 == -(-nu // B) and all(nch == -(-nb // 8) or l == 0 for l, (nb, nch, _) in enumerate(levels))
    mixed = nl > 1 and levels[1][2] < levels[1][0]
    assert (8 * nch0 < nb0) == mixed and (not mixed or levels[1][0] - levels[1][2] == nb0 - 8 * nch0)
    count = [0]

    def inv(Dm):
        return sweep_inverse(Dm, mutant, count)
    D0, G0, R0 = level0_blocks(S, b, B, max(8 * nch0, nb0) + 2)
    fill = norhs = None
    if mutant in ("fill_dropped", "fill_scaled") and nch0 > 1:
        fill = (1, 0.0 if mutant == "fill_dropped" else 1.0 + 1e-9)
    if mutant == "short_block_rhs" and nu % B and (nb0 - 1) // 8 < nch0:
        norhs = ((nb0 - 1) // 8, (nb0 - 1) % 8)
    cur = (D0[:8 * nch0], G0[:8 * nch0], R0[:8 * nch0])
    outs, xup = [], None
    for l, (nb, nch, nred) in enumerate(levels):
        if l == nl - 1 and top16:
            assert l > 0 and nb <= 16
            xup = _top16(cur[0], cur[1], cur[2], nb, inv, mutant == "top_order")
            break
        out = _reduce(cur[0], cur[1], cur[2], inv, fill if l == 0 else None, norhs if l == 0 else None)
        outs.append(out)
        if l == nl - 1:
            assert nch == 1 and nb <= 8
            xup = _back(out["W"], inv(out["sepD"]) @ out["sepR"], np.zeros((1, B, 3)))
            outs.pop()
            break
        nb1, nch1, nred1 = levels[l + 1]
        assert nred1 == nch and nb1 == nch + (max(0, nb0 - 8 * nch0) if l == 0 else 0) and (l == 0 or nred1 == nb1)
        D = np.zeros((8 * nch1, B, B))
        D[:] = np.eye(B)
        G, R = np.zeros((8 * nch1, B, B)), np.zeros((8 * nch1, B, 3))
        D[:nred1], R[:nred1], G[1:nred1] = out["sepD"], out["sepR"], out["extG"][1:]
        D[:nred1 - 1] += out["extD"][1:]
        R[:nred1 - 1] += out["extR"][1:]
        if nb1 > nred1:
            lb = 8 * nred1 + np.arange(nb1 - nred1) + (1 if mutant == "mixed_offset" else 0)
            D[nred1:nb1], G[nred1:nb1], R[nred1:nb1] = D0[lb], G0[lb], R0[lb]
        cur = (D, G, R)
    xraw = np.zeros((0, B, 3))
    for l in range(len(outs) - 1, -1, -1):
        nb, nch, nred = levels[l]
        x7 = xup[:nch]
        xext = np.concatenate([np.zeros((1, B, 3)), xup[:nch - 1]])
        if mutant == "seam_neighbour" and l == 0 and nch > 1:
            xext[1] = xup[1]                                   # chunk 1's left neighbour: its own separator
        if l == 0 and mixed:
            xraw = xup[levels[1][2]:levels[1][0]]
        xup = _back(outs[l]["W"], x7, xext)
    if info is not None:
        info["dead"] = count[0]
    return np.concatenate([xup.reshape(-1, 3), xraw.reshape(-1, 3)])[:nu]


# ---- references and the comparison ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _references(system, B, levels, top16):
    case = CASE[system]
    nu, bw = case["nu"], case["bw"]
    S64, b64 = operator(case, np.float64)
    info = {}
    x_bcr = bcr_solve64(S64, b64, B, levels, top16, info=info)
    dead, S64, b64 = _without_dead(S64, b64)
    if nu <= DENSE_MAX:
        x_lu = np.linalg.solve(dense_from_band(S64), b64)
    else:
        from scipy.linalg import solveh_banded
        x_lu = solveh_banded(np.ascontiguousarray(S64[:, bw:].T), b64, lower=True)
    Sld, bld = operator(case, LD)
    dead_ld, Sld, bld = _without_dead(Sld, bld)
    assert np.array_equal(dead, dead_ld)
    if nu <= DENSE_MAX:
        x_ld = chol_solve_ld(dense_from_band(Sld), bld, bw)
    else:
        x_ld = band_chol_solve(Sld, bld)
    x_lu[dead] = 0.0
    scale = float(np.abs(x_ld).max())
    e_lu = float(np.abs(x_lu - x_ld).max()) / scale
    e_bcr = float(np.abs(x_bcr - x_ld).max()) / scale
    return dict(x_ld=x_ld, x_lu64=x_lu, x_bcr64=x_bcr, scale=scale, e_lu=e_lu, e_bcr=e_bcr, e_ref=max(e_lu, e_bcr),
                floor=nu * EPS, dead=dead, ndead=info["dead"], res_bcr64=residual_ld(case, x_bcr))


def references(case, block=None, levels=None, top16=None):
    """The three references of a case (computed once); block / levels / top16: what the handle reports (default: what the
    case is named for)."""
    levels = case["levels"] if levels is None else levels
    return _references(case["system"], case["B"] if block is None else block, tuple(tuple(lv) for lv in levels),
                       case["top16"] if top16 is None else top16)


def restated(case, mutant=None):
    """x_bcr64 of the case at the level shape it is named for, with a mutant."""
    S, b = operator(case, np.float64)
    return bcr_solve64(S, b, case["B"], case["levels"], case["top16"], mutant=mutant)


def ratio(ref, X):
    """The comparison of the module docstring (nan when X is not finite)."""
    with np.errstate(all="ignore"):
        err = float(np.abs(np.asarray(X, dtype=LD) - ref["x_ld"]).max()) / ref["scale"]
    return err / max(ref["e_ref"], ref["floor"])


def residual_ld(case, X):
    """max over the three columns of ||b - L X|| / ||b||, formed in long double."""
    S, b = operator(case, LD)
    with np.errstate(all="ignore"):
        r = b - band_matvec(S, np.asarray(X, dtype=LD))
        return float(np.sqrt((r * r).sum(0) / (b * b).sum(0)).max())
