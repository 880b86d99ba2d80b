"""Cases for the rotation-variance query and the edge diagnostics (irotavg_graph_rotation_variance,
irotavg_graph_edge_diagnostics: irotavg_amd/csrc/marginals.hip, edgediag.hip) AT THE BLOCK EDGES of their own factorisation:
block counts at and next to a power of two, free-view counts that fill the last block / the last 64-row tile exactly, every
block size, boundary slots on the band assembly, spans of 33 ... 63 views at blocks of 32, closure counts at the 64-column
tile edges of Z / S and at the planner's limit, more pairs than one chunk of the pair solve, and the dense route at its
64-row seams and at the route boundary. Shared by test_variance_cases_cpu.py (the table, the references, what the tolerance
can see) and test_gpu_variance_edges.py. A plain module: building a case needs no device.

A case is a view sequence -- every view tied to its `band` predecessors, fixed views included -- plus extra edges, with
seeded weights U(0.1, 3), ground-truth rotations and measurements that carry N(0, 0.01^2) rad of noise. The extra edges are
appended behind the band edges, the closures among them last but for the additions of b8_fixed3.

What a case must reach is COMPUTED HERE by restating the planner's rule (bcr_plan, bcr.hip), never read from the device.
With band = the widest span <= 32 between free views and nfar = the number of spans > 32 between free views:

    handle block   B = 0                          if nfar > 1024 (2048 from 8192 free views on), or
                                                  if nu <= 2048 and the handle was not created with band_direct = 1,
                   B = 8 if band <= 8 else 4 ceil(band / 4)   otherwise;
    closure        <=>  both ends free, span > 32, ends at least two blocks of B rows apart;
    route          dense if nu <= 2048 (whatever the handle is), band if B > 0, pcg otherwise.

`live` is the number of closures of weight > 0 (k of marginals.hip: the columns of Z, the order of S), ldZ = max(64, k
rounded up to 64). A tenth, ROUNDED DOWN, of a case's closures have weight zero -- so a case of fewer than ten closures
(b12_256: 5, b28_74: 1) has none, where test_gpu_edge_diagnostics.closure_case would kill one: b28_74 is there for k = 1, and
the dead closures of a short list are b12_256_k0's. b16_129 keeps all 64 alive. The cases
b20_128, b24_128 and lim_1024 therefore have live = 57, 59 and 922; their twins b20_128_k63, b24_128_k65 and lim_1024_k1024
keep every closure alive and put k itself on the tile edge and on the limit. b12_256_k0 has all five closures dead: k = 0
with a closure list that is not empty.
"""
import numpy as np

from irotavg_amd import synth

FAR_MAX = 1024        # closures a graph of fewer than 8192 free views keeps on the direct solver (kBcrMaxFar / 2)
DENSE_MAX = 2048      # free views up to which both queries run on the dense inverse
PAIR_CHUNK = 1024     # kPairChunk of marginals.hip: pair columns per multi right-hand-side solve
BOTH_REFS_MAX = 2100  # free views up to which the CPU test holds the block references to the dense inverse


# ---- the planner's rule, restated -----------------------------------------------------------------------------------------
def block_size(band):
    return 8 if band <= 8 else 4 * -(-band // 4)


def plan(I, n, f, band_direct=0):
    """dict(B, nb, closures (edge ids), route, band, nfar) of an edge list, by the rule of the module docstring."""
    ij = np.asarray(I, dtype=np.int64) - f
    nu = n - f
    free = (ij[:, 0] >= 0) & (ij[:, 1] >= 0)
    span = np.abs(ij[:, 0] - ij[:, 1])
    near = free & (span <= 32)
    band = int(span[near].max()) if near.any() else 0
    nfar = int((free & (span > 32)).sum())
    if band_direct < 0 or nfar > (FAR_MAX if nu < 8192 else 2 * FAR_MAX) or (band_direct == 0 and nu <= DENSE_MAX):
        B = 0
    else:
        B = block_size(band)
    far = np.zeros(len(ij), dtype=bool)
    if B:
        far = free & (span > 32) & (np.abs(ij[:, 0] // B - ij[:, 1] // B) >= 2)
    route = "dense" if nu <= DENSE_MAX else ("band" if B else "pcg")
    return dict(B=B, nb=-(-nu // B) if B else 0, closures=np.flatnonzero(far), route=route, band=band, nfar=nfar)


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def band_edges(n, band):
    """(i, j), i < j, every view j tied to its min(band, j) predecessors, grouped by j, nearest predecessor first."""
    jj = np.repeat(np.arange(n, dtype=np.int64), band)
    dd = np.tile(np.arange(1, band + 1, dtype=np.int64), n)
    keep = jj - dd >= 0
    return np.stack([jj[keep] - dd[keep], jj[keep]], 1)


def draw_closures(rng, nu, B, ncl):
    """ncl distinct pairs of rows at least 2 B + 64 apart, each listed reversed with probability one half."""
    gap = 2 * B + 64
    seen, out = set(), []
    while len(out) < ncl:
        i = int(rng.integers(0, nu - gap))
        j = int(rng.integers(i + gap, nu))
        if (i, j) in seen:
            continue
        seen.add((i, j))
        out.append((j, i) if rng.random() < 0.5 else (i, j))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def pick_pairs(n, f, rng, I, k):
    """k pairs as test_gpu_rotation_variance.pick_pairs builds them: random ones, i == j, a fixed view, edge endpoints.
    (A copy, so that this module needs neither pytest nor the library: the two must stay the same.)"""
    P = rng.integers(0, n, size=(k - 6, 2))
    e = np.asarray(I)[rng.integers(0, len(I), size=3)]
    return np.concatenate([P, [[0, 0], [f, f], [0, n - 1]], e]).astype(np.int32)


def placed_pairs(nu, f, unit, closure_rows):
    """The pairs a case adds to pick_pairs', as views: both ends in block 0, both ends in the last block, the last real row
    with the first, one pair across every power-of-two seam (unit 2^k - 1, unit 2^k), both ends of three closures. unit: the
    block size on the band route, 64 (the tile of the dense sweep) on the dense one."""
    last0 = (nu - 1) // unit * unit
    rows = [(0, min(unit, nu) - 1), (last0, nu - 1), (nu - 1, 0)]
    s = unit
    while s < nu:
        rows.append((s - 1, s))
        s *= 2
    rows += [tuple(e) for e in closure_rows[:3]]
    return np.array(rows, dtype=np.int64).reshape(-1, 2) + f


def make_case(name, nu, f, band, *, B, nb, closures, route, ncl=0, zero="tenth", extra=None, npairs=60, opts=None,
              more_pairs=(), seed=0):
    """One case. B / nb / closures / route: what the table claims for it (test_variance_cases_cpu.py holds the claim to
    plan()). ncl: closures drawn at least 2 B + 64 rows long; zero: "tenth" | "none" | "all" of them at weight zero.
    extra(rng, I, nu, f) -> view pairs appended behind the drawn closures."""
    n = nu + f
    rng = np.random.default_rng([211, nu, f, band, ncl, seed])
    I = band_edges(n, band)
    m_band = len(I)
    cl = draw_closures(rng, nu, block_size(band), ncl) + f
    I = np.concatenate([I, cl])
    if extra is not None:
        I = np.concatenate([I, np.asarray(extra(rng, I, nu, f), dtype=np.int64).reshape(-1, 2)])
    I = I.astype(np.int32)
    m = len(I)
    opts = dict(opts or {})
    P = plan(I, n, f, opts.get("band_direct", 0))
    d = rng.uniform(0.1, 3.0, size=m)
    far = P["closures"]
    nzero = {"tenth": len(far) // 10, "none": 0, "all": len(far)}[zero]
    d[far[:nzero]] = 0.0
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(m, 3))), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    unit = P["B"] if route != "dense" and P["B"] else 64
    add = placed_pairs(nu, f, unit, I[far].astype(np.int64) - f)
    add = np.concatenate([add, np.asarray(more_pairs, dtype=np.int64).reshape(-1, 2)])
    pairs = np.concatenate([pick_pairs(n, f, rng, I, npairs - len(add)), add]).astype(np.int32)
    assert len(pairs) == npairs and pairs.min() >= 0 and pairs.max() < n
    live = int((d[far] != 0).sum())
    return dict(name=name, n=n, nu=nu, f=f, band=band, I=I, QQ=QQ, Q=Qgt, d=d, opts=opts, pairs=pairs, m_band=m_band,
                claim=dict(B=B, nb=nb, closures=closures, route=route),
                B=P["B"], nb=P["nb"], closures=len(far), route=P["route"], far=far, live=live,
                ldZ=max(64, -(-live // 64) * 64), plan_band=P["band"], nfar=P["nfar"])


def span40(rng, I, nu, f):
    """b32_span: edges (a, a + 40) for 60 rows a, one in each of the blocks 1 ... 60: 30 with a % 32 < 24 (the far end lies in the
    NEXT block: part of the block tridiagonal operator) and 30 with a % 32 >= 24 (two blocks on: a closure)."""
    blocks = np.arange(1, 61) * 32
    off = np.where(np.arange(60) % 2 == 0, rng.integers(0, 24, size=60), rng.integers(24, 32, size=60))
    a = blocks + off
    e = np.stack([a, a + 40], 1) + f
    flip = rng.random(60) < 0.5
    e[flip] = e[flip][:, ::-1]
    return e


def span33(rng, I, nu, f):
    """b8_span33: ten edges of span 33 at blocks of 8 rows (the shortest edge the planner counts as long), every second one
    listed reversed."""
    a = np.sort(rng.choice(nu - 33, size=10, replace=False))
    e = np.stack([a, a + 33], 1) + f
    e[1::2] = e[1::2][:, ::-1]
    return e


def fixed3(rng, I, nu, f):
    """b8_fixed3: what the boundary slots and make_A's edge-drop quirk see on the band assembly. From each of the three fixed
    views four edges to free views near and far, two listed (fixed, free) -- kept: +1 at the free end -- and two listed
    (free, fixed) -- dropped; a fixed-fixed edge; 20 band edges a second time; 20 band edges reversed; one self loop."""
    out = []
    for v in range(f):
        to = f + rng.choice(nu, size=4, replace=False)
        out += [(v, to[0]), (v, to[1]), (to[2], v), (to[3], v)]
    out.append((2, 0))
    freefree = np.flatnonzero((I[:, 0] >= f) & (I[:, 1] >= f))
    pick = I[rng.choice(freefree, size=40, replace=False)]
    out += [tuple(e) for e in pick[:20]] + [tuple(e[::-1]) for e in pick[20:]]
    out.append((f + nu // 2, f + nu // 2))
    return np.array(out, dtype=np.int64)


def _cases():
    C = []

    def add(name, nu, f, band, **k):
        C.append(make_case(name, nu, f, band, **k))

    def band(name, B, nu, f=1, ncl=0, closures=None, **k):
        add(name, nu, f, B, B=B, nb=-(-nu // B), closures=ncl if closures is None else closures, route="band", ncl=ncl, **k)
    # ---- the band route: block counts, padding, block sizes ---------------------------------------------------------------
    band("b8_257", 8, 2049, npairs=PAIR_CHUNK + 1)
    band("b8_511", 8, 4088)
    band("b8_512", 8, 4096)
    band("b8_513", 8, 4097)
    band("b12_256", 12, 3072, ncl=5)
    band("b12_256_k0", 12, 3072, ncl=5, zero="all")
    band("b16_129", 16, 2064, ncl=64, zero="none", npairs=PAIR_CHUNK + 1)
    band("b20_128", 20, 2560, f=2, ncl=63)
    band("b20_128_k63", 20, 2560, f=2, ncl=63, zero="none")
    band("b24_128", 24, 3072, ncl=65)
    band("b24_128_k65", 24, 3072, ncl=65, zero="none")
    band("b28_74", 28, 2072, ncl=1)
    band("b32_65", 32, 2049)
    band("b32_127", 32, 4064)
    band("b32_128", 32, 4096, npairs=PAIR_CHUNK + 1)
    band("b32_span", 32, 2080, closures=30, extra=span40)
    band("b8_span33", 8, 2049, closures=10, extra=span33)
    band("b8_fixed3", 8, 2056, f=3, extra=fixed3)
    # ---- the planner's limit ----------------------------------------------------------------------------------------------
    band("lim_1024", 12, 3000, ncl=1024)
    band("lim_1024_k1024", 12, 3000, ncl=1024, zero="none")
    add("lim_1025", 3000, 1, 12, B=0, nb=0, closures=0, route="pcg", ncl=1025)
    # ---- the dense route ---------------------------------------------------------------------------------------------------
    for nu in (1, 2, 63, 64, 65):
        add("d_%d" % nu, nu, 1, 6, B=0, nb=0, closures=0, route="dense", npairs=12 if nu < 63 else 60,
            more_pairs=[(1, 0)] if nu == 1 else ())
    add("d_2048", 2048, 1, 8, B=0, nb=0, closures=0, route="dense")
    add("d_2048_direct", 2048, 1, 8, B=8, nb=256, closures=0, route="dense", opts=dict(band_direct=1))
    return C


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)
BAND = [c["name"] for c in CASES if c["route"] == "band"]
DENSE = [c["name"] for c in CASES if c["route"] == "dense"]
MANY_PAIRS = ("b8_257", "b16_129", "b32_128")


def pairs_of(case):
    return [(int(a), int(b)) for a, b in case["pairs"]]


def zero_pairs(case):
    """The pairs the definition makes zero: i == j, or both ends fixed."""
    P, f = case["pairs"], case["f"]
    return (P[:, 0] == P[:, 1]) | ((P[:, 0] < f) & (P[:, 1] < f))
