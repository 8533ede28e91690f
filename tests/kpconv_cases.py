"""Cases, a float64 reference and derived error bounds for the KPConv aggregation kernels (csrc/kpconv.hip): the two launchers'
outputs wf [n_q, n_kp, c] (forward) and grad_feat [n_s, c] (backward, for a given grad_wf).  numpy only;
tests/test_kpconv_cases_cpu.py proves the cases are what they claim, that a plain fp32 evaluation of the formulas meets the
bounds and that wrong variants miss them; tests/test_kpconv_edges_hip.py runs the cases on the device.

    w[i,k,n]  = max(0, 1 - |(support[j] - query[i]) - K[k]| / extent)   j = neighbors[i,n]; the entry is skipped for j outside [0, n_s)
    wf[i,k,:] = sum_n w[i,k,n] * x[j,:]
    gf[j,:]  += sum_k w[i,k,n] * g[i,k,:]

max is torch.clamp(min=0)'s: a NaN influence stays NaN.  Every bound is in units of u = 2^-24 and is derived in DESIGN.md
("KPConv aggregation: cases and bounds").
"""
from functools import lru_cache

import numpy as np

U = 2.0 ** -24
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
PADS = (-1, None, INT_MAX, INT_MIN)  # None: n_s, the shadow point
W_A, W_B = 1.0, 5.0                  # |dw| <= u * (W_A * (|rel|_1 + d) / extent + W_B)

# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------------
KP_WAVES, MAX_C, MAX_NB, MAX_KP = 4, 64, 64, 32


def lds_bytes(n_nb, c, n_kp):
    """KpLayout::bytes()"""
    ws = n_nb | 1
    kp_floats = (3 * n_kp + 3) & ~3
    w_off = 4 * n_nb + max(n_nb, n_kp) * c
    wave_floats = (w_off + n_kp * ws + 3) & ~3
    return 4 * (kp_floats + KP_WAVES * wave_floats)


def grid_cap_queries(cus):
    """queries one pass of the persistent grid covers: 16 workgroups per CU, four waves each"""
    return 16 * cus * KP_WAVES


def small_div(t, d):
    """(int)(((float)t + 0.5f) * (1.0f / d)) in fp32, elementwise"""
    inv = np.float32(1) / np.asarray(d, np.float32)
    return ((np.asarray(t, np.float32) + np.float32(0.5)) * inv).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """query [n_q, 3], support [n_s, 3], x [n_s, c], kp [n_kp, 3], g [n_q, n_kp, c] fp32; nb [n_q, n_nb] int32 (int64 where a
    value needs it); extent a float that fp32 holds exactly.  marks: what the case promises beyond the bounds."""

    def __init__(self, name, query, support, nb, x, kp, extent, g, **marks):
        self.name, self.extent, self.marks = name, float(np.float32(extent)), marks
        f = lambda a: np.ascontiguousarray(a, np.float32)
        self.query, self.support, self.x, self.kp, self.g = f(query), f(support), f(x), f(kp), f(g)
        self.nb = np.ascontiguousarray(nb)
        assert self.nb.dtype in (np.int32, np.int64)
        self.n_q, self.n_nb = self.nb.shape
        self.n_s, self.c = self.x.shape
        self.n_kp = self.kp.shape[0]
        assert self.query.shape == (self.n_q, 3) and self.support.shape == (self.n_s, 3) and self.g.shape == (self.n_q, self.n_kp, self.c)
        assert 1 <= self.c <= MAX_C and 1 <= self.n_nb <= MAX_NB and 1 <= self.n_kp <= MAX_KP
        for a in (self.query, self.support, self.x, self.kp, self.g, self.nb):
            a.setflags(write=False)
        self._ref = None

    @property
    def valid(self):
        return (self.nb >= 0) & (self.nb < self.n_s)

    @property
    def lds(self):
        return lds_bytes(self.n_nb, self.c, self.n_kp)

    def reference(self):
        """computed once, never written to"""
        if self._ref is None:
            self._ref = Reference(self)
        return self._ref

    def replace(self, name=None, **arrays):
        a = dict(query=self.query, support=self.support, nb=self.nb, x=self.x, kp=self.kp, g=self.g)
        a.update(arrays)
        return Case(name or self.name, a["query"], a["support"], a["nb"], a["x"], a["kp"], self.extent, a["g"], **self.marks)


def kernel_points(rng, n_kp, extent):
    """the origin, then points at 0.4 .. 1 extent from it in random directions"""
    v = rng.standard_normal((n_kp, 3))
    v *= (rng.uniform(0.4, 1.0, (n_kp, 1)) * extent) / np.linalg.norm(v, axis=1, keepdims=True)
    v[0] = 0
    return v.astype(np.float32)


def neighbour_rows(rng, n_q, n_nb, n_s, counts, pads=(-1,), prefix=False):
    """rows with counts[i] valid entries: a prefix of the row (ball_query's padding) or scattered positions, order random; the
    rest is padding drawn from `pads`"""
    pad_values = np.array([n_s if p is None else p for p in pads], np.int64)
    nb = pad_values[rng.integers(0, len(pad_values), (n_q, n_nb))]
    for i, nv in enumerate(counts):
        pos = np.arange(nv) if prefix else np.sort(rng.permutation(n_nb)[:nv])
        nb[i, pos] = rng.integers(0, n_s, nv)
    return nb.astype(np.int32)


def random_case(name, seed, n_q, n_s, n_nb, c, n_kp, counts=None, pads=(-1,), prefix=False, extent=0.04, shift=None, **marks):
    """support and queries uniform in a cube of side 2 extent (a fifth to a third of the influences are positive, the others
    clamp), neighbours drawn from the whole support"""
    rng = np.random.default_rng(seed)
    extent = float(np.float32(extent))
    support = (rng.random((n_s, 3)) * 2 * extent).astype(np.float32)
    query = (rng.random((n_q, 3)) * 2 * extent).astype(np.float32)
    if shift is not None:  # rounded once more: the reference starts from the fp32 coordinates
        support, query = support + np.asarray(shift, np.float32), query + np.asarray(shift, np.float32)
    if counts is None:
        counts = rng.integers(0, n_nb + 1, n_q)
    nb = neighbour_rows(rng, n_q, n_nb, n_s, counts, pads, prefix) if n_s > 0 else \
        np.array([-1, 0, 1, INT_MAX, INT_MIN], np.int32)[rng.integers(0, 5, (n_q, n_nb))]
    return Case(name, query, support, nb, rng.standard_normal((n_s, c), dtype=np.float32), kernel_points(rng, n_kp, extent), extent,
                rng.standard_normal((n_q, n_kp, c), dtype=np.float32), **marks)


# -- divisor sweeps ---------------------------------------------------------------------------------------------------
SWEEP_Q, SWEEP_S = 130, 300


def c_sweep_case(c):  # not cached: 64 of them, each used once per test
    """n_nb = 64, n_kp = 32: rows 0..5 and the last have all 64 neighbours valid, so t reaches 64 c - 1 (staging of the rows,
    the backward's slots) and 32 c - 1 (the forward's outputs) for the divisor c"""
    rng = np.random.default_rng(4000 + c)
    counts = rng.integers(0, 65, SWEEP_Q)
    counts[:6] = 64
    counts[-1] = 64
    return random_case(f"c{c}", 5000 + c, SWEEP_Q, SWEEP_S, 64, c, 32, counts=counts, prefix=bool(c % 2))


@lru_cache(maxsize=None)
def n_valid_sweep_case():
    """every valid count 0..64 twice, shuffled, at scattered positions of the row; padding of all four kinds; n_kp = 32, so the
    influence loop's t reaches 32 n_valid - 1 for every divisor n_valid"""
    counts = np.random.default_rng(77).permutation(np.repeat(np.arange(65), 2))
    return random_case("nvalid", 78, SWEEP_Q, SWEEP_S, 64, 5, 32, counts=counts, pads=PADS)


# -- n_kp and n_nb edges ----------------------------------------------------------------------------------------------
KP_EDGES, NB_EDGES = (1, 2, 15, 16, 31, 32), (1, 2, 63, 64)
EDGE_SHAPES = [(k, n) for k in KP_EDGES for n in NB_EDGES]


@lru_cache(maxsize=None)
def edge_case(n_kp, n_nb):
    """37 queries (ten workgroups, the last with one wave at work), c = 7; rows 0..3 full, row 4 empty"""
    rng = np.random.default_rng(100 * n_kp + n_nb)
    counts = rng.integers(0, n_nb + 1, 37)
    counts[:4], counts[4] = n_nb, 0
    return random_case(f"kp{n_kp}-nb{n_nb}", 9000 + 100 * n_kp + n_nb, 37, 50, n_nb, 7, n_kp, counts=counts, pads=PADS)


# -- LDS --------------------------------------------------------------------------------------------------------------
LDS_SHAPES = {"small": (64, 34, 15), "mid": (64, 40, 15), "large": (64, 64, 15), "max": (64, 64, 32)}  # c, n_nb, n_kp
LDS_ORDER = ("small", "max", "small", "mid", "large")


@lru_cache(maxsize=None)
def lds_case(which):
    c, n_nb, n_kp = LDS_SHAPES[which]
    counts = np.random.default_rng(len(which)).integers(0, n_nb + 1, 21)
    counts[:5] = n_nb
    return random_case(f"lds-{which}", 300 + n_nb + n_kp, 21, 90, n_nb, c, n_kp, counts=counts)


# -- query counts -----------------------------------------------------------------------------------------------------
QUERY_COUNTS = (1, 3, 4, 5)


@lru_cache(maxsize=None)
def query_count_case(n_q):
    return random_case(f"nq{n_q}", 600 + n_q, n_q, 40, 9, 6, 15, counts=[9] * n_q)


@lru_cache(maxsize=None)
def past_cap_case(cus):
    """c = 3, n_nb = 4, three queries past one pass of the grid.  The waves that take a second query meet the stale-LDS
    sequences: full -> empty, full -> one valid, one valid -> full; every other wave has one query"""
    cap = grid_cap_queries(cus)
    n_q = cap + 3
    counts = np.random.default_rng(cus).integers(0, 5, n_q)
    counts[[0, 1, 2]] = (4, 4, 1)
    counts[[cap, cap + 1, cap + 2]] = (0, 1, 4)
    return random_case(f"past-cap-{cus}", 700, n_q, 500, 4, 3, 15, counts=counts, pads=PADS, cap=cap)


# -- degenerate supports ----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def single_support_case():
    return random_case("ns1", 801, 11, 1, 6, 4, 15, pads=PADS)


@lru_cache(maxsize=None)
def empty_support_case():
    return random_case("ns0", 802, 7, 0, 6, 4, 15)


# -- exact geometry ---------------------------------------------------------------------------------------------------
LATTICE = 1.0 / 16
EXACT_EXTENT = 5 * LATTICE
EXACT_KP = np.array([(0, 0, 0), (3, 4, 0), (0, -3, 4), (-4, 0, 3), (0, 0, -5)], np.float64) * LATTICE   # all at 0 or extent from the origin
# offsets from a kernel point (lattice units, 3-4-5 and 6-8-10 triples): ON it, at EXTENT, at TWICE the extent
ON, AT_EXTENT, TWICE = "on", "extent", "twice"
EXACT_OFFSETS = {ON: [(0, 0, 0)], AT_EXTENT: [(5, 0, 0), (0, 3, -4), (-4, 0, 3)], TWICE: [(0, -10, 0), (6, 8, 0), (0, 8, -6)]}


def exact_case(nonfinite=False):
    """Every query has ONE valid neighbour, at a scattered slot of a row of 5, placed at query + K[k] + offset: d to K[k] is 0,
    extent or 2 extent exactly (designated: rows of (query, k, kind)).  Support rows 0 and n_s - 1 are referenced by nobody: only a
    padded entry taken for an index (clamped, wrapped) would read them.

    nonfinite: NaN and +-Inf feature rows - reached with w == 1 (ON), with w exactly 0 (AT_EXTENT, TWICE) and rows 0 / n_s - 1,
    which are NaN and reached by padding only."""
    rng = np.random.default_rng(31)
    designated, query, support, rows = [], [], [np.zeros(3)], []
    for kind, offsets in EXACT_OFFSETS.items():
        for k in range(len(EXACT_KP)):
            for off in offsets:
                q = rng.integers(0, 64, 3) * LATTICE
                designated.append((len(query), k, kind))
                query.append(q)
                rows.append(len(support))
                support.append(q + EXACT_KP[k] + np.array(off) * LATTICE)
    support.append(np.full(3, 2.0))
    n_q, n_s, n_nb, c = len(query), len(support), 5, 6
    nb = np.array([-1, n_s, INT_MAX, INT_MIN], np.int64)[rng.integers(0, 4, (n_q, n_nb))]
    nb[np.arange(n_q), rng.integers(0, n_nb, n_q)] = rows
    x = rng.standard_normal((n_s, c), dtype=np.float32)
    marks = dict(designated=tuple(designated))
    if nonfinite:
        x[0], x[-1] = np.nan, np.nan
        poison = {}
        for kind in EXACT_OFFSETS:
            qs = [i for i, k, kd in designated if kd == kind]
            poison[kind] = qs[:3]
            x[rows[qs[0]], :] = np.nan
            x[rows[qs[1]], ::2] = np.inf
            x[rows[qs[1]], 1::2] = -np.inf
            x[rows[qs[2]], 0], x[rows[qs[2]], 1], x[rows[qs[2]], 2] = np.inf, -np.inf, np.nan
        marks["poison"] = poison
    return Case("exact-nonfinite" if nonfinite else "exact", np.array(query), np.array(support), nb.astype(np.int32), x, EXACT_KP,
                EXACT_EXTENT, rng.standard_normal((n_q, len(EXACT_KP), c), dtype=np.float32), **marks)


# -- the rest ---------------------------------------------------------------------------------------------------------
OFF_ORIGIN = (1000.0, -2000.0, 500.0)


@lru_cache(maxsize=None)
def off_origin_case():
    return random_case("off-origin", 901, 60, 120, 24, 5, 15, shift=OFF_ORIGIN)


@lru_cache(maxsize=None)
def duplicate_row_case():
    """row 3 holds one index 40 times; rows 4 and 5 hold two and three indices in turn; the others are random"""
    base = random_case("dup-row", 902, 20, 64, 40, 5, 15, counts=[40] * 20)
    nb = base.nb.copy()
    nb[3] = 17
    nb[4] = np.tile([5, 9], 20)
    nb[5] = np.tile([5, 9, 17, 9], 10)
    return base.replace(nb=nb)


@lru_cache(maxsize=None)
def one_support_row_case():
    """every slot of every query points at support row 0: hits = n_q * n_nb atomics on each float of one row"""
    base = random_case("one-row", 903, 48, 32, 16, 5, 15, counts=[16] * 48)
    return base.replace(nb=np.zeros_like(base.nb))


@lru_cache(maxsize=None)
def plain_case():
    """the case the misaligned and permuted launches run: 41 queries, scattered valid entries, c odd"""
    return random_case("plain", 904, 41, 70, 13, 9, 15, pads=PADS)


def nonfinite_coordinate_case():
    """a NaN and an Inf coordinate in a support point and in a query.  Support 7 (NaN) and 11 (+Inf in x) are in several rows;
    query 3 has a NaN; query 9 has +Inf in x and points at support 11 (Inf - Inf: NaN) and at finite points (infinitely far: 0)"""
    base = random_case("nonfinite-xyz", 905, 40, 60, 8, 4, 15, counts=[8] * 20 + [5] * 20)
    support, query, nb = base.support.copy(), base.query.copy(), base.nb.copy()
    support[7, 1], support[11, 0] = np.nan, np.inf
    query[3, 2], query[9, 0] = np.nan, np.inf
    nb[nb == 7] = 8
    nb[nb == 11] = 12
    nb[[0, 5, 21], [2, 0, 1]] = 7
    nb[[1, 5, 9], [3, 4, 6]] = 11
    return base.replace(query=query, support=support, nb=nb)


def out_of_int32_neighbours(case):
    """int64 neighbours for the operator: the padding replaced by values beyond int32 whose low words are valid indices"""
    nb = case.nb.astype(np.int64)
    pad = ~case.valid
    far = np.array([2 ** 32 + 1, -2 ** 32 + 2, 2 ** 40, -2 ** 40 + 3, 2 ** 31, -2 ** 31 - 1, 2 ** 63 - 1, -2 ** 63], np.int64)
    nb[pad] = far[np.arange(int(pad.sum())) % len(far)]
    return nb


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ---------------------------------------------------------------------------------------------------------------------
class Reference:
    """w, bw [n_q, n_kp, n_nb] (0 at skipped entries); wf, wf_bound [n_q, n_kp, c]; gf, gf_bound [n_s, c]; hits [n_s].
    Non-finite elements of wf / gf are expected bit patterns (NaN, +-Inf), their bounds are not used."""

    def __init__(self, case):
        c = case
        valid = c.valid
        self.valid, self.n_valid = valid, valid.sum(1)
        self.j = np.where(valid, c.nb, 0).astype(np.int64)
        if c.n_s == 0:
            self.w = self.bw = np.zeros((c.n_q, c.n_kp, c.n_nb))
            self.wf = self.wf_bound = np.zeros((c.n_q, c.n_kp, c.c))
            self.gf = self.gf_bound = np.zeros((0, c.c))
            self.hits = np.zeros(0, np.int64)
            self.r = np.full((c.n_q, c.n_kp, c.n_nb), np.inf)
            return
        S, Q, K, e = c.support.astype(np.float64), c.query.astype(np.float64), c.kp.astype(np.float64), c.extent
        with np.errstate(invalid="ignore", over="ignore"):
            rel = S[self.j] - Q[:, None, :]                                        # [q, n, 3]
            d = np.sqrt(((rel[:, None, :, :] - K[None, :, None, :]) ** 2).sum(-1))  # [q, k, n]
            r = d / e
            w = np.maximum(0.0, 1.0 - r)                                           # NaN stays NaN
            raw = U * (W_A * (np.abs(rel).sum(-1)[:, None, :] + d) / e + W_B)
            bw = np.where(r - 1.0 > raw, 0.0, raw)                                 # both sides clamp: exactly 0
            bw = np.where(np.isinf(r), 0.0, bw)                                    # infinitely far: exactly 0
        v3 = valid[:, None, :]
        self.r = np.where(v3, r, np.inf)
        self.w, self.bw = np.where(v3, w, 0.0), np.where(v3, bw, 0.0)
        xg = np.where(valid[:, :, None], c.x.astype(np.float64)[self.j], 0.0)       # [q, n, c]: a skipped entry reads no row
        g = c.g.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            self.wf = np.einsum("qkn,qnc->qkc", self.w, xg)
            self.wf_bound = np.einsum("qkn,qnc->qkc", self.bw + self.n_valid[:, None, None] * U * np.abs(self.w), np.abs(xg))
            a = np.einsum("qkn,qkc->qnc", self.w, g)
            A = np.einsum("qkn,qkc->qnc", np.abs(self.w), np.abs(g))
            D = np.einsum("qkn,qkc->qnc", self.bw, np.abs(g))
            rows = self.j[valid]
            self.hits = np.bincount(rows, minlength=c.n_s)
            self.gf, SA, SD = np.zeros((c.n_s, c.c)), np.zeros((c.n_s, c.c)), np.zeros((c.n_s, c.c))
            np.add.at(self.gf, rows, a[valid])
            np.add.at(SA, rows, A[valid])
            np.add.at(SD, rows, D[valid])
            self.gf_bound = (c.n_kp + self.hits)[:, None] * U * SA + SD
        for arr in (self.w, self.bw, self.wf, self.wf_bound, self.gf, self.gf_bound):
            arr.setflags(write=False)


class OutsideBound(AssertionError):
    pass


def fraction_of_bound(got, want, bound, what):
    """largest |got - want| / bound over the elements with a finite want and bound > 0; raises OutsideBound where a finite
    element misses its bound (bound 0: must be equal; a NaN misses it) or a non-finite want is not reproduced exactly"""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return 0.0
    finite = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        same = (np.isnan(want) & np.isnan(got)) | (got == want)
        err = np.abs(got - want)
        bad = np.where(finite, ~(err <= bound), ~same)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise OutsideBound(f"{what}: {int(bad.sum())} of {got.size} elements outside the bound, first at {i}: got {got[i]!r} "
                           f"want {want[i]!r} bound {bound[i]!r}")
    live = finite & (bound > 0)
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def check_forward(got, case, what=""):
    """wf of the forward launcher -> fraction of the bound used"""
    ref = case.reference()
    got = np.asarray(got).reshape(case.n_q, case.n_kp, case.c)
    empty = ref.n_valid == 0
    assert not got[empty].any() and not np.signbit(got[empty]).any(), f"{what}{case.name}: a query without neighbours must give +0"
    return fraction_of_bound(got, ref.wf, ref.wf_bound, f"{what}{case.name} forward")


def check_backward(got, case, what=""):
    """grad_feat of the backward launcher (into a zeroed buffer) -> fraction of the bound used"""
    ref = case.reference()
    got = np.asarray(got)
    untouched = ref.hits == 0
    assert not got[untouched].any(), f"{what}{case.name}: a support row nobody points at must stay exactly 0"
    return fraction_of_bound(got, ref.gf, ref.gf_bound, f"{what}{case.name} backward")


def check_exact_geometry(got, case):
    """the bit-exact promises of exact_case(): ON gives the feature row bit for bit, AT_EXTENT and TWICE give +0"""
    got = np.asarray(got).reshape(case.n_q, case.n_kp, case.c)
    ref = case.reference()
    for i, k, kind in case.marks["designated"]:
        (n,) = np.flatnonzero(ref.valid[i])
        row = case.x[ref.j[i, n]]
        if kind == ON:
            assert ref.w[i, k, n] == 1.0
            fin = np.isfinite(row)
            assert np.array_equal(got[i, k][fin].view(np.int32), row[fin].view(np.int32)) and np.array_equal(got[i, k], row, equal_nan=True), \
                f"{case.name}: query {i} on K[{k}]: not the feature row"
        elif np.isfinite(row).all():
            assert ref.w[i, k, n] == 0.0 and ref.r[i, k, n] == (1.0 if kind == AT_EXTENT else 2.0)
            assert not got[i, k].any() and not np.signbit(got[i, k]).any(), f"{case.name}: query {i}, K[{k}] at {kind}: not +0"


# ---------------------------------------------------------------------------------------------------------------------
# the same formulas in plain fp32 numpy (the reference side of the margin check), and wrong variants of them
# ---------------------------------------------------------------------------------------------------------------------
def influences_f32(case, kp=None, clamp=True, valid=None):
    """-> (w [n_q, n_kp, n_nb] fp32, 0 at skipped entries; d [n_q, n_kp, n_nb] fp32): every operation rounded on its own"""
    valid = case.valid if valid is None else valid
    j = np.where(valid, case.nb, 0).astype(np.int64)
    kp = case.kp if kp is None else kp
    with np.errstate(invalid="ignore", over="ignore"):
        rel = case.support[j] - case.query[:, None, :]
        diff = rel[:, None, :, :] - kp[None, :, None, :]
        sq = diff * diff
        d = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        w = np.float32(1) - d / np.float32(case.extent)
        if clamp:
            w = np.maximum(np.float32(0), w)
    assert w.dtype == np.float32
    return np.where(valid[:, None, :], w, np.float32(0)), d


def aggregate_f32(case, w, valid=None):
    """-> (wf, gf) fp32 from fp32 influences, in the kernels' order: neighbours in index order (forward), kernel points in order
    then one addition per (query, slot) (backward); product and sum rounded separately"""
    valid = case.valid if valid is None else valid
    j = np.where(valid, case.nb, 0).astype(np.int64)
    xg = np.where(valid[:, :, None], case.x[j], np.float32(0))
    wf = np.zeros((case.n_q, case.n_kp, case.c), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(case.n_nb):
            wf = np.where(valid[:, n, None, None], wf + w[:, :, n, None] * xg[:, None, n, :], wf)
        acc = np.zeros((case.n_q, case.n_nb, case.c), np.float32)
        for k in range(case.n_kp):
            acc = acc + w[:, k, :, None] * case.g[:, k, None, :]
        gf = np.zeros((case.n_s, case.c), np.float32)
        np.add.at(gf, j[valid], acc[valid])
    assert wf.dtype == np.float32 and gf.dtype == np.float32
    return wf, gf


def evaluate_f32(case):
    if case.n_s == 0:
        return np.zeros((case.n_q, case.n_kp, case.c), np.float32), np.zeros((0, case.c), np.float32)
    return aggregate_f32(case, influences_f32(case)[0])


def variant_next_kernel_point(case):
    """the influence taken against kernel point k + 1 (cyclically)"""
    return aggregate_f32(case, influences_f32(case, kp=np.roll(case.kp, -1, axis=0))[0])


def small_neighbour(case, floor=1e-3):
    """(query, slot) of the valid neighbour whose largest influence is the smallest one above `floor`"""
    ref = case.reference()
    top = np.where(ref.valid, ref.w.max(1), np.inf)
    top[top < floor] = np.inf
    i, n = np.unravel_index(np.argmin(top), top.shape)
    assert np.isfinite(top[i, n])
    return int(i), int(n)


def variant_dropped_neighbour(case):
    """one valid neighbour of small weight (see small_neighbour) skipped"""
    valid = case.valid.copy()
    valid[small_neighbour(case)] = False
    return aggregate_f32(case, influences_f32(case, valid=valid)[0], valid=valid)


def variant_unclamped(case):
    return aggregate_f32(case, influences_f32(case, clamp=False)[0])


def variant_quotient_forward(case, t):
    """the forward's quotient t / c one too small at output float t (k >= 1): the lane reads w[k - 1] and, with ch + c for ch,
    the NEXT neighbour's staged row (past the last one: stale LDS, taken as 0)"""
    w = influences_f32(case)[0]
    wf, gf = aggregate_f32(case, w)
    k, ch = divmod(t, case.c)
    assert k >= 1
    valid = case.valid
    order = np.argsort(~valid, axis=1, kind="stable")                     # the compaction: valid slots first, order kept
    j = np.take_along_axis(np.where(valid, case.nb, 0), order, 1).astype(np.int64)
    wk = np.take_along_axis(w[:, k - 1, :], order, 1)
    nv = valid.sum(1)
    acc = np.zeros(case.n_q, np.float32)
    for n in range(case.n_nb):
        staged = np.where(n + 1 < nv, case.x[j[:, min(n + 1, case.n_nb - 1)], ch], np.float32(0))
        acc = np.where(n < nv, acc + wk[:, n] * staged, acc)
    wf = wf.copy()
    wf[:, k, ch] = acc
    return wf, gf


def variant_quotient_backward(case, t):
    """the backward's quotient t / c one too small at slot float t (n >= 1): the contribution of (compacted neighbour n,
    channel ch) is computed for neighbour n - 1 with the next kernel point's gradient row and added to float ch + c of ITS row -
    modelled by what is certain: the right element misses its contribution (queries with more than n valid neighbours)"""
    w = influences_f32(case)[0]
    n, ch = divmod(t, case.c)
    assert n >= 1
    valid = case.valid
    slot = np.argsort(~valid, axis=1, kind="stable")[:, n]                 # the original slot of compacted neighbour n
    hit = np.flatnonzero(valid.sum(1) > n)
    j = np.where(valid, case.nb, 0).astype(np.int64)
    acc = np.zeros((case.n_q, case.n_nb, case.c), np.float32)
    for k in range(case.n_kp):
        acc = acc + w[:, k, :, None] * case.g[:, k, None, :]
    acc[hit, slot[hit], ch] = 0
    gf = np.zeros((case.n_s, case.c), np.float32)
    np.add.at(gf, j[valid], acc[valid])
    return aggregate_f32(case, w)[0], gf


def variant_quotient_influence(case, t, n_valid):
    """stage_query's quotient t / n_valid one too small at t, for the queries with that valid count: the influence of
    (k, n) = divmod(t, n_valid) is stored at w[k - 1][n + n_valid], which nobody reads, and w[k][n] keeps what the LDS held -
    taken as 0"""
    k, n = divmod(t, n_valid)
    valid = case.valid
    w = influences_f32(case)[0].copy()
    order = np.argsort(~valid, axis=1, kind="stable")
    rows = np.flatnonzero(valid.sum(1) == n_valid)
    assert len(rows)
    w[rows, k, order[rows, n]] = 0
    return aggregate_f32(case, w)
