"""Cases, float64 references and derived error bounds for the oldest operators: the segment softmax (csrc/softmax.hip), the row
gathers (grouping / interpolation) and the CSR <-> CSC helpers (csrc/misc.hip).  numpy only; tests/test_pair_ops_cases_cpu.py
proves the cases are what they claim and that the bounds are met by the C oracle and missed by wrong variants,
tests/test_pair_ops_hip.py runs them on the device.

The softmax launcher picks its kernel from (N, h) alone (csrc/softmax.hip, few_rows_many_heads):

    N <  20000 and h > 4     seg_softmax_*_block_kernel   one workgroup per row, 4 * ppw pairs per pass, partials through LDS
    otherwise                seg_softmax_*_kernel         one wave per row, ppw pairs per pass, 4 rows per workgroup

with hp = next_pow2(h) capped at 64 the lanes one pair's heads occupy, ppw = 64 / hp, and ceil(h / hp) trips of the head loop
(two for h > 64, the second over a partial group).  At h <= 4 the block kernel is unreachable: both N of the table run the wave
kernel there, on 50 and on 5000 workgroups.

Every bound below is in units of u = 2^-24 (fp32 unit roundoff) and is derived in DESIGN.md ("Pair operators: cases and bounds").
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126  # smallest normal fp32: the floor for terms that underflow

# ---------------------------------------------------------------------------------------------------------------------
# the launcher's own conditions, restated
# ---------------------------------------------------------------------------------------------------------------------
WAVE, BLOCK = "wave", "block"
HEADS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 33, 64, 65, 100)
ROWS = (200, 20000)
FAMILIES = ("flat0", "flat_hi", "flat_lo", "normal", "wide", "dominant", "masked")
FLAT_LEVEL = {"flat0": 0.0, "flat_hi": 3e38, "flat_lo": -3e38}
LONG = {"flat0": (1024, 1500), "normal": (1024,), "wide": (1500,)}  # the families that also get the long rows


def hp(h):
    p = 1
    while p < h and p < 64:
        p <<= 1
    return p


def ppw(h):
    return 64 // hp(h)


def kernel_of(N, h):
    return BLOCK if (N < 20000 and h > 4) else WAVE


def stride(N, h):
    """pairs one pass of the row's loop covers"""
    return ppw(h) * (4 if kernel_of(N, h) == BLOCK else 1)


def trips(h):
    return -(-h // hp(h))


def region(N, h):
    """(kernel, lanes per pair, trips of the head loop): what decides which code a launch runs"""
    return kernel_of(N, h), hp(h), trips(h)


def lengths(N, h):
    """the smallest lengths at which a stride or combine error can appear, and the long rows"""
    s = stride(N, h)
    return sorted({1, s - 1, s, s + 1, 2 * s + 1, 1024, 1500} - {0})


def short_lengths(N, h):
    return [n for n in lengths(N, h) if n < 1024]


# ---------------------------------------------------------------------------------------------------------------------
# softmax cases
# ---------------------------------------------------------------------------------------------------------------------
Row = namedtuple("Row", "row start length family")


class SoftmaxCase:
    """x [M, h] fp32 logits, gy [M, h] fp32 upstream gradient, offsets [N + 1] i32; rows: the non-empty rows"""

    def __init__(self, h, N, offsets, x, gy, rows):
        self.name, self.h, self.N = f"h{h}-N{N}", h, N
        self.offsets, self.x, self.gy, self.rows = offsets, x, gy, rows
        self.M = int(x.shape[0])
        for a in (offsets, x, gy):
            a.setflags(write=False)
        self._ref = None

    def reference(self):
        """(want [M, h] f64, bound [M, h] f64) of the forward, computed once and never written to"""
        if self._ref is None:
            want, bound = softmax_fwd_bound(self.x, self.offsets)
            want.setflags(write=False), bound.setflags(write=False)
            self._ref = (want, bound)
        return self._ref


def _wide_position(length, s, role):
    last_pass = ((length - 1) // s) * s
    return {"first": 0, "last": length - 1, "mid": last_pass + (length - 1 - last_pass) // 2}[role]


def _wide_roles(N, h):
    """length -> where the maximum sits: first pair, last pair, or the middle of the last pass (partial wherever the length
    allows one).  Later entries win where lengths coincide (small strides)."""
    s = stride(N, h)
    roles = {}
    for length, role in ((1, "first"), (s - 1, "mid"), (s, "last"), (s + 1, "last"), (2 * s + 1, "first"), (1500, "mid")):
        if length > 0:
            roles[length] = role
    return roles


def _fill(rng, family, length, h, N):
    if family in FLAT_LEVEL:
        return np.full((length, h), FLAT_LEVEL[family], np.float32)
    x = rng.standard_normal((length, h), dtype=np.float32)
    heads = np.arange(h)
    if family == "wide":  # span exactly 80 (length >= 2): the maximum at a chosen pair, one pair 80 below it
        level = ((heads % 5) * 7 - 10).astype(np.float32)
        pos = _wide_position(length, stride(N, h), _wide_roles(N, h)[length])
        x = level + rng.uniform(-79.0, -1.0, (length, h)).astype(np.float32)
        if length >= 2:
            x[(pos + 1 + rng.integers(0, length - 1)) % length] = level - np.float32(80)
        x[pos] = level
    elif family == "dominant":  # one logit 100 above the rest: at the last pair on even heads, anywhere on odd ones
        pos = np.where(heads % 2 == 0, length - 1, rng.integers(0, length, h))
        x[pos, heads] += np.float32(100)
    elif family == "masked":  # -inf next to finite entries: at least one finite and (length >= 2) one masked per head
        mask = rng.random((length, h)) < 0.3
        keep = rng.integers(0, length, h)
        if length >= 2:
            mask[(keep + 1) % length, heads] = True
        mask[keep, heads] = False
        x[mask] = -np.inf
    return np.ascontiguousarray(x, np.float32)


def _row_positions(N, count):
    """rows 0..3 (the four waves of the first workgroup), N-4..N-1 (the last), the rest in the middle with 0, 1 or 2 empty
    rows between them"""
    mid, r = [], N // 4
    for i in range(count - 8):
        mid.append(r)
        r += (1, 3, 2)[i % 3]
    assert r < N - 4
    return [0, 1, 2, 3] + mid + [N - 4, N - 3, N - 2, N - 1]


@lru_cache(maxsize=None)
def softmax_case(h, N):
    rng = np.random.default_rng(1000 * h + N % 1000 + 7)
    plan = [(f, n) for f in FAMILIES for n in short_lengths(N, h)] + [(f, n) for f, ns in LONG.items() for n in ns]
    plan = [plan[i] for i in rng.permutation(len(plan))]
    pos = _row_positions(N, len(plan))
    lens = np.zeros(N, np.int64)
    lens[pos] = [n for _, n in plan]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = np.concatenate([_fill(rng, f, n, h, N) for f, n in plan])
    gy = rng.standard_normal(x.shape, dtype=np.float32)
    rows = tuple(Row(r, int(offsets[r]), n, f) for r, (f, n) in zip(pos, plan))
    return SoftmaxCase(h, N, offsets, x, gy, rows)


SOFTMAX_CASES = [(h, N) for h in HEADS for N in ROWS]


def softmax_id(hn):
    return "h%d-N%d-%s" % (hn[0], hn[1], kernel_of(hn[1], hn[0]))


# the non-finite case: (h, N) of its base cases, one per kernel
NONFINITE_BASES = ((12, 200), (12, 20000), (65, 200))


def nonfinite_variant(case):
    """-> (x with three poisoned (row, head): a NaN, a +inf, only -inf; poisoned [M, h] bool: the elements that must be NaN).
    Every other element must keep the bits it has without the poison."""
    x = case.x.copy()
    poisoned = np.zeros(x.shape, bool)
    s = stride(case.N, case.h)
    rows = [r for r in case.rows if r.family == "normal" and r.length > s][:3]
    assert len(rows) == 3
    for r, head, what in zip(rows, (0, case.h // 2, case.h - 1), ("nan", "inf", "all_ninf")):
        seg = slice(r.start, r.start + r.length)
        if what == "nan":
            x[r.start + r.length // 2, head] = np.nan
        elif what == "inf":
            x[r.start + r.length - 1, head] = np.inf
        else:
            x[seg, head] = -np.inf
        poisoned[seg, head] = True
    return x, poisoned


# ---------------------------------------------------------------------------------------------------------------------
# float64 references and bounds: softmax
# ---------------------------------------------------------------------------------------------------------------------
def _segments(offsets):
    o = np.asarray(offsets, np.int64)
    for i in np.flatnonzero(o[1:] > o[:-1]):
        yield int(i), int(o[i]), int(o[i + 1])


def softmax_f64(x, offsets):
    out = np.zeros(x.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for _, s, e in _segments(offsets):
            xs = x[s:e].astype(np.float64)
            ex = np.exp(xs - xs.max(0))
            out[s:e] = ex / ex.sum(0)
    return out


def softmax_bwd_f64(y, gy, offsets):
    """y * (gy - sum_seg(y * gy)) from a given y"""
    out = np.zeros(y.shape, np.float64)
    for _, s, e in _segments(offsets):
        ys, gs = y[s:e].astype(np.float64), gy[s:e].astype(np.float64)
        out[s:e] = ys * (gs - (ys * gs).sum(0))
    return out


def softmax_fwd_bound(x, offsets):
    """-> (want, bound): |got - want| <= want * (len + span + 8) * 2u + 2^-126 per element; span = max |x - max x| over the
    (segment, head)'s finite entries (a -inf entry is exactly 0 and adds no rounding)"""
    want = softmax_f64(x, offsets)
    bound = np.full(x.shape, TINY)
    with np.errstate(invalid="ignore"):
        for _, s, e in _segments(offsets):
            xs = x[s:e].astype(np.float64)
            d = np.abs(xs - xs.max(0))
            span = np.where(np.isfinite(d), d, 0.0).max(0)
            bound[s:e] = want[s:e] * ((e - s) + span + 8) * 2 * U + TINY
    return want, bound


def softmax_bwd_bound(y, gy, offsets):
    """-> (want, bound) from the device's own fp32 y: |got - want| <= y * (len + 8) * 2u * max_seg |gy| + 2^-126"""
    want = softmax_bwd_f64(y, gy, offsets)
    bound = np.full(y.shape, TINY)
    for _, s, e in _segments(offsets):
        bound[s:e] = np.abs(y[s:e].astype(np.float64)) * ((e - s) + 8) * 2 * U * np.abs(gy[s:e].astype(np.float64)).max(0) + TINY
    return want, bound


def fraction_of_bound(got, want, bound, what, rows=None):
    """largest |got - want| / bound; raises where an element misses its bound (a NaN misses it)"""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        frac = np.abs(got - want) / bound
    bad = ~(frac <= 1.0)
    if bad.any():
        i = np.argwhere(bad)[0]
        where = ""
        if rows is not None:
            hit = [r for r in rows if r.start <= i[0] < r.start + r.length]
            where = f" (row {hit[0].row}, pair {i[0] - hit[0].start} of {hit[0].length}, {hit[0].family})" if hit else " (outside every row)"
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements outside the bound, first at {tuple(i)}{where}: "
                             f"got {got[tuple(i)]!r} want {want[tuple(i)]!r} bound {bound[tuple(i)]!r}")
    return float(frac.max())


def check_softmax_fwd(got, case, what=""):
    want, bound = case.reference()
    masked = np.isneginf(case.x)
    assert not np.asarray(got)[masked].any(), f"{what}{case.name}: a -inf logit must give exactly 0"
    return fraction_of_bound(got, want, bound, f"{what}{case.name} forward", case.rows)


def check_softmax_bwd(got, y, case, what=""):
    want, bound = softmax_bwd_bound(y, case.gy, case.offsets)
    assert not np.asarray(got)[np.asarray(y) == 0].any(), f"{what}{case.name}: the gradient where y == 0 must be exactly 0"
    return fraction_of_bound(got, want, bound, f"{what}{case.name} backward", case.rows)


# ---------------------------------------------------------------------------------------------------------------------
# CSC / CSR
# ---------------------------------------------------------------------------------------------------------------------
def csc_ref(index_0, index_1, n_keys):
    """the key-major view: a stable argsort of index_1 -> (offsets [n_keys + 1], pair [M], query [M]), all i32"""
    order = np.argsort(index_1, kind="stable")
    offsets = np.searchsorted(index_1[order], np.arange(n_keys + 1), side="left")
    return offsets.astype(np.int32), order.astype(np.int32), np.asarray(index_0)[order].astype(np.int32)


def csr_expand_ref(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)


CSC_ROWS = (1, 2, 3, 4, 5, 255, 256, 257)
CSC_PAIRS = (1, 255, 256, 257)
CSC_KEY_MODES = ("equal", "sharded", "fewer")                    # n_keys == N, 2N + 3, N // 2
CSC_KEY_USES = ("random", "no_first", "no_last", "no_middle", "one_key")
EMPTY_ROWS = {1: (), 2: (0,), 3: (1,), 4: (0, 3)}                # N >= 5: the first, the middle and the last row

CscCase = namedtuple("CscCase", "name N n_keys M offsets index_0 index_1 mode use")


def csc_n_keys(N, mode):
    return {"equal": N, "sharded": 2 * N + 3, "fewer": N // 2}[mode]


def csc_case_exists(N, mode, use):
    """`fewer` needs N >= 2; leaving a key out needs a second key, leaving a middle run out a first and a last one too"""
    nk = csc_n_keys(N, mode)
    return nk >= {"random": 1, "one_key": 1, "no_first": 2, "no_last": 2, "no_middle": 3}[use]


def _csc_case(N, mode, use, M):
    nk = csc_n_keys(N, mode)
    rng = np.random.default_rng(N * 100003 + M * 101 + CSC_KEY_MODES.index(mode) * 7 + CSC_KEY_USES.index(use))
    empty = EMPTY_ROWS.get(N, (0, N // 2, N - 1))
    live = np.setdiff1d(np.arange(N), empty)
    lens = np.zeros(N, np.int64)
    lens[live] = rng.multinomial(M, np.full(len(live), 1.0 / len(live)))
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    if use == "random":
        keys = np.arange(nk)
    elif use == "no_first":
        keys = np.arange(1, nk)
    elif use == "no_last":
        keys = np.arange(nk - 1)
    elif use == "no_middle":  # only the first and the last third are used
        keys = np.concatenate([np.arange(max(1, nk // 3)), np.arange(nk - max(1, nk // 3), nk)])
    else:
        keys = np.array([nk // 2])
    index_1 = keys[rng.integers(0, len(keys), M)].astype(np.int32)
    at = int(rng.integers(0, M))  # where the pair list allows it, the far end of the key range is in use: one fill at a time
    if use == "no_first":
        index_1[at] = nk - 1
    elif use == "no_last":
        index_1[at] = 0
    elif use == "no_middle" and M >= 2:
        index_1[at], index_1[(at + 1) % M] = 0, nk - 1
    index_0 = csr_expand_ref(offsets)
    return CscCase(f"N{N}-{mode}-{use}-M{M}", N, nk, M, offsets, index_0, index_1, mode, use)


@lru_cache(maxsize=None)
def csc_cases(N):
    return tuple(_csc_case(N, mode, use, M) for mode in CSC_KEY_MODES for use in CSC_KEY_USES for M in CSC_PAIRS
                 if csc_case_exists(N, mode, use))


# segment lengths 0, 1, 63, 64, 65 and 1500 for expand and matches: an empty segment in the middle / at both ends
MATCH_LENS = {"mid_empty": (1, 63, 0, 64, 65, 1500, 1), "edge_empty": (0, 1500, 0, 0, 65, 64, 63, 1, 0)}


def match_list(name, dtype=np.int32):
    offsets = np.concatenate([[0], np.cumsum(MATCH_LENS[name])]).astype(np.int32)
    return offsets, csr_expand_ref(offsets).astype(dtype)


def match_mutations(name, dtype):
    """-> [(what, offsets, index)]: the matching list with ONE defect each (the swap moves two offsets)"""
    offsets, index = match_list(name, dtype)
    N, M = len(offsets) - 1, len(index)
    out = []

    def wrong_id(what, m, value):
        bad = index.copy()
        bad[m] = value
        out.append((what, offsets, bad))

    for i in range(N):
        s, e = int(offsets[i]), int(offsets[i + 1])
        if e > s:
            wrong_id(f"first_of_{i}", s, i - 1 if i > 0 else 1)     # the previous segment's id
            wrong_id(f"last_of_{i}", e - 1, i + 1)                   # the next segment's id
        if e - s == 1500:
            for p in (63, 64, 65):
                wrong_id(f"pair_{p}_of_{i}", s + p, i + 1)
            if dtype == np.int64:                                     # right in the low word only
                wrong_id(f"high_word_of_{i}", s + 64, i + (1 << 32))
    for what, at, value in (("offsets_0", 0, 1), ("offsets_N_short", N, M - 1), ("offsets_N_long", N, M + 1)):
        bad = offsets.copy()
        bad[at] = value
        out.append((what, bad, index))
    i = next(i for i in range(1, N - 1) if offsets[i] != offsets[i + 1])
    bad = offsets.copy()
    bad[i], bad[i + 1] = offsets[i + 1], offsets[i]
    out.append(("offsets_swapped", bad, index))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# row gathers
# ---------------------------------------------------------------------------------------------------------------------
SRC_ROWS = 50
UNREFERENCED = 25  # the `ends` family leaves this row alone
GATHER_C, GATHER_NSAMPLE, GATHER_M, GATHER_K = (1, 3, 48, 65), (1, 16, 33), (1, 257), (1, 3, 8)
INDEX_FAMILIES = ("random", "identity", "same", "ends")
WEIGHT_KINDS = ("invdist", "zero", "signs")

GroupCase = namedtuple("GroupCase", "name inp idx go")
GatherCase = namedtuple("GatherCase", "name inp idx weight go preset")


def _indices(rng, family, m, j):
    if family == "random":
        idx = rng.integers(0, SRC_ROWS, (m, j))
    elif family == "identity":  # m * j <= 50: every destination has at most one contribution
        idx = (np.arange(m * j) % SRC_ROWS).reshape(m, j)
    elif family == "same":      # one destination takes all m * j contributions
        idx = np.full((m, j), 17)
    else:                       # row 0 and the last row present, one row never referenced
        idx = rng.integers(1, SRC_ROWS - 1, (m, j))
        idx[idx == UNREFERENCED] = UNREFERENCED + 1
        idx.flat[0] = 0
        idx.flat[-1] = SRC_ROWS - 1
    return np.ascontiguousarray(idx, np.int32)


def _weights(rng, kind, n, k):
    if kind == "signs":
        return rng.standard_normal((n, k), dtype=np.float32)
    d = rng.random((n, k), dtype=np.float32) + np.float32(0.01)
    w = np.float32(1) / (d + np.float32(1e-8))
    w = w / w.sum(1, keepdims=True, dtype=np.float32)
    if kind == "zero":
        w[::2, 0] = 0
    return np.ascontiguousarray(w, np.float32)


@lru_cache(maxsize=None)
def group_cases(c):
    out = []
    for ns in GATHER_NSAMPLE:
        for m in GATHER_M:
            for fi, fam in enumerate(INDEX_FAMILIES):
                rng = np.random.default_rng(c * 7919 + ns * 131 + m * 17 + fi)
                out.append(GroupCase(f"c{c}-ns{ns}-m{m}-{fam}", rng.standard_normal((SRC_ROWS, c), dtype=np.float32),
                                     _indices(rng, fam, m, ns), rng.standard_normal((m, ns, c), dtype=np.float32)))
    return tuple(out)


@lru_cache(maxsize=None)
def gather_cases(c):
    out = []
    for k in GATHER_K:
        for n in GATHER_M:
            for fi, fam in enumerate(INDEX_FAMILIES):
                for wi, kind in enumerate(WEIGHT_KINDS):
                    rng = np.random.default_rng(c * 7919 + k * 131 + n * 17 + fi * 3 + wi + 1)
                    out.append(GatherCase(f"c{c}-k{k}-n{n}-{fam}-{kind}", rng.standard_normal((SRC_ROWS, c), dtype=np.float32),
                                          _indices(rng, fam, n, k), _weights(rng, kind, n, k),
                                          rng.standard_normal((n, c), dtype=np.float32), np.zeros((n, c), np.float32)))
    rng = np.random.default_rng(c + 99)  # the forward adds onto what the caller passed
    out.append(GatherCase(f"c{c}-k3-n257-random-signs-preset", rng.standard_normal((SRC_ROWS, c), dtype=np.float32),
                          _indices(rng, "random", 257, 3), _weights(rng, "signs", 257, 3),
                          rng.standard_normal((257, c), dtype=np.float32), rng.standard_normal((257, c), dtype=np.float32)))
    return tuple(out)


def grouping_f64(inp, idx):
    return inp.astype(np.float64)[idx]


def scatter_sum_f64(rows, terms, n_rows):
    """-> (sum, K, S) per destination element: the float64 sum of `terms [T, c]` onto rows `rows [T]`, the number of
    contributions and the sum of their absolute values"""
    c = terms.shape[1]
    total, S = np.zeros((n_rows, c)), np.zeros((n_rows, c))
    np.add.at(total, rows, terms)
    np.add.at(S, rows, np.abs(terms))
    K = np.bincount(rows, minlength=n_rows).astype(np.float64)[:, None] * np.ones(c)
    return total, K, S


def grouping_bwd_f64(go, idx, n_rows):
    return scatter_sum_f64(idx.reshape(-1), go.reshape(idx.size, -1).astype(np.float64), n_rows)


def gather_fwd_f64(inp, idx, weight, preset):
    """-> (want, sum |terms|), the preset among the terms"""
    terms = inp.astype(np.float64)[idx] * weight.astype(np.float64)[:, :, None]
    return preset.astype(np.float64) + terms.sum(1), np.abs(preset.astype(np.float64)) + np.abs(terms).sum(1)


def gather_fwd_f32(inp, idx, weight, preset):
    """the kernel's own order: from the preset, i = 0 .. k-1, every product and every sum rounded to fp32 on its own"""
    o = preset.astype(np.float32).copy()
    for i in range(idx.shape[1]):
        o = o + inp[idx[:, i]] * weight[:, i:i + 1]
    assert o.dtype == np.float32
    return o


def gather_bwd_terms_f32(go, idx, weight):
    """-> (rows [n * k], fp32 products [n * k, c]) in the kernel's term order"""
    n, k = idx.shape
    terms = go[:, None, :] * weight[:, :, None]
    assert terms.dtype == np.float32
    return idx.reshape(-1), terms.reshape(n * k, -1)


def gather_bwd_f64(go, idx, weight, n_rows):
    n, k = idx.shape
    terms = go.astype(np.float64)[:, None, :] * weight.astype(np.float64)[:, :, None]
    return scatter_sum_f64(idx.reshape(-1), terms.reshape(n * k, -1), n_rows)


def check_atomic_sum(got, want, K, S, exact, what, products=False):
    """|got - want| <= K * u * S (twice that where the terms are rounded products); where K <= 1 the bits of `exact`
    (zero for rows nobody references); -> largest fraction of the bound among the elements with K >= 2"""
    got = np.asarray(got)
    one = K <= 1
    assert np.array_equal(got[one], exact[one]), f"{what}: an element with at most one contribution is not exact"
    bound = K * U * S * (2 if products else 1)
    many = ~one
    if not many.any():
        return 0.0
    return fraction_of_bound(got[many], want[many], np.maximum(bound[many], 1e-300), what)


def check_gather_fwd(got, case, what):
    got = np.asarray(got)
    restated = gather_fwd_f32(case.inp, case.idx, case.weight, case.preset)
    assert np.array_equal(got, restated), f"{what}: differs from the fp32 restatement in {int((got != restated).sum())} elements"
    want, S = gather_fwd_f64(case.inp, case.idx, case.weight, case.preset)
    return fraction_of_bound(got, want, np.maximum(case.idx.shape[1] * 2 * U * S, 1e-300), what)


def check_grouping_bwd(got, case, what):
    want, K, S = grouping_bwd_f64(case.go, case.idx, SRC_ROWS)
    return check_atomic_sum(got, want, K, S, want.astype(np.float32), what)


def check_gather_bwd(got, case, what):
    want, K, S = gather_bwd_f64(case.go, case.idx, case.weight, SRC_ROWS)
    rows, terms = gather_bwd_terms_f32(case.go, case.idx, case.weight)
    exact = np.zeros((SRC_ROWS, terms.shape[1]), np.float32)
    exact[rows] = terms  # right where K == 1, unused elsewhere
    return check_atomic_sum(got, want, K, S, exact, what, products=True)


# the operator-level case: P.interpolation onto a batch whose second support element has two points (k = 3: the kNN fills the
# third slot with the element's first row at distance 1e5)
def interpolation_case():
    rng = np.random.default_rng(5)
    xyz = rng.random((42, 3), dtype=np.float32)          # support: 40 points, then 2
    new_xyz = rng.random((90, 3), dtype=np.float32)      # queries: 60 on the first element, 30 on the second
    return dict(xyz=xyz, new_xyz=new_xyz, offset=np.array([40, 42], np.int32), new_offset=np.array([60, 90], np.int32),
                feat=rng.standard_normal((42, 5), dtype=np.float32), k=3)


def interpolation_f64(feat, idx, dist):
    """the wrapper's weights (1 / (d + 1e-8), normalised) and sum in float64 -> (want, bound).  The device computes the weights
    in fp32: d + 1e-8 and the reciprocal (2u), a sum of k positive terms (k - 1)u and a division (u), so each weight is within
    (k + 2)u of the float64 one; the product adds u and the sum of k terms ku: (2k + 3)u, stated as (2k + 6)u of sum |terms|."""
    k = idx.shape[1]
    r = 1.0 / (dist.astype(np.float64) + 1e-8)
    w = r / r.sum(1, keepdims=True)
    terms = feat.astype(np.float64)[idx] * w[:, :, None]
    return terms.sum(1), (2 * k + 6) * U * np.abs(terms).sum(1)
