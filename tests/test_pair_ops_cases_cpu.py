"""CPU: the cases of tests/pair_ops_cases.py are what they claim, the C oracle meets the derived bounds on every one of them
(so a correct fp32 implementation can), and deliberately wrong numpy variants miss them (so the helpers have teeth).  No HIP."""
import numpy as np
import pytest

from oracle import pointops_ref as ref
from tests import pair_ops_cases as C

BLOCK_HEADS = [h for h in C.HEADS if h > 4]


def _key_bits(n):  # csrc/misc.hip key_bits
    b = 1
    while (1 << b) < n:
        b += 1
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the softmax table
# ---------------------------------------------------------------------------------------------------------------------
def test_kernel_of_is_the_launchers_condition():
    for N in (1, 3, 4, 5, 199, 200, 19999, 20000, 20001, 10 ** 6):
        for h in range(1, 130):
            few_rows_many_heads = N < 20000 and h > 4
            assert (C.kernel_of(N, h) == C.BLOCK) == few_rows_many_heads
            p = C.hp(h)
            assert p in (1, 2, 4, 8, 16, 32, 64) and (p >= h or p == 64) and (p == 1 or p // 2 < h)
            assert C.ppw(h) * p == 64
            assert C.stride(N, h) == C.ppw(h) * (4 if few_rows_many_heads else 1)
            assert C.trips(h) == len(range(0, h, p))


def test_table_covers_every_region():
    regions = {C.region(N, h) for h, N in C.SOFTMAX_CASES}
    want = {(C.WAVE, p, 1) for p in (1, 2, 4, 8, 16, 32, 64)} | {(C.WAVE, 64, 2)}
    want |= {(C.BLOCK, p, 1) for p in (8, 16, 32, 64)} | {(C.BLOCK, 64, 2)}
    assert regions == want
    # at h <= 4 both N run the wave kernel (the block kernel is unreachable there); at h > 4 the two N are the two kernels
    for h in C.HEADS:
        kernels = [C.kernel_of(N, h) for N in C.ROWS]
        assert kernels == ([C.WAVE, C.WAVE] if h <= 4 else [C.BLOCK, C.WAVE])
    # the widths the older tests never reached: a butterfly that starts at bit 3, 4 or 5, none at all, and a second trip over
    # a partial group (1 and 36 heads of 64)
    assert {C.hp(h) for h in BLOCK_HEADS} == {8, 16, 32, 64}
    assert [h % 64 for h in C.HEADS if C.trips(h) == 2] == [1, 36]
    assert 33 in C.HEADS and C.hp(33) == 64 and C.trips(33) == 1  # a single, partial group


@pytest.mark.parametrize("hn", C.SOFTMAX_CASES, ids=C.softmax_id)
def test_softmax_case_is_what_it_claims(hn):
    h, N = hn
    c = C.softmax_case(h, N)
    s = C.stride(N, h)
    assert c.x.shape == c.gy.shape == (c.M, h) and c.x.dtype == c.gy.dtype == np.float32 and c.offsets.shape == (N + 1,)
    assert c.offsets[0] == 0 and c.offsets[-1] == c.M and c.M < 8000 and 20 <= len(c.rows) <= 45
    lens = np.diff(c.offsets)
    live = np.flatnonzero(lens)
    assert sorted(live.tolist()) == sorted(r.row for r in c.rows)
    assert set(range(4)) <= set(live) and set(range(N - 4, N)) <= set(live)  # the first and the last workgroup of the wave kernel
    gaps = np.diff(live[4:-4])
    assert {1, 2, 3} <= set(gaps.tolist())  # adjacent rows, and one or two empty rows between
    # every length boundary for every family; the long rows where a dropped pair weighs least
    for fam in C.FAMILIES:
        got = sorted(r.length for r in c.rows if r.family == fam)
        assert got == sorted(C.short_lengths(N, h) + list(C.LONG.get(fam, ()))), (fam, got)
    assert {1, s, s + 1, 2 * s + 1, 1024, 1500} <= {r.length for r in c.rows} and (s == 1 or s - 1 in {r.length for r in c.rows})
    wide_at = set()
    beyond_first_pass = False
    for r in c.rows:
        x = c.x[r.start:r.start + r.length]
        if r.family in C.FLAT_LEVEL:
            assert (x == np.float32(C.FLAT_LEVEL[r.family])).all() and np.isfinite(x).all()
        elif r.family == "wide":
            top = x.argmax(0)
            assert (top == top[0]).all() and ((x == x.max(0)).sum(0) == 1).all()
            assert r.length == 1 or ((x.max(0) - x.min(0)) == 80).all()
            last_pass = ((r.length - 1) // s) * s
            wide_at |= {"first"} if top[0] == 0 else set()
            wide_at |= {"last"} if top[0] == r.length - 1 and r.length > 1 else set()
            wide_at |= {"partial"} if top[0] >= last_pass and (r.length % s or s == 1) and r.length > s else set()
        elif r.family == "dominant":
            srt = np.sort(x, 0)
            assert r.length == 1 or (srt[-1] - srt[-2] > 90).all()
            beyond_first_pass |= r.length > s and bool((x.argmax(0)[::2] == r.length - 1).all())  # the even heads
        elif r.family == "masked":
            assert np.isfinite(x).any(0).all() and (r.length == 1 or np.isneginf(x).any(0).all())
            assert not np.isnan(x).any() and not np.isposinf(x).any()
        else:
            assert r.family == "normal" and np.isfinite(x).all()
    assert wide_at == {"first", "last", "partial"}, wide_at
    assert beyond_first_pass


def test_nonfinite_variants_poison_three_heads_of_three_rows():
    for h, N in C.NONFINITE_BASES:
        c = C.softmax_case(h, N)
        x, poisoned = C.nonfinite_variant(c)
        changed = ~((x == c.x) | (np.isnan(x) & np.isnan(c.x)))
        assert changed.any() and not (changed & ~poisoned).any()
        rows = [r for r in c.rows if poisoned[r.start:r.start + r.length].any()]
        assert len(rows) == 3 and poisoned.any(0).sum() == 3
        want = C.softmax_f64(x, c.offsets)
        assert np.isnan(want[poisoned]).all() and not np.isnan(want[~poisoned]).any()
    assert {C.kernel_of(N, h) for h, N in C.NONFINITE_BASES} == {C.WAVE, C.BLOCK}


# ---------------------------------------------------------------------------------------------------------------------
# the bounds are reachable: the C oracle (a sequential fp32 loop) meets them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hn", C.SOFTMAX_CASES, ids=C.softmax_id)
def test_oracle_meets_the_softmax_bounds(hn):
    c = C.softmax_case(*hn)
    y = ref.segment_softmax(c.x, c.offsets)
    f = C.check_softmax_fwd(y, c, "oracle ")
    b = C.check_softmax_bwd(ref.segment_softmax_backward(y, c.gy, c.offsets), y, c, "oracle ")
    assert f <= 1 and b <= 1


def test_oracle_meets_the_softmax_bounds_over_lengths_and_spans():
    """lengths 1 .. 1500 and spans 1 .. 200: a sequential fp32 sum, the least accurate correct order, stays inside"""
    rng = np.random.default_rng(3)
    worst_f = worst_b = 0.0
    for span in (1, 10, 80, 200):
        lens = np.array([1, 2, 7, 63, 64, 65, 300, 1024, 1500])
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        x = (-span * rng.random((int(offsets[-1]), 2))).astype(np.float32)
        for s, e in zip(offsets[:-1], offsets[1:]):
            x[s] = 0
            x[e - 1] = -span if e - s > 1 else 0
        gy = rng.standard_normal(x.shape, dtype=np.float32)
        y = ref.segment_softmax(x, offsets)
        want, bound = C.softmax_fwd_bound(x, offsets)
        worst_f = max(worst_f, C.fraction_of_bound(y, want, bound, f"span {span} forward"))
        want, bound = C.softmax_bwd_bound(y, gy, offsets)
        worst_b = max(worst_b, C.fraction_of_bound(ref.segment_softmax_backward(y, gy, offsets), want, bound, f"span {span} backward"))
    assert 0 < worst_f < 0.5 and 0 < worst_b < 0.5, (worst_f, worst_b)  # reachable with room, not vacuous


@pytest.mark.parametrize("c", C.GATHER_C)
def test_oracle_meets_the_gather_bounds(c):
    for g in C.group_cases(c):
        assert np.array_equal(ref.grouping(g.inp, g.idx), C.grouping_f64(g.inp, g.idx).astype(np.float32)), g.name
        C.check_grouping_bwd(ref.grouping_backward(g.go, g.idx, C.SRC_ROWS), g, g.name)
    for g in C.gather_cases(c):
        n, k = g.idx.shape
        out = g.preset.copy()
        ref.lib().oracle_interpolation_forward(n, c, k, ref._p(g.inp), ref._p(g.idx), ref._p(g.weight), ref._p(out))
        C.check_gather_fwd(out, g, g.name)
        C.check_gather_bwd(ref.interpolation_backward(g.go, g.idx, g.weight, C.SRC_ROWS), g, g.name)


# ---------------------------------------------------------------------------------------------------------------------
# the helpers have teeth
# ---------------------------------------------------------------------------------------------------------------------
def _faulty_softmax(c, fault):
    """the kernels' arithmetic in fp32 numpy with one defect"""
    s, per_wave = C.stride(c.N, c.h), C.ppw(c.h)
    out = np.zeros_like(c.x)
    with np.errstate(all="ignore"):
        for r in c.rows:
            x = c.x[r.start:r.start + r.length]
            p = np.arange(r.length)
            summed = np.ones(r.length, bool)
            if fault == "drop_last_pair":
                summed = p < r.length - 1
            elif fault == "lose_a_wave_partial":  # block kernel: the pairs of wave 3 never reach the sum
                summed = (p % s) // per_wave != 3
            mx = (x[p < s] if fault == "first_pass_max" else x).max(0)
            ex = np.exp(x - mx)
            y = ex / ex[summed].sum(0, dtype=np.float32)
            if fault == "skip_second_trip":
                y[:, 64:] = 0
            assert y.dtype == np.float32
            out[r.start:r.start + r.length] = y
    return out


def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_helper_accepts_the_faultless_emulation():
    for hn in C.SOFTMAX_CASES:
        c = C.softmax_case(*hn)
        C.check_softmax_fwd(_faulty_softmax(c, None), c, "emulation ")


@pytest.mark.parametrize("fault,applies", [
    ("drop_last_pair", lambda N, h: True),
    ("lose_a_wave_partial", lambda N, h: C.kernel_of(N, h) == C.BLOCK),
    ("first_pass_max", lambda N, h: True),
    ("skip_second_trip", lambda N, h: C.trips(h) == 2),
])
def test_softmax_helper_rejects(fault, applies):
    cases = [hn for hn in C.SOFTMAX_CASES if applies(hn[1], hn[0])]
    assert cases
    for hn in cases:  # every case of every region the fault applies to, not just one
        c = C.softmax_case(*hn)
        assert _rejects(C.check_softmax_fwd, _faulty_softmax(c, fault), c), (fault, c.name)


def test_softmax_backward_helper_rejects_a_dropped_pair():
    for hn in C.SOFTMAX_CASES:
        c = C.softmax_case(*hn)
        y = ref.segment_softmax(c.x, c.offsets)
        gx = np.zeros_like(y)
        for r in c.rows:
            ys, gs = y[r.start:r.start + r.length], c.gy[r.start:r.start + r.length]
            gx[r.start:r.start + r.length] = ys * (gs - (ys[:-1] * gs[:-1]).sum(0, dtype=np.float32))
        assert _rejects(C.check_softmax_bwd, gx, y, c), c.name


def _faulty_csc(c, fault):
    """csc_finish_kernel after the sort, in numpy: the head fill per pair, the tail fill after the last one"""
    if fault == "unstable":  # descending pair ids inside a key
        order = np.lexsort((-np.arange(c.M), c.index_1))
    else:
        order = np.argsort(c.index_1, kind="stable")
    keys = c.index_1[order]
    offsets = np.full(c.n_keys + 1, -1, np.int32)
    for t in range(c.M):
        offsets[(keys[t - 1] if t else -1) + 1:keys[t] + 1] = t
    offsets[keys[-1] + (2 if fault == "tail_off_by_one" else 1):] = c.M
    offsets[c.n_keys] = c.M
    return offsets, order.astype(np.int32), c.index_0[order]


def _same_csc(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("N", C.CSC_ROWS)
def test_csc_equality_rejects_wrong_builds(N):
    unstable = tail = 0
    for c in C.csc_cases(N):
        want = C.csc_ref(c.index_0, c.index_1, c.n_keys)
        assert _same_csc(_faulty_csc(c, None), want), c.name
        repeats = len(np.unique(c.index_1)) < c.M
        assert _same_csc(_faulty_csc(c, "unstable"), want) == (not repeats), c.name
        unstable += repeats
        last_unused = c.index_1.max() < c.n_keys - 1  # unused keys at the end: the first of them is skipped
        assert _same_csc(_faulty_csc(c, "tail_off_by_one"), want) == (not last_unused), c.name
        tail += last_unused
    assert tail > 0 and (unstable > 0 or N == 1)
    if N == 1:  # one query row still has repeated keys once there are two pairs
        assert any(len(np.unique(c.index_1)) < c.M for c in C.csc_cases(1))


# ---------------------------------------------------------------------------------------------------------------------
# the CSC / CSR tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.CSC_ROWS)
def test_csc_cases_are_what_they_claim(N):
    cases = C.csc_cases(N)
    assert {c.M for c in cases} == set(C.CSC_PAIRS)
    assert {c.mode for c in cases} == ({"equal", "sharded"} if N == 1 else set(C.CSC_KEY_MODES))
    for c in cases:
        assert c.n_keys == C.csc_n_keys(N, c.mode) >= 1 and (c.mode != "fewer" or c.n_keys < N)
        assert c.offsets.shape == (N + 1,) and c.offsets[0] == 0 and c.offsets[-1] == c.M == len(c.index_1)
        assert 0 <= c.index_1.min() and c.index_1.max() < c.n_keys
        assert np.array_equal(c.index_0, C.csr_expand_ref(c.offsets))
        used = np.unique(c.index_1)
        lens = np.diff(c.offsets)
        if N >= 5:
            assert lens[0] == lens[N // 2] == lens[-1] == 0
        if c.use == "no_first":
            assert used[0] > 0 and used[-1] == c.n_keys - 1
        elif c.use == "no_last":
            assert used[-1] < c.n_keys - 1 and used[0] == 0
        elif c.use == "no_middle":
            third = max(1, c.n_keys // 3)
            assert not ((used >= third) & (used < c.n_keys - third)).any()
            assert c.M < 2 or (used[0] == 0 and used[-1] == c.n_keys - 1)
        elif c.use == "one_key":
            assert len(used) == 1
    assert {u for c in cases for u in [c.use]} >= {"random", "one_key"}
    if N >= 3:
        assert {c.use for c in cases} == set(C.CSC_KEY_USES)


def test_csc_table_crosses_the_radix_bit_boundaries():
    bits = {_key_bits(c.n_keys) for N in C.CSC_ROWS for c in C.csc_cases(N)}
    assert {1, 2, 3, 4, 7, 8, 9, 10} <= bits
    n_keys = {c.n_keys for N in C.CSC_ROWS for c in C.csc_cases(N)}
    assert {255, 256, 257} <= n_keys and {1, 2, 3, 4, 5} <= n_keys  # both sides of 2^8, and the smallest


@pytest.mark.parametrize("name", sorted(C.MATCH_LENS))
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_match_mutations_are_single_defects(name, dtype):
    offsets, index = C.match_list(name, dtype)
    lens = np.diff(offsets)
    assert set(lens.tolist()) == {0, 1, 63, 64, 65, 1500} and index.dtype == dtype
    assert 0 in lens[1:-1].tolist()  # an empty segment in the middle of a matching list
    assert np.array_equal(index, np.repeat(np.arange(len(lens)), lens))
    muts = C.match_mutations(name, dtype)
    names = [m[0] for m in muts]
    assert len(set(names)) == len(names)
    big = int(np.flatnonzero(lens == 1500)[0])
    assert {f"pair_{p}_of_{big}" for p in (63, 64, 65)} <= set(names)
    assert {"offsets_0", "offsets_N_short", "offsets_N_long", "offsets_swapped"} <= set(names)
    assert {f"{end}_of_{i}" for i in np.flatnonzero(lens) for end in ("first", "last")} <= set(names)
    assert (f"high_word_of_{big}" in names) == (dtype == np.int64)
    for what, o, i in muts:
        assert o.dtype == np.int32 and i.dtype == dtype and o.shape == offsets.shape and i.shape == index.shape
        d_o, d_i = np.flatnonzero(o != offsets), np.flatnonzero(i != index)
        if what == "offsets_swapped":
            assert len(d_i) == 0 and len(d_o) == 2 and d_o[1] == d_o[0] + 1 and o[d_o[0]] == offsets[d_o[1]] and o[d_o[1]] == offsets[d_o[0]]
        else:
            assert len(d_o) + len(d_i) == 1, what
        if what.startswith("pair_"):
            assert d_i[0] - offsets[big] == int(what.split("_")[1])
        if what.startswith("high_word"):
            assert i[d_i[0]].astype(np.int32) == index[d_i[0]]  # right when truncated to 32 bits


# ---------------------------------------------------------------------------------------------------------------------
# the gather tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.GATHER_C)
def test_gather_cases_are_what_they_claim(c):
    groups, gathers = C.group_cases(c), C.gather_cases(c)
    assert {g.idx.shape for g in groups} == {(m, ns) for m in C.GATHER_M for ns in C.GATHER_NSAMPLE}
    assert {g.idx.shape for g in gathers} == {(n, k) for n in C.GATHER_M for k in C.GATHER_K}
    for g in groups + gathers:
        fam = g.name.split("-")[3]
        assert g.inp.shape == (C.SRC_ROWS, c) and g.idx.dtype == np.int32 and 0 <= g.idx.min() and g.idx.max() < C.SRC_ROWS
        counts = np.bincount(g.idx.reshape(-1), minlength=C.SRC_ROWS)
        if fam == "same":
            assert counts.max() == g.idx.size and (counts > 0).sum() == 1
        elif fam == "identity":
            assert np.array_equal(g.idx.reshape(-1), np.arange(g.idx.size) % C.SRC_ROWS) and (g.idx.size > C.SRC_ROWS or counts.max() == 1)
        elif fam == "ends":
            assert counts[C.UNREFERENCED] == 0 and counts[C.SRC_ROWS - 1] > 0 and (g.idx.size == 1 or counts[0] > 0)
        if g.idx.size > 4 * C.SRC_ROWS and fam != "identity":
            assert counts.max() > 2  # repeats abound
    kinds = {g.name.split("-")[4] for g in gathers}
    assert kinds == set(C.WEIGHT_KINDS)
    for g in gathers:
        kind = g.name.split("-")[4]
        if kind == "signs":
            assert g.idx.size < 4 or ((g.weight > 0).any() and (g.weight < 0).any())
        else:
            assert (g.weight >= 0).all() and np.allclose(g.weight.sum(1)[1::2], 1, atol=1e-5)
            assert (kind == "zero") == bool((g.weight == 0).any())
    assert sum(bool(g.preset.any()) for g in gathers) == 1


def test_gather_helpers_reject_a_lost_contribution():
    g = next(x for x in C.group_cases(3) if x.name == "c3-ns16-m1-same")
    want, _, _ = C.grouping_bwd_f64(g.go, g.idx, C.SRC_ROWS)
    C.check_grouping_bwd(want.astype(np.float32), g, g.name)
    lost = want.copy()
    lost[17] -= g.go[0, 9]  # one of 16 contributions to the row
    assert _rejects(C.check_grouping_bwd, lost.astype(np.float32), g, g.name)
    unref = want.astype(np.float32)
    unref[3, 0] = np.float32(1e-30)  # a row nobody references must stay exactly zero
    assert _rejects(C.check_grouping_bwd, unref, g, g.name)
    w = next(x for x in C.gather_cases(3) if x.name == "c3-k8-n1-same-invdist")
    want, _, _ = C.gather_bwd_f64(w.go, w.idx, w.weight, C.SRC_ROWS)
    C.check_gather_bwd(want.astype(np.float32), w, w.name)
    lost = want.copy()
    lost[17] -= w.go[0] * w.weight[0, 7]
    assert _rejects(C.check_gather_bwd, lost.astype(np.float32), w, w.name)
    fused = C.gather_fwd_f64(w.inp, w.idx, w.weight, w.preset)[0].astype(np.float32)  # right to the last bit of float64, not the kernel's order
    assert _rejects(C.check_gather_fwd, fused, w, w.name)
