"""CPU: the table of tests/seg_loss_cases.py is what it claims - every label is what the restated choices of csrc/seg_loss.hip give, the
constants are the source's, every value of every claim is reached for fp32 and for f16 - and it can fail: in the numpy models of one
workgroup the kernel's own indexing stages every element of a tile once, in a word of its own below SL_TILE_WORDS, and forms every
gradient element with its own row's state; each seeded one-line mistake changes the model output of named cases, or is said to be
merely slower; what no model can see is listed with the GPU assertion that sees it.  No HIP."""
import os
import re

import numpy as np
import pytest

from tests import seg_loss_cases as L

TESTS = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(os.path.dirname(TESTS), "stratified_transformer_amd", "csrc", "seg_loss.hip")) as _f:
    SRC = _f.read()


def _one(pattern):
    found = re.findall(pattern, SRC)
    assert len(found) == 1, (pattern, found)
    return found[0]


SL_TILE_WORDS = int(_one(r"constexpr int SL_TILE_WORDS = (\d+) \* (\d+);")[0]) * int(_one(r"constexpr int SL_TILE_WORDS = (\d+) \* (\d+);")[1])
HALF_TYPE = "f16"                                                              # the half type for which every claim value is reached


def _tiles(case, mistake=None):
    """(rows of the tile, how many such tiles) for the distinct tile heights of a case: full tiles and the last one"""
    n_tiles = L.tile_count(case.n, case.c, mistake)
    return sorted({L.tile_rows(case.n, case.c, t, mistake) for t in (0, n_tiles - 1)})


def test_the_constants_are_the_sources():
    assert int(_one(r"constexpr int SL_MAX_C = (\d+);")) == L.SL_MAX_C and int(_one(r"constexpr int SL_THREADS = (\d+);")) == L.SL_THREADS
    assert _one(r"int tile_rows_of\(int c\) \{ return c <= (\d+) \? (\d+) : (\d+); \}") == ("32", "256", "128")
    assert [L.tile_rows_of(c) for c in (1, 31, 32, 33, 34, 64)] == [256, 256, 256, 128, 128, 128]
    assert _one(r"constexpr int SL_BINS = (\d+) \* SL_MAX_C \+ (\d+);") == ("3", "2") and L.bins_of(64) == 194 and L.bins_of(1) == 5
    assert len(re.findall(r"stride = c \| 1", SRC)) == 1 and [L.stride_of(c) for c in (1, 2, 32, 33, 64)] == [1, 3, 33, 33, 65]
    assert len(re.findall(r"per = x_type == POINTOPS2_ROWS_F32 \? 4 : 8", SRC)) == 2 and [L.per_of(r) for r in ("f32", "f16", "bf16")] == [4, 8, 8]
    assert len(re.findall(r"grid = tiles < partial_rows \? tiles : partial_rows", SRC)) == 1
    assert len(re.findall(r"cap = num_cus\(\) \* 8", SRC)) == 1 and len(re.findall(r"dim3\(tiles < cap \? tiles : cap\)", SRC)) == 1
    assert len(re.findall(r"\(int\)aligned16\(logits\), logits", SRC)) == 1                       # the forward's vec
    assert len(re.findall(r"\(int\)\(aligned16\(logits\) && aligned16\(grad_logits\)\)", SRC)) == 1   # the backward's
    assert len(re.findall(r"t \+= gridDim\.x", SRC)) == 2
    # the fullest tiles fill SL_TILE_WORDS exactly (C = 32) or stay below it (C = 64)
    assert SL_TILE_WORDS == 256 * L.stride_of(32) and 128 * L.stride_of(64) <= SL_TILE_WORDS
    assert max(L.tile_rows_of(c) * L.stride_of(c) for c in range(1, L.SL_MAX_C + 1)) == SL_TILE_WORDS
    from stratified_transformer_amd import pointops2_cuda
    assert pointops2_cuda.SEG_LOSS_PARTIAL_ROWS == L.PARTIAL_ROWS and pointops2_cuda.SEG_LOSS_MAX_C == L.SL_MAX_C


def test_the_vector_conditions():
    for rows in ("f32", "f16", "bf16"):
        assert L.forward_vec(rows, False) and not L.forward_vec(rows, True)
        assert [L.backward_vec(rows, a, b) for a in (False, True) for b in (False, True)] == [True, False, False, False]
    assert L.forward_grid(600, 19) == 3 and L.forward_grid(600, 19, 2) == 2 and L.forward_grid(300000, 19) == 1024
    assert L.backward_grid(300000, 19, 256) == 1172 and L.backward_grid(128 * 2049, 33, 256) == 2048


def test_every_claim_is_what_the_choices_give():
    assert len({c[:6] for c in L.CASES}) == len(L.CASES) and len({L.case_id(c) for c in L.CASES}) == len(L.CASES)
    for case in L.CASES:
        want = L.claims_of(case.rows, case.c, case.n, case.misaligned, case.partial_rows)
        assert {k: getattr(case, k) for k in L.CLAIMS} == want, case
        assert 1 <= case.c <= L.SL_MAX_C and 1 <= case.n <= 8321 and (case.eps == 0.0 or case.c >= 2)
        assert case.partial_rows is None or 1 <= case.partial_rows <= L.PARTIAL_ROWS
        # the claims against a second statement
        tiles = -(-case.n // case.tile)
        assert case.finish == min(tiles, case.partial_rows or 1024) and (case.per_wg == "more") == (tiles > case.finish)
        assert (case.parity == "even") == (L.stride_of(case.c) == case.c + 1)
        if case.path != "scalar":
            per = L.per_of(case.rows)
            if case.c % per == 0:
                assert case.pieces == "inside"
            if case.c * 2 < per:
                assert case.pieces == "multi"
            assert (case.path == "tail") == any((tr * case.c) % per != 0 for tr in _tiles(case))


def test_every_claim_value_is_reached_for_fp32_and_a_half_type():
    for rows in ("f32", HALF_TYPE):
        cases = L.select(rows=rows)
        assert {c.tile for c in cases} == {256, 128}, rows
        assert {c.parity for c in cases} == {"even", "odd"}, rows
        assert {kind for c in cases for kind in c.pieces.split("+")} == {"inside", "straddle", "multi", "none"}, rows
        assert {c.path for c in cases} == {"vector", "tail", "scalar"}, rows
        assert {c.last for c in cases} >= {"1", "rows_per - 1", "rows_per", "rows_per + 1"}, rows
        assert {c.per_wg for c in cases} == {"1", "more"}, rows
        assert {c.finish for c in cases} >= {1, 63, 64, 65}, rows
        for tile in (256, 128):                                                # both heights at every boundary count and on every path
            assert {c.last for c in cases if c.tile == tile} >= {"rows_per - 1", "rows_per", "rows_per + 1"}, (rows, tile)
            assert {c.path for c in cases if c.tile == tile} == {"vector", "tail", "scalar"}, (rows, tile)


def test_the_table_holds_the_cases_the_gaps_were_found_at():
    have = {(c.rows, c.c) for c in L.CASES}
    for c in (1, 2, 3, 5, 7, 8, 16, 19, 31, 32, 33, 34, 64):
        assert ("f32", c) in have, c
    for rows in ("f16", "bf16"):
        for c in (1, 2, 3, 7, 8, 32, 33, 64):
            assert (rows, c) in have, (rows, c)
        assert L.select(rows=rows, misaligned=True), rows
    for rows in ("f32", "f16"):
        for c, tile in ((32, 256), (33, 128)):                                 # both sides of one and of two tile heights, n on the boundary
            assert L.tile_rows_of(c) == tile
            ns = {case.n for case in L.select(rows=rows, c=c, misaligned=False, partial_rows=None, eps=0.0)}
            assert ns >= {tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1}, (rows, c)
        assert {case.partial_rows for case in L.CASES if case.rows == rows and -(-case.n // case.tile) == 3} >= {1, 2, 3}
        assert {case.partial_rows for case in L.CASES if case.rows == rows and -(-case.n // case.tile) >= 65} >= {63, 64, 65}
    assert L.select(rows="f32", c=32, n=256)[0].tile * L.stride_of(32) == SL_TILE_WORDS            # the fullest LDS tile
    # smoothing beside the piece kinds it has never met
    assert L.select(rows="f32", c=2, eps=0.1) and all(L.select(rows=r, c=c, eps=0.1) for r in ("f16", "bf16") for c in (7, 33))


def test_the_inputs_of_every_case_interleave_the_row_kinds():
    for case in L.CASES:
        p = L.case_inputs(case.c, case.n, seed=case.c + case.n)               # (asserts one valid row and, from 3 rows on, one of each other kind)
        valid = (p["t"] >= 0) & (p["t"] < case.c) & (p["t"] != L.IGNORE)
        assert np.array_equal(p["kinds"], np.arange(case.n) % 3) and np.array_equal(valid, p["kinds"] == 0)
        assert p["x"].shape == (case.n, case.c) and p["x"].dtype == np.float32 and p["t"].dtype == np.int64
        per = L.per_of(case.rows)
        if "multi" in case.pieces and case.n >= 8:                             # a piece over three rows and more holds every kind of row
            start = next(s for s in range(0, case.n * case.c, per) if (s % case.c + per - 1) // case.c >= 2)
            assert set(p["kinds"][(start + np.arange(per)) // case.c].tolist()) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------------
# the models: the kernel's own indexing passes, each seeded mistake is seen or said to be harmless
# ---------------------------------------------------------------------------------------------------------------------
def _staging(case, mistake=None):
    """-> (written once, no word shared, below SL_TILE_WORDS, the row walker finds (r, col) at r * stride + col) over a case's tiles"""
    vec, stride = L.forward_vec(case.rows, case.misaligned), L.stride_of(case.c)
    once = apart = below = placed = True
    for tr in _tiles(case, mistake):
        word, writes = L.forward_staging(tr, case.c, case.rows, vec, mistake)
        le = np.arange(tr * case.c)
        once &= bool((writes == 1).all())
        apart &= len(np.unique(word)) == word.size
        below &= bool(word.max() < SL_TILE_WORDS and word.min() >= 0)
        placed &= np.array_equal(word, (le // case.c) * stride + le % case.c)
    return once, apart, below, placed


def _backward(case, mistake=None):
    """-> (every element uses its own row and column, every element stored once); grad_logits aligned as the operator's"""
    vec = L.backward_vec(case.rows, case.misaligned, False)
    own = once = True
    for tr in _tiles(case, mistake):
        row, col, writes = L.backward_walk(tr, case.c, case.rows, vec, mistake)
        le = np.arange(tr * case.c)
        own &= np.array_equal(row, le // case.c) and np.array_equal(col, le % case.c)
        once &= bool((writes == 1).all())
    return own, once


def _walk(case, mistake=None):
    """-> (every tile taken once, from its own first row) by the forward's grid"""
    grid = L.forward_grid(case.n, case.c, case.partial_rows, mistake)
    visits, first, _ = L.tile_walk(case.n, case.c, grid, mistake)
    return bool((visits == 1).all()), np.array_equal(first, np.arange(visits.size) * L.tile_rows_of(case.c, mistake))


def _claims_hold(case, mistake=None):
    want = L.claims_of(case.rows, case.c, case.n, case.misaligned, case.partial_rows, mistake)
    return all(getattr(case, k) == v for k, v in want.items() if v is not None)


def _verdict(case, mistake=None):
    return dict(staging=_staging(case, mistake), backward=_backward(case, mistake), walk=_walk(case, mistake), claims=_claims_hold(case, mistake))


@pytest.fixture(scope="module")
def verdicts():
    return {m: {L.case_id(c): _verdict(c, m) for c in L.CASES} for m in (None,) + tuple(L.MISTAKES)}


def test_the_models_with_the_kernels_own_indexing(verdicts):
    for name, v in verdicts[None].items():
        assert v == dict(staging=(True,) * 4, backward=(True, True), walk=(True, True), claims=True), name


def test_the_backward_walk_with_a_misaligned_gradient_alone():
    """logits aligned, grad_logits not: the all-scalar loop, every element once and with its own row"""
    for case in L.select(misaligned=False):
        assert not L.backward_vec(case.rows, False, True)
        for tr in _tiles(case):
            row, col, writes = L.backward_walk(tr, case.c, case.rows, False)
            assert np.array_equal(row, np.arange(tr * case.c) // case.c) and (writes == 1).all()


def _changed(verdicts, mistake, part=None):
    return {name for name, v in verdicts[mistake].items() if (v if part is None else v[part]) != (verdicts[None][name] if part is None else verdicts[None][name][part])}


def test_each_seeded_mistake_is_seen_by_named_cases(verdicts):
    by_id = {L.case_id(c): c for c in L.CASES}
    changed = {m: _changed(verdicts, m) for m in L.MISTAKES}
    for m in L.MISTAKES:
        print(f"{m}: the model output of {len(changed[m])} of {len(by_id)} cases changes, e.g. {sorted(changed[m])[:3]}")
        assert changed[m], m
    vec = {k for k, c in by_id.items() if c.path != "scalar"}
    # the row advance: wherever a piece leaves its first row, and nowhere else
    assert changed["mid-piece row advance dropped"] == {k for k, c in by_id.items() if {"straddle", "multi"} & set(c.pieces.split("+"))}
    assert _changed(verdicts, "mid-piece row advance dropped", "staging") == set()             # (the forward has no row state)
    assert {"f16-c1-n257", "f16-c3-n255", "bf16-c2-n257", "f32-c1-n257", "f32-c19-n511", "f16-c33-n128"} <= changed["mid-piece row advance dropped"]
    # the other type's per: every vector case but the one row of 32 halves, whose four pieces start in row 0 under either per
    assert changed["r from the other row type's per"] == vec - {"f16-c32-n1"}
    assert {"f32-c8-n256", "f16-c8-n256", "f16-c64-n128", "bf16-c1-n256"} <= changed["r from the other row type's per"]
    # the tail from `pieces`: elements written twice wherever whole pieces exist; the same values, so slower and no more
    assert changed["tail starts at pieces"] == vec
    for k in vec:
        once, apart, below, placed = verdicts["tail starts at pieces"][k]["staging"]
        assert not once and apart and below and placed and verdicts["tail starts at pieces"][k]["backward"] == (True, False)
    # the tile switch: the claims of C = 32 / 33 / 33 and 34; only the last leaves the LDS tile
    assert changed["tile height switched at c < 32"] == {k for k, c in by_id.items() if c.c == 32}
    assert changed["tile height switched at c <= 33"] == {k for k, c in by_id.items() if c.c == 33}
    assert changed["tile height switched at c <= 34"] == {k for k, c in by_id.items() if c.c in (33, 34)}
    for m in ("tile height switched at c < 32", "tile height switched at c <= 33"):
        assert all(verdicts[m][k]["staging"] == (True,) * 4 and not verdicts[m][k]["claims"] for k in changed[m]), m
    assert {k for k in by_id if not verdicts["tile height switched at c <= 34"][k]["staging"][2]} == {"f32-c34-n257"}
    assert 256 * L.stride_of(33) == SL_TILE_WORDS < 256 * L.stride_of(34)
    # the stride: every word still its own and below the end - bank conflicts at even C, nothing else
    assert changed["row stride c instead of c | 1"] == {k for k, c in by_id.items() if c.parity == "even" and c.n >= 2}   # (one row has no stride)
    assert all(verdicts["row stride c instead of c | 1"][k]["staging"] == (True, True, True, False) for k in changed["row stride c instead of c | 1"])
    # the walk: a step of 1 wherever a second workgroup exists; first_row wherever a workgroup has a second trip
    assert changed["grid-stride step of 1"] == {k for k, c in by_id.items() if c.finish >= 2}
    assert changed["first_row from the workgroup index"] == {k for k, c in by_id.items() if c.per_wg == "more"}
    assert {"f32-c19-n600-p1", "f32-c19-n600-p2", "f16-c33-n300-p1", "f32-c33-n8321-p63", "f16-c33-n8321-p64"} <= changed["first_row from the workgroup index"]


def test_every_mistake_is_wrong_on_the_device_with_an_assertion_or_merely_slower(verdicts):
    with open(os.path.join(TESTS, "test_seg_loss_edges_hip.py")) as f:
        gpu_tests = set(re.findall(r"^def (test_\w+)\(", f.read(), re.M))
    for m, (device, where) in L.MISTAKES.items():
        assert device in ("wrong", "slower") and (where in gpu_tests if device == "wrong" else where is None), m
    for m, where in L.DEVICE_ONLY.items():
        assert m not in L.MISTAKES and where in gpu_tests, m
    # "slower" is a statement about the models: every element still lands once-or-twice in its own word inside the tile, with its own row
    for m in (m for m, (device, _) in L.MISTAKES.items() if device == "slower"):
        for name, v in verdicts[m].items():
            assert v["staging"][1] and v["staging"][2] and v["backward"][0] and v["walk"] == (True, True), (m, name)
    # "wrong": an element in another row's word or past the tile, another row's state, or a tile taken twice or from the wrong row
    for m in (m for m, (device, _) in L.MISTAKES.items() if device == "wrong"):
        assert any(not (v["staging"][2] and v["staging"][3] and v["backward"][0] and all(v["walk"])) for v in verdicts[m].values()), m
