"""CPU: the table of tests/row_lanes_cases.py is what it claims - every label is what RowShape computes, the table reaches every kernel
instance, segment width, fill and boundary - and the properties tests/test_row_lanes_hip.py asserts on the device have teeth: in a numpy
model of one workgroup's lanes the correct indexing gives the exact sums and keeps replicated columns replicated, and each of four
seeded indexing mistakes breaks one of the two on at least one entry.  No HIP."""
import numpy as np
import pytest

from tests import row_lanes_cases as L

SEGS = (1, 2, 4, 8, 16, 32, 64)


def _shape(w, rows="f32"):
    return L.shape_of(w.c, w.misaligned, rows)


def test_every_label_is_what_row_shape_computes():
    assert len({(w.c, w.misaligned) for w in L.WIDTHS}) == len(L.WIDTHS)
    for w in L.WIDTHS:
        for rows in ("f32", "f16", "bf16"):                                    # one element off is off for 16-byte and for 8-byte chunks alike
            s = _shape(w, rows)
            assert (s.vec, s.iter, s.seg) == (w.vec, w.iter, w.seg), (w, rows, s)
            assert L.fill_of(s) == w.fill and L.last_has_one_lane(s) == w.last_one, (w, rows, s)
            assert s.per_wave == 64 // s.seg and s.rows_per_wg == 4 * s.per_wave and 1 <= w.c <= L.MAX_C
            assert sum(L.live_lanes(s, it) for it in range(s.iter)) == s.chunks and s.chunks * s.vec == w.c
            assert (s.vec, s.iter) in L.INSTANCES


def test_the_table_holds_the_widths_the_gaps_were_found_at():
    have = {(w.c, w.misaligned) for w in L.WIDTHS}
    for c in (4, 8, 12, 16, 20, 32, 64, 128, 252, 256, 260, 384, 512, 516, 768, 1020, 1024):
        assert (c, False) in have and L.shape_of(c, False).vec == 4, c
    for c in (1, 2, 3, 5, 7, 63, 65, 70, 1022, 1023):
        assert (c, False) in have and L.shape_of(c, False).vec == 1, c
    for c in (64, 96, 1024):
        assert (c, True) in have and L.shape_of(c, True).vec == 1, c


def test_chunked_for_restates_the_launchers():
    assert L.chunked_for(48, 4, False) and L.chunked_for(48, 2, False)
    assert not L.chunked_for(48, 4, True) and not L.chunked_for(48, 2, True)    # 4 bytes off 16, 2 bytes off 8
    assert not L.chunked_for(70, 4, False) and not L.chunked_for(7, 2, False)


def test_the_mislabelled_width_is_a_chunked_row():
    """c = 100 on an aligned allocation: 25 chunks in a 32-lane segment, not one channel a lane"""
    assert L.row_shape(100, L.chunked_for(100, 4, False)) == (4, 1, 25, 32, 2, 8)
    assert L.row_shape(100, False)[:4] == (1, 16, 100, 64)
    assert L.row_shape(70, L.chunked_for(70, 4, False))[:4] == (1, 16, 70, 64)   # the width that does run (1, 16) unaided


def test_all_five_instances_for_each_row_type():
    table = {(w.c, w.misaligned) for w in L.WIDTHS}
    for rows, cases in L.TYPE_CASES.items():
        assert set(cases) <= table and len(set(cases)) == len(cases), rows
        seen = {(s.vec, s.iter) for s in (L.shape_of(c, m, rows) for c, m in cases)}
        assert seen == set(L.INSTANCES), (rows, seen)
    assert {(w.vec, w.iter) for w in L.WIDTHS} == set(L.INSTANCES)
    for inst, (c, m) in L.INSTANCE_WIDTHS.items():
        assert (c, m) in table and L.shape_of(c, m)[:2] == inst


def test_every_segment_width_full_and_partial():
    for vec in (4, 1):
        assert {w.seg for w in L.WIDTHS if w.vec == vec and w.iter == 1} == set(SEGS), vec
        for seg in SEGS[2:]:                                                   # (a segment of 1 or 2 lanes holds exactly 1 or 2 chunks: always full)
            assert {w.fill for w in L.WIDTHS if w.vec == vec and w.iter == 1 and w.seg == seg} == {"full", "partial"}, (vec, seg)
        for seg in SEGS[:2]:
            assert {w.fill for w in L.WIDTHS if w.vec == vec and w.iter == 1 and w.seg == seg} == {"full"}, (vec, seg)


def test_the_long_rows_with_one_live_lane_in_the_last_iteration_and_full():
    for inst in ((4, 2), (4, 4), (1, 16)):
        rows = [w for w in L.WIDTHS if (w.vec, w.iter) == inst]
        assert any(w.last_one for w in rows) and any(w.fill == "full" for w in rows), inst
        for w in rows:
            s, used = _shape(w), L.used_iterations(_shape(w))
            assert all(L.live_lanes(s, it) == 64 for it in range(used - 1)) and all(L.live_lanes(s, it) == 0 for it in range(used, s.iter))
            assert L.live_lanes(s, used - 1) == (1 if w.last_one else s.chunks - 64 * (used - 1))
    assert L.used_iterations(L.shape_of(1023, False)) == 16 and L.live_lanes(L.shape_of(1023, False), 15) == 63   # all sixteen in use
    assert L.used_iterations(L.shape_of(516, False)) == 3 and L.used_iterations(L.shape_of(65, False)) == 2


def test_row_counts_lie_where_their_names_say():
    for w in L.WIDTHS:
        s = _shape(w)
        names = L.row_count_names(s)
        assert names["per_wave - 1"] < s.per_wave == names["per_wave"] < names["per_wave + 1"]
        assert names["rows_per_wg - 1"] < s.rows_per_wg < names["rows_per_wg + 1"]
        big = names["3 * rows_per_wg + per_wave + 1"]
        assert big == L.big_count(s) and big // s.rows_per_wg == 3 and big % s.rows_per_wg == s.per_wave + 1   # wave 1 of the fourth workgroup: one live row
        assert big <= 3 * 256 + 65
        counts = L.row_counts(s)
        assert counts == sorted(set(counts)) and counts[0] >= 1 and set(counts) == {n for n in names.values() if n >= 1}
        assert L.row_counts(s, training=True) == [n for n in counts if n >= 2]
        assert {s.per_wave, s.per_wave + 1, s.rows_per_wg + 1, big} <= set(counts)


def test_partial_row_counts():
    counts = L.partial_row_counts(48)
    shape = L.row_shape(48, True)
    assert [L.partial_rows(n, shape) for n in counts] == [63, 64, 65]
    assert counts == [1008, 1024, 1025]
    assert L.partial_rows(counts[0] + 1, shape) == 64 and L.partial_rows(counts[1] + 1, shape) == 65 and L.partial_rows(counts[2] - 1, shape) == 64
    assert L.partial_rows(400000, shape) == 1024 and L.partial_rows(4099, shape) == 257 and L.partial_rows(333, shape) == 21   # the neighbours' cases
    assert max(counts) <= 3 * 256 + 65 + 256                                   # (c = 48: sixteen rows a workgroup)


# ---------------------------------------------------------------------------------------------------------------------
# the model: correct indexing passes, each seeded mistake is caught
# ---------------------------------------------------------------------------------------------------------------------
def _verdict(w, mistake):
    """-> (the sums are exact, replicated columns stay replicated) on the entry's largest row count"""
    s = _shape(w)
    n = L.big_count(s) if w.c <= 128 else 2 * s.rows_per_wg + 1                 # (wide rows: fewer of them, the model is a Python loop)
    x = L.model_inputs(n, w.c, seed=w.c)
    exact = np.array_equal(L.model_column_sums(x, s, mistake), x.sum(0)) and np.array_equal(L.model_row_sums(x, s, mistake), x.sum(1))
    r = L.model_inputs(n, w.c, seed=w.c + 1, replicated=True)
    cols = L.model_column_sums(r, s, mistake)
    return exact, bool((cols == cols[0]).all())


@pytest.fixture(scope="module")
def verdicts():
    return {m: {(w.c, w.misaligned): _verdict(w, m) for w in L.WIDTHS} for m in (None,) + L.MISTAKES}


def test_the_model_with_correct_indexing(verdicts):
    assert all(v == (True, True) for v in verdicts[None].values())


def test_each_seeded_mistake_is_caught(verdicts):
    by_key = {(w.c, w.misaligned): w for w in L.WIDTHS}
    caught = {m: {k for k, (exact, same) in verdicts[m].items() if not (exact and same)} for m in L.MISTAKES}
    unequal = {m: {k for k, (_, same) in verdicts[m].items() if not same} for m in L.MISTAKES}
    for m in L.MISTAKES:
        print(f"{m}: caught at {len(caught[m])} of {len(by_key)} widths, {len(unequal[m])} of them by unequal replicated columns")
        assert caught[m], m
    # where each must show: an idle lane exists; a segment has a second lane to take; a row has more than 64 chunks
    assert caught["idle lanes not masked"] == {k for k, w in by_key.items() if w.fill == "partial"}
    assert caught["butterfly started at seg / 2"] == {k for k, w in by_key.items() if w.seg >= 2}
    assert caught["lane0 taken without & 63"] == {k for k, w in by_key.items() if w.iter > 1}
    assert caught["it dropped"] == {k for k, w in by_key.items() if w.iter > 1}
    # the exact property alone sees the butterfly wherever a segment is partly idle, and the lane0 slip wherever the read leaves `red`
    assert unequal["butterfly started at seg / 2"] and unequal["lane0 taken without & 63"]
