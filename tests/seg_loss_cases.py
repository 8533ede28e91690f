"""Cases for csrc/seg_loss.hip (pointops.segmentation_loss), the one hot kernel with a row layout of its own: the host- and device-side
choices restated, two numpy models of one workgroup - where the forward stages every element of a tile in LDS, and whose row state the
backward uses for every element - a model of the grid-stride tile walk, a table of cases with what each claims to reach, the inputs of
a case, and the indexing mistakes with which tests/test_seg_loss_cases_cpu.py shows that the table can fail.  numpy only.

    tile      256 rows for C <= 32, 128 above; staged as fp32 at a row stride of C | 1 words in SL_TILE_WORDS words of LDS
    piece     16 bytes of a tile = per = 4 fp32 or 8 half elements; inside one row, over two rows, or over three and more (C < per)
    vec       forward: logits 16-byte aligned; backward: logits and grad_logits aligned.  Otherwise one element a lane; the elements
              behind the last whole piece of a tile always go one a lane (the tail)
    grids     forward min(tiles, rows of `partials`), backward min(tiles, 8 * CUs); workgroup b takes the tiles b, b + grid, ...
    finish    one wave adds the forward grid's double partials, lane l taking l, l + 64, ...
"""
from collections import namedtuple

import numpy as np

SL_MAX_C, SL_THREADS, WAVE = 64, 256, 64
PARTIAL_ROWS = 1024                  # pointops2_cuda.SEG_LOSS_PARTIAL_ROWS: what the operator offers
ELEM_BYTES = {"f32": 4, "f16": 2, "bf16": 2}
IGNORE = 255                         # as tests/test_loss_hip.py


# ---------------------------------------------------------------------------------------------------------------------
# the choices of seg_loss.hip, restated.  `mistake` names one of MISTAKES (None: the kernel's own rule).
# ---------------------------------------------------------------------------------------------------------------------
def tile_rows_of(c, mistake=None):
    edge = {"tile height switched at c < 32": 31, "tile height switched at c <= 33": 33, "tile height switched at c <= 34": 34}.get(mistake, 32)
    return 256 if c <= edge else 128


def stride_of(c, mistake=None):
    return c if mistake == "row stride c instead of c | 1" else c | 1


def per_of(rows):
    return 16 // ELEM_BYTES[rows]


def bins_of(c):
    """[0, c) pred == target, [c, 2c) pred, [2c, 3c) target, 3c valid rows, 3c + 1 labels out of range"""
    return 3 * c + 2


def aligned16(rows, misaligned):
    """a [n, *] operand is an allocation (aligned) or a contiguous view one element into one"""
    return ((ELEM_BYTES[rows] if misaligned else 0) % 16) == 0


def forward_vec(rows, misaligned):
    return aligned16(rows, misaligned)


def backward_vec(rows, logits_misaligned, grad_misaligned):
    return aligned16(rows, logits_misaligned) and aligned16(rows, grad_misaligned)


def tile_count(n, c, mistake=None):
    return -(-n // tile_rows_of(c, mistake))


def forward_grid(n, c, partial_rows=None, mistake=None):
    return min(tile_count(n, c, mistake), PARTIAL_ROWS if partial_rows is None else partial_rows)


def backward_grid(n, c, cus, mistake=None):
    return min(tile_count(n, c, mistake), 8 * cus)


def tile_rows(n, c, t, mistake=None):
    """Tiles::rows(t)"""
    return min(n - t * tile_rows_of(c, mistake), tile_rows_of(c, mistake))


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def _piece_start(pieces, c, per, mistake):
    p = np.arange(pieces)
    wrong = {4: 8, 8: 4}[per] if mistake == "r from the other row type's per" else per
    r = (p * wrong) // c
    return p, r, p * per - r * c


def _tail_start(pieces, per, mistake):
    return pieces if mistake == "tail starts at pieces" else pieces * per


def forward_staging(tr, c, rows, vec, mistake=None):
    """One tile of tr rows through the forward's two staging loops -> (word [tr * c], writes [tr * c]): the LDS word that element le of
    the tile (row le // c, column le % c in global memory) is last written to, and how often it is written.  The piece walk is the
    kernel's: r = (p * per) / c, col = p * per - r * c, then per elements with `if (++col == c) col = 0, ++r`."""
    per, stride, elems = per_of(rows), stride_of(c, mistake), tr * c
    pieces = elems // per if vec else 0
    word, writes = np.full(elems, -1, np.int64), np.zeros(elems, np.int64)
    p, r, col = _piece_start(pieces, c, per, mistake)
    for k in range(per):
        le = p * per + k                                                       # v[k] of piece p is this element
        word[le] = r * stride + col
        writes[le] += 1
        col = col + 1
        wrap = col == c
        col, r = np.where(wrap, 0, col), r + wrap
    for le in range(_tail_start(pieces, per, mistake), elems):
        r1 = le // c
        word[le] = r1 * stride + (le - r1 * c)
        writes[le] += 1
    return word, writes


def backward_walk(tr, c, rows, vec, mistake=None):
    """One tile through the backward's two loops -> (row [tr * c], col [tr * c], writes): the row whose (label, maximum, log-sum) the
    kernel holds when it forms element le's gradient, the column it compares with the label, and how often le is stored.  The row
    state is reloaded mid-piece on the kernel's condition `++col == c && k + 1 < per && r + 1 < tr`."""
    per, elems = per_of(rows), tr * c
    pieces = elems // per if vec else 0
    row, colu, writes = np.full(elems, -1, np.int64), np.full(elems, -1, np.int64), np.zeros(elems, np.int64)
    p, r, col = _piece_start(pieces, c, per, mistake)
    state = r.copy()                                                           # rs = row_state(row0 + r)
    for k in range(per):
        le = p * per + k
        row[le], colu[le] = state, col
        writes[le] += 1
        col = col + 1
        adv = (col == c) & (k + 1 < per) & (r + 1 < tr)
        if mistake == "mid-piece row advance dropped":
            adv = np.zeros_like(adv)
        r = r + adv
        col, state = np.where(adv, 0, col), np.where(adv, r, state)
    for le in range(_tail_start(pieces, per, mistake), elems):
        r1 = le // c
        row[le], colu[le] = r1, le - r1 * c
        writes[le] += 1
    return row, colu, writes


def tile_walk(n, c, grid, mistake=None):
    """The loop `for (t = blockIdx.x; t < tiles.count; t += gridDim.x)` over a whole grid -> (visits [tiles], first_row [tiles],
    trips): how often each tile is taken, the first row used for it (the last visit's), the most trips of one workgroup."""
    tiles, rows_per = tile_count(n, c, mistake), tile_rows_of(c, mistake)
    visits, first, trips = np.zeros(tiles, np.int64), np.full(tiles, -1, np.int64), 0
    step = 1 if mistake == "grid-stride step of 1" else grid
    for b in range(grid):
        mine = range(b, tiles, step)
        trips = max(trips, len(mine))
        for t in mine:
            visits[t] += 1
            first[t] = (b if mistake == "first_row from the workgroup index" else t) * rows_per
    return visits, first, trips


# Indexing mistakes, one line each, applied to the restated choices and the models above.  "model": some case's model output or
# claim changes (tests/test_seg_loss_cases_cpu.py names the cases).  "device": what the mistake would do on the GPU - "wrong", with
# the assertion of tests/test_seg_loss_edges_hip.py that sees it, or "slower": the same results by a worse route.
MISTAKES = {
    "mid-piece row advance dropped": ("wrong", "test_every_case_against_the_oracle"),
    "r from the other row type's per": ("wrong", "test_every_case_against_the_oracle"),
    "tail starts at pieces": ("slower", None),                                 # the elements of whole pieces written twice, the same values
    "tile height switched at c < 32": ("slower", None),                        # C = 32 in 128-row tiles: half the LDS tile unused
    "tile height switched at c <= 33": ("slower", None),                       # C = 33 at 256 rows * 33 words fills SL_TILE_WORDS exactly
    "tile height switched at c <= 34": ("wrong", "test_every_case_against_the_oracle"),   # 256 rows * 35 words: past the LDS tile
    "row stride c instead of c | 1": ("slower", None),                         # even C: the rows of a wave share LDS banks
    "grid-stride step of 1": ("wrong", "test_partial_rows"),                   # forward: tiles counted again; backward: rewritten, slower
    "first_row from the workgroup index": ("wrong", "test_partial_rows"),
}
# Mistakes that change no model output - the models hold one tile or the walk, not the histogram, the barriers or the label's width - with
# the GPU assertion that sees each.
DEVICE_ONLY = {
    "histogram zeroed per tile, not per workgroup": "test_partial_rows",                        # counts, rows equal to the 1024-row run's
    "trailing __syncthreads() dropped (the next tile staged under the row walkers)": "test_partial_rows",   # stat bit-equal
    "counts stored, not added": "test_partial_rows",                                            # the second forward doubles them
    "finish adds `blocks` rounded down to whole waves": "test_partial_rows",                    # 63 / 65 rows of partials
    "label narrowed to int before the range check": "test_labels_outside_32_bits",
    "ignore_index narrowed to int": "test_labels_outside_32_bits",
    "backward's second trip from the first trip's rows": "test_backward_grid_stride",
    "shift gradient written only beside grad_logits": "test_backward_with_one_gradient",
}


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
# what an entry claims: tile (256 / 128), parity of C ("even": stride C + 1, "odd": stride C), pieces (the kinds of 16-byte piece in
# a full tile, "+"-joined from inside / straddle / multi; "none": no vector path), path ("vector": whole pieces only, "tail": pieces and
# a scalar tail in some tile, "scalar": one element a lane), last (the rows of the last tile: "1", "rows_per - 1", "rows_per",
# "rows_per + 1" = a further tile of one row, or "other"), per_wg (the most tiles of one forward workgroup: "1" or "more"), finish
# (the rows of partials seg_loss_finish_kernel adds).
Case = namedtuple("Case", "rows c n misaligned partial_rows eps tile parity pieces path last per_wg finish")
CLAIMS = Case._fields[6:]


def piece_kinds(c, rows, tr):
    """the kinds of piece in a tile of tr rows"""
    per = per_of(rows)
    start = np.arange((tr * c) // per) * per
    covered = (start % c + per - 1) // c + 1
    names = [name for name, hit in (("inside", covered == 1), ("straddle", covered == 2), ("multi", covered >= 3)) if hit.any()]
    return "+".join(names) if names else "none"


def last_name(n, c):
    rows_per, tiles = tile_rows_of(c), tile_count(n, c)
    last = n - (tiles - 1) * rows_per
    if last == 1:
        return "rows_per + 1" if tiles >= 2 else "1"
    return {rows_per - 1: "rows_per - 1", rows_per: "rows_per"}.get(last, "other")


def claims_of(rows, c, n, misaligned, partial_rows, mistake=None):
    """what the restated choices give for an entry"""
    vec, per, rows_per = forward_vec(rows, misaligned), per_of(rows), tile_rows_of(c, mistake)
    tiles, grid = tile_count(n, c, mistake), forward_grid(n, c, partial_rows, mistake)
    tails = any((tile_rows(n, c, t, mistake) * c) % per for t in (0, tiles - 1))       # (the tiles before the last are full ones)
    return dict(tile=rows_per, parity="odd" if c % 2 else "even", pieces=piece_kinds(c, rows, min(n, rows_per)) if vec else "none",
                path="scalar" if not vec else "tail" if tails else "vector", last=last_name(n, c) if mistake is None else None,
                per_wg="1" if -(-tiles // grid) == 1 else "more", finish=grid)


CASES = [
    Case("f32", 1, 257, False, None, 0.0, 256, "odd", "multi", "tail", "rows_per + 1", "1", 2),
    Case("f32", 2, 255, False, None, 0.1, 256, "even", "straddle", "tail", "rows_per - 1", "1", 1),
    Case("f32", 3, 256, False, None, 0.0, 256, "odd", "straddle", "vector", "rows_per", "1", 1),
    Case("f32", 5, 255, False, None, 0.0, 256, "odd", "inside+straddle", "tail", "rows_per - 1", "1", 1),
    Case("f32", 7, 513, False, None, 0.0, 256, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 3),
    Case("f32", 8, 256, False, None, 0.0, 256, "even", "inside", "vector", "rows_per", "1", 1),
    Case("f32", 16, 257, False, None, 0.0, 256, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("f32", 19, 511, False, None, 0.0, 256, "odd", "inside+straddle", "tail", "rows_per - 1", "1", 2),
    Case("f32", 31, 512, False, None, 0.0, 256, "odd", "inside+straddle", "vector", "rows_per", "1", 2),
    Case("f32", 32, 1, False, None, 0.0, 256, "even", "inside", "vector", "1", "1", 1),
    Case("f32", 32, 255, False, None, 0.0, 256, "even", "inside", "vector", "rows_per - 1", "1", 1),
    Case("f32", 32, 256, False, None, 0.0, 256, "even", "inside", "vector", "rows_per", "1", 1),
    Case("f32", 32, 257, False, None, 0.0, 256, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("f32", 32, 511, False, None, 0.0, 256, "even", "inside", "vector", "rows_per - 1", "1", 2),
    Case("f32", 32, 512, False, None, 0.0, 256, "even", "inside", "vector", "rows_per", "1", 2),
    Case("f32", 32, 513, False, None, 0.0, 256, "even", "inside", "vector", "rows_per + 1", "1", 3),
    Case("f32", 33, 127, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per - 1", "1", 1),
    Case("f32", 33, 128, False, None, 0.0, 128, "odd", "inside+straddle", "vector", "rows_per", "1", 1),
    Case("f32", 33, 129, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 2),
    Case("f32", 33, 255, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per - 1", "1", 2),
    Case("f32", 33, 256, False, None, 0.0, 128, "odd", "inside+straddle", "vector", "rows_per", "1", 2),
    Case("f32", 33, 257, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 3),
    Case("f32", 34, 257, False, None, 0.0, 128, "even", "inside+straddle", "tail", "rows_per + 1", "1", 3),
    Case("f32", 64, 1, False, None, 0.0, 128, "even", "inside", "vector", "1", "1", 1),
    Case("f32", 64, 127, False, None, 0.0, 128, "even", "inside", "vector", "rows_per - 1", "1", 1),
    Case("f32", 64, 128, False, None, 0.0, 128, "even", "inside", "vector", "rows_per", "1", 1),
    Case("f32", 64, 129, False, None, 0.0, 128, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("f32", 19, 333, True, None, 0.0, 256, "odd", "none", "scalar", "other", "1", 2),
    Case("f32", 32, 257, True, None, 0.0, 256, "even", "none", "scalar", "rows_per + 1", "1", 2),
    Case("f32", 64, 129, True, None, 0.0, 128, "even", "none", "scalar", "rows_per + 1", "1", 2),
    Case("f32", 19, 600, False, 1, 0.0, 256, "odd", "inside+straddle", "vector", "other", "more", 1),
    Case("f32", 19, 600, False, 2, 0.0, 256, "odd", "inside+straddle", "vector", "other", "more", 2),
    Case("f32", 19, 600, False, 3, 0.0, 256, "odd", "inside+straddle", "vector", "other", "1", 3),
    Case("f32", 33, 8321, False, 63, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "more", 63),
    Case("f32", 33, 8321, False, 64, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "more", 64),
    Case("f32", 33, 8321, False, 65, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "more", 65),
    Case("f16", 1, 257, False, None, 0.0, 256, "odd", "multi", "tail", "rows_per + 1", "1", 2),
    Case("f16", 2, 256, False, None, 0.0, 256, "even", "multi", "vector", "rows_per", "1", 1),
    Case("f16", 3, 255, False, None, 0.0, 256, "odd", "multi", "tail", "rows_per - 1", "1", 1),
    Case("f16", 5, 513, False, None, 0.0, 256, "odd", "straddle+multi", "tail", "rows_per + 1", "1", 3),
    Case("f16", 7, 257, False, None, 0.1, 256, "odd", "straddle", "tail", "rows_per + 1", "1", 2),
    Case("f16", 8, 256, False, None, 0.0, 256, "even", "inside", "vector", "rows_per", "1", 1),
    Case("f16", 16, 511, False, None, 0.0, 256, "even", "inside", "vector", "rows_per - 1", "1", 2),
    Case("f16", 19, 333, False, None, 0.0, 256, "odd", "inside+straddle", "tail", "other", "1", 2),
    Case("f16", 32, 1, False, None, 0.0, 256, "even", "inside", "vector", "1", "1", 1),
    Case("f16", 32, 255, False, None, 0.0, 256, "even", "inside", "vector", "rows_per - 1", "1", 1),
    Case("f16", 32, 256, False, None, 0.0, 256, "even", "inside", "vector", "rows_per", "1", 1),
    Case("f16", 32, 257, False, None, 0.0, 256, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("f16", 32, 511, False, None, 0.0, 256, "even", "inside", "vector", "rows_per - 1", "1", 2),
    Case("f16", 32, 512, False, None, 0.0, 256, "even", "inside", "vector", "rows_per", "1", 2),
    Case("f16", 32, 513, False, None, 0.0, 256, "even", "inside", "vector", "rows_per + 1", "1", 3),
    Case("f16", 33, 127, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per - 1", "1", 1),
    Case("f16", 33, 128, False, None, 0.0, 128, "odd", "inside+straddle", "vector", "rows_per", "1", 1),
    Case("f16", 33, 129, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 2),
    Case("f16", 33, 255, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per - 1", "1", 2),
    Case("f16", 33, 256, False, None, 0.0, 128, "odd", "inside+straddle", "vector", "rows_per", "1", 2),
    Case("f16", 33, 257, False, None, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 3),
    Case("f16", 33, 129, False, None, 0.1, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 2),
    Case("f16", 64, 127, False, None, 0.0, 128, "even", "inside", "vector", "rows_per - 1", "1", 1),
    Case("f16", 64, 128, False, None, 0.0, 128, "even", "inside", "vector", "rows_per", "1", 1),
    Case("f16", 64, 129, False, None, 0.0, 128, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("f16", 1, 255, True, None, 0.0, 256, "odd", "none", "scalar", "rows_per - 1", "1", 1),
    Case("f16", 8, 257, True, None, 0.0, 256, "even", "none", "scalar", "rows_per + 1", "1", 2),
    Case("f16", 33, 129, True, None, 0.0, 128, "odd", "none", "scalar", "rows_per + 1", "1", 2),
    Case("f16", 33, 300, False, 1, 0.0, 128, "odd", "inside+straddle", "tail", "other", "more", 1),
    Case("f16", 33, 300, False, 2, 0.0, 128, "odd", "inside+straddle", "tail", "other", "more", 2),
    Case("f16", 33, 300, False, 3, 0.0, 128, "odd", "inside+straddle", "tail", "other", "1", 3),
    Case("f16", 33, 8321, False, 63, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "more", 63),
    Case("f16", 33, 8321, False, 64, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "more", 64),
    Case("f16", 33, 8321, False, 65, 0.0, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "more", 65),
    Case("bf16", 1, 256, False, None, 0.0, 256, "odd", "multi", "vector", "rows_per", "1", 1),
    Case("bf16", 2, 257, False, None, 0.0, 256, "even", "multi", "tail", "rows_per + 1", "1", 2),
    Case("bf16", 3, 257, False, None, 0.0, 256, "odd", "multi", "tail", "rows_per + 1", "1", 2),
    Case("bf16", 7, 255, False, None, 0.1, 256, "odd", "straddle", "tail", "rows_per - 1", "1", 1),
    Case("bf16", 8, 255, False, None, 0.0, 256, "even", "inside", "vector", "rows_per - 1", "1", 1),
    Case("bf16", 32, 257, False, None, 0.0, 256, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("bf16", 33, 128, False, None, 0.0, 128, "odd", "inside+straddle", "vector", "rows_per", "1", 1),
    Case("bf16", 33, 129, False, None, 0.1, 128, "odd", "inside+straddle", "tail", "rows_per + 1", "1", 2),
    Case("bf16", 64, 129, False, None, 0.0, 128, "even", "inside", "vector", "rows_per + 1", "1", 2),
    Case("bf16", 7, 129, True, None, 0.0, 256, "odd", "none", "scalar", "other", "1", 1),
]


def case_id(case):
    part = "" if case.partial_rows is None else f"-p{case.partial_rows}"
    return f"{case.rows}-c{case.c}-n{case.n}{'-mis' if case.misaligned else ''}{part}{'-eps' if case.eps else ''}"


def select(**want):
    return [case for case in CASES if all(getattr(case, k) == v for k, v in want.items())]


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of a case
# ---------------------------------------------------------------------------------------------------------------------
def row_kinds(n):
    """0 valid, 1 ignored, 2 out of range: period 3, so the rows under one multi-row piece are of every kind"""
    return np.arange(n) % 3


def case_inputs(c, n, seed, ignore_index=IGNORE):
    """-> dict(x [n, c] f32, t [n] int64, sp [n, 3] f32, s [n, 3] f32, kinds [n]).  Valid rows carry the targets 0, 1, ... C - 1, 0, ...:
    neighbouring valid rows differ (C >= 2); out-of-range rows alternate between C and -1.  x and sp are rounded to the row type by
    the caller, who then sets s[0, 0] = sp[0, 0] (sign(0) = 0)."""
    rng = np.random.default_rng(seed)
    kinds = row_kinds(n)
    j = np.arange(n) // 3
    t = np.where(kinds == 0, j % c, np.where(kinds == 1, ignore_index, np.where(j % 2 == 0, c, -1))).astype(np.int64)
    assert not (0 <= ignore_index < c)
    valid = (t >= 0) & (t < c) & (t != ignore_index)
    assert np.array_equal(valid, kinds == 0) and valid.any()
    if n >= 3:
        assert (t == ignore_index).any() and (~valid & (t != ignore_index)).any()
    if c >= 2 and n >= 4:
        tv = t[valid]
        assert (tv[1:] != tv[:-1]).all()
    x = (3.0 * rng.standard_normal((n, c))).astype(np.float32)
    sp, s = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    return dict(x=x, t=t, sp=sp, s=s, kinds=kinds)
