"""Cases for the kernels that put rows [n, c] on the lanes by csrc/row_lanes.h - rownorm.hip (residual_norm, residual_norm_stream) and
batchnorm.hip (batch_norm_act and the launchers behind sync_batch_norm_act): the host-side choice of a kernel instance and a segment
width restated, a table of widths that reaches every instance, segment width and fill, the row counts that sit on the boundaries the
choice creates, and a numpy model of one workgroup's lanes with which tests/test_row_lanes_cases_cpu.py shows that an indexing mistake
breaks the properties tests/test_row_lanes_hip.py asserts on the device.  numpy only.

    lane = (row slot, chunk): a chunk is VEC channels (4: one 16-byte / 8-byte access; 1: the fallback), a row of `chunks` <= 64 chunks
    takes a segment of seg = the next power of two lanes, 64 / seg rows sit side by side in a wave; longer rows take the whole wave,
    every lane ITER chunks 64 apart.  Five instances (VEC, ITER): (4,1) (4,2) (4,4) (1,1) (1,16).
"""
from collections import namedtuple

import numpy as np

WAVE, RN_WAVES, RN_THREADS, MAX_C = 64, 4, 256, 1024
RED_GROUPS = 64                      # column_reduce: row b of `partials` goes to group b % 64
PARTIAL_ROWS_CAP = 1024              # RESIDUAL_NORM_PARTIAL_ROWS, BATCH_NORM_PARTIAL_ROWS
INSTANCES = ((4, 1), (4, 2), (4, 4), (1, 1), (1, 16))
ELEM_BYTES = {"f32": 4, "f16": 2, "bf16": 2}

Shape = namedtuple("Shape", "vec iter chunks seg per_wave rows_per_wg")


def row_shape(c, chunked):
    """RowShape(c, chunked), and SegLanes' per_wave"""
    vec = 4 if chunked else 1
    chunks = c // vec
    if chunks <= WAVE:
        it, seg = 1, 1
        while seg < chunks:
            seg <<= 1
    else:
        seg = WAVE
        it = 16 if vec == 1 else 2 if chunks <= 2 * WAVE else 4
    return Shape(vec, it, chunks, seg, WAVE // seg, RN_WAVES * (WAVE // seg))


def chunked_for(c, elem_bytes, misaligned):
    """the launchers' condition: c % 4 == 0 and every [n, c] operand aligned for the chunk accesses - 16 bytes for fp32 rows, 8 for half
    rows.  misaligned: the operands are contiguous views one element into an aligned buffer (c % 4 == 0 keeps every later row as
    aligned as the first)."""
    need = 16 if elem_bytes == 4 else 8
    return c % 4 == 0 and ((elem_bytes if misaligned else 0) % need) == 0


def shape_of(c, misaligned, rows="f32"):
    return row_shape(c, chunked_for(c, ELEM_BYTES[rows], misaligned))


def used_iterations(shape):
    return -(-shape.chunks // WAVE) if shape.iter > 1 else 1


def live_lanes(shape, it):
    """the lanes of a segment with chunk0 + 64 * it < chunks"""
    return int(min(max(shape.chunks - WAVE * it, 0), shape.seg))


def fill_of(shape):
    """"full": every lane of the segment has a chunk in every iteration of the instance"""
    return "full" if shape.chunks == shape.seg * shape.iter else "partial"


def last_has_one_lane(shape):
    """an instance of several iterations whose last used iteration has a single live lane"""
    return shape.iter > 1 and live_lanes(shape, used_iterations(shape) - 1) == 1


# (c, misaligned) and what the entry claims: the instance, the segment width, "full" / "partial", and whether the last used iteration has
# one live lane.  tests/test_row_lanes_cases_cpu.py holds every claim against row_shape.
Width = namedtuple("Width", "c misaligned vec iter seg fill last_one")
_F, _P = "full", "partial"
WIDTHS = [
    # four channels a lane, a segment per row: 64, 32, 16, 8, 4, 2 and 1 rows side by side in a wave
    Width(4, False, 4, 1, 1, _F, False), Width(8, False, 4, 1, 2, _F, False), Width(12, False, 4, 1, 4, _P, False),
    Width(16, False, 4, 1, 4, _F, False), Width(20, False, 4, 1, 8, _P, False), Width(32, False, 4, 1, 8, _F, False),
    Width(48, False, 4, 1, 16, _P, False), Width(64, False, 4, 1, 16, _F, False), Width(100, False, 4, 1, 32, _P, False),
    Width(128, False, 4, 1, 32, _F, False), Width(252, False, 4, 1, 64, _P, False), Width(256, False, 4, 1, 64, _F, False),
    # two and four chunks a lane
    Width(260, False, 4, 2, 64, _P, True), Width(384, False, 4, 2, 64, _P, False), Width(512, False, 4, 2, 64, _F, False),
    Width(516, False, 4, 4, 64, _P, True), Width(768, False, 4, 4, 64, _P, False), Width(1020, False, 4, 4, 64, _P, False),
    Width(1024, False, 4, 4, 64, _F, False),
    # one channel a lane: c % 4 != 0 ...
    Width(1, False, 1, 1, 1, _F, False), Width(2, False, 1, 1, 2, _F, False), Width(3, False, 1, 1, 4, _P, False),
    Width(5, False, 1, 1, 8, _P, False), Width(7, False, 1, 1, 8, _P, False), Width(13, False, 1, 1, 16, _P, False),
    Width(29, False, 1, 1, 32, _P, False), Width(63, False, 1, 1, 64, _P, False),
    Width(65, False, 1, 16, 64, _P, True), Width(70, False, 1, 16, 64, _P, False), Width(1022, False, 1, 16, 64, _P, False),
    Width(1023, False, 1, 16, 64, _P, False),
    # ... or a chunkable width behind a misaligned view
    Width(4, True, 1, 1, 4, _F, False), Width(8, True, 1, 1, 8, _F, False), Width(16, True, 1, 1, 16, _F, False),
    Width(32, True, 1, 1, 32, _F, False), Width(64, True, 1, 1, 64, _F, False), Width(96, True, 1, 16, 64, _P, False),
    Width(1024, True, 1, 16, 64, _F, False),
]

# per row type a part of WIDTHS that still takes all five instances, each also at a one-lane tail or full
TYPE_CASES = {
    "f32": [(16, False), (100, False), (260, False), (512, False), (1020, False), (5, False), (64, True), (65, False), (1023, False)],
    "f16": [(12, False), (32, False), (256, False), (260, False), (512, False), (516, False), (1024, False), (7, False), (63, False),
            (64, True), (65, False), (1023, False), (1024, True)],
    "bf16": [(4, False), (8, False), (20, False), (128, False), (252, False), (384, False), (768, False), (3, False), (16, True),
             (70, False), (96, True), (1022, False)],
}

# one width per instance, the one-lane tail where the instance has one
INSTANCE_WIDTHS = {(4, 1): (100, False), (4, 2): (260, False), (4, 4): (516, False), (1, 1): (63, False), (1, 16): (65, False)}


def width_id(w):
    c, misaligned = w[0], w[1]
    return f"c{c}{'mis' if misaligned else ''}"


def row_count_names(shape):
    """the row counts on the boundaries of a shape, by name: around the rows of one wave, around those of one workgroup, and three
    workgroups' rows plus a wave's plus one (every wave of a workgroup takes a second turn where the grid is capped, and the last wave
    holds one live row beside dead ones)"""
    pw, wg = shape.per_wave, shape.rows_per_wg
    return {"per_wave - 1": pw - 1, "per_wave": pw, "per_wave + 1": pw + 1, "rows_per_wg - 1": wg - 1, "rows_per_wg + 1": wg + 1,
            "3 * rows_per_wg + per_wave + 1": 3 * wg + pw + 1}


def row_counts(shape, training=False):
    """the distinct values >= 1 (batch norm in training mode: >= 2) of row_count_names, ascending"""
    return sorted({n for n in row_count_names(shape).values() if n >= (2 if training else 1)})


def big_count(shape):
    return 3 * shape.rows_per_wg + shape.per_wave + 1


def partial_rows(n, shape, cap=PARTIAL_ROWS_CAP):
    """the rows of `partials` a reduction over n rows leaves: the operators offer min(cap, (n + 3) // 4) rows, RowShape::grid takes
    div_up(n, rows_per_wg) of them at most"""
    offered = min(cap, max(1, (n + 3) // 4))
    return min(offered, -(-n // shape.rows_per_wg))


def partial_row_counts(c=48):
    """n at which column_reduce is fed RED_GROUPS - 1, RED_GROUPS and RED_GROUPS + 1 partial rows: the last group empty, one row in every
    group, a second row in group 0.  The first two are the largest such n (the last workgroup full), the third the smallest (the
    last workgroup holds one row)."""
    shape = row_shape(c, c % 4 == 0)
    rows = {}
    for n in range(1, 4 * PARTIAL_ROWS_CAP * shape.rows_per_wg):
        rows.setdefault(partial_rows(n, shape), []).append(n)
        if partial_rows(n, shape) > RED_GROUPS + 1:
            break
    return [max(rows[RED_GROUPS - 1]), max(rows[RED_GROUPS]), min(rows[RED_GROUPS + 1])]


# ---------------------------------------------------------------------------------------------------------------------
# one workgroup's lanes, modelled: which value lands where.  x [n, c] holds small integers in float64, so every sum is exact and a wrong
# result is a wrong index, never rounding.
# ---------------------------------------------------------------------------------------------------------------------
MISTAKES = ("idle lanes not masked", "butterfly started at seg / 2", "lane0 taken without & 63", "it dropped")


def _lane_values(x, shape, mistake):
    """v [wave, lane, it, e, turn]: what each lane of one workgroup loads per turn of its row loop (a grid of one workgroup: a wave's
    rows are per_wave * (wave + 4 * turn) + sub), live [wave, lane, turn].  An idle lane that is not masked reads on past its row's end
    (zeros past the buffer)."""
    n, c = x.shape
    flat = np.concatenate([x.reshape(-1), np.zeros(WAVE * 16 * 4)])
    turns = -(-n // shape.rows_per_wg)
    v = np.zeros((RN_WAVES, WAVE, shape.iter, shape.vec, turns))
    live = np.zeros((RN_WAVES, WAVE, turns), bool)
    for w in range(RN_WAVES):
        for lane in range(WAVE):
            sub, chunk0 = lane // shape.seg, lane & (shape.seg - 1)
            for t in range(turns):
                row = shape.per_wave * (w + RN_WAVES * t) + sub
                if row >= n:
                    continue
                live[w, lane, t] = True
                for it in range(shape.iter):
                    chunk = chunk0 + it * WAVE
                    if chunk < shape.chunks or mistake == "idle lanes not masked":
                        at = row * c + chunk * shape.vec
                        v[w, lane, it, :, t] = flat[at:at + shape.vec]
    return v, live


def model_row_sums(x, shape, mistake=None):
    """seg_sum of a row's channels as the kernels form it: each lane adds its chunks, an xor butterfly over the strides 1 .. seg / 2
    spreads the sum over the segment -> [n], read from the lane with chunk0 == 0 as the forward's `stat` is"""
    n = x.shape[0]
    v, live = _lane_values(x, shape, mistake)
    out = np.zeros(n)
    first = max(shape.seg // 2, 1) if mistake == "butterfly started at seg / 2" else 1
    for w in range(RN_WAVES):
        for t in range(v.shape[-1]):
            s = v[w, :, :, :, t].sum(axis=(1, 2))
            st = first
            while st < shape.seg:
                s = s + s[np.arange(WAVE) ^ st]
                st <<= 1
            for lane in range(0, WAVE, shape.seg):
                if live[w, lane, t]:
                    out[shape.per_wave * (w + RN_WAVES * t) + lane // shape.seg] = s[lane]
    return out


def model_column_sums(x, shape, mistake=None):
    """workgroup_columns with `+`: each lane adds its rows per channel, the segments of a wave merge by an xor butterfly over the strides
    seg .. 32, the waves through `red`, thread ch reads entry (it, lane0) of every wave -> [c].  A read past `red` gives 0."""
    n, c = x.shape
    v, _ = _lane_values(x, shape, mistake)
    v = v.sum(-1)                                                              # [wave, lane, it, e]
    st = max(shape.seg // 2, 1) if mistake == "butterfly started at seg / 2" else shape.seg
    while st < WAVE:
        v = v + v[:, np.arange(WAVE) ^ st]
        st <<= 1
    red = np.zeros(RN_THREADS * shape.iter * shape.vec)
    for w in range(RN_WAVES):
        for it in range(shape.iter):
            for lane in range(WAVE):
                at = ((w * shape.iter + it) * WAVE + lane) * shape.vec
                red[at:at + shape.vec] = v[w, lane, it]
    out = np.zeros(c)
    for ch in range(c):
        chunk = ch // shape.vec
        e = ch - chunk * shape.vec
        it = 0 if mistake == "it dropped" else chunk >> 6
        lane0 = chunk if mistake == "lane0 taken without & 63" else chunk & 63
        for w in range(RN_WAVES):
            at = ((w * shape.iter + it) * WAVE + lane0) * shape.vec + e
            out[ch] += red[at] if at < red.size else 0.0
    return out


def model_inputs(n, c, seed, replicated=False):
    """small integers; replicated: every column holds column 0's"""
    x = np.random.default_rng(seed).integers(1, 8, (n, c)).astype(np.float64)
    return np.repeat(x[:, :1], c, 1) if replicated else x
