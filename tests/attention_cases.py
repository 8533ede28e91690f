"""Cases, float64 references and derived error bounds for the pair-list attention operators: A1 `attention_step1_v2`
(csrc/attention.hip), A2 `dot_prod_with_idx_v3` and A4 `attention_step2_with_rel_pos_value_v2` (csrc/rpe.hip, rpe_bwd_mfma.hip,
rpe_fallback.hip) and the fused `fused.window_attention` built on them.  numpy only; tests/test_attention_cases_cpu.py pins the
dispatch below to the sources, proves that the case table reaches every region, that a correct fp32 implementation (the C oracle,
a numpy emulation of the fixed-point histogram) meets the bounds and that wrong variants miss them; tests/test_attention_hip.py
runs the cases on the device.  DESIGN.md 2.3 has the derivations.

The dispatch (`path_of`).  Every rel-pos launcher first looks at `table_rows` (L); without it the generic global-memory kernels run.

    op           condition                                family           heads per workgroup            LDS images (narr)
    a1_fwd       always                                   rows             LPG = D / 4 (clamped loads)    q row only
                 N < 20000: head groups on blockIdx.y (y-groups), else one y and a loop over the groups (y-loop)
    a1_bwd       always (grad_q: gather by query)         rows             HC = 4 per pass               -
                 grad_k: the same gather by key with a CSC, else scatter_atomic_kernel (keyside)
    a2_fwd       L given                                  lds-slice        pick_hg(narr = 2)             Tq, Tk
    a2_bwd       L given, d = 16, CSC, L <= 80            mfma             min(h, 3)                     T (rows) + histograms
                 L given, otherwise, CSC                  lds-slice        pick_hg(narr = 2)             T, G  (by query, by key)
                 L given, otherwise, no CSC               lds-slice        pick_hg(narr = 4)  keyside    Tq, Gq, Tk, Gk
    a4_fwd       L given                                  lds-slice        pick_hg(narr = 1)             Tv
    a4_bwd       L given, d = 16, CSC, L <= 80            mfma             min(h, 3)                     T + histograms
                 L given, otherwise                       lds-slice        pick_hg(narr = 2)             Tv, Gv (keyside without CSC)
    any of A2/A4 L not given                              fallback-global  one thread per (pair, head)   -
    wlogit_fwd   d = 16 (the wrapper refuses others)      lds-slice        pick_hg(narr = 2)             Tq, Tk
    wattn_bwd    CSC and L <= 80                          mfma             min(h, 3)                     2 (Tv, Tq)
                 otherwise                                operators        the A4 / softmax / A1 / A2 backward launchers

    pick_hg(h, L, D, narr): per_head = narr * 3 * L * D * 4 bytes; hg = floor(72 KiB / per_head) capped at 3 and at h;
    hg = 0 and per_head <= 150 KiB: one head, one workgroup per CU (big_lds); above 150 KiB: error "rel-pos table slice does not
    fit in LDS", raised before any launch.  In L, for (narr, D):

        (1, 16)            HG 3: L <= 128   HG 2: <= 192   HG 1: <= 384   big: <= 800   error: >= 801
        (1, 32), (2, 16)   HG 3: L <= 64    HG 2: <= 96    HG 1: <= 192   big: <= 400   error: >= 401
        (2, 32), (4, 16)   HG 3: L <= 32    HG 2: <= 48    HG 1: <= 96    big: <= 200   error: >= 201
        (4, 32)            HG 3: L <= 16    HG 2: <= 24    HG 1: <= 48    big: <= 100   error: >= 101

    mfma: table_grad_kernel<HG, TA> with TA = 4 bin tiles for L <= 64, 5 for 64 < L <= 80; a row is walked in segments of
    16 * TG_MAXP = 128 pairs, each with a fixed-point scale of its own.  The fused kernels keep a row's logits in registers up to
    PPW * WL_MAXP = PPW * WB_MAXP = 128 pairs and park them in the output beyond.
    row_order: the kernels of the launch that take their rows in window order: N >= 2048 (pointops.row_order_of) AND a grid
    that is a multiple of 8 (RowSlots, the table gradient's `share` remap).  The one-slot-per-wave grids of A1 always are; a
    persistent walker has walk_blocks(N, groups, waves, per CU) = min(ceil(N / waves), cap) workgroups: at N = 2048 the 8-wave
    walkers have 256 and take the order, the 12-wave ones (A2 forward, fused logits, table gradients) have 171 and do not; at
    N = 2112 both do (264 and 176).  Figures for a whole MI355X (256 CUs, none held).

Every case is a seeded CSR pair list with N_k = N, rel_idx in [0, L) everywhere, and finite operands with |x| in [2^-8, 2^4] or 0.
The axes of the table are listed at `SPECS`.  Bounds are per element in units of u = 2^-24; none is hand-picked.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.pair_ops_cases import U, csc_ref, fraction_of_bound, softmax_bwd_f64, softmax_f64, softmax_fwd_bound

# ---------------------------------------------------------------------------------------------------------------------
# the launchers' own conditions, restated (tests/test_attention_cases_cpu.py pins every constant to the sources)
# ---------------------------------------------------------------------------------------------------------------------
LDS_BUDGET = 72 * 1024      # rpe_common.h kLdsBudget
ONE_WG_LIMIT = 150 * 1024   # rpe.hip pick_hg: one workgroup per CU up to here
HG_CAP = 3                  # rpe.hip pick_hg, rpe_common.h with_head_group
MFMA_L_MAX = 80             # rpe_bwd_mfma.hip, rpe.hip (A4 backward), fused.py
TA4_L_MAX = 64              # rpe_bwd_mfma.hip: TableGeo<HG, 4> up to here, <HG, 5> beyond
A1_LOOP_N = 20000           # attention.hip: head groups over blockIdx.y below
ROW_ORDER_N = 2048          # pointops.row_order_of, common.h rows_in_order
TG_WAVES, TG_MAXP, WL_MAXP, WB_MAXP, HC = 12, 8, 8, 8, 4
SEGMENT = 16 * TG_MAXP      # pairs of one fixed-point segment
NUM_CUS = 256               # common.h kNumCU
# walk_blocks(rows, groups, waves per workgroup, workgroups per CU) of the persistent walkers, by launcher and kernel role
WALKERS = {"a2_fwd": {"walk": (12, 2)}, "a4_fwd": {"walk": (8, 3)}, "mfma_bwd": {"walk": (8, 4), "tables": (TG_WAVES, 2)},
           "wattn_bwd": {"walk": (8, 2), "tables": (TG_WAVES, 2)}}
ORDER_N = 2112              # an N >= 2048 at which N / 8 = 264 and N / 12 = 176 are both multiples of 8
HEADS = (1, 2, 3, 4, 5, 7)
OPS = ("a1_fwd", "a1_bwd", "a2_fwd", "a2_bwd", "a4_fwd", "a4_bwd", "wlogit_fwd", "wattn_bwd")

Path = namedtuple("Path", "family D HG hgn_last TA narr lds_bytes big_lds keyside a1_grid row_order")


def lpg(d):
    return d // 4


def ppw(d):
    return 64 // lpg(d)


def pick_hg(h, L, D, narr):
    per_head = narr * 3 * L * D * 4
    hg = LDS_BUDGET // per_head
    if hg < 1:
        return 1 if per_head <= ONE_WG_LIMIT else 0
    return min(hg, HG_CAP, h)


def _last(h, g):
    """heads in the last group of g"""
    return h - (-(-h // g) - 1) * g


def walk_blocks(rows, groups, waves_per_block, per_cu):
    """rpe_common.h walk_blocks on a whole MI355X with no CU held: grid.x of a persistent walker"""
    cap = NUM_CUS * per_cu
    if groups > 1:
        cap = max(NUM_CUS * per_cu // groups, NUM_CUS // 2)
    return max(1, min(-(-rows // waves_per_block), cap))


def _ordered(N, groups, walkers):
    """the kernels of a launch that take their rows in window order: N >= 2048 AND a grid that is a multiple of 8 (RowSlots and
    the table gradient's `share` remap fall back to the index order otherwise).  walkers: None for the one-slot-per-wave grids
    (ordered_grid: always a multiple of 8), else {role: (waves per workgroup, workgroups per CU)}"""
    if N < ROW_ORDER_N:
        return ()
    if walkers is None:
        return ("walk",)
    return tuple(role for role, (wpb, per_cu) in walkers.items() if walk_blocks(N, groups, wpb, per_cu) % 8 == 0)


def _slice(h, d, L, narr, keyside, N=0, walkers=None):
    hg = pick_hg(h, L, d, narr)
    if hg == 0:
        return Path("error", d, 0, 0, None, narr, narr * 3 * L * d * 4, True, False, None, ())
    lds = narr * hg * 3 * L * d * 4
    order = _ordered(N, -(-h // hg), walkers) if walkers else ()
    return Path("lds-slice", d, hg, _last(h, hg), None, narr, lds, lds > LDS_BUDGET, keyside, None, order)


def _mfma(h, L, narr, N, walkers):
    hg = min(h, HG_CAP)
    lds = narr * hg * 3 * L * 16 * 4
    return Path("mfma", 16, hg, _last(h, hg), 4 if L <= TA4_L_MAX else 5, narr, lds, lds > LDS_BUDGET, False, None,
                _ordered(N, -(-h // hg), walkers))


def path_of(op, N, h, d, L, csc, table_rows=True):
    """what the launchers pick for `op` on N query rows, h heads of d, tables of L rows, with or without a CSC view"""
    assert op in OPS and d in (16, 32)
    if op == "a1_fwd":
        return Path("rows", d, lpg(d), _last(h, lpg(d)), None, 0, 4 * h * d * 4, False, False, "y-groups" if N < A1_LOOP_N else "y-loop",
                    _ordered(N, 1, None))
    if op == "a1_bwd":
        return Path("rows", d, HC, _last(h, HC), None, 0, 0, False, not csc, None, _ordered(N, 1, None))
    if op == "wlogit_fwd":
        assert d == 16 and table_rows
        return _slice(h, 16, L, 2, False, N, WALKERS["a2_fwd"])
    if op == "wattn_bwd":
        assert d == 16 and table_rows
        if csc and L <= MFMA_L_MAX:
            return _mfma(h, L, 2, N, WALKERS["wattn_bwd"])
        return Path("operators", 16, 0, 0, None, 0, 0, False, not csc, None, ())
    if not table_rows:
        return Path("fallback-global", d, 1, 1, None, 0, 0, False, op.endswith("bwd"), None, ())
    if op == "a2_fwd":
        return _slice(h, d, L, 2, False, N, WALKERS["a2_fwd"])
    if op == "a4_fwd":
        return _slice(h, d, L, 1, False, N, WALKERS["a4_fwd"])
    if d == 16 and csc and 1 <= L <= MFMA_L_MAX:  # a2_bwd, a4_bwd
        return _mfma(h, L, 1, N, WALKERS["mfma_bwd"])
    if op == "a2_bwd":  # (the by-query / by-key slice kernels of the backwards stride the grid by index)
        return _slice(h, d, L, 2 if csc else 4, not csc)
    return _slice(h, d, L, 2, not csc)


def kernel_id(p):
    s = f"{p.family}-D{p.D}"
    if p.family in ("rows", "lds-slice", "mfma"):
        s += f"-HG{p.HG}.{p.hgn_last}"
    if p.TA:
        s += f"-TA{p.TA}"
    if p.narr:
        s += f"-n{p.narr}"
    return s + ("-big" if p.big_lds and p.family != "error" else "") + ("-key" if p.keyside else "")


def path_id(p):
    return kernel_id(p) + (f"-{p.a1_grid}" if p.a1_grid else "") + ("-ord:" + "+".join(p.row_order) if p.row_order else "")


def facets(op, p):
    """what a launch of `op` on path p covers: the kernel instance with its head-group guards, the way rows are handed out and,
    for the A1 forward, the grid"""
    out = {"kernel:" + kernel_id(p)}
    for role in ROLES.get((op, p.family), ()):
        out.add(f"rows:{p.family}:{role}:{'order' if role in p.row_order else 'index'}")
    if p.a1_grid:
        out.add(f"grid:D{p.D}:{p.a1_grid}")
    return out


# the kernel roles of a launch that CAN take their rows in window order
ROLES = {("a1_fwd", "rows"): ("walk",), ("a1_bwd", "rows"): ("walk",), ("a2_fwd", "lds-slice"): ("walk",), ("a4_fwd", "lds-slice"): ("walk",),
         ("wlogit_fwd", "lds-slice"): ("walk",), ("a2_bwd", "mfma"): ("walk", "tables"), ("a4_bwd", "mfma"): ("walk", "tables"),
         ("wattn_bwd", "mfma"): ("walk", "tables")}
L_SCAN = 802  # one past the first L at which no (narr, D) fits any more


@lru_cache(maxsize=None)
def all_facets(op):
    """every facet `op` can have for h in HEADS, d in {16, 32} (the fused pair: 16), any L, N on both sides of its thresholds"""
    ds = (16,) if op in ("wlogit_fwd", "wattn_bwd") else (16, 32)
    trs = (True,) if op.startswith(("a1", "w")) else (True, False)
    out = set()
    for h in HEADS:
        for d in ds:
            for csc in (True, False):
                for tr in trs:
                    for L in (range(1, L_SCAN) if not op.startswith("a1") else (16,)):
                        out |= facets(op, path_of(op, 300, h, d, L, csc, tr))
                    for N in (ROW_ORDER_N - 1, ROW_ORDER_N, ORDER_N, A1_LOOP_N - 1, A1_LOOP_N):
                        for L in (16, 64, 81, 100):
                            out |= facets(op, path_of(op, N, h, d, L, csc, tr))
    return frozenset(out)


def hg_edges(op, d, csc):
    """-> [(L, h)]: both sides of every change of (family, HG, big_lds) of `op` along L, one L inside the big-LDS region, the last
    L that fits and the first that does not; h the smallest head count that shows the change"""
    pts, prev, big = [], None, []
    for L in range(1, L_SCAN + 1):
        p = path_of(op, 300, 3, d, L, csc)
        key = (p.family, p.HG, p.big_lds)
        if p.family != "error" and p.big_lds:
            big.append(L)
        if prev is not None and key != prev:
            h = 3 if 3 in (prev[1], key[1]) else 2 if 2 in (prev[1], key[1]) else 2 if key[0] != "error" else 1
            pts += [(L - 1, h), (L, h)]
        prev = key
        if p.family == "error":
            break
    if big:
        pts.append((big[len(big) // 2], 2))
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
Spec = namedtuple("Spec", "name N h d L csc table_rows layout ops")
SPECIAL = {"full": (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 256, 257),   # 0, 1, PPW - 1, PPW, PPW + 1 for both PPW, the segment edges
           "small": (1, 7, 8, 9, 15, 16, 17, 129),
           "sparse": (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 257)}
LAYOUT_N = {"full": 300, "small": 40}
KEY_A, KEY_B, KEY_SAME = 7, 11, 13      # shared by 257 queries, by 129 queries, the one key of the same-key row
BIN_Q, BIN_K = 1, 2                      # bins only the small-weight segments use (by query, by key), L >= 8
FUSED_H, FUSED_L = (1, 2, 4, 5), (17, 64, 80)


def _specs():
    table = {}

    def add(tag, h, d, L, csc=True, tr=True, layout="full", ops=("a1", "a2", "a4"), N=None):
        N = LAYOUT_N[layout] if N is None else N
        key = (N, h, d, L, csc, tr, layout)
        old = table.get(key)
        merged = tuple(o for o in ("a1", "a2", "a4", "fused") if o in ops or (old and o in old[1]))
        table[key] = (old[0] if old else tag, merged)

    for h in HEADS:                                   # heads x head dim with a CSC; d = 16: the MFMA instances, both tile counts
        add("heads", h, 16, 48)
        add("heads", h, 16, 80)
        add("heads", h, 32, 24)
        add("heads-nocsc", h, 16, 24, csc=False)      # KEYSIDE = true, scatter_atomic_kernel
        add("heads-nocsc", h, 32, 16, csc=False)
    for L in (1, 15, 16, 17, 63, 64, 65, 79, 80, 81):  # both table-gradient tile counts; 81 falls to the slice kernels
        add("L", 5, 16, L)
    for h in FUSED_H:                                 # the fused module on the 127 / 128 / 129-pair rows
        for L in FUSED_L:
            add("fused", h, 16, L, ops=("a1", "a2", "a4", "fused"))
    add("fused-nocsc", 5, 16, 17, csc=False, ops=("a2", "a4", "fused"))
    for d in (16, 32):                                # pick_hg edges of every (narr, D), taken from path_of
        for csc in (True, False):
            for op in ("a4_fwd", "a2_fwd", "a2_bwd", "a4_bwd"):   # an edge runs its own operator only: the three-head edges of
                for L, h in hg_edges(op, d, csc):                 # one (narr, D) would be big-LDS launches of another
                    add("edge", h, d, L, csc=csc, layout="small", ops=(op[:2],) + (("fused",) if op == "a2_fwd" and d == 16 else ()))
    for N in (A1_LOOP_N, A1_LOOP_N - 1):              # the two grids of the A1 forward
        for h in (3, 5):
            for d in (16, 32):
                add("a1grid", h, d, 16, layout="sparse", ops=("a1",), N=N)
    for N in (ORDER_N, ROW_ORDER_N, ROW_ORDER_N - 1):  # rows in window order: every walker, the 8-wave walkers only, none
        for h in (2, 4):
            add("order", h, 16, 64, layout="sparse", ops=("a1", "a2", "a4", "fused"), N=N)
    add("order", 3, 32, 24, layout="sparse", N=ROW_ORDER_N)
    for h in (1, 5):                                  # table_rows unset: the global-memory kernels
        for d in (16, 32):
            add("fallback", h, d, 48, csc=False, tr=False, ops=("a2", "a4"))
    out = []
    for (N, h, d, L, csc, tr, layout), (tag, ops) in table.items():
        name = f"{tag}-N{N}-h{h}-d{d}-L{L}-{'csc' if csc else 'nocsc'}" + ("" if tr else "-noL")
        out.append(Spec(name, N, h, d, L, csc, tr, layout, ops))
    return tuple(out)


SPECS = _specs()
OPS_OF = {"a1": ("a1_fwd", "a1_bwd"), "a2": ("a2_fwd", "a2_bwd"), "a4": ("a4_fwd", "a4_bwd"), "fused": ("wlogit_fwd", "wattn_bwd")}


def paths(spec, group):
    return tuple(path_of(op, spec.N, spec.h, spec.d, spec.L, spec.csc, spec.table_rows) for op in OPS_OF[group])


def specs_of(group):
    return [s for s in SPECS if group in s.ops]


def spec_id(group):
    return lambda s: s.name + "-" + "-".join(path_id(p) for p in paths(s, group))


def _vals(rng, shape, scale, zeros=0.03):
    """finite, |x| in [2^-8, 2^4] or exactly 0"""
    x = rng.standard_normal(shape) * scale
    mag = np.clip(np.abs(x), 2.0 ** -8, 2.0 ** 4)
    x = np.where(x < 0, -mag, mag)
    x[rng.random(shape) < zeros] = 0
    return np.ascontiguousarray(x, np.float32)


# The weights of the small-weight segments alternate between these two: exact at the segment's own scale (2^29), and each a
# quarter step BELOW its rounded value at the scale of a segment that holds a 16 (2^17), so a reused scale is off by 32 steps
# while the true bin sum nearly cancels (a sequential fp32 sum stays well inside the bound too)
SMALL_W = (2.0 ** -8 * (1 + 2.0 ** -11), -(2.0 ** -8) * (1 + 3 * 2.0 ** -11))
ANCHOR_W = 16.0


class Case:
    """one pair list with its operands (all read-only): offsets [N + 1], index_1 [M], rel_idx [M, 3] i32; q, k, v, go_rows
    [N, h, d]; table_q, table_k, table_v [L, h, d, 3]; go_pairs, attn [M, h] f32 (attn: the weights of A4, any sign)"""

    def __init__(self, spec):
        self.spec = spec
        N, h, d, L, layout = spec.N, spec.h, spec.d, spec.L, spec.layout
        rng = np.random.default_rng(N * 1000003 + h * 10007 + d * 101 + L * 7 + spec.csc * 3 + spec.table_rows)
        special = SPECIAL[layout]
        if layout == "sparse":   # about 48 non-empty rows; the first partners DEscend with the row index (see below)
            live = sorted(set([4, 5, N - 6, N - 5] + np.linspace(N // 8, 7 * N // 8, 44).astype(int).tolist()))
            at = live[2:2 + len(special)]
        else:                    # empty rows at 0..3, N-4..N-1 and mid-table
            mid = (N // 2, N // 2 + 1, N // 2 + 2) if layout == "full" else (N // 2,)
            live = [r for r in range(4, N - 4) if r not in mid]
            at = live[5::23][:len(special)] if layout == "full" else live[1::4][:len(special)]
        assert len(at) == len(special)
        lens = np.zeros(N, np.int64)
        lens[live] = rng.integers(2, 7, len(live))
        lens[at] = special
        self.row_with = dict(zip(special, at))
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        M = int(offsets[-1])
        index_1 = rng.integers(0, N, M).astype(np.int32)
        allowed = np.array([b for b in range(L) if L < 8 or b not in (BIN_Q, BIN_K)])
        rel = allowed[rng.integers(0, len(allowed), (M, 3))].astype(np.int32)
        go_pairs, attn = _vals(rng, (M, h), 1.0), _vals(rng, (M, h), 0.4)
        starts = offsets[:-1]
        plain = [r for r in live if r not in at]
        if L <= 96:  # the bins a dropped tile would lose are in use on every axis
            for i, b in enumerate(sorted({L - 1, min(64, L - 1), min(16 * (L // 16), L - 1)})):
                for ax in range(3):
                    rel[starts[plain[-1 - (3 * i + ax)]], ax] = b
        self.scale_rows = layout == "full" and L >= 8
        if layout == "full":
            same_key, same_rel, long_row = self.row_with[127], self.row_with[129], self.row_with[257]
            for key in (KEY_A, KEY_B, KEY_SAME):
                index_1[index_1 == key] = key + 1
            rows_a = [r for r in live if r not in (same_key, same_rel)][:257]
            rows_b = [r for r in live if r not in (same_key, same_rel) and lens[r] >= 2][:129]
            index_1[starts[rows_a]] = KEY_A                  # one key shared by 257 queries, one by 129: CSC rows past 128 pairs
            index_1[starts[rows_b] + 1] = KEY_B
            index_1[offsets[same_key]:offsets[same_key + 1]] = KEY_SAME
            if self.scale_rows:  # second segments whose weights are 2^12 below the first segment's largest, in bins of their own
                s = offsets[long_row]
                of_key = np.flatnonzero(index_1 == KEY_A)
                for first, sel, b in ((s, np.arange(s + SEGMENT, s + 2 * SEGMENT), BIN_Q), (of_key[0], of_key[SEGMENT:2 * SEGMENT], BIN_K)):
                    rel[sel] = b
                    go_pairs[sel] = attn[sel] = np.resize(np.float32(SMALL_W), len(sel))[:, None]
                    go_pairs[first] = attn[first] = ANCHOR_W
            rel[offsets[same_rel]:offsets[same_rel + 1]] = allowed[[3 % len(allowed), 4 % len(allowed), 5 % len(allowed)]]
        elif layout == "sparse":
            firsts = np.sort(rng.choice(N, len(live), replace=False))[::-1]
            firsts[0], firsts[-1] = N - 1, 0
            index_1[starts[live]] = firsts
        self.N, self.h, self.d, self.L, self.M, self.live = N, h, d, L, M, tuple(live)
        self.offsets, self.index_1, self.rel_idx = offsets, index_1, np.ascontiguousarray(rel)
        self.q, self.k, self.v = _vals(rng, (N, h, d), 0.5), _vals(rng, (N, h, d), 1.0), _vals(rng, (N, h, d), 1.0)
        self.table_q, self.table_k, self.table_v = (_vals(rng, (L, h, d, 3), 0.3) for _ in range(3))
        self.go_rows, self.go_pairs, self.attn = _vals(rng, (N, h, d), 1.0), go_pairs, attn
        self.n_max = int(lens.max())
        for a in self.arrays().values():
            a.setflags(write=False)
        # derived: the query and the position in its row of every pair; the key-major view and the position in it
        self.row = np.repeat(np.arange(N), lens)
        self.pos = np.arange(M) - offsets[self.row]
        self.lens = lens
        self.csc_offsets, self.csc_pair, _ = csc_ref(self.row, index_1, N)
        self.cpos = np.empty(M, np.int64)
        self.cpos[self.csc_pair] = np.arange(M) - self.csc_offsets[index_1[self.csc_pair]]
        self.key_count = np.diff(self.csc_offsets).astype(np.int64)
        self._cache = {}

    def arrays(self):
        names = "offsets index_1 rel_idx q k v table_q table_k table_v go_rows go_pairs attn"
        return {n: getattr(self, n) for n in names.split()}


@lru_cache(maxsize=16)
def case(spec):
    return Case(spec)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements, one per operator, forward and backward.  `fault`: the same with one defect (FAULTS)
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("prev_table_slice", "last_head_not_stored", "bins_from_64_dropped", "bins_of_the_partial_tile_dropped",
          "second_segment_dropped", "second_segment_reuses_scale", "last_pair_dropped", "slot_past_end_added",
          "key_side_from_query_table", "axes_swapped", "gather_chunk_skipped")


class _Model:
    def __init__(self, c, fault=None):
        self.c, self.fault = c, fault
        f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
        self.q, self.k, self.v, self.gr = f64(c.q), f64(c.k), f64(c.v), f64(c.go_rows)
        self.tq, self.tk, self.tv = f64(c.table_q), f64(c.table_k), f64(c.table_v)
        self.row, self.j, self.rel = c.row, c.index_1.astype(np.int64), c.rel_idx.astype(np.int64)
        self.keep = np.ones(c.M)
        self.extra_rows = self.extra_pairs = np.zeros(0, np.int64)
        ends = c.offsets[1:][c.lens > 0].astype(np.int64)
        if fault == "last_pair_dropped":
            self.keep[ends - 1] = 0
        if fault == "slot_past_end_added":  # the slot behind the row: the next row's first pair (the last row: its own last pair)
            self.extra_rows, self.extra_pairs = np.flatnonzero(c.lens > 0), np.minimum(ends, c.M - 1)
        self.axes = (0, 2, 1) if fault == "axes_swapped" else (0, 1, 2)

    # table sums per pair [M, h, d]: T[r0, ., ., 0] + T[r1, ., ., 1] + T[r2, ., ., 2], or the sum of the absolute values
    def tsum(self, T, absolute=False):
        T = np.abs(T) if absolute else T
        out = sum(T[self.rel[:, self.axes[ax]], :, :, ax] for ax in range(3))
        if self.fault == "prev_table_slice" and self.c.h >= 2 and not absolute:
            out[:, -1] = out[:, -2]
        return out

    def per_pair(self, x):
        return x * self.keep.reshape((-1,) + (1,) * (x.ndim - 1))

    def rowsum(self, terms):
        out = np.zeros((self.c.N,) + terms.shape[1:])
        np.add.at(out, self.row, self.per_pair(terms))
        np.add.at(out, self.extra_rows, terms[self.extra_pairs])
        return out

    def keysum(self, terms):
        out = np.zeros((self.c.N,) + terms.shape[1:])
        np.add.at(out, self.j, self.per_pair(terms))
        return out

    def scatter(self, w, X, xidx, side):
        """table gradient [L, h, d, 3]: entry (r, hh, i, ax) sums w[m, hh] * X[xidx[m], hh, i] over the pairs with rel[m, ax] == r"""
        c = self.c
        mask = self.keep.copy()
        if self.fault == "second_segment_dropped":
            at = c.pos if side == "q" else c.cpos
            mask[(at >= SEGMENT) & (at < 2 * SEGMENT)] = 0
        terms = (w * mask[:, None])[:, :, None] * X[xidx]
        out = np.zeros((c.L, c.h, c.d, 3))
        for ax in range(3):
            g = np.zeros((c.L, c.h, c.d))
            np.add.at(g, self.rel[:, self.axes[ax]], terms)
            if side == "q" and len(self.extra_pairs):
                np.add.at(g, self.rel[self.extra_pairs, ax], w[self.extra_pairs][:, :, None] * X[self.extra_rows])
            out[..., ax] = g
        if self.fault == "bins_from_64_dropped":
            out[64:] = 0
        if self.fault == "bins_of_the_partial_tile_dropped":
            out[16 * (c.L // 16):] = 0
        return out

    def finish(self, outs, gathers=()):
        c = self.c
        if self.fault == "last_head_not_stored":
            for o in outs.values():
                o[:, -1] = 0
        if self.fault == "gather_chunk_skipped":
            for name in gathers:
                outs[name][:, HC * ((c.h - 1) // HC):] = 0
        return outs

    def a1(self, gp=None):
        gp = np.asarray(self.c.go_pairs if gp is None else gp, np.float64)
        qm, km = self.q[self.row], self.k[self.j]
        return self.finish({"a1.out": self.per_pair(np.einsum("mhd,mhd->mh", qm, km)), "a1.gq": self.rowsum(gp[:, :, None] * km),
                            "a1.gk": self.keysum(gp[:, :, None] * qm)}, ("a1.gq", "a1.gk"))

    def a2(self, gp=None):
        gp = np.asarray(self.c.go_pairs if gp is None else gp, np.float64)
        qm, km, Tq, Tk = self.q[self.row], self.k[self.j], self.tsum(self.tq), self.tsum(self.tk)
        Tkk = Tq if self.fault == "key_side_from_query_table" else Tk
        return self.finish({"a2.out": self.per_pair((qm * Tq + km * Tk).sum(2)), "a2.gq": self.rowsum(gp[:, :, None] * Tq),
                            "a2.gk": self.keysum(gp[:, :, None] * Tkk), "a2.gtq": self.scatter(gp, self.q, self.row, "q"),
                            "a2.gtk": self.scatter(gp, self.k, self.j, "k")})

    def a4(self, at=None):
        at = np.asarray(self.c.attn if at is None else at, np.float64)
        vt, gm = self.v[self.j] + self.tsum(self.tv), self.gr[self.row]
        return self.finish({"a4.out": self.rowsum(at[:, :, None] * vt), "a4.ga": self.per_pair((vt * gm).sum(2)),
                            "a4.gv": self.keysum(at[:, :, None] * gm), "a4.gt": self.scatter(at, self.gr, self.row, "q")}, ("a4.gv",))

    def fused(self, attn=None):
        """the operator chain: softmax(A1 + A2) -> A4, and its backward for go_rows; attn: everything behind the softmax from
        this one (the device's own) instead"""
        c = self.c
        a = softmax_f64(self.a1()["a1.out"] + self.a2()["a2.out"], c.offsets) if attn is None else np.asarray(attn, np.float64)
        f = self.a4(a)
        dl = softmax_bwd_f64(a, f["a4.ga"], c.offsets)
        b1, b2 = self.a1(dl), self.a2(dl)
        return {"f.out": f["a4.out"], "f.gq": b1["a1.gq"] + b2["a2.gq"], "f.gk": b1["a1.gk"] + b2["a2.gk"], "f.gv": f["a4.gv"],
                "f.gtq": b2["a2.gtq"], "f.gtk": b2["a2.gtk"], "f.gtv": f["a4.gt"], "f.attn": a, "ga": f["a4.ga"], "dl": dl}

    def run(self, group):
        return getattr(self, group)()


def model(c, group, fault=None):
    """{name: float64 array} of the operator group `a1`, `a2`, `a4` or `fused` (the whole chain in float64) on case c"""
    key = (group, fault)
    if fault is not None:
        return _Model(c, fault).run(group)
    if key not in c._cache:
        c._cache[key] = _Model(c).run(group)
    return c._cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def _segments(c, side):
    """the segments of 128 pairs the table-gradient kernel cuts its rows into (side q: CSR rows; k: CSC rows)
    -> (segment of every pair [M], pairs per segment [S], the X row of every segment [S], index within its row [S])"""
    rows, at, lens = (c.row, c.pos, c.lens) if side == "q" else (c.index_1.astype(np.int64), c.cpos, c.key_count)
    per_row = -(-lens // SEGMENT)
    base = np.concatenate([[0], np.cumsum(per_row)])
    seg = base[rows] + at // SEGMENT
    S = int(base[-1])
    xrow = np.repeat(np.arange(len(lens)), per_row)
    nth = np.arange(S) - base[xrow]
    return seg, np.bincount(seg, minlength=S), xrow, nth


def _bits(n):
    return np.floor(np.log2(np.maximum(n, 1))).astype(np.int64) + 1  # n < 2^bits


def fixed_point_bound(c, w, X, side, HG, dw=None):
    """Bound [L, h, d, 3] of the fixed-point table gradient (csrc/rpe_bwd_mfma.hip) for weights w [M, h] and rows X.  Per entry
    (r, head, i, ax), over the segments that have a pair with rel[., ax] == r:
        sum  count(seg, r, ax) * w_max(seg, head group) * 2^(bits(n_seg) - 30) * |X[row, head, i]|        each term's quantisation
      + (K + 2) * 2u * sum |H_seg(r, ax, head)| * |X[row, head, i]|        float(bin), the fp32 chain over K segments, the flush
    dw: a bound on the error of w itself (the fused backward's grad_logit / attn): it enters w_max and H and adds sum dw * |X|."""
    signed = np.asarray(w, np.float64)
    w = np.abs(signed)
    dw = np.zeros_like(w) if dw is None else dw
    seg, n, xrow, _ = _segments(c, side)
    S, h, L = len(n), c.h, c.L
    group = np.arange(h) // HG
    wmax = np.zeros((S, group[-1] + 1))
    np.maximum.at(wmax, (seg[:, None], group[None, :]), w + dw)
    quantum = wmax[:, group] * (2.0 ** (_bits(n) - 30))[:, None]     # [S, h]
    absX = np.abs(np.asarray(X, np.float64))
    out = np.zeros((L, h, c.d, 3))
    for ax in range(3):
        keys, inv, count = np.unique(seg * L + c.rel_idx[:, ax], return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        su, ru = keys // L, keys % L
        H, dH = np.zeros((len(keys), h)), np.zeros((len(keys), h))
        np.add.at(H, inv, signed)
        np.add.at(dH, inv, dw)
        x = absX[xrow[su]]
        q_term, h_term, K = np.zeros((L, h, c.d)), np.zeros((L, h, c.d)), np.bincount(ru, minlength=L)
        np.add.at(q_term, ru, (count[:, None] * quantum[su] + dH)[:, :, None] * x)
        np.add.at(h_term, ru, (np.abs(H) + dH)[:, :, None] * x)
        out[..., ax] = q_term + (K + 2)[:, None, None] * 2 * U * h_term
    return out


def emulate_table_grad(c, w, X, side, HG, reuse_scale=False):
    """The fixed-point scheme in numpy, fp32 in and out: row_scale as written, round to nearest even to an integer, integer sums,
    float of the sum, fp32 products added in fp32 in segment order.  reuse_scale: a row's second segment takes the first one's
    scale (a fault)."""
    w, X = np.asarray(w, np.float32), np.asarray(X, np.float32)
    seg, n, xrow, nth = _segments(c, side)
    S, h, L = len(n), c.h, c.L
    group = np.arange(h) // HG
    wmax = np.zeros((S, group[-1] + 1), np.float32)
    np.maximum.at(wmax, (seg[:, None], group[None, :]), np.abs(w))
    E = (wmax.view(np.uint32) >> 23).astype(np.int64) - 126          # max|w| < 2^E
    shift = np.clip(30 - _bits(n)[:, None] - E, -126, 126)
    if reuse_scale:
        second = np.flatnonzero(nth == 1)
        shift[second] = shift[second - 1]
    shift = shift[:, group]                                           # [S, h]
    fixed = np.rint(w.astype(np.float64) * 2.0 ** shift[seg]).astype(np.int64)
    out = np.zeros((L, h, c.d, 3), np.float32)
    for ax in range(3):
        keys, inv = np.unique(seg * L + c.rel_idx[:, ax], return_inverse=True)
        inv = inv.reshape(-1)
        su, ru = keys // L, keys % L
        hist = np.zeros((len(keys), h), np.int64)
        np.add.at(hist, inv, fixed)
        assert np.abs(hist).max(initial=0) < 2 ** 30
        a = hist.astype(np.float32)
        b = (X[xrow[su]].astype(np.float64) * 2.0 ** -shift[su][:, :, None]).astype(np.float32)
        g = np.zeros((L, h, c.d), np.float32)
        np.add.at(g, ru, a[:, :, None] * b)
        out[..., ax] = g
    return out


def _floor(b):
    return np.maximum(b, 1e-300)  # an element nothing contributes to must be exactly zero


def _atomic_table_bound(c, m, w_abs, X, xidx, dw=None):
    """K * 2u * S for the table flushes: K pairs contribute to the entry (LDS float atomics in any order, one global atomic per
    workgroup that has a part); dw as in fixed_point_bound"""
    dw = np.zeros_like(w_abs) if dw is None else dw
    S = m.scatter(w_abs + dw, np.abs(X), xidx, "q")
    K = np.stack([np.bincount(c.rel_idx[:, ax], minlength=c.L) for ax in range(3)], -1)[:, None, None, :]
    return K * 2 * U * S + m.scatter(dw, np.abs(X), xidx, "q")


def _table_bound(c, m, group, w, X, xidx, side, dw=None):
    """the bound of a table gradient of `group` on the path its backward takes"""
    bwd = paths(c.spec, group)[1]
    if bwd.family == "mfma":
        return fixed_point_bound(c, w, X, side, bwd.HG, dw)
    return _atomic_table_bound(c, m, np.abs(np.asarray(w, np.float64)), X, xidx, dw)


def reference(c, group):
    """{name: (want, bound)} for the outputs of `a1`, `a2` or `a4` on case c, from the arithmetic of the kernels that path_of
    names.  n roundings of a sum: n * 2u * sum |terms| (any order); the table sum (T0 + T1) + T2 counts 2, v + T one more."""
    key = ("reference", group)
    if key in c._cache:
        return c._cache[key]
    m = _Model(c)
    want = model(c, group)
    d, lens, K = c.d, c.lens[:, None, None], c.key_count[:, None, None]
    gp, at = np.abs(np.asarray(c.go_pairs, np.float64)), np.abs(np.asarray(c.attn, np.float64))
    aq, ak, av, ag = (np.abs(x) for x in (m.q, m.k, m.v, m.gr))
    if group == "a1":
        B = {"a1.out": d * 2 * U * np.einsum("mhd,mhd->mh", aq[m.row], ak[m.j]),
             "a1.gq": lens * 2 * U * m.rowsum(gp[:, :, None] * ak[m.j]),
             "a1.gk": K * 2 * U * m.keysum(gp[:, :, None] * aq[m.row])}
    elif group == "a2":
        Tq, Tk = m.tsum(m.tq, True), m.tsum(m.tk, True)
        B = {"a2.out": (2 * d + 2) * 2 * U * (aq[m.row] * Tq + ak[m.j] * Tk).sum(2),
             "a2.gq": (lens + 2) * 2 * U * m.rowsum(gp[:, :, None] * Tq),
             "a2.gk": (K + 2) * 2 * U * m.keysum(gp[:, :, None] * Tk),
             "a2.gtq": _table_bound(c, m, "a2", c.go_pairs, m.q, m.row, "q"),
             "a2.gtk": _table_bound(c, m, "a2", c.go_pairs, m.k, m.j, "k")}
    else:
        vt = av[m.j] + m.tsum(m.tv, True)
        B = {"a4.out": (lens + 3) * 2 * U * m.rowsum(at[:, :, None] * vt),
             "a4.ga": (d + 3) * 2 * U * (vt * ag[m.row]).sum(2),
             "a4.gv": K * 2 * U * m.keysum(at[:, :, None] * ag[m.row]),
             "a4.gt": _table_bound(c, m, "a4", c.attn, m.gr, m.row, "q")}
    out = {name: (want[name], _floor(B[name])) for name in B}
    c._cache[key] = out
    return out


def _per_row(c, x, how):
    """x [M, h] (non-negative for `max`) reduced over every row and handed back to the row's pairs"""
    out = np.zeros((c.N, c.h))
    (np.maximum if how == "max" else np.add).at(out, c.row, x)
    return out[c.row]


def fused_reference(c, logits, attn):
    """{name: (want, bound)} of the fused module, every stage from what the DEVICE produced in front of it, so that each bound is
    as tight as the separate operators'.
    f.attn: the softmax of `logits` [M, h] fp32 - the sum of the device's own A1 and A2 outputs, which the fused kernel forms
        term for term - in float64, at DESIGN 2.2's want * (len + span + 8) * 2u + 2^-126.
    f.out: A4's forward on `attn` [M, h] fp32, the softmax the fused forward saved, at A4's (len + 3) * 2u * S.
    Backward, from the same attn: grad_attn as A4's, (d + 3) * 2u * S: dga.  The row dot of len terms: ddot = sum attn * dga +
        (len + 1) * 2u * sum attn (|grad_attn| + dga).  grad_logit = attn * (grad_attn - dot) with the softmax backward's
        (len + 8) * 2u * max |grad_attn|: ddl = attn * (dga + ddot + that).  grad_logit never leaves the device, so
        ddl is carried on: grad_q / grad_k: sum ddl * (|k| + |T|) plus (len + 4) roundings (two sums and their add; without a CSC
        both operators add into one buffer: K + 4); grad_v: K * 2u * S; the tables of grad_logit with dw = ddl, the value table
        as A4's."""
    logits, attn = np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(attn, np.float32)
    key = ("fused", hash(logits.tobytes()), hash(attn.tobytes()))
    if key in c._cache:
        return c._cache[key]
    m = _Model(c)
    a = attn.astype(np.float64)
    want = m.fused(a)
    aq, ak, av, ag = (np.abs(x) for x in (m.q, m.k, m.v, m.gr))
    vt = av[m.j] + m.tsum(m.tv, True)
    lens = c.lens[c.row][:, None].astype(np.float64)
    L3, K = c.lens[:, None, None], c.key_count[:, None, None]
    B = {"f.out": (L3 + 3) * 2 * U * m.rowsum(a[:, :, None] * vt)}
    ga, dl = want["ga"], want["dl"]
    dga = (c.d + 3) * 2 * U * (vt * ag[m.row]).sum(2)
    ddot = _per_row(c, a * dga, "sum") + (lens + 1) * 2 * U * _per_row(c, a * (np.abs(ga) + dga), "sum")
    ddl = a * (dga + ddot + (lens + 8) * 2 * U * _per_row(c, np.abs(ga) + dga, "max"))
    wq, wk = ak[m.j] + m.tsum(m.tq, True), aq[m.row] + m.tsum(m.tk, True)
    B["f.gq"] = m.rowsum(ddl[:, :, None] * wq) + (L3 + 4) * 2 * U * m.rowsum((np.abs(dl) + ddl)[:, :, None] * wq)
    B["f.gk"] = m.keysum(ddl[:, :, None] * wk) + (K + 4) * 2 * U * m.keysum((np.abs(dl) + ddl)[:, :, None] * wk)
    B["f.gv"] = K * 2 * U * m.keysum(a[:, :, None] * ag[m.row])
    B["f.gtq"] = _table_bound(c, m, "fused", dl, m.q, m.row, "q", ddl)
    B["f.gtk"] = _table_bound(c, m, "fused", dl, m.k, m.j, "k", ddl)
    B["f.gtv"] = _table_bound(c, m, "fused", a, m.gr, m.row, "q")
    out = {name: (want[name], _floor(B[name])) for name in B}
    out["f.attn"] = softmax_fwd_bound(logits, c.offsets)
    c._cache[key] = out
    return out


def check(c, group, name, got, what="", refs=None):
    """the largest fraction of its bound over every element of output `name`; raises above 1.  refs: fused_reference(...)"""
    want, bound = (reference(c, group) if refs is None else refs)[name]
    return fraction_of_bound(got, want, bound, f"{what}{c.spec.name} {name}")


# which outputs a second call must repeat bit for bit: everything that is not summed with float atomics
def repeatable(spec, group):
    fwd, bwd = paths(spec, group)
    fb = bwd.family == "fallback-global"
    if group == "a1":
        return ["a1.out", "a1.gq"] + (["a1.gk"] if spec.csc else [])
    if group == "a2":
        return ["a2.out"] + ([] if fb else ["a2.gq"]) + (["a2.gk"] if spec.csc and not fb else [])
    if group == "a4":
        return ([] if fb else ["a4.out"]) + ["a4.ga"] + (["a4.gv"] if spec.csc and not fb else [])
    return ["f.attn", "f.out"] + (["f.gq", "f.gk", "f.gv"] if bwd.family == "mfma" else [])


# ---------------------------------------------------------------------------------------------------------------------
# which outputs of which cases must reject which fault
# ---------------------------------------------------------------------------------------------------------------------
TABLE_GRADS = {"a2": ("a2.gtq", "a2.gtk"), "a4": ("a4.gt",), "fused": ("f.gtq", "f.gtk", "f.gtv")}


def must_catch(spec, group, fault):
    """the outputs of `group` on this case that the fault changes by more than any rounding (empty: it does not apply)"""
    if group == "a1":
        fwd, bwd = paths(spec, "a1")
        part_f, part_b = fwd.hgn_last < fwd.HG, bwd.hgn_last < bwd.HG
        return {"last_head_not_stored": (["a1.out"] if part_f else []) + (["a1.gq"] + (["a1.gk"] if spec.csc else []) if part_b else []),
                "last_pair_dropped": ["a1.out", "a1.gq"], "slot_past_end_added": ["a1.gq"],
                "gather_chunk_skipped": (["a1.gq"] + (["a1.gk"] if spec.csc else [])) if part_b else []}.get(fault, [])
    fwd, bwd = paths(spec, group)
    if "error" in (fwd.family, bwd.family):
        return []
    if group == "fused":
        return _must_catch_fused(spec, fwd, bwd).get(fault, [])
    fb = bwd.family == "fallback-global"
    part_f = fwd.family != "fallback-global" and fwd.hgn_last < fwd.HG
    part_b = not fb and bwd.hgn_last < bwd.HG
    mfma = bwd.family == "mfma"
    L, full = spec.L, spec.layout == "full"
    tg = list(TABLE_GRADS[group])
    out_f = ["a2.out"] if group == "a2" else ["a4.out"]
    rows_b = ["a2.gq", "a2.gk"] if group == "a2" else ["a4.ga"]           # the backward outputs that read a table sum
    all_b = ["a2.gq", "a2.gk"] + tg if group == "a2" else ["a4.ga", "a4.gv"] + tg
    by_query = ["a2.gq", "a2.gtq"] if group == "a2" else ["a4.out", "a4.gt"]
    return {
        "prev_table_slice": (out_f if part_f else []) + (rows_b if part_b else []),
        "last_head_not_stored": (out_f if part_f else []) + (all_b if part_b else []),
        "bins_from_64_dropped": tg if mfma and L > 64 else [],
        "bins_of_the_partial_tile_dropped": tg if mfma and L % 16 else [],
        "second_segment_dropped": [t for t in tg if full or t != "a2.gtk"] if mfma else [],  # a key row past 128 pairs: `full` only
        "second_segment_reuses_scale": tg if mfma and full and L >= 8 else [],
        "last_pair_dropped": out_f + (["a2.gq", "a2.gtq"] if group == "a2" else ["a4.ga", "a4.gt"]),
        "slot_past_end_added": by_query,
        "key_side_from_query_table": ["a2.gk"] if group == "a2" else [],
        "axes_swapped": (out_f + rows_b + tg) if L >= 2 else [],
        "gather_chunk_skipped": ["a4.gv"] if group == "a4" and spec.csc and not fb and spec.h % HC else [],
    }[fault]


def _must_catch_fused(spec, fwd, bwd):
    """A fault in the forward shows in f.attn (against the softmax of the device's logits); everything behind is referred to the
    attn at hand, so what a fault does to attn alone cancels there.  Without the fused backward the head groups are the A2
    backward's.  (The scale fault needs weights made for it, and grad_logit is the module's own; gather_accum is not on the
    fused path.)"""
    mfma, L, full = bwd.family == "mfma", spec.L, spec.layout == "full"
    b = bwd if mfma else paths(spec, "a2")[1]
    part_f, part_b = fwd.hgn_last < fwd.HG, b.family in ("lds-slice", "mfma") and b.hgn_last < b.HG
    tg = list(TABLE_GRADS["fused"])
    by_query = ["f.out", "f.gq", "f.gtq", "f.gtv"]
    return {
        "prev_table_slice": (["f.attn"] if part_f else []) + (["f.gq", "f.gk"] if part_b else []),
        "last_head_not_stored": ["f.attn"] if part_f else ["f.gq", "f.gk", "f.gv"] + tg if part_b else [],
        "bins_from_64_dropped": tg if mfma and L > 64 else [],
        "bins_of_the_partial_tile_dropped": tg if mfma and L % 16 else [],
        "second_segment_dropped": [t for t in tg if full or t != "f.gtk"] if mfma else [],
        "last_pair_dropped": ["f.attn"] + by_query,
        "slot_past_end_added": by_query,
        "key_side_from_query_table": ["f.gk"],
        "axes_swapped": ["f.attn", "f.out", "f.gq", "f.gk"] + tg if L >= 2 else [],
    }


def forward_fault(spec, fault):
    """does the fault, on this case, change the fused forward's attn"""
    return "f.attn" in must_catch(spec, "fused", fault)
