"""CPU: the dispatch restated in tests/attention_cases.py is the sources', its case table reaches every region, the C oracle and a
numpy emulation of the fixed-point histogram meet the derived bounds on every case (so a correct fp32 implementation can), and
numpy variants with one fault each miss them wherever they apply (so the bounds have teeth).  No HIP."""
import os
import re

import numpy as np
import pytest

from oracle import pointops_ref as ref
from tests import attention_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stratified_transformer_amd")
GROUPS = ("a1", "a2", "a4", "fused")


def _src(*path):
    with open(os.path.join(PKG, *path)) as f:
        return f.read()


def _all(pattern, text, count):
    found = re.findall(pattern, text)
    assert len(found) == count, f"{pattern!r}: {len(found)} matches, expected {count}"
    return found


# ---------------------------------------------------------------------------------------------------------------------
# path_of is the launchers' dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    common, rpe_common = _src("csrc", "common.h"), _src("csrc", "rpe_common.h")
    rpe, mfma, attention = _src("csrc", "rpe.hip"), _src("csrc", "rpe_bwd_mfma.hip"), _src("csrc", "attention.hip")
    pointops, fused = _src("pointops.py"), _src("fused.py")
    a, b = _all(r"constexpr size_t kLdsBudget = (\d+) \* (\d+);", rpe_common, 1)[0]
    assert int(a) * int(b) == C.LDS_BUDGET
    a, b = _all(r"if \(per_head <= (\d+) \* (\d+)\) return 1;", rpe, 1)[0]
    assert int(a) * int(b) == C.ONE_WG_LIMIT
    assert _all(r"const size_t per_head = \(size_t\)narr \* 3 \* L \* D \* sizeof\(float\);", rpe, 1)
    assert _all(r"int hg = \(int\)\(kLdsBudget / per_head\);", rpe, 1)
    assert _all(r"if \(hg > (\d+)\) hg = (\d+);", rpe, 1) == [(str(C.HG_CAP),) * 2]
    assert _all(r"if \(heads >= (\d+)\) f\(std::integral_constant<int, (\d+)>\{\}\);", rpe_common, 1) == [(str(C.HG_CAP),) * 2]
    assert _all(r"else if \(heads == 2\) f\(std::integral_constant<int, 2>\{\}\);", rpe_common, 1)
    # narr of every slice launch: A2 forward and the fused logits 2, A2 backward 2 with a CSC and 4 without, A4 forward 1, backward 2
    assert _all(r"with_table_slice<D>\(h, L, ([^,]+),", rpe, 4) == ["2", "co ? 2 : 4", "1", "2"]
    assert _all(r"with_table_slice<16>\(h, L, (\d+),", rpe, 1) == ["2"]
    assert _all(r'set_error\("rel-pos table slice does not fit in LDS"\)', rpe, 1)
    # the matrix-core backward: d = 16, a CSC, L <= 80; four bin tiles up to 64 rows, five beyond
    assert _all(r"if \(co && hdim == 16 && L <= (\d+)\)", rpe, 1) == [str(C.MFMA_L_MAX)]
    assert _all(r"hdim != 16 \|\| co == nullptr \|\| L < 1 \|\| L > (\d+)\) return false;", mfma, 2) == [str(C.MFMA_L_MAX)] * 2
    assert _all(r"if \(hdim != 16 \|\| L < 1 \|\| L > (\d+)\) return false;", mfma, 1) == [str(C.MFMA_L_MAX)]
    assert _all(r"if \(L <= (\d+)\) \{?\s*launch_table_grad<4>", mfma, 3) == [str(C.TA4_L_MAX)] * 3
    assert _all(r"else \{?\s*launch_table_grad<5>", mfma, 3)
    assert _all(r"if csc is not None and L <= (\d+):", fused, 1) == [str(C.MFMA_L_MAX)]
    assert _all(r"if hdim != 16:\n\s+raise RuntimeError\(\"window_attention: d != 16", fused, 1)
    assert _all(r"constexpr int TG_WAVES = (\d+);", mfma, 1) == [str(C.TG_WAVES)]
    assert _all(r"constexpr int TG_MAXP = (\d+);", mfma, 1) == [str(C.TG_MAXP)]
    assert _all(r"constexpr int WB_MAXP = (\d+);", mfma, 1) == [str(C.WB_MAXP)]
    assert _all(r"constexpr int WL_MAXP = (\d+);", rpe, 1) == [str(C.WL_MAXP)]
    assert _all(r"end - cur <= 16 \* TG_MAXP", mfma, 1) and _all(r"min\(end, cur \+ 16 \* TG_MAXP\)", mfma, 1)
    assert C.SEGMENT == 16 * C.TG_MAXP == C.ppw(16) * C.WL_MAXP == C.ppw(16) * C.WB_MAXP == 128
    assert _all(r"if \(np <= WL_MAXP\)", rpe, 1) and _all(r"if \(e > s && np <= WB_MAXP\)", mfma, 1)
    # A1: the two grids of the forward, four heads per pass of the gathers
    assert _all(r"dim3\(blocks, N < (\d+) \? div_up\(h, D / 4\) : 1\)", attention, 1) == [str(C.A1_LOOP_N)]
    assert _all(r"constexpr int LPG = Geo<D>::LPG, PPW = Geo<D>::PPW, HC = (\d+);", attention, 1) == [str(C.HC)]
    assert _all(r"div_up\(h, (\d+)\)\)", attention, 2) == [str(C.HC)] * 2
    # the walkers' geometry and the row order
    assert _all(r"static constexpr int LPG = D / (\d+);", common, 1) == ["4"] and C.lpg(16) == 4 and C.lpg(32) == 8
    assert _all(r"static constexpr int PPW = (\d+) / LPG;", common, 1) == ["64"] and C.ppw(16) == 16 and C.ppw(32) == 8
    assert _all(r"opts\.row_order_rows == n_rows && n_rows >= (\d+)\)", common, 1) == [str(C.ROW_ORDER_N)]
    assert _all(r"if not ROW_ORDER or N < (\d+) ", pointops, 2) == [str(C.ROW_ORDER_N)] * 2
    # ... which a kernel follows only on a grid that is a multiple of 8: the walkers' grids
    assert _all(r"if \(order_ != nullptr && \(gridDim\.x & 7\) == 0\)", common, 1)
    assert _all(r"const int share = \(rord != nullptr && \(gridDim\.x & 7\) == 0\) \?", mfma, 1)
    assert _all(r"inline int ordered_grid\(int n_rows, int rows_per_wg\) \{ return 8 \* div_up\(", common, 1)
    assert _all(r"constexpr int kNumCU = (\d+);", common, 1) == [str(C.NUM_CUS)]
    assert _all(r"int cap = cus \* per_cu;\s+if \(groups > 1\) cap = max\(cus \* per_cu / groups, cus / 2\);\s+return max\(1, min\(want, cap\)\);", rpe_common, 1)
    W = C.WALKERS
    assert _all(r"walk_blocks\(N, ngroups, (\d+), (\d+)\), ngroups\), dim3\((\d+)\)", rpe, 5) == [
        ("12", "2", "768"), ("12", "2", "768"), ("4", "2", "256"), ("8", "3", "512"), ("4", "2", "256")]   # A2 fwd, fused logits, A2 bwd by query, A4 fwd, A4 bwd by query
    assert W["a2_fwd"]["walk"] == (12, 2) and W["a4_fwd"]["walk"] == (8, 3)
    assert _all(r"walk_blocks\(NK?, groups, (\d+), (\d+)\), groups\), dim3\(512\)", mfma, 5) == [("8", "4")] * 3 + [("8", "2")] * 2
    assert W["mfma_bwd"]["walk"] == (8, 4) and W["wattn_bwd"]["walk"] == (8, 2)
    assert _all(r"walk_blocks\(N, groups, TG_WAVES, (\d+)\), groups\), dim3\(TG_WAVES \* 64\)", mfma, 1) == ["2"]
    assert W["mfma_bwd"]["tables"] == W["wattn_bwd"]["tables"] == (C.TG_WAVES, 2)
    # N = 2048: the 8-wave walkers have 256 workgroups, the 12-wave ones 171; at ORDER_N both have a multiple of 8
    assert (C.walk_blocks(2048, 1, 8, 4), C.walk_blocks(2048, 2, 12, 2), C.walk_blocks(C.ORDER_N, 2, 12, 2), C.walk_blocks(C.ORDER_N, 1, 8, 3)) == (256, 171, 176, 264)
    assert C.ORDER_N >= C.ROW_ORDER_N and C.ORDER_N % 8 == 0 and C.ORDER_N % 12 == 0   # (no partial last workgroup either)


def test_pick_hg_regions_are_the_docstring_table():
    """the thresholds in L of every (narr, D), from the byte counts alone"""
    table = {(1, 16): (128, 192, 384, 800), (1, 32): (64, 96, 192, 400), (2, 16): (64, 96, 192, 400),
             (2, 32): (32, 48, 96, 200), (4, 16): (32, 48, 96, 200), (4, 32): (16, 24, 48, 100)}
    for (narr, D), (l3, l2, l1, big) in table.items():
        for L in range(1, big + 50):
            want = 3 if L <= l3 else 2 if L <= l2 else 1 if L <= big else 0
            assert C.pick_hg(7, L, D, narr) == want, (narr, D, L)
            assert C.pick_hg(2, L, D, narr) == min(want, 2) and C.pick_hg(1, L, D, narr) == min(want, 1)
        per_head = narr * 3 * D * 4
        assert per_head * l1 <= C.LDS_BUDGET < per_head * (l1 + 1) and per_head * big == C.ONE_WG_LIMIT


def test_path_of_follows_the_launchers_order_of_tests():
    P = C.path_of
    assert P("a2_bwd", 300, 5, 16, 80, True).family == "mfma" and P("a2_bwd", 300, 5, 16, 81, True).family == "lds-slice"
    assert P("a2_bwd", 300, 5, 16, 80, False) == P("a2_bwd", 300, 5, 16, 80, False)._replace(family="lds-slice", narr=4, keyside=True)
    assert P("a2_bwd", 300, 5, 32, 24, True)._asdict() | dict(lds_bytes=0) == dict(
        family="lds-slice", D=32, HG=3, hgn_last=2, TA=None, narr=2, lds_bytes=0, big_lds=False, keyside=False, a1_grid=None, row_order=())
    assert P("a4_bwd", 300, 4, 16, 65, True)[:6] == ("mfma", 16, 3, 1, 5, 1) and P("a4_bwd", 300, 4, 16, 64, True).TA == 4
    assert P("a4_bwd", 300, 4, 16, 64, False)[:6] == ("lds-slice", 16, 3, 1, None, 2) and P("a4_bwd", 300, 4, 16, 64, False).keyside
    assert P("a2_fwd", 300, 2, 16, 400, True).big_lds and P("a2_fwd", 300, 2, 16, 400, True).lds_bytes == C.ONE_WG_LIMIT
    assert P("a2_fwd", 300, 2, 16, 401, True).family == "error" and P("a4_fwd", 300, 2, 16, 401, True).family == "lds-slice"
    assert P("a2_fwd", 300, 5, 16, 48, True, table_rows=False).family == "fallback-global"
    assert P("a2_bwd", 300, 5, 16, 48, True, table_rows=False).family == "fallback-global"  # L is looked at before the CSC
    assert P("a1_fwd", 19999, 5, 16, 1, True).a1_grid == "y-groups" and P("a1_fwd", 20000, 5, 16, 1, True).a1_grid == "y-loop"
    assert (P("a1_fwd", 300, 5, 16, 1, True).HG, P("a1_fwd", 300, 5, 16, 1, True).hgn_last) == (4, 1)
    assert (P("a1_fwd", 300, 5, 32, 1, True).HG, P("a1_fwd", 300, 5, 32, 1, True).hgn_last) == (8, 5)
    assert P("a1_bwd", 300, 7, 32, 1, False).keyside and P("a1_bwd", 300, 7, 32, 1, False).hgn_last == 3
    assert not P("a4_fwd", 2047, 2, 16, 64, True).row_order and P("a4_fwd", 2048, 2, 16, 64, True).row_order == ("walk",)
    assert P("a2_fwd", 2048, 2, 16, 64, True).row_order == () and P("a2_fwd", 2112, 4, 16, 64, True).row_order == ("walk",)  # 171, 176 workgroups
    assert P("a2_bwd", 2048, 4, 16, 64, True).row_order == ("walk",) and P("a2_bwd", 2112, 4, 16, 64, True).row_order == ("walk", "tables")
    assert P("wattn_bwd", 2112, 4, 16, 64, True).row_order == ("walk", "tables") and P("a1_bwd", 2048, 5, 32, 1, False).row_order == ("walk",)
    assert P("a2_bwd", 2112, 4, 32, 24, True).row_order == ()  # the slice backwards stride the grid by index
    assert P("wattn_bwd", 300, 3, 16, 80, True)[:6] == ("mfma", 16, 3, 3, 5, 2) and P("wattn_bwd", 300, 3, 16, 81, True).family == "operators"
    assert P("wattn_bwd", 300, 3, 16, 64, False).family == "operators" and P("wlogit_fwd", 300, 3, 16, 401, True).family == "error"


@pytest.mark.parametrize("group", GROUPS)
def test_the_case_table_reaches_every_region(group):
    for i, op in enumerate(C.OPS_OF[group]):
        want = C.all_facets(op)
        reached = {}
        for s in C.specs_of(group):
            for f in C.facets(op, C.paths(s, group)[i]):
                reached.setdefault(f, s.name)
        for f in sorted(want):
            print(f"region {op} {f} <- {reached.get(f)}")
        assert set(reached) == set(want), (op, sorted(set(want) ^ set(reached)))


def test_the_edge_cases_come_from_path_of():
    """both sides of every HG change, the last L that fits and the first that does not, for every (narr, D) a launcher can ask for"""
    have = {(s.d, s.csc, s.L) for s in C.SPECS if s.layout == "small"}
    for op, narrs in (("a4_fwd", {True: 1, False: 1}), ("a2_fwd", {True: 2, False: 2}), ("a2_bwd", {True: 2, False: 4}), ("a4_bwd", {True: 2, False: 2})):
        for d in (16, 32):
            for csc in (True, False):
                narr = narrs[csc]
                last = C.ONE_WG_LIMIT // (narr * 3 * d * 4)
                big = [L for L in range(1, last + 1) if C.path_of(op, 300, 1, d, L, csc).big_lds and C.path_of(op, 300, 1, d, L, csc).family == "lds-slice"]
                assert big and big[-1] == last and (d, csc, last) in have and (d, csc, last + 1) in have
                assert C.path_of(op, 300, 1, d, last, csc).lds_bytes == C.ONE_WG_LIMIT and C.path_of(op, 300, 1, d, last + 1, csc).family == "error"
                assert any((d, csc, L) in have for L in big[1:-1]), "one L inside the big-LDS region"
                for L in range(2, last + 2):
                    a, b = C.path_of(op, 300, 3, d, L - 1, csc), C.path_of(op, 300, 3, d, L, csc)
                    if (a.family, a.HG, a.big_lds) != (b.family, b.HG, b.big_lds):
                        assert (d, csc, L - 1) in have and (d, csc, L) in have, (op, d, csc, L)
    # the big-LDS launches stay small: one or two heads, the 40-row layout (an edge case runs the operator it is an edge of)
    assert all(s.h in (1, 2) and s.layout == "small" for s in C.SPECS for g in s.ops if g != "a1" for p in C.paths(s, g) if p.big_lds and p.family == "lds-slice")


# ---------------------------------------------------------------------------------------------------------------------
# the cases are what they claim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", C.SPECS, ids=lambda s: s.name)
def test_case_is_what_it_claims(spec):
    c = C.case(spec)
    N, h, d, L, M = spec.N, spec.h, spec.d, spec.L, c.M
    assert c.offsets.shape == (N + 1,) and c.offsets[0] == 0 and c.offsets[-1] == M and (np.diff(c.offsets) >= 0).all() and 0 < M < 10000
    assert c.index_1.shape == (M,) and c.index_1.min() >= 0 and c.index_1.max() < N
    assert c.rel_idx.shape == (M, 3) and c.rel_idx.min() >= 0 and c.rel_idx.max() < L   # nothing may read outside a table
    for name, a in c.arrays().items():
        assert not a.flags.writeable and a.flags.c_contiguous
        if a.dtype == np.float32:
            mag = np.abs(a[a != 0])
            assert np.isfinite(a).all() and mag.min() >= 2.0 ** -8 and mag.max() <= 2.0 ** 4, name
        else:
            assert a.dtype == np.int32
    lens = np.diff(c.offsets)
    assert not lens[:4].any() and not lens[N - 4:].any() and (spec.layout == "sparse" or not lens[N // 2])
    assert set(C.SPECIAL[spec.layout]) <= set(lens.tolist())
    assert {0, 1, C.ppw(d) - 1, C.ppw(d), C.ppw(d) + 1, 129} <= set(lens.tolist())
    if spec.layout in ("full", "sparse"):
        assert {127, 128, 129, 257} <= set(lens.tolist())
    if spec.layout == "full":
        assert 256 in lens and c.key_count[C.KEY_A] == 257 and c.key_count[C.KEY_B] == 129   # CSC rows across the 128-pair segment
        r = c.row_with[127]
        assert (c.index_1[c.offsets[r]:c.offsets[r + 1]] == C.KEY_SAME).all()               # one row, one key
        r = c.row_with[129]
        assert len(np.unique(c.rel_idx[c.offsets[r]:c.offsets[r + 1]], axis=0)) == 1        # one bin per axis takes the whole row
    if spec.layout == "sparse":
        first = c.index_1[c.offsets[:-1][lens > 0]]
        assert len(c.live) < 60 and (np.diff(first) <= 0).all() and first[0] == N - 1 and first[-1] == 0  # first partners against the index order
    if L <= 96:
        for ax in range(3):
            assert {L - 1, min(64, L - 1), min(16 * (L // 16), L - 1)} <= set(c.rel_idx[:, ax].tolist())
    if c.scale_rows:  # the bins of the small-weight segments are theirs alone, and the weights there are 2^12 below the first segment's largest
        for b, at in ((C.BIN_Q, c.pos), (C.BIN_K, c.cpos)):
            sel = (c.rel_idx == b).any(1)
            assert sel.sum() >= 120 and (c.rel_idx[sel] == b).all() and ((at[sel] >= 128) & (at[sel] < 256)).all()
            small = np.resize(np.float32(C.SMALL_W), 128)[:, None]
            assert (c.go_pairs[sel] == small).all() and (c.attn[sel] == small).all() and (np.float64(small) * 2.0 ** 29 % 1 == 0).all()
            first = np.flatnonzero((at == 0) & np.isin(c.row if b == C.BIN_Q else c.index_1, (c.row if b == C.BIN_Q else c.index_1)[sel]))
            assert len(first) == 1 and (c.go_pairs[first] == C.ANCHOR_W).all() and (c.attn[first] == C.ANCHOR_W).all()
    # the key-major view is the stable transposition
    assert np.array_equal(c.index_1[c.csc_pair], np.sort(c.index_1, kind="stable")) and (np.diff(c.cpos[c.csc_pair]) <= 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds are reachable: the C oracle (sequential fp32) and the fixed-point emulation stay inside on every case
# ---------------------------------------------------------------------------------------------------------------------
def _oracle(c, group):
    a = c.arrays()
    o, i1, rel = a["offsets"], a["index_1"], a["rel_idx"]
    if group == "a1":
        gq, gk = ref.attention_step1_v2_backward(a["go_pairs"], a["q"], a["k"], i1, o)
        return {"a1.out": ref.attention_step1_v2(a["q"], a["k"], i1, o), "a1.gq": gq, "a1.gk": gk}
    if group == "a2":
        args = (a["q"], o, a["k"], i1, a["table_q"], a["table_k"], rel)
        gq, gk, gtq, gtk = ref.dot_prod_with_idx_v3_backward(a["go_pairs"], *args)
        return {"a2.out": ref.dot_prod_with_idx_v3(*args), "a2.gq": gq, "a2.gk": gk, "a2.gtq": gtq, "a2.gtk": gtk}
    if group == "a4":
        args = (a["attn"], a["v"], o, i1, a["table_v"], rel)
        ga, gv, gt = ref.attention_step2_with_rel_pos_value_v2_backward(a["go_rows"], *args)
        return {"a4.out": ref.attention_step2_with_rel_pos_value_v2(*args), "a4.ga": ga, "a4.gv": gv, "a4.gt": gt}
    args2 = (a["q"], o, a["k"], i1, a["table_q"], a["table_k"], rel)
    logits = ref.attention_step1_v2(a["q"], a["k"], i1, o) + ref.dot_prod_with_idx_v3(*args2)
    attn = ref.segment_softmax(logits, o)
    args4 = (attn, a["v"], o, i1, a["table_v"], rel)
    ga, gv, gtv = ref.attention_step2_with_rel_pos_value_v2_backward(a["go_rows"], *args4)
    dl = ref.segment_softmax_backward(attn, ga, o)
    gq1, gk1 = ref.attention_step1_v2_backward(dl, a["q"], a["k"], i1, o)
    gq2, gk2, gtq, gtk = ref.dot_prod_with_idx_v3_backward(dl, *args2)
    return {"f.out": ref.attention_step2_with_rel_pos_value_v2(*args4), "f.gq": gq1 + gq2, "f.gk": gk1 + gk2, "f.gv": gv,
            "f.gtq": gtq, "f.gtk": gtk, "f.gtv": gtv, "f.attn": attn, "logits": logits}


@pytest.fixture(scope="module")
def one_thread():
    """the oracle's table gradients are merged from per-thread copies: one thread makes its sums sequential and repeatable"""
    n = ref.num_threads()
    ref.set_num_threads(1)
    yield
    ref.set_num_threads(n)


def _runs(spec, group):
    return all(p.family != "error" for p in C.paths(spec, group))


@pytest.mark.parametrize("group", GROUPS)
def test_the_oracle_meets_every_bound(one_thread, group):
    worst = {}
    for spec in C.specs_of(group):
        if not _runs(spec, group):
            continue
        c = C.case(spec)
        outs = _oracle(c, group)
        refs = C.fused_reference(c, outs.pop("logits"), outs["f.attn"]) if group == "fused" else None
        for name, got in outs.items():
            f = C.check(c, group, name, got, "oracle ", refs)
            if f > worst.get(name, (0, ""))[0]:
                worst[name] = (f, spec.name)
    for name, (f, where) in sorted(worst.items()):
        print(f"fraction oracle {name} {f:.4f} {where}")
    assert worst and max(f for f, _ in worst.values()) <= 1


def _emulated(c, group, reuse_scale=False):
    """the table gradients of the matrix-core path from the fixed-point emulation"""
    HG = C.paths(c.spec, group)[1].HG
    if group == "a2":
        return {"a2.gtq": C.emulate_table_grad(c, c.go_pairs, c.q, "q", HG, reuse_scale),
                "a2.gtk": C.emulate_table_grad(c, c.go_pairs, c.k, "k", HG, reuse_scale)}
    return {"a4.gt": C.emulate_table_grad(c, c.attn, c.go_rows, "q", HG, reuse_scale)}


@pytest.mark.parametrize("group", ("a2", "a4"))
def test_the_fixed_point_emulation_meets_the_table_bound(group):
    worst, n = {}, 0
    for spec in C.specs_of(group):
        if C.paths(spec, group)[1].family != "mfma":
            continue
        c = C.case(spec)
        n += 1
        for name, got in _emulated(c, group).items():
            f = C.check(c, group, name, got, "emulation ")
            if f > worst.get(name, (0, ""))[0]:
                worst[name] = (f, spec.name)
    for name, (f, where) in sorted(worst.items()):
        print(f"fraction emulation {name} {f:.4f} {where}")
    assert n >= 30 and max(f for f, _ in worst.values()) <= 1


# ---------------------------------------------------------------------------------------------------------------------
# the bounds are not vacuous: one fault each, rejected on every output of every case it applies to
# ---------------------------------------------------------------------------------------------------------------------
def _rejected(c, group, name, got, refs=None):
    try:
        C.check(c, group, name, got, refs=refs)
    except AssertionError:
        return True
    return False


def _fused_mutant(c, fault):
    """the fused module with one fault, and the references the GPU test would hold it to: the logits of the (sound) separate
    operators, and the attn the faulty module itself saved - its own where the fault reaches the forward, the true one otherwise"""
    true = C.model(c, "fused")
    logits = (C.model(c, "a1")["a1.out"] + C.model(c, "a2")["a2.out"]).astype(np.float32)
    attn = None if C.forward_fault(c.spec, fault) else true["f.attn"].astype(np.float32)
    got = C._Model(c, fault).fused(attn)
    return got, C.fused_reference(c, logits, got["f.attn"])


@pytest.mark.parametrize("fault", C.FAULTS)
def test_every_fault_is_rejected_wherever_it_applies(fault):
    caught, missed = {}, []
    for group in GROUPS:
        for spec in C.specs_of(group):
            names = C.must_catch(spec, group, fault)
            if not names:
                continue
            c = C.case(spec)
            refs = None
            if group == "fused":
                got, refs = _fused_mutant(c, fault)
            else:
                got = _emulated(c, group, reuse_scale=True) if fault == "second_segment_reuses_scale" else C.model(c, group, fault)
            for name in names:
                (caught.setdefault(name, []) if _rejected(c, group, name, got[name], refs) else missed).append(spec.name + " " + name)
    for name, where in sorted(caught.items()):
        print(f"mutant {fault} {name} rejected on {len(where)} cases")
    assert caught and not missed, f"{fault}: accepted on {missed[:10]}"


def test_which_cases_catch_which_fault():
    """the claims of must_catch, against the paths: a fault that needs a partial head group, a tile or a long row is claimed by
    exactly the cases that have one"""
    for spec in C.SPECS:
        for group in spec.ops:
            if not _runs(spec, group):
                continue
            fwd, bwd = C.paths(spec, group)
            claims = {f: C.must_catch(spec, group, f) for f in C.FAULTS}
            heads = (fwd, bwd if bwd.family != "operators" else C.paths(spec, "a2")[1])  # (no fused backward: the A2 backward's groups)
            partial = any(p.family in ("rows", "lds-slice", "mfma") and p.hgn_last < p.HG for p in heads)
            assert bool(claims["last_head_not_stored"]) == partial, spec.name
            assert claims["last_pair_dropped"] and claims["slot_past_end_added"]
            if group != "a1":
                mfma = bwd.family == "mfma"
                assert bool(claims["bins_from_64_dropped"]) == (mfma and bwd.TA == 5)
                assert bool(claims["bins_of_the_partial_tile_dropped"]) == (mfma and spec.L % 16 != 0)
                assert bool(claims["second_segment_dropped"]) == mfma
                assert bool(claims["axes_swapped"]) == (spec.L >= 2)
    # every fault of the list has cases on every instance it can hit
    hit = {(f, C.kernel_id(C.paths(s, g)[1])) for s in C.SPECS for g in s.ops for f in C.FAULTS if C.must_catch(s, g, f)}
    for last in (1, 2):  # the partial groups of the matrix-core backward: HG = min(h, 3), so only HG 3 has one
        for TA in (4, 5):
            assert {("last_head_not_stored", f"mfma-D16-HG3.{last}-TA{TA}-n1"), ("prev_table_slice", f"mfma-D16-HG3.{last}-TA{TA}-n1")} <= hit
    assert {f for f, _ in hit} == set(C.FAULTS)
