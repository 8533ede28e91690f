"""CPU: the harness of tests/test_cell_edges_hip.py (tests/cell_edges.py) against the oracle - the float64 restatement of the
operator chain, the non-finite row sets predicted from the pair list, and the input conditions of the saturated-softmax cases that
need no cell plan.  No HIP compute runs here."""
import numpy as np
import pytest
import torch

from tests import cell_edges as ce
from tests.util import window_problem


def _problem(scale=1.0, seed=3, n=3000, h=3):
    p = window_problem(n, seed=seed, h=h, d=16)
    p["q"] = p["q"] * np.float32(scale)
    return p, p["index_0"], p["index_1"], p["offsets"], p["rel_idx"], p["go_rows"]


def test_float64_restatement_agrees_with_the_oracle():
    """At the standing operand distribution (s = 1) the numpy float64 chain and the oracle agree at the standing bars of
    test_cell_attention_matches_the_oracle, forward and all six gradients; the softmax weights too."""
    p, i0, i1, offs, rel, go = _problem()
    want, wg = ce._oracle_attention(p, i1, offs, rel, go)
    out, g, lg = ce.attention_f64(p, i0, i1, offs, rel, go)
    np.testing.assert_allclose(ce.softmax_f64(lg, offs), ce._oracle_softmax(p, i1, offs, rel), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(out, want, **ce.FTOL)
    for name in ("q", "k", "v"):
        np.testing.assert_allclose(g[name], wg[name], err_msg=name, **ce.GTOL)
    for name in ce._TABLES:
        s = max(1.0, float(np.abs(wg[name]).max()))
        np.testing.assert_allclose(g[name] / s, wg[name] / s, err_msg=name, **ce.TTOL)
    # forward only: no gradients, the same output
    out2, g2, _ = ce.attention_f64(p, i0, i1, offs, rel)
    assert g2 is None and np.array_equal(out, out2)


@pytest.mark.parametrize("kind", ce.POISONS)
def test_predicted_nonfinite_rows_are_the_oracles(kind):
    """One poisoned row (row 0, a row in the middle, row n - 1): the rows of out / grad_q / grad_k / grad_v that the oracle's chain
    leaves non-finite are exactly the sets computed from the pair list, and the table gradients are non-finite where predicted.  The
    precondition of the prediction - no oracle softmax weight is exactly 0, so the oracle has no 0 * inf of its own - is asserted."""
    p, i0, i1, offs, rel, go = _problem()
    n = p["q"].shape[0]
    sm = ce._oracle_softmax(p, i1, offs, rel)
    assert np.isfinite(sm).all() and (sm > 0).all()
    for r in (0, 1234, n - 1):
        pp, gg = ce.poison(p, go, kind, r)
        out, g = ce._oracle_attention(pp, i1, offs, rel, gg)
        rows, tabs = ce.predicted_nonfinite(n, i0, i1, kind, r)
        got = dict(out=out, q=g["q"], k=g["k"], v=g["v"])
        for name in ce.ROWS:
            assert np.array_equal(ce.nonfinite_rows(got[name]), rows[name]), (kind, r, name, int(ce.nonfinite_rows(got[name]).sum()), int(rows[name].sum()))
        for name in ce._TABLES:
            assert (not np.isfinite(g[name]).all()) == tabs[name], (kind, r, name)
        holders, keys = int(rows["q"].sum()), int(rows["k"].sum())
        assert holders >= 1 and keys > holders
        if kind in ("q_nan", "go_inf"):
            assert holders == 1 and keys == offs[r + 1] - offs[r]
        # the check itself passes on the oracle's own result ...
        ce.check_poisoned(kind, got, {t: g[t] for t in ce._TABLES}, got, {t: g[t] for t in ce._TABLES})


def test_check_poisoned_catches_a_leak_a_swallowed_nan_and_a_wrong_value():
    p, i0, i1, offs, rel, go = _problem(n=1500)
    pp, gg = ce.poison(p, go, "v_inf", 0)
    out, g = ce._oracle_attention(pp, i1, offs, rel, gg)
    want = dict(out=out, q=g["q"], k=g["k"], v=g["v"])
    tabs = {t: g[t] for t in ce._TABLES}
    clean = int(np.flatnonzero(~ce.nonfinite_rows(out))[0])
    dirty = int(np.flatnonzero(ce.nonfinite_rows(out))[0])
    leak = dict(want, out=out.copy())
    leak["out"][clean, 0, 3] = np.nan
    with pytest.raises(AssertionError, match="1 rows wrongly non-finite"):
        ce.check_poisoned("leak", leak, tabs, want, tabs)
    lost = dict(want, out=out.copy())
    lost["out"][dirty] = 0.0
    with pytest.raises(AssertionError, match="1 rows wrongly finite"):
        ce.check_poisoned("lost", lost, tabs, want, tabs)
    off = dict(want, v=g["v"].copy())
    off["v"][clean, 0, 0] += 1e-3
    with pytest.raises(AssertionError, match="off v"):
        ce.check_poisoned("off", off, tabs, want, tabs)
    assert not np.isfinite(tabs["table_q"]).all() and np.isfinite(tabs["table_v"]).all()
    with pytest.raises(AssertionError, match="swallowed"):
        ce.check_poisoned("swallowed", want, dict(tabs, table_q=np.nan_to_num(tabs["table_q"], posinf=0.0, neginf=0.0)), want, tabs)
    spread = dict(tabs, table_v=tabs["table_v"].copy())
    spread["table_v"][0, 0, 0, 0] = np.inf
    with pytest.raises(AssertionError, match="the oracle's is finite"):
        ce.check_poisoned("spread", want, spread, want, tabs)


def test_poison_rows_picks_the_last_key_of_the_largest_ragged_cell():
    nk = np.array([16, 21, 32, 37, 5])
    kbase = np.concatenate([[0], np.cumsum(nk)])
    keys = np.arange(kbase[-1]) + 100
    rows = ce.poison_rows(nk, kbase, keys, 500)
    assert rows == dict(row0=0, last_key_of_ragged_cell=100 + kbase[4] - 1, last_row=499)


@pytest.mark.parametrize("s,least,most", [(4.0, 0.0, 0.25), (16.0, 0.25, 1.0), (64.0, 0.9, 1.0)])
def test_scaled_queries_saturate_the_oracles_softmax(s, least, most):
    """q scaled by 16 or 64: the oracle stays finite, at least a quarter (16x) of its weights are exactly 0 and some row is one-hot into
    the 2^30 histogram; at 4x the softmax is not saturated, which is why the cases use 16x."""
    p, i0, i1, offs, rel, go = _problem(scale=s)
    sm = ce._oracle_softmax(p, i1, offs, rel)
    out, g = ce._oracle_attention(p, i1, offs, rel, go, sm=sm)
    assert np.isfinite(out).all() and all(np.isfinite(x).all() for x in g.values())
    res = ce.saturation_conditions(ce.logits_f64(p, i0, i1, rel), sm, offs)
    assert least <= res["zero_fraction"] <= most, res
    if s >= 16:
        ce.assert_saturated(res, multi_chunk=False)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_packed_scales_saturate_the_oracles_softmax(dtype):
    """The packed launchers' cases pass scale = 64 * _SCALES[dtype] (q' = 19.2, 12.2, 16 times a standard normal, rounded by torch in
    the row type as _oracle_operands does): still at least a quarter of the oracle's weights are exactly 0, everything finite."""
    p, i0, i1, offs, rel, go = _problem()
    td = dict(float16=torch.float16, bfloat16=torch.bfloat16, float32=torch.float32)[dtype]
    scale = 64 * ce._SCALES[dtype]
    for x in ("q", "k", "v"):
        t = torch.from_numpy(p[x]).to(td)
        p[x] = ((t * scale) if x == "q" else t).float().numpy()
    sm = ce._oracle_softmax(p, i1, offs, rel)
    out, _ = ce._oracle_attention(p, i1, offs, rel, None, sm=sm)
    assert np.isfinite(out).all()
    ce.assert_saturated(ce.saturation_conditions(ce.logits_f64(p, i0, i1, rel), sm, offs), multi_chunk=False)


def test_saturation_conditions_read_the_chunks_of_a_row():
    """Rows of 300 keys in slot order (three chunks of 128): the maximum's chunk and a rise of the running maximum by more than 88
    between two chunks are found; rows of cells with at most 128 keys are not counted."""
    def one_row(peaks):
        lg = np.zeros((300, 1))
        for slot, val in peaks.items():
            lg[slot, 0] = val
        e = np.exp(lg - lg.max())
        return lg, (e / e.sum()).astype(np.float32)
    rows = [one_row({5: 30.0}), one_row({299: 30.0}), one_row({10: 1.0, 200: 100.0}), one_row({0: 200.0, 290: 150.0})]
    for _, w in rows[2:]:
        w[w < 1e-30] = 0.0  # (as fp32 __expf flushes them)
    lg, sm = (np.concatenate([r[i] for r in rows]) for i in (0, 1))
    offs = np.arange(5, dtype=np.int32) * 300
    slot, nk = np.tile(np.arange(300), 4), np.full(1200, 300)
    res = ce.saturation_conditions(lg, sm, offs, slot, nk)
    assert (res["multi_chunk_rows"], res["max_in_first_chunk"], res["max_in_last_chunk"], res["rescale_underflows"]) == (4, 2, 1, 1), res
    assert res["one_hot_rows"] == 4 and res["zero_fraction"] > 0.49
    ce.assert_saturated(res, multi_chunk=True)
    small = ce.saturation_conditions(lg, sm, offs, slot, np.full(1200, 128))
    assert small["multi_chunk_rows"] == 0
    with pytest.raises(AssertionError):
        ce.assert_saturated(small, multi_chunk=True)


def test_check_against_f64_holds_the_kernel_to_the_oracles_own_error():
    f64 = dict(out=np.linspace(-1, 1, 64).reshape(4, 1, 16))
    oracle = dict(out=(f64["out"] + 1e-3).astype(np.float32))
    bars = ce.standing_bars(backward=False)
    ok = dict(out=(f64["out"] - 3.9e-3).astype(np.float32))
    r = ce.check_against_f64("ok", ok, oracle, f64, bars)
    assert 3.8 < r["out"][2] < 4.0
    with pytest.raises(AssertionError):
        ce.check_against_f64("bad", dict(out=(f64["out"] + 4.2e-3).astype(np.float32)), oracle, f64, bars)
    # below the standing bar the oracle's error does not matter
    exact = dict(out=f64["out"].astype(np.float32))
    ce.check_against_f64("standing", dict(out=(f64["out"] + 5e-5).astype(np.float32)), exact, f64, bars)
    with pytest.raises(AssertionError, match="non-finite"):
        ce.check_against_f64("nan", dict(out=np.full((4, 1, 16), np.nan, np.float32)), oracle, f64, bars)
