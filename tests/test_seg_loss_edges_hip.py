"""GPU (-m gpu): csrc/seg_loss.hip at the edges of its own layout - every case of tests/seg_loss_cases.py (tile heights, row strides,
16-byte pieces inside a row, over two rows and over up to eight, the scalar tail, the all-scalar path, row counts on the tile
boundaries), the forward with fewer rows of `partials` than tiles, the finishing kernel at 63 / 64 / 65 partials, the backward's
grid-stride loop, its two alignment conditions and NULL gradients, labels and an ignore_index outside 32 bits, smoothing on half rows -
against the float64 oracle of tests/loss_oracle.py.  The helpers and the bar are tests/test_loss_hip.py's:

    grad_logits, grad_shift_pred, ce, l1, total:   err(fused) <= 4 * err(composite) + u * max|want|,  u by the output's type
    counts, rows:                                  equal to the oracle's
    stat[:, 0]:                                    bit-equal to the row maximum of the widened logits
    rows that are not valid:                       grad_logits exactly +0
    another launch shape (partial rows, alignment, a NULL gradient), a label outside 32 bits instead of ignore_index: the same bits

The inputs (seg_loss_cases.case_inputs): valid, ignored and out-of-range rows with period 3, neighbouring valid rows with different
targets, so that a row state taken from the wrong row of a piece shows as a non-zero ignored row or a misplaced 1 - w.  torch's
composite traps an out-of-range label on the device, so it is given the same rows with every label that is not valid set to its
ignore_index: the same arithmetic.

Measured on one MI355X (max abs error against float64, fused / composite; per family the worst case of each output; 256 CUs):
    fp32 aligned (30 cases)   ce 6.5e-07 / 6.5e-07   l1 5.5e-08 / 6.4e-08   total 3.9e-07 / 8.2e-08   grad_logits 6.8e-08 / 1.1e-07   grad_shift_pred 5.0e-09 / 5.0e-09
    fp32 misaligned           ce 2.0e-07 / 2.7e-07   l1 4.9e-08 / 7.0e-08   total 2.5e-07 / 2.5e-07   grad_logits 4.1e-09 / 3.7e-09   grad_shift_pred 3.4e-11 / 3.4e-11
    f16 aligned (31 cases)    ce 3.9e-07 / 3.9e-07   l1 5.9e-08 / 6.0e-08   total 3.4e-07 / 3.4e-07   grad_logits 2.1e-04 / 2.1e-04   grad_shift_pred 4.1e-05 / 4.1e-05
    f16 misaligned            ce 1.4e-07 / 1.4e-07   l1 5.1e-08 / 5.1e-08   total 1.0e-07 / 1.0e-07   grad_logits 7.5e-06 / 7.5e-06   grad_shift_pred 2.4e-07 / 2.4e-07
    bf16 (10 cases)           ce 3.9e-07 / 3.9e-07   l1 5.7e-08 / 6.2e-08   total 3.2e-07 / 3.2e-07   grad_logits 6.1e-05 / 6.1e-05   grad_shift_pred 2.6e-06 / 2.6e-06
    (the largest gradient figures are the one-row cases: a / n_valid = 1)
    smooth_eps 0.1, upstream (0.5, 0.25, 1): fp32 C=2 grad_logits 1.6e-09 / 2.8e-09; f16 C=7 7.5e-06 / 7.5e-06, C=33 1.5e-05 / 1.5e-05; bf16 C=7 6.1e-05 / 6.1e-05,
        C=33 1.2e-04 / 1.2e-04
    lse rebuilt from stat: 6.8e-07 on values up to 13.3 at the worst
    1, 2, 3 partial rows for 3 tiles, 63, 64, 65 for 66: stat, counts, rows the bits of the 1024-row run; the losses the same figures at every
        count, e.g. f32 C=33 n=8321 ce 7.0e-08 / 7.0e-08, f16 C=33 n=300 ce 8.4e-08 / 5.6e-07
    backward grid stride, f16 C=33 n=262149: 2049 tiles on 2048 workgroups; ce 1.9e-07 / 1.9e-07  grad_logits 3.0e-08 / 3.0e-08; the last
        tile's 5 rows 2.8e-08 on gradients up to 1.1e-05.  0.49 s, the longest test here (oracle and composite included)
    labels outside 32 bits: C=19 ce 1.9e-07 / 1.9e-07  grad_logits 2.4e-09 / 1.2e-09; C=64 ce 2.1e-07 / 2.6e-07  grad_logits 2.5e-09 / 1.2e-09
    f32 logits beside bf16 shift_pred: grad_shift_pred 9.6e-07 / 9.6e-07   l1 3.7e-08 / 3.7e-08
What these tests found: f16-c32-n1 (a single row: two non-zero L1 terms) had l1 5.96e-08 / 0.00e+00 against a bar of 4 * 0 + 2^-24 * 0.7995 =
4.77e-08.  The float64 value 0.79950517416 is itself an fp32 number and the composite happens to land on it; the kernel's fp32 subtraction
rounded the term 2.30340636 to 2.30340624 and the sum ended one fp32 step (5.96e-08) below.  The forward now takes |shift_pred - shift| in
double, as the sum it goes into: l1 is the float64 value rounded once, at most 2^-24 * |l1| off whatever the composite does.  With it that
case has l1 0.00e+00 / 0.00e+00 (ce 1.42e-07 / 1.42e-07, grad_logits 2.08e-04 / 2.08e-04), and the f16 family's worst l1 is 5.9e-08 / 6.0e-08;
the figures above are of that kernel.
Every test prints its figures.
"""
import time

import numpy as np
import pytest
import torch

from tests import loss_oracle as O
from tests import seg_loss_cases as L
from tests import test_loss_hip as T

pytestmark = pytest.mark.gpu

U, DTYPES, _bits, _f64 = T.U, T.DTYPES, T._bits, T._f64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


@pytest.fixture(scope="module")
def C():
    from stratified_transformer_amd import pointops2_cuda
    return pointops2_cuda


def _p(rows, c, n, seed, misaligned=False, eps=0.0, sname=None, ignore=L.IGNORE):
    """the operands of tests/test_loss_hip.py's helpers, from seg_loss_cases.case_inputs rounded to the row types"""
    raw, sname = L.case_inputs(c, n, seed, ignore), sname or rows
    p = dict(x=torch.from_numpy(raw["x"]).to(DTYPES[rows]), t=torch.from_numpy(raw["t"]), sp=torch.from_numpy(raw["sp"]).to(DTYPES[sname]),
             s=torch.from_numpy(raw["s"]))
    p["s"][0, 0] = p["sp"][0, 0].float()                                                    # sign(0) = 0
    p.update(misaligned=misaligned, eps=eps, weight=0.5, lname=rows, sname=sname, ignore=ignore)
    return p


def _case_p(case):
    return _p(case.rows, case.c, case.n, seed=1000 * case.c + case.n, misaligned=case.misaligned, eps=case.eps)


def _valid(p):
    return O.valid_rows(p["t"].numpy(), p["x"].shape[1], p["ignore"])


def _composite(p, g):
    """torch's chain on the same rows, every label that is not valid set to -100 = its ignore_index (torch traps the others)"""
    t = torch.where(torch.from_numpy(_valid(p)), p["t"], torch.full_like(p["t"], -100))
    assert bool((((t >= 0) & (t < p["x"].shape[1])) | (t == -100)).all())
    return T._composite(dict(p, t=t, ignore=-100), g)


def _bars(p, got, comp, want, losses_only=False):
    """the standing bar on every float output -> (ok, figures)"""
    ok, figures = True, []
    for k, name in enumerate(("ce", "l1", "total")):
        fine, fig = T._under_bar(name, got["losses"][k], comp["losses"][k], want["losses"][k], U["f32"])
        ok, figures = ok and fine, figures + [fig]
    if not losses_only:
        for name, u in (("grad_logits", U[p["lname"]]), ("grad_shift_pred", U[p["sname"]])):
            fine, fig = T._under_bar(name, got[name], comp[name], want[name], u)
            ok, figures = ok and fine, figures + [fig]
    return ok, figures


def _check(P, p, label, g=(0.0, 0.0, 1.0)):
    """the operator against the oracle and the composite -> (want, got)"""
    want, got, comp = T._oracle(p, g), T._fused(P, p, g), _composite(p, g)
    n, c = p["x"].shape
    assert got["grad_logits"].dtype == p["x"].dtype and tuple(got["grad_logits"].shape) == (n, c)
    assert got["grad_shift_pred"].dtype == p["sp"].dtype and tuple(got["grad_shift_pred"].shape) == (n, 3)
    ok, figures = _bars(p, got, comp, want)
    print(f"segmentation_loss {label}: " + "  ".join(figures) + ("" if ok else "   <-- over the bar"))
    assert np.array_equal(got["counts"].cpu().numpy(), want["counts"]), (got["counts"].tolist(), want["counts"].tolist())
    assert got["rows"].tolist() == want["rows"].tolist()
    assert ok
    invalid = torch.from_numpy(~_valid(p)).cuda()
    assert not bool(_bits(got["grad_logits"][invalid]).any())                               # exactly zero (and +0)
    assert float(got["grad_shift_pred"][0, 0]) == 0.0
    return want, got


def _forward(C, p, x, sp, s, partial_rows=L.PARTIAL_ROWS, ints=None):
    """pointops2_cuda.seg_loss_forward -> dict(stat, counts, rows, losses); ints: (counts, rows) to accumulate into"""
    n, c = x.shape
    stat = torch.full((n, 2), float("nan"), device="cuda")
    partials = torch.full((partial_rows, 2), float("nan"), device="cuda", dtype=torch.float64)
    counts, rows = ints or (torch.zeros(3, c, device="cuda", dtype=torch.int64), torch.zeros(2, device="cuda", dtype=torch.int64))
    losses = torch.empty(3, device="cuda")
    C.seg_loss_forward(n, c, x, p["t"].cuda(), sp, s, p["ignore"], p["eps"], p["weight"], stat, partials, counts, rows, losses)
    torch.cuda.synchronize()
    return dict(stat=stat, counts=counts, rows=rows, losses=losses)


def _operands(p, misaligned=None):
    mis = p["misaligned"] if misaligned is None else misaligned
    return T._to(p["x"], mis), T._to(p["sp"], mis), T._to(p["s"], mis)


def _stat_is_the_row_maximum(p, stat):
    return torch.equal(_bits(stat[:, 0].cpu()), _bits(p["x"].float().max(dim=1)[0]))


# ---- every case of the table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_every_case_against_the_oracle(P, C, case):
    """the operator under the bar, then the launcher for stat"""
    p = _case_p(case)
    tiles = L.tile_count(case.n, case.c)
    label = (f"{L.case_id(case)} [tile {case.tile}, {case.parity} C, pieces {case.pieces}, {case.path}, last tile {case.last}; {tiles} tiles, "
             f"forward grid {case.finish}, {L.bins_of(case.c)} bins]")
    want, got = _check(P, p, label)
    x, sp, s = _operands(p)
    assert (x.data_ptr() % 16 != 0) == case.misaligned
    fwd = _forward(C, p, x, sp, s, case.partial_rows or L.PARTIAL_ROWS)
    assert _stat_is_the_row_maximum(p, fwd["stat"])
    lse = _f64(fwd["stat"]).sum(1)
    err, top = float(np.abs(lse - want["lse"]).max()), float(np.abs(want["lse"]).max())
    print(f"    stat: maximum bit-equal, lse err {err:.2e} on values up to {top:.2f}")
    assert err <= 4 * U["f32"] * top                                                        # tests/test_loss_hip.py's bar on the rebuilt lse
    assert np.array_equal(fwd["counts"].cpu().numpy(), want["counts"]) and fwd["rows"].tolist() == want["rows"].tolist()
    if case.partial_rows is None:                                                           # the operator's own launch shape: its bits
        assert torch.equal(_bits(fwd["losses"]), _bits(got["losses"]))
    else:
        ok, figures = _bars(p, fwd, _composite(p, (0.0, 0.0, 1.0)), want, losses_only=True)
        print(f"    {case.partial_rows} partial rows for {tiles} tiles: " + "  ".join(figures))
        assert ok and case.partial_rows <= tiles


# ---- fewer rows of partials than tiles; the finishing kernel at 63 / 64 / 65 ---------------------------------------------------
PARTIAL_FAMILIES = sorted({(c.rows, c.c, c.n): None for c in L.CASES if c.partial_rows is not None})


@pytest.mark.parametrize("rows,c,n", PARTIAL_FAMILIES, ids=lambda v: str(v))
def test_partial_rows(C, rows, c, n):
    """the forward's loop over several tiles per workgroup: the histogram lives across them, the staging buffer is reused behind the
    trailing barrier; counts and rows are ACCUMULATED"""
    family = [case for case in L.CASES if (case.rows, case.c, case.n) == (rows, c, n) and case.partial_rows is not None]
    tiles = L.tile_count(n, c)
    assert len(family) == 3 and all(case.partial_rows <= tiles for case in family)
    p = _case_p(family[0])
    want, comp = T._oracle(p), _composite(p, (0.0, 0.0, 1.0))
    x, sp, s = _operands(p)
    base = _forward(C, p, x, sp, s)
    assert np.array_equal(base["counts"].cpu().numpy(), want["counts"]) and base["rows"].tolist() == want["rows"].tolist()
    for case in family:
        run = _forward(C, p, x, sp, s, case.partial_rows)
        ok, figures = _bars(p, run, comp, want, losses_only=True)
        print(f"seg_loss_forward {rows} C={c} n={n}: {tiles} tiles on {L.forward_grid(n, c, case.partial_rows)} workgroups "
              f"({case.partial_rows} partial rows, {-(-tiles // case.partial_rows)} tiles a workgroup at most): " + "  ".join(figures))
        assert L.forward_grid(n, c, case.partial_rows) == case.partial_rows
        for name in ("stat", "counts", "rows"):
            assert torch.equal(_bits(run[name]), _bits(base[name])), (case.partial_rows, name)
        assert ok
        again = _forward(C, p, x, sp, s, case.partial_rows, ints=(run["counts"], run["rows"]))      # un-zeroed: exactly doubled
        assert torch.equal(again["counts"], 2 * base["counts"]) and torch.equal(again["rows"], 2 * base["rows"])
        assert torch.equal(_bits(again["stat"]), _bits(base["stat"])) and torch.equal(_bits(again["losses"][1:2]), _bits(run["losses"][1:2]))


# ---- the backward's grid-stride loop --------------------------------------------------------------------------------------------
def test_backward_grid_stride(P):
    """tiles = 8 * CUs + 1 at C = 33, f16: the smallest shape whose first workgroup takes a second trip of `t += gridDim.x`.  About
    262 000 rows and 17 MB on a 256-CU part."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c, extra = 33, 5
    n = 128 * 8 * cus + extra
    tiles, grid = L.tile_count(n, c), L.backward_grid(n, c, cus)
    assert tiles == 8 * cus + 1 == grid + 1 and L.tile_walk(n, c, grid)[2] == 2
    t0 = time.perf_counter()
    p = _p("f16", c, n, seed=77)
    want, got = _check(P, p, f"f16 C={c} n={n}: backward {tiles} tiles on {grid} workgroups ({cus} CUs), forward on {L.forward_grid(n, c)}")
    last = slice(n - extra, n)                                                              # the second trip's rows
    kinds = L.row_kinds(n)[last]
    g = got["grad_logits"][last]
    assert not bool(_bits(g[torch.from_numpy(kinds != 0).cuda()]).any()) and bool((g[torch.from_numpy(kinds == 0).cuda()] != 0).any())
    err = float(np.abs(_f64(g) - want["grad_logits"][last]).max())
    print(f"    the last tile's {extra} rows: grad_logits err {err:.2e} on values up to {float(np.abs(want['grad_logits'][last]).max()):.2e}; "
          f"{time.perf_counter() - t0:.2f} s with the oracle and the composite")
    assert tiles > grid


# ---- the backward's vector condition and NULL gradients -------------------------------------------------------------------------
def _backward(C, p, x, sp, s, stat, rows, g, grad_x_misaligned=False, want_x=True, want_sp=True):
    n, c = x.shape
    gx = gsp = None
    if want_x:
        gx = T._to(torch.full((n, c), float("nan"), dtype=x.dtype), grad_x_misaligned)
        assert (gx.data_ptr() % 16 != 0) == grad_x_misaligned
    if want_sp:
        gsp = torch.full((n, 3), float("nan"), dtype=sp.dtype, device="cuda")
    C.seg_loss_backward(n, c, x, p["t"].cuda(), stat, sp, s, torch.tensor(g, device="cuda"), rows, p["ignore"], p["eps"], p["weight"], gx, gsp)
    torch.cuda.synchronize()
    return gx, gsp


@pytest.mark.parametrize("rows", ["f32", "f16"])
def test_backward_alignment(P, C, rows):
    """the vector path needs logits AND grad_logits aligned; the operator always allocates an aligned grad_logits"""
    c, n, g = 19, 333, (0.5, 0.25, 1.0)
    p = _p(rows, c, n, seed=81)
    _, got = _check(P, p, f"{rows} C={c} n={n}, upstream (0.5, 0.25, 1): the all-aligned run", g)
    x, sp, s = _operands(p, False)
    xm = T._to(p["x"], True)
    fwd = _forward(C, p, x, sp, s)
    base = _backward(C, p, x, sp, s, fwd["stat"], fwd["rows"], g)
    assert torch.equal(_bits(base[0]), _bits(got["grad_logits"])) and torch.equal(_bits(base[1]), _bits(got["grad_shift_pred"]))   # the operator's run
    for name, xx, gmis in (("aligned logits, misaligned grad_logits", x, True), ("misaligned logits, aligned grad_logits", xm, False),
                           ("both misaligned", xm, True)):
        assert L.backward_vec(rows, xx is xm, gmis) is False
        run = _backward(C, p, xx, sp, s, fwd["stat"], fwd["rows"], g, grad_x_misaligned=gmis)
        same = torch.equal(_bits(run[0]), _bits(base[0])) and torch.equal(_bits(run[1]), _bits(base[1]))
        print(f"    {name}: {'the same bits' if same else 'OTHER BITS'}")
        assert same, name


@pytest.mark.parametrize("rows", ["f32", "f16"])
def test_backward_with_one_gradient(P, C, rows):
    """grad_logits without grad_shift_pred and the reverse: a NULL pointer at the launcher, requires_grad on one input at the operator"""
    c, n, g = 19, 333, (0.5, 0.25, 1.0)
    p = _p(rows, c, n, seed=82)
    x, sp, s = _operands(p, False)
    fwd = _forward(C, p, x, sp, s)
    both = _backward(C, p, x, sp, s, fwd["stat"], fwd["rows"], g)
    assert not bool(torch.isnan(both[0]).any()) and not bool(torch.isnan(both[1]).any())    # each fully written
    gx, none = _backward(C, p, x, sp, s, fwd["stat"], fwd["rows"], g, want_sp=False)
    assert none is None and torch.equal(_bits(gx), _bits(both[0]))
    none, gsp = _backward(C, p, x, sp, s, fwd["stat"], fwd["rows"], g, want_x=False)
    assert none is None and torch.equal(_bits(gsp), _bits(both[1]))
    for which in ("logits", "shift_pred"):
        xl, spl = x.clone().requires_grad_(which == "logits"), sp.clone().requires_grad_(which == "shift_pred")
        res = P.segmentation_loss(xl, p["t"].cuda(), spl, s, ignore_index=p["ignore"], offset_weight=p["weight"])
        res.losses.backward(torch.tensor(g, device="cuda"))
        torch.cuda.synchronize()
        if which == "logits":
            assert spl.grad is None and torch.equal(_bits(xl.grad), _bits(both[0]))
        else:
            assert xl.grad is None and torch.equal(_bits(spl.grad), _bits(both[1]))
    print(f"seg_loss_backward {rows} C={c} n={n}: grad_logits alone and grad_shift_pred alone, at the launcher and at the operator: the bits of the run with both")


# ---- labels are long long ---------------------------------------------------------------------------------------------------------
WILD = (2 ** 32 + 3, -2 ** 63, 2 ** 63 - 1)


@pytest.mark.parametrize("ignore", [L.IGNORE, 2 ** 40], ids=["ignore255", "ignore2p40"])
@pytest.mark.parametrize("c", [19, 64])
def test_labels_outside_32_bits(P, c, ignore):
    """2**32 + 3 is not class 3, -2**63 and 2**63 - 1 are not in range: each is counted in rows[1] and skipped.  An ignore_index of 2**40
    carried by real rows is compared as 64 bits.  Every class and every bin is populated, 3 C + 1 (at C = 64 the last word of the
    histogram) included."""
    n, g = 600, (0.5, 0.25, 1.0)
    p = _p("f32", c, n, seed=90 + c, ignore=ignore)
    first = (np.arange(n) % 3 == 0) & (np.arange(n) // 3 < c)                               # the first valid row of every class: predicted right
    p["x"][torch.from_numpy(first), p["t"][torch.from_numpy(first)]] += 40.0
    want, ignored = _check(P, p, f"fp32 C={c} n={n}, ignore_index {ignore} ({L.bins_of(c)} bins)", g)
    assert (want["counts"] > 0).all() and want["rows"][0] == 200 and want["rows"][1] == 200  # every class in every count, both row bins
    assert int((p["t"] == ignore).sum()) == 200
    spots = [1, 301, 598]                                                                   # ignored rows of the first, second and third tile (C = 64)
    assert all(int(p["t"][r]) == ignore for r in spots)
    for r, label in zip(spots, WILD):
        p["t"][r] = label
    got = T._fused(P, p, g)
    assert got["rows"].tolist() == [200, 203] and ignored["rows"].tolist() == [200, 200]
    for name in ("losses", "counts", "grad_logits", "grad_shift_pred"):
        assert torch.equal(_bits(got[name]), _bits(ignored[name])), name
    assert np.array_equal(got["counts"].cpu().numpy(), T._oracle(p, g)["counts"])
    print(f"    labels {WILD}: rows {got['rows'].tolist()}, everything else the bits of the run where they are ignore_index")


# ---- smoothing and mixed row types at the piece edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.select(eps=0.1), ids=L.case_id)
def test_smoothing_under_an_upstream_gradient(P, case):
    """smooth_eps = 0.1 at C = 2 (eps / (C - 1) = eps) in fp32 and on half rows of 7 and 33 classes, the three losses weighted"""
    assert (case.rows, case.c) in {("f32", 2), ("f16", 7), ("f16", 33), ("bf16", 7), ("bf16", 33)}
    _check(P, _case_p(case), f"{L.case_id(case)} smooth_eps {case.eps}, upstream (0.5, 0.25, 1)", (0.5, 0.25, 1.0))


@pytest.mark.parametrize("rows,sname,misaligned", [("f32", "bf16", False), ("f32", "bf16", True), ("bf16", "f32", False), ("f32", "f16", True)])
def test_shift_rows_of_another_type(P, rows, sname, misaligned):
    """a half shift_pred beside fp32 logits (and the reverse), aligned and one element into its buffer"""
    p = _p(rows, 19, 511, seed=95, misaligned=misaligned, sname=sname)
    _check(P, p, f"{rows} logits, {sname} shift_pred C=19 n=511{' misaligned' if misaligned else ''}", (0.5, 0.25, 1.0))
