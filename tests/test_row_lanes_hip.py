"""GPU (-m gpu): the kernels that put rows on the lanes by csrc/row_lanes.h - pointops.residual_norm, residual_norm_stream, batch_norm_act
and the launchers behind sync_batch_norm_act - on the table of tests/row_lanes_cases.py: every kernel instance (VEC, ITER), every
segment width full and partly idle, rows one chunk past a boundary, and row counts on either side of a wave's and a workgroup's rows.
tests/test_row_lanes_cases_cpu.py proves the table reaches what it claims.

Bars: none of its own.  The inputs, the composites and the bars are those of tests/test_rownorm_hip.py, tests/test_rownorm_stream_hip.py,
tests/test_batchnorm_hip.py and tests/test_syncbn_hip.py, called as they stand: err(fused) <= 4 * err(composite) + u * max|want| against the
float64 oracles, the composite run on the GPU in the same test.
Exact properties ("Row lanes: cases"):
  replicated column   every channel of x, dO, the residual, gamma, beta and the running statistics holds channel 0's values: every channel of
                      o, dx, dgamma, dbeta, running_mean, running_var carries channel 0's bits (batch norm; a lane owns the same rows for all
                      its channels and every merge tree is the same function of the shape for every column)
  replicated row      all rows, row scales and incoming gradients equal: every row of z, o, stat, dx, dy carries row 0's bits, and those of
                      the row run alone (rownorm; a row's sums never leave its segment)
  poison              a NaN and a +Inf stay in their row (rownorm) / channel (batch norm) at every segment width, the last live lane
                      beside the idle ones included: the oracle's set of non-finite entries, everything else bit-identical to the clean run
  column_reduce       63, 64 and 65 rows of partials: the bars above, and two runs give the same bits

Measured on one MI355X (worst max abs error against float64 over the cases of an instance, fused / composite; the cases: widths x row counts
x the variants of the test):
    residual_norm fp32        (4,1)  140 cases   o 9.5e-07/1.0e-06   dx 7.7e-06/1.6e-05   dy 5.1e-06/1.6e-05   dgamma 8.8e-06/1.0e-05   dbeta 8.5e-06/1.9e-05
                              (4,2)   30         o 6.5e-07/6.5e-07   dx 6.1e-07/7.2e-07   dy 7.0e-07/7.2e-07   dgamma 1.8e-06/2.1e-06   dbeta 1.2e-06/1.9e-06
                              (4,4)   40         o 9.2e-07/8.3e-07   dx 7.3e-07/6.5e-07   dy 7.8e-07/6.9e-07   dgamma 2.5e-06/3.6e-06   dbeta 1.3e-06/1.9e-06
                              (1,1)  152         o 6.3e-07/6.3e-07   dx 3.3e-06/3.1e-06   dy 3.1e-06/3.1e-06   dgamma 4.0e-06/6.6e-06   dbeta 8.5e-06/1.2e-05
                              (1,16)  60         o 1.1e-06/9.3e-07   dx 6.1e-07/6.7e-07   dy 7.8e-07/7.2e-07   dgamma 2.8e-06/3.6e-06   dbeta 1.1e-06/1.9e-06
      (before the rows of c = 2, 3 were spread - _spread - (1,1) read o 1.2e-05/1.2e-05, dx 1.1e-03/1.1e-03: a variance below eps, on both sides alike)
    stream f16, y,o=f16       (4,1)   17 cases   o 1.1e-03/1.2e-03   dx 1.9e-03/3.1e-03   dy 1.9e-03/3.7e-03   dgamma 4.1e-06/8.6e-06   dbeta 3.8e-06/3.8e-06
                              (4,2)   10         o 1.9e-03/1.9e-03   dx 1.9e-03/2.7e-03   dy 2.6e-03/4.3e-03   dgamma 1.9e-06/2.8e-06   dbeta 2.4e-07/2.4e-07
                              (4,4)   10         o 1.9e-03/1.9e-03   dx 1.9e-03/2.8e-03   dy 1.9e-03/3.6e-03   dgamma 1.7e-06/2.4e-06   dbeta 2.4e-07/2.4e-07
                              (1,1)   16         o 9.7e-04/9.8e-04   dx 1.9e-03/2.3e-03   dy 1.9e-03/3.2e-03   dgamma 2.5e-06/5.1e-06   dbeta 1.1e-06/8.3e-07
                              (1,16)  15         o 1.9e-03/1.9e-03   dx 1.9e-03/2.9e-03   dy 1.9e-03/3.9e-03   dgamma 2.4e-06/2.3e-06   dbeta 2.4e-07/3.0e-07
    stream f16, y,o=f32       all five, 68       o 6.3e-07/7.7e-07   dx 1.9e-03/2.9e-03   dy 5.5e-07/2.9e-03   dgamma 4.8e-06/1.1e-05   dbeta 4.2e-06/9.6e-06
    stream bf16, y,o=bf16     (4,1)   29 cases   o 1.5e-02/1.5e-02   dx 2.8e-02/5.4e-02   dy 3.1e-02/5.1e-02   dgamma 7.4e-06/8.3e-06   dbeta 2.9e-06/2.9e-06
                              (4,2)    5         o 7.8e-03/7.8e-03   dx 1.5e-02/1.8e-02   dy 1.6e-02/3.0e-02   dgamma 1.5e-06/2.7e-06   dbeta 0/0
                              (4,4)    5         o 1.4e-02/1.4e-02   dx 1.5e-02/2.2e-02   dy 1.6e-02/2.9e-02   dgamma 1.4e-06/1.9e-06   dbeta 1.2e-07/1.2e-07
                              (1,1)   12         o 7.7e-03/7.6e-03   dx 1.2e-02/3.4e-02   dy 3.1e-02/4.9e-02   dgamma 5.3e-06/7.5e-06   dbeta 0/0
                              (1,16)  15         o 1.5e-02/1.5e-02   dx 1.5e-02/2.3e-02   dy 1.6e-02/4.5e-02   dgamma 1.4e-06/2.7e-06   dbeta 0/0
    stream bf16, y,o=f32      all five, 66       o 7.4e-07/9.3e-07   dx 2.1e-02/3.0e-02   dy 2.7e-06/3.0e-02   dgamma 6.6e-06/9.9e-06   dbeta 8.2e-06/1.5e-05
    batch_norm_act fp32       (4,1)   66 cases   o 2.5e-06/2.5e-06   dx 9.8e-05/9.8e-05   dgamma 1.9e-05/2.7e-05   dbeta 7.1e-06/8.7e-06   running_mean 6.2e-08/6.2e-08   running_var 2.8e-07/2.8e-07
                              (4,2)   12         o 2.0e-05/2.0e-05   dx 4.0e-03/4.0e-03   dgamma 3.2e-05/3.2e-05   dbeta 8.5e-07/1.0e-06   running_mean 6.6e-08/6.6e-08   running_var 2.7e-07/2.8e-07
                              (4,4)   16         o 4.4e-05/4.4e-05   dx 2.4e-03/2.4e-03   dgamma 3.1e-05/3.1e-05   dbeta 1.1e-06/1.3e-06   running_mean 6.7e-08/7.0e-08   running_var 2.8e-07/2.8e-07
                              (1,1)   72         o 1.2e-06/1.5e-06   dx 9.1e-05/9.0e-05   dgamma 6.6e-06/9.1e-06   dbeta 8.9e-06/1.2e-05   running_mean 6.2e-08/6.2e-08   running_var 2.8e-07/2.7e-07
                              (1,16)  24         o 4.3e-05/4.3e-05   dx 5.0e-03/5.0e-03   dgamma 5.2e-05/5.2e-05   dbeta 1.4e-06/1.2e-06   running_mean 6.2e-08/7.0e-08   running_var 2.8e-07/3.0e-07
      (the long rows run at n = 2, 3, 5: a column of two rows whose values nearly coincide, on both sides alike)
    batch_norm_act f16        (4,1)   32 cases   o 1.9e-03/2.9e-03   dx 1.7e-02/1.7e-02   dgamma 8.0e-06/7.8e-04   dbeta 3.8e-06/7.5e-04
                              (4,2)   16         o 1.9e-03/2.3e-03   dx 5.6e-02/5.6e-02   dgamma 1.1e-06/4.0e-04   dbeta 7.6e-07/4.8e-04
                              (4,4)   16         o 1.9e-03/2.9e-03   dx 2.6e-02/2.6e-02   dgamma 1.7e-06/5.8e-04   dbeta 7.6e-07/3.9e-04
                              (1,1)   28         o 1.9e-03/2.4e-03   dx 9.7e-04/9.7e-04   dgamma 3.1e-06/9.4e-04   dbeta 1.5e-06/8.1e-04
                              (1,16)  24         o 1.9e-03/2.9e-03   dx 2.6e-02/2.6e-02   dgamma 2.2e-06/5.8e-04   dbeta 7.6e-07/5.0e-04
    batch_norm_act bf16       (4,1)   54 cases   o 1.5e-02/2.1e-02   dx 4.8e-02/4.8e-02   dgamma 1.5e-05/1.0e-02   dbeta 1.2e-05/8.7e-03
                              (4,2)    8         o 1.5e-02/2.2e-02   dx 3.1e-02/1.6e-01   dgamma 1.3e-06/3.9e-03   dbeta 7.6e-07/3.9e-03
                              (4,4)    8         o 1.5e-02/2.1e-02   dx 2.1e-01/2.1e-01   dgamma 1.7e-06/3.9e-03   dbeta 7.6e-07/3.3e-03
                              (1,1)   24         o 1.4e-02/1.7e-02   dx 7.0e-03/7.0e-03   dgamma 5.7e-06/5.0e-03   dbeta 3.1e-06/4.9e-03
                              (1,16)  24         o 1.6e-02/2.3e-02   dx 1.2e-01/1.2e-01   dgamma 1.3e-06/3.8e-03   dbeta 7.6e-07/2.8e-03
    batch_norm_act eval fp32  all five            o 6.3e-07/6.3e-07   dx 3.2e-07/2.8e-07   dgamma 2.3e-06/2.6e-06   dbeta 1.8e-06/1.8e-06
    batch_norm_act_stats, n=1000 c=48   1 row of partials: mean 9.2e-07/6.0e-05  rstd 1.5e-06/1.9e-06  variance of the 1e3 + N(0,1) column 1.058554 for 1.058551
                                        2 rows:            mean 9.2e-07/6.0e-05  rstd 2.1e-07/1.9e-06  variance 1.058551 for 1.058551
    replicated columns, replicated rows, poison: exact at every width; column_reduce at 63, 64, 65 rows: inside the bars, the same bits twice.
Narrow widths (c = 1, 2, 3: dgamma and dbeta have fewer than four entries) take conditioned inputs, chosen from the float64 oracle alone
before anything runs on the device (_spread, _conditioned).  On the plain seeds two of the 1130 cases the bar is applied to were over it,
both reproduced to the digit by restating the kernel's fp32 arithmetic in numpy, neither an index or an order that could be better:
    batch norm c = 1, n = 255: dgamma 3.82e-06 / 6.29e-09.  One workgroup, one row a lane, the 255 terms added by a balanced tree.  dgamma
        is 63.99..; float64's value lay 6e-09 from an fp32 value, torch returned that value and the kernel its neighbour, one ulp = 2^-18
        = 3.815e-06 away; the bar left 4 * 6e-09 + 2^-24 * 63.99 = 3.81e-06, under one ulp of the result.
    residual_norm c = 2, n = 127, row scale: dgamma 8.33e-06 / 1.03e-06 on 24.0.  4.2e-06 of it came from one row whose two values differ
        by 2e-3 (variance 1.1e-06, under eps: rstd = 290 multiplies the rounding of the row's mean into xhat), 2.7e-06 is the rounding of
        the sum of 127 terms (1.4 ulp of 24).  The composite forms the same terms.
With the conditioned inputs every case is inside the bar on the first run; the seeds of the widths from four channels up are untouched.
Before chan_merge formed its results in double (csrc/batchnorm.hip), test_batch_norm_training_fp32[c8mis] at n = 7 gave dx 1.28e-06 /
2.43e-07: the Chan tree over seven one-row lanes rounded the mean three times a level; now 4.8e-07.
Every test prints its figures.
"""
import numpy as np
import pytest
import torch

from tests import batchnorm_oracle as BO
from tests import row_lanes_cases as L
from tests import rownorm_oracle as RO
from tests import rownorm_stream_oracle as SO
from tests import test_batchnorm_hip as BN
from tests import test_rownorm_hip as RN
from tests import test_rownorm_stream_hip as RS
from tests import test_syncbn_hip as SB

pytestmark = pytest.mark.gpu

IDS = [L.width_id(w) for w in L.WIDTHS]
TYPED = [(t, c, m) for t in ("f16", "bf16") for c, m in L.TYPE_CASES[t]]
TYPED_IDS = [f"{t}-{L.width_id((c, m))}" for t, c, m in TYPED]
INSTANCES = list(L.INSTANCE_WIDTHS.values())
RN_ARGS = ("x", "y", "s", "gamma", "beta", "go", "gz")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _tag(c, misaligned, rows="f32"):
    s = L.shape_of(c, misaligned, rows)
    return s, f"({s.vec},{s.iter}) seg={s.seg} c={c}{' misaligned' if misaligned else ''}"


def _loss_like(p):
    """dO of the rownorm cases as tests/test_batchnorm_hip.py makes it and for that file's reason: N(0, 1) plus a mean of 0.25 and a 0.25
    share of x's own deviation in its row.  With the zero-mean dO of tests/test_rownorm_hip.py, dgamma and dbeta are sums that cancel (c = 2,
    n = 129: dbeta = 2.08 and -0.13 from |terms| adding to 100) while the rounding of their partial sums does not, so the bar's
    u * max|want| scales with nothing, and at the one, two or three channels of the narrow widths there is no maximum over channels to
    even the two noises out: that case gave 9.7e-07 fused / 1.4e-07 composite, and 1.2e-06 for numpy's own fp32 sum."""
    x = p["x"].float()
    p["go"] = (p["go"].float() + 0.25 + 0.25 * (x - x.mean(1, keepdim=True))).to(p["go"].dtype)
    return p


NARROW = 4                                                                     # widths below it: dgamma and dbeta have one, two or three entries
MANTISSA = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}


def _off_grid(v, dtype):
    """every non-zero value of the float64 array v lies at least an eighth of an ulp from the values `dtype` holds - or is one of them to
    the last bit of float64: a sum that is exact in every precision and every order (dbeta of a bf16 dO), 0 / 0 on the two sides"""
    v = np.asarray(v, np.float64).ravel()
    v = v[np.isfinite(v) & (v != 0)]
    near = torch.from_numpy(v).to(dtype).double().numpy()
    v, near = v[near != 0], near[near != 0]
    ulp = 2.0 ** (np.floor(np.log2(np.abs(near))) - MANTISSA[dtype])
    return bool(((v == near) | (np.abs(v - near) >= ulp / 8)).all())


def _spread(p):
    """rows of two or three channels whose values nearly coincide: where the float64 variance of z is below 1/16, x[:, 0] moves by 1 (as
    _settle moves x off a kink).  rstd multiplies the rounding of the row's mean - half an ulp of the mean, not of z - mean - into xhat, by
    up to 316 where the variance falls under eps, on both sides alike; nothing in the bar scales with it.  From 1/16 on it is at most 4."""
    if not 1 < p["x"].shape[1] < NARROW:
        return p
    for _ in range(20):
        z = RN._f64(p["x"]) + (0.0 if p["y"] is None else RN._f64(p["y"]) * (1.0 if p["s"] is None else RN._f64(p["s"])[:, None]))
        bad = z.var(1) < 1.0 / 16
        if not bad.any():
            return p
        p["x"][:, 0] = (p["x"][:, 0].float() + torch.from_numpy(bad).float()).to(p["x"].dtype)
    raise AssertionError("the rows did not spread")


def _conditioned(c, seed, build, results):
    """build(seed), or for a narrow width the first of build(seed), build(seed + 1009), ... at which every result tensor of fewer than four
    entries is _off_grid in float64 - a choice made from the oracle alone, before anything runs on the device.  The bar allows
    4 * err(composite) + u * max|want|, and u * max|want| is between half an ulp and one ulp of the largest result.  Where float64's value
    lies on an fp32 value the composite can return exactly that, and the bar is then under one ulp of a sum of n rounded terms, which no
    order of fp32 additions promises (c = 1, n = 255: float64's dgamma 6e-09 from an fp32 value, torch on it, the kernel's balanced
    tree on its neighbour).  With four entries or more a tensor's worst entry evens this out, as tests/test_batchnorm_hip.py notes for
    C = 1.  An eighth of an ulp off the grid, either side's error is at least that, and the bar at least one ulp."""
    if c >= NARROW:
        return build(seed)
    for k in range(2000):
        p = build(seed + 1009 * k)
        if all(_off_grid(v, dt) for v, dt in results(p) if v is not None and 0 < np.size(v) < NARROW):
            return p
    raise AssertionError("no seed keeps the narrow results off the grid")


def _rownorm_results(p, want):
    f32 = torch.float32
    return [(want["o"], p["odt"]), (want["dx"], p["x"].dtype), (want["dy"], None if p["y"] is None else p["y"].dtype), (want["dgamma"], f32), (want["dbeta"], f32)]


def _bn_results(p, mode=None):
    want, f32 = BN._oracle(p, mode or BN._mode()), torch.float32
    return [(want["o"], p["x"].dtype), (want["dx"], p["x"].dtype)] + [(want[k], f32) for k in ("dgamma", "dbeta", "running_mean", "running_var")]


def _hold(failed, label, check):
    """run one case of a test that loops over row counts; the test fails at its end, so that its output holds every case's figures"""
    try:
        check()
    except AssertionError:
        failed.append(label)


def _same(t, first):
    """every slice of t along `first`'s broadcast carries first's bits"""
    return torch.equal(t, first.expand_as(t))


# ---- a. against the oracle over the whole table ----
@pytest.mark.parametrize("w", L.WIDTHS, ids=IDS)
def test_residual_norm_fp32(P, w):
    (s, tag), failed = _tag(w.c, w.misaligned), []
    for n in L.row_counts(s):
        for with_s in (True, False):
            build = lambda seed: _loss_like(_spread(RN._inputs(n, w.c, "f32", "f32", with_s, seed=seed, misaligned=w.misaligned)))
            p = _conditioned(w.c, w.c + n, build, lambda q: _rownorm_results(q, RO.residual_norm(*(RN._f64(q[k]) for k in RN_ARGS))))
            label = f"fp32 {tag} n={n} s={'mask' if with_s else 'None'}"
            _hold(failed, label, lambda: RN._check(P, p, label, "f32", "f32"))
    assert not failed, failed


@pytest.mark.parametrize("tname,c,misaligned", TYPED, ids=TYPED_IDS)
def test_residual_norm_half_stream(P, tname, c, misaligned):
    """(y, o) in the stream's type with a row scale, and in f32 without"""
    (s, tag), failed = _tag(c, misaligned, tname), []
    for n in L.row_counts(s):
        for with_s, yo in ((True, tname), (False, "f32")):
            build = lambda seed: _loss_like(_spread(RS._inputs(n, c, tname, yo, yo, with_s, seed=seed, misaligned=misaligned)))
            p = _conditioned(c, c + n, build, lambda q: _rownorm_results(q, SO.residual_norm_stream(
                RS._f32(q["x"]), RS._f32(q["y"]), RS._f32(q["s"]), RS._f64(q["gamma"]), RS._f64(q["beta"]), RS._f64(q["go"]), RS._f64(q["gz"]), tname)))
            label = f"{tname} y,o={yo} {tag} n={n} s={'mask' if with_s else 'None'}"
            _hold(failed, label, lambda: RS._check(P, p, label, yo, yo))
    assert not failed, failed


@pytest.mark.parametrize("w", L.WIDTHS, ids=IDS)
def test_batch_norm_training_fp32(P, w):
    (s, tag), failed = _tag(w.c, w.misaligned), []
    for n in L.row_counts(s, training=True):
        p = _conditioned(w.c, w.c + n, lambda seed: BN._inputs(n, w.c, "f32", "f32", "leaky_relu", seed=seed, misaligned=w.misaligned), _bn_results)
        label = f"fp32 {tag} n={n} leaky_relu residual=f32"
        _hold(failed, label, lambda: BN._check(P, p, label))
    assert not failed, failed


@pytest.mark.parametrize("c,misaligned", INSTANCES, ids=[L.width_id(k) for k in INSTANCES])
def test_batch_norm_eval_fp32(P, c, misaligned):
    """the running statistics normalise: Channels' scale_is_var branch, once per instance"""
    s, tag = _tag(c, misaligned)
    mode, n = BN._mode(training=False), L.big_count(s)
    p = BN._inputs(n, c, "f32", "f32", "relu", seed=c + n + 2, mode=mode, misaligned=misaligned)
    BN._check(P, p, f"eval fp32 {tag} n={n} relu residual=f32", mode)


@pytest.mark.parametrize("tname,c,misaligned", TYPED, ids=TYPED_IDS)
def test_batch_norm_half_rows(P, tname, c, misaligned):
    """the residual in fp32 and in the rows' own type; a misaligned half view is 2 bytes off the 8-byte chunk"""
    (s, tag), failed = _tag(c, misaligned, tname), []
    for n in L.row_counts(s, training=True):
        for rname in ("f32", tname):
            p = _conditioned(c, c + n + 1, lambda seed: BN._inputs(n, c, tname, rname, "leaky_relu", seed=seed, misaligned=misaligned), _bn_results)
            label = f"{tname} {tag} n={n} leaky_relu residual={rname}"
            _hold(failed, label, lambda: BN._check(P, p, label))
    assert not failed, failed


# ---- b. the sync launchers, once per instance ----
@pytest.mark.parametrize("c,misaligned", INSTANCES, ids=[L.width_id(k) for k in INSTANCES])
def test_sync_launchers_per_instance(P, c, misaligned):
    """two emulated ranks of rows_per_wg + 1 and per_wave rows: bn_row_kernel, bn_merge_kernel and the SYNC dx pass at this instance"""
    s, tag = _tag(c, misaligned)
    sizes = (s.rows_per_wg + 1, s.per_wave)
    print(f"sync launchers {tag} ranks={sizes}")
    SB._check(P, sizes, c, rname="f32", misaligned=misaligned)


# ---- c. replicated column, exact ----
def _replicate_columns(p):
    c = p["x"].shape[1]
    for k in ("x", "go", "res"):
        p[k] = p[k][:, :1].expand(-1, c).contiguous()
    for k in ("gamma", "beta", "rm", "rv"):
        p[k] = p[k][:1].expand(c).contiguous()
    return p


@pytest.mark.parametrize("w", L.WIDTHS, ids=IDS)
def test_replicated_column_batch_norm(P, w):
    for xname in ("f32", "f16"):
        s, tag = _tag(w.c, w.misaligned, xname)
        n = L.big_count(s)
        for training in (True, False):
            mode = BN._mode(training=training)
            p = _replicate_columns(BN._inputs(n, w.c, xname, "f32", "leaky_relu", seed=w.c + 5, mode=mode, misaligned=w.misaligned))
            got = BN._fused(P, p, mode)
            off = []
            for name in ("o", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
                b = BN._bits(got[name])
                assert bool(torch.isfinite(got[name].float()).all()), name
                if not _same(b, b[..., :1]):
                    off.append(name)
            print(f"replicated column {xname} {tag} n={n} training={training}: " + ("every channel carries channel 0's bits" if not off else f"DIFFER: {off}"))
            assert not off, (xname, training, off)


# ---- d. replicated row, exact ----
def _replicate_rows(p, n, keep):
    for k in ("x", "y", "go", "gz"):
        p[k] = p[k][:1].expand(n, -1).contiguous()
    p["mask"], p["s"] = torch.ones(n), torch.full((n,), 1.0 / keep)
    return p


def _stat_rows(p, n):
    """stat [n, 2] of the forward, read through the binding"""
    from stratified_transformer_amd import pointops2_cuda as C
    mis, c = p["misaligned"], p["x"].shape[1]
    x, y = RS._to(p["x"], mis), RS._to(p["y"], mis)
    z, o, stat = RS._to(torch.empty_like(p["x"]), mis), RS._to(torch.empty(n, c, dtype=p["odt"]), mis), torch.empty(n, 2, device="cuda")
    C.residual_norm_stream_forward(n, c, x, y, p["s"].cuda(), p["gamma"].cuda(), p["beta"].cuda(), 1e-5, z, o, stat)
    torch.cuda.synchronize()
    return stat


def _replicated_rows(P, make, fused, c, misaligned, rows, label):
    s, tag = _tag(c, misaligned, rows)
    alone = _replicate_rows(make(1), 1, RN.KEEP)
    one, stat1 = fused(P, alone), _stat_rows(alone, 1)
    for n in (s.per_wave + 1, L.big_count(s)):                                 # the last wave: one live row beside per_wave - 1 dead ones
        p = _replicate_rows(make(1), n, RN.KEEP)
        got, stat = fused(P, p), _stat_rows(p, n)
        off = [name for name in ("z", "o", "dx", "dy") if not _same(RN._bits(got[name]), RN._bits(one[name]))]
        if not _same(RN._bits(stat), RN._bits(stat1)):
            off.append("stat")
        print(f"replicated row {label} {tag} n={n}: " + ("every row carries the bits of the row run alone" if not off else f"DIFFER: {off}"))
        assert not off, (n, off)
        assert bool(torch.isfinite(got["o"].float()).all() and torch.isfinite(got["dx"].float()).all())


@pytest.mark.parametrize("w", L.WIDTHS, ids=IDS)
def test_replicated_row_residual_norm(P, w):
    make = lambda n: RN._inputs(n, w.c, "f32", "f32", True, seed=w.c + 7, misaligned=w.misaligned)
    _replicated_rows(P, make, RN._fused, w.c, w.misaligned, "f32", "fp32")


@pytest.mark.parametrize("tname,c,misaligned", TYPED, ids=TYPED_IDS)
def test_replicated_row_half_stream(P, tname, c, misaligned):
    make = lambda n: RS._inputs(n, c, tname, tname, tname, True, seed=c + 7, misaligned=misaligned)
    _replicated_rows(P, make, RS._fused, c, misaligned, tname, tname)


# ---- e. poison stays put, at every segment width ----
def _clone(p):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}


def _poisoned_rows(P, p, want_of, fused, s, label):
    """a NaN in the last channel of the row at the last slot of the first wave, a +Inf in channel 0 of the first row of the second wave"""
    n, c = p["x"].shape
    clean = _clone(p)
    bad = [s.per_wave - 1, s.per_wave]
    p["y"][bad[0], c - 1] = float("nan")
    p["x"][bad[1], 0] = float("inf")
    want, got, ref = want_of(p), fused(P, p), fused(P, clean)
    rows = [r for r in range(n) if r not in bad]
    for name in ("z", "o", "dx", "dy"):
        g = RN._f64(got[name])
        assert np.array_equal(np.isfinite(g), np.isfinite(want[name])), name                # the oracle's set of non-finite entries
        assert np.array_equal(np.isnan(g), np.isnan(want[name])), name
        assert not np.isfinite(want[name][bad]).all() and np.isfinite(want[name][rows]).all(), name
        assert torch.equal(RN._bits(got[name][rows]), RN._bits(ref[name][rows])), name      # the other rows: as without the poison
    for name in ("dgamma", "dbeta"):
        assert np.array_equal(np.isfinite(RN._f64(got[name])), np.isfinite(want[name])), name
        assert np.array_equal(np.isnan(RN._f64(got[name])), np.isnan(want[name])), name
    print(f"poisoned rows {label} n={n}: rows {bad} hold the oracle's {int((~np.isfinite(want['o'])).sum())} non-finite o, "
          f"the other {len(rows)} rows keep their bits")


@pytest.mark.parametrize("w", L.WIDTHS, ids=IDS)
def test_poisoned_rows_residual_norm(P, w):
    s, tag = _tag(w.c, w.misaligned)
    p = RN._inputs(s.rows_per_wg + 1, w.c, "f32", "f32", False, seed=w.c + 21, misaligned=w.misaligned)
    want_of = lambda q: RO.residual_norm(*(RN._f64(q[k]) for k in ("x", "y", "s", "gamma", "beta", "go", "gz")))
    _poisoned_rows(P, p, want_of, RN._fused, s, f"fp32 {tag}")


@pytest.mark.parametrize("c,misaligned", L.TYPE_CASES["f16"], ids=[L.width_id(k) for k in L.TYPE_CASES["f16"]])
def test_poisoned_rows_half_stream(P, c, misaligned):
    s, tag = _tag(c, misaligned, "f16")
    p = RS._inputs(s.rows_per_wg + 1, c, "f16", "f16", "f16", False, seed=c + 21, misaligned=misaligned)
    want_of = lambda q: SO.residual_norm_stream(RS._f32(q["x"]), RS._f32(q["y"]), None, RS._f64(q["gamma"]), RS._f64(q["beta"]), RS._f64(q["go"]),
                                                RS._f64(q["gz"]), "f16")
    _poisoned_rows(P, p, want_of, RS._fused, s, f"f16 {tag}")


@pytest.mark.parametrize("w", L.WIDTHS, ids=IDS)
def test_poisoned_channels_batch_norm(P, w):
    """a NaN in channel c - 1 - the last live lane, beside the idle ones of a partial segment - and a +Inf in channel 0 (c == 1: the NaN
    alone); the three channels that share a chunk with either keep their bits too"""
    s, tag = _tag(w.c, w.misaligned)
    n, c, mode = L.big_count(s), w.c, BN._mode()
    p = BN._inputs(n, c, "f32", None, "leaky_relu", seed=c + 21, misaligned=w.misaligned)
    clean = _clone(p)
    p["x"][n // 2, c - 1] = float("nan")
    bad = [c - 1]
    if c > 1:
        p["x"][s.per_wave, 0] = float("inf")
        bad.append(0)
    want, got, ref = BN._oracle(p, mode), BN._fused(P, p, mode), BN._fused(P, clean, mode)
    cols = [k for k in range(c) if k not in bad]
    for name in ("o", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
        g, wn = BN._f64(got[name]), want[name]
        assert np.array_equal(np.isfinite(g), np.isfinite(wn)), name                         # the oracle's set of non-finite entries
        assert np.isfinite(wn[..., cols]).all(), name
        if name != "dbeta":                                                                 # (leaky_relu's derivative of a NaN is its slope: dbeta stays finite)
            assert not np.isfinite(wn[..., bad]).any(), name
        assert torch.equal(BN._bits(got[name][..., cols]), BN._bits(ref[name][..., cols])), name   # the other channels: as without the poison
    print(f"poisoned channels fp32 {tag} n={n}: channels {bad} hold the oracle's non-finite entries, the other {len(cols)} keep their bits")


# ---- f. column_reduce at 63, 64 and 65 rows of partials ----
@pytest.mark.parametrize("k", [0, 1, 2], ids=["63 rows", "64 rows", "65 rows"])
def test_column_reduce_around_its_groups(P, k):
    c = 48
    n, shape = L.partial_row_counts(c)[k], L.shape_of(c, False)
    rows = L.partial_rows(n, shape)
    assert rows == L.RED_GROUPS - 1 + k
    p = _loss_like(RN._inputs(n, c, "f32", "f32", True, seed=c + n))
    a = RN._check(P, p, f"fp32 c={c} n={n} ({rows} rows of partials) s=mask", "f32", "f32")
    b = RN._fused(P, p)
    for name in a:
        assert torch.equal(RN._bits(a[name]), RN._bits(b[name])), name
    p = BN._inputs(n, c, "f32", "f32", "leaky_relu", seed=c + n)
    a = BN._check(P, p, f"fp32 c={c} n={n} ({rows} rows of partials) leaky_relu residual=f32")
    b = BN._fused(P, p, BN._mode())
    for name in a:
        assert torch.equal(BN._bits(a[name]), BN._bits(b[name])), name


@pytest.mark.parametrize("rows", [1, 2])
def test_statistics_from_one_and_two_rows_of_partials(P, rows):
    """batch_norm_act_stats through the binding with `rows` rows of partials at n = 1000, c = 48: one or two workgroups, every wave takes
    sixteen or eight turns of its row loop, so the shift K of a channel is chosen in the first and kept.  Column 1 holds 1e3 + N(0, 1).
    mean and rstd under the standing bar against torch's var_mean on the GPU, the variance read back from rstd under test_hard_columns' bar."""
    from stratified_transformer_amd import pointops2_cuda as C
    n, c = 1000, 48
    p = BN._inputs(n, c, "f32", None, "none", seed=rows)
    p["x"][:, 1] = 1e3 + torch.randn(n, generator=torch.Generator().manual_seed(1))
    x = p["x"].cuda()
    stat = torch.empty(2, c, device="cuda")
    C.batch_norm_act_stats(n, c, x, torch.empty(rows, 3, c, device="cuda"), 1e-5, 0.0, None, None, stat)
    var_c, mean_c = torch.var_mean(x, 0, unbiased=False)
    torch.cuda.synchronize()
    want = BO.batch_norm_act(BN._f64(p["x"]), BN._f64(p["gamma"]), BN._f64(p["beta"]))
    figures, ok = [], True
    for name, g, comp in (("mean", stat[0], mean_c), ("rstd", stat[1], 1.0 / torch.sqrt(var_c + 1e-5))):
        e_f, e_c = (float(np.abs(BN._f64(t) - want[name]).max()) for t in (g, comp))
        top = float(np.abs(want[name]).max())
        figures.append(f"{name} {e_f:.2e}/{e_c:.2e}")
        ok = ok and e_f <= 4 * e_c + BN.U[torch.float32] * top
    var = 1.0 / BN._f64(stat[1]) ** 2 - 1e-5
    v_err = float(np.abs(var - BN._f64(p["x"]).var(0)).max())
    print(f"batch_norm_act_stats {rows} row(s) of partials n={n} c={c}: " + "  ".join(figures) + f"  variance {v_err:.2e} (column 1: {var[1]:.6f} for "
          f"{float(BN._f64(p['x'][:, 1]).var()):.6f})" + ("" if ok else "   <-- over the bar"))
    assert ok and v_err <= 1e-3
