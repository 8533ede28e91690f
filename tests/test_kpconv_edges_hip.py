"""GPU (-m gpu): the KPConv aggregation kernels (csrc/kpconv.hip) at their limits and staging edges: the cases of
tests/kpconv_cases.py through the C-ABI launchers kpconv_aggregate_{forward,backward}_launcher into NaN-filled (forward) and zeroed
(backward) buffers, every element against the float64 reference within the bound derived in DESIGN.md ("KPConv aggregation: cases
and bounds"), exact zeros and bit-exact expectations where the case promises them; the integer and non-finite cases through
pointops.kpconv as well, at the bars of tests/test_kpconv_hip.py (the matrix products sit there).
tests/test_kpconv_cases_cpu.py proves that a plain fp32 evaluation meets the bounds and that wrong variants miss them.  Each test
prints the largest fraction of its bound (`fraction kpconv_fwd <case> <value>`).

Measured on one MI355X, fraction of the bound used, forward / backward (a plain fp32 numpy evaluation uses 0.44 / 0.29):

    c-sweep (worst of c = 1..64)  0.356 / 0.176      nvalid        0.241 / 0.078      past-cap-256   0.441 / 0.016
    kp1-nb1   0.201 / 0.131   kp1-nb2   0.139 / 0.138   kp1-nb63   0.252 / 0.143   kp1-nb64   0.136 / 0.119
    kp2-nb1   0.154 / 0.146   kp2-nb2   0.200 / 0.157   kp2-nb63   0.182 / 0.211   kp2-nb64   0.181 / 0.085
    kp15-nb1  0.216 / 0.091   kp15-nb2  0.277 / 0.138   kp15-nb63  0.203 / 0.054   kp15-nb64  0.190 / 0.028
    kp16-nb1  0.191 / 0.058   kp16-nb2  0.263 / 0.146   kp16-nb63  0.209 / 0.069   kp16-nb64  0.249 / 0.055
    kp31-nb1  0.247 / 0.134   kp31-nb2  0.318 / 0.110   kp31-nb63  0.277 / 0.034   kp31-nb64  0.329 / 0.062
    kp32-nb1  0.302 / 0.063   kp32-nb2  0.287 / 0.107   kp32-nb63  0.244 / 0.029   kp32-nb64  0.270 / 0.015
    lds-small (45 632 B) 0.227 / 0.146   lds-max (103 296 B) 0.215 / 0.115   lds-mid (53 568 B) 0.242 / 0.164
    lds-large (85 440 B) 0.179 / 0.133   nq1 0.127 / 0.147   nq3 0.144 / 0.165   nq4 0.190 / 0.160   nq5 0.201 / 0.286
    ns1 0.252 / 0.015   ns0 0 / 0   exact 0.046 / 0.039   off-origin 0.276 / 0.079   dup-row 0.191 / 0.090
    one-row 0.205 / 0.007   plain 0.278 / 0.112 (permuted: the same)   exact-nonfinite 0.046 / 0.039   nonfinite-xyz 0.334 / 0.171

Before the clamp in stage_query was changed from fmaxf to a comparison, nonfinite-xyz gave no NaN at all where the reference has
300 of 2400 (forward); every other case passed unchanged.  The figures tests/test_kpconv_hip.py quotes for the fp32 torch
evaluation, measured for pointops.kpconv itself on its 21 000-point scene (max absolute error against the float64 oracle):
forward 1.6e-6 / 2.4e-6 / 6.8e-6 on values <= 5.1 / 6.0 / 13.4, grad x 4.5e-6 / 3.6e-6 / 3.0e-6 on values <= 17, grad weight
1.0e-3 / 1.2e-3 / 4.4e-4 on values <= 437 / 511 / 418 (2.4e-6 / 2.3e-6 / 1.1e-6 of the scale), for (3 -> 48) / (6 -> 48) / (12 -> 12).
"""
import numpy as np
import pytest
import torch

from tests import kpconv_cases as C

pytestmark = pytest.mark.gpu

FTOL = dict(rtol=2e-5, atol=1e-4)   # tests/test_kpconv_hip.py: the operator's bars
GTOL = dict(rtol=2e-5, atol=2e-4)
TTOL = dict(rtol=2e-4, atol=2e-4)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def L():
    from stratified_transformer_amd import pointops2_cuda
    return pointops2_cuda


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _dev(a, odd=False, fill=None, shape=None):
    """a on the device; odd: a view that starts one element into its storage (4 bytes off every wider alignment)"""
    if a is not None:
        t = torch.from_numpy(np.array(a))  # a copy: the cases are read-only
        shape = t.shape
    else:
        t = torch.full(tuple(shape), fill, dtype=torch.float32)
    if not odd:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + t.element_size()
    return view


def _run(L, case, odd=False):
    """both launchers -> (wf [n_q, n_kp, c], grad_feat [n_s, c]) as numpy"""
    c = case
    assert c.nb.dtype == np.int32
    q, s, nb, x, kp, g = (_dev(a, odd) for a in (c.query, c.support, c.nb, c.x, c.kp, c.g))
    wf = _dev(None, odd, float("nan"), (c.n_q, c.n_kp, c.c))
    gf = _dev(None, odd, 0.0, (c.n_s, c.c))
    L.kpconv_aggregate_forward(c.n_q, c.n_s, c.n_nb, c.c, c.n_kp, q, s, nb, x, kp, c.extent, wf)
    L.kpconv_aggregate_backward(c.n_q, c.n_s, c.n_nb, c.c, c.n_kp, q, s, nb, kp, c.extent, g, gf)
    torch.cuda.synchronize()
    return wf.cpu().numpy(), gf.cpu().numpy()


def _check(L, case, odd=False, quiet=False):
    wf, gf = _run(L, case, odd)
    f, b = C.check_forward(wf, case), C.check_backward(gf, case)
    if not quiet:
        print(f"fraction kpconv_fwd {case.name} {f:.4f}")
        print(f"fraction kpconv_bwd {case.name} {b:.4f}")
    return wf, gf, f, b


# ---------------------------------------------------------------------------------------------------------------------
# the launchers
# ---------------------------------------------------------------------------------------------------------------------
def test_divisor_sweep_over_c(L):
    """c = 1..64 at n_nb = 64, n_kp = 32: every divisor c of small_div with t up to 64 c - 1 and 32 c - 1 (c >= 33 also runs the
    big-LDS opt-in, c = 64 at the maximum)"""
    worst_f = worst_b = 0.0
    for c in range(1, 65):
        _, _, f, b = _check(L, C.c_sweep_case(c), quiet=True)
        worst_f, worst_b = max(worst_f, f), max(worst_b, b)
    print(f"fraction kpconv_fwd c-sweep {worst_f:.4f}")
    print(f"fraction kpconv_bwd c-sweep {worst_b:.4f}")


def test_divisor_sweep_over_n_valid(L):
    """every valid count 0..64 at scattered positions, padding -1 / n_s / INT_MAX / INT_MIN"""
    _check(L, C.n_valid_sweep_case())


@pytest.mark.parametrize("shape", C.EDGE_SHAPES, ids=lambda s: "kp%d-nb%d" % s)
def test_kernel_point_and_neighbour_count_edges(L, shape):
    _check(L, C.edge_case(*shape))


def test_lds_sizes_in_one_process(L):
    """below 48 KiB, the maximum, below again, between 48 and 64 KiB, above 64 KiB: an attribute set for one launch does not
    break the next"""
    for which in C.LDS_ORDER:
        case = C.lds_case(which)
        print(f"lds {which} {case.lds} B")
        _check(L, case)


@pytest.mark.parametrize("n_q", C.QUERY_COUNTS)
def test_query_counts_around_one_workgroup(L, n_q):
    _check(L, C.query_count_case(n_q))


def test_one_launch_past_the_persistent_grid(L):
    """n_q = 64 * CUs + 3: three waves take a second query and stage it over the first one's LDS (full -> empty, full -> one
    neighbour, one -> full)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = C.past_cap_case(cus)
    cap = case.marks["cap"]
    assert case.n_q == 64 * cus + 3
    wf, _, _, _ = _check(L, case)
    assert not wf[cap].any()  # the empty row after a full one: nothing of the full row's staging left


def test_single_and_empty_support(L):
    _check(L, C.single_support_case())
    case = C.empty_support_case()
    wf, gf, _, _ = _check(L, case)
    assert wf.shape == (case.n_q, case.n_kp, case.c) and not wf.any() and not np.signbit(wf).any() and gf.shape == (0, case.c)


def test_exact_geometry(L):
    """a neighbour on K[k]: the feature row bit for bit; at the extent and at twice the extent: +0"""
    case = C.exact_case()
    wf, _, _, _ = _check(L, case)
    C.check_exact_geometry(wf, case)


def test_off_origin_scene(L):
    _check(L, C.off_origin_case())


def test_duplicate_indices(L):
    """one index through a whole row (the atomics of one wave collide), and every slot of every query on support row 0"""
    _check(L, C.duplicate_row_case())
    _check(L, C.one_support_row_case())


def test_misaligned_operands(L):
    """every pointer argument one float into its storage; the forward is the aligned launch's bit for bit"""
    case = C.plain_case()
    wf, _, _, _ = _check(L, case)
    wf_odd, _, _, _ = _check(L, case, odd=True, quiet=True)
    assert np.array_equal(wf.view(np.int32), wf_odd.view(np.int32))


def test_permuted_queries_give_the_same_rows(L):
    """the same queries in another row order (other waves, other workgroups): the same output rows bit for bit"""
    case = C.plain_case()
    perm = np.random.default_rng(1).permutation(case.n_q)
    assert (perm != np.arange(case.n_q)).mean() > 0.9
    wf, _ = _run(L, case)
    moved = case.replace(name="plain-permuted", query=case.query[perm], nb=case.nb[perm], g=case.g[perm])
    wf_p, _, _, _ = _check(L, moved)
    assert np.array_equal(wf_p.view(np.int32), wf[perm].view(np.int32))


def test_nonfinite_feature_rows(L):
    """NaN / +-Inf rows reached with weight 1, with weight exactly 0 (0 * Inf = NaN) and only by padding (never read): the
    NaN pattern and the signs of the infinities are the reference's, everything else is inside its bound"""
    case = C.exact_case(nonfinite=True)
    wf, gf, _, _ = _check(L, case)
    C.check_exact_geometry(wf, case)
    assert np.isfinite(gf).all()  # the backward reads no feature row


def test_nonfinite_coordinates(L):
    """torch.clamp(min=0) keeps a NaN influence; Inf - Inf is NaN; a finite point infinitely far away weighs exactly 0"""
    _check(L, C.nonfinite_coordinate_case())


# ---------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------
def _same_pattern_and_close(got, want, what, scale=False, **tol):
    got, want = np.asarray(got, np.float64), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and np.array_equal(np.isinf(got), inf), f"{what}: infinities"
    fin = np.isfinite(want)
    s = max(1.0, float(np.abs(want[fin]).max())) if scale and fin.any() else 1.0
    np.testing.assert_allclose(got[fin] / s, want[fin] / s, err_msg=what, **tol)


def _check_operator(P, case, nb=None, out=8):
    """pointops.kpconv forward and backward against the float64 reference times a weight [n_kp, c, out]"""
    from stratified_transformer_amd import _lib
    rng = np.random.default_rng(case.n_q + case.c)
    weight = rng.standard_normal((case.n_kp, case.c, out), dtype=np.float32)
    go = rng.standard_normal((case.n_q, out), dtype=np.float32)
    w2 = weight.astype(np.float64).reshape(case.n_kp * case.c, out)
    # the reference's grad_wf: grad_out @ weight^T (fp32 on the device: its rounding is far inside the bars)
    ref = case.replace(g=(go.astype(np.float64) @ w2.T).reshape(case.n_q, case.n_kp, case.c)).reference()
    xg, wg = _dev(case.x).requires_grad_(True), _dev(weight).requires_grad_(True)
    got = P.kpconv(_dev(case.query), _dev(case.support), _dev(case.nb if nb is None else nb), xg, _dev(case.kp), wg, case.extent)
    assert got.dtype == torch.float32 and tuple(got.shape) == (case.n_q, out)
    before = _lib.CALLS[0]
    got.backward(_dev(go))
    torch.cuda.synchronize()
    launches = _lib.CALLS[0] - before
    with np.errstate(invalid="ignore", over="ignore"):
        wf2 = ref.wf.reshape(case.n_q, case.n_kp * case.c)
        want, want_gw = wf2 @ w2, (wf2.T @ go.astype(np.float64)).reshape(case.n_kp, case.c, out)
    _same_pattern_and_close(got.detach().cpu().numpy(), want, f"{case.name} forward", **FTOL)
    _same_pattern_and_close(xg.grad.cpu().numpy(), ref.gf, f"{case.name} grad x", **GTOL)
    _same_pattern_and_close(wg.grad.cpu().numpy(), want_gw, f"{case.name} grad weight", scale=True, **TTOL)
    return got.detach(), launches


def test_operator_int64_and_out_of_int32_padding(P):
    """int64 neighbours whose padding lies beyond int32 with valid-looking low words: skipped, as the int32 padding is"""
    case = C.plain_case()
    got32, _ = _check_operator(P, case)
    got64, _ = _check_operator(P, case, nb=case.nb.astype(np.int64))
    far, _ = _check_operator(P, case, nb=C.out_of_int32_neighbours(case))
    assert torch.equal(got64, got32) and torch.equal(far, got32)


def test_operator_nonfinite_cases(P):
    _check_operator(P, C.exact_case(nonfinite=True))
    _check_operator(P, C.nonfinite_coordinate_case())


def test_operator_empty_support(P):
    """n_s = 0 with n_q > 0: the forward is all zeros, the backward makes no launch"""
    got, launches = _check_operator(P, C.empty_support_case())
    assert not got.cpu().numpy().any() and launches == 0
