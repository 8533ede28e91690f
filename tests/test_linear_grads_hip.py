"""GPU (-m gpu): the Linear parameter gradients on csrc/linear_grads.hip - pointops.linear_param_grads, pointops.linear_rows and the
nn.Linear forwards of layers.fuse_linear_grads - on the cases of tests/linear_grads_cases.py against tests/linear_grads_oracle.py.

Bars.
  integer-valued operands:   grad_weight and grad_bias equal the integer reference bit for bit (every order of summation is exact there)
  random operands:           |. - float64| <= gamma_N * sum |g x|  (sum |g| for the bias) per element, gamma_N = N u / (1 - N u), u = 2^-24:
                             the bound of ANY order of N fp32 multiply-adds, independent of the chunking
  two runs, other addresses: the same bits
  inf / NaN operands:        the float64 reference's set of non-finite elements, every other element within its bound
  the layers:                the forward bit for bit torch's; weight.grad / bias.grad fp32 and within the bound above, computed from the
                             operands as the GEMM saw them (x and weight after autocast's cast, the incoming gradient as it arrived);
                             x.grad - torch's own GEMM on either side - within (gamma_out (1 + u_s) + u_s) * sum |g w|, where u_s is the
                             unit roundoff of the type the GEMM stores its fp32 sums in: 0 in fp32 (the bar is gamma_out * sum |g w|),
                             2^-11 under autocast(f16), whose result no bound without that rounding could hold on either side
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import linear_grads_cases as C
from tests import linear_grads_oracle as O

pytestmark = pytest.mark.gpu
R = C.R
IDS = [C.case_id(c) for c in C.CASES]


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    return pointops


def _np(t):
    return t.detach().cpu().numpy()


def _run(P, idx, kind):
    c = C.CASES[idx]
    x, g = C.operands(idx, kind, "cuda")
    assert (x.is_contiguous() and g.is_contiguous()) == (c["view"] != "strided")
    dW, db = P.linear_param_grads(x, g, bias=c["bias"])
    assert dW.dtype == torch.float32 and tuple(dW.shape) == (c["out"], c["in"]) and dW.is_contiguous()
    assert (db is None) == (not c["bias"])
    if db is not None:
        assert db.dtype == torch.float32 and tuple(db.shape) == (c["out"],)
    return _np(dW), None if db is None else _np(db)


@pytest.mark.parametrize("idx", range(len(C.CASES)), ids=IDS)
def test_integer_operands_give_the_exact_sums_bit_for_bit(P, idx):
    dW, db = _run(P, idx, "int")
    want_W, want_b = C.expected(idx, "int")
    assert np.array_equal(dW.view(np.uint32), (want_W + 0.0).view(np.uint32)), f"{(dW != want_W).sum()} of {dW.size} elements differ"
    if db is not None:
        assert np.array_equal(db.view(np.uint32), (want_b + 0.0).view(np.uint32))


def _within(got, want, tol, what):
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max err {err.max(initial=0):.3e}, max err / bound {np.max(err / np.maximum(tol, 1e-300), initial=0):.3f}")
    assert (err <= tol).all(), f"{what}: {(err > tol).sum()} of {err.size} elements outside the bound, worst {np.max(err - tol):.3e} over it"


@pytest.mark.parametrize("idx", range(len(C.CASES)), ids=IDS)
def test_random_operands_stay_inside_the_bound_of_any_summation_order(P, idx):
    dW, db = _run(P, idx, "random")
    want = C.expected(idx, "random")
    _within(dW, want["dW"], want["tol_W"], "grad_weight")
    if db is not None:
        _within(db, want["db"], want["tol_b"], "grad_bias")


@pytest.mark.parametrize("idx", [i for i, c in enumerate(C.CASES) if c["n"] in (R + 1, 3 * R + 5) and c["view"] is None][::2] +
                         [i for i, c in enumerate(C.CASES) if (c["in"], c["out"]) == (384, 1536)][:1], ids=lambda i: IDS[i])
def test_two_runs_and_other_addresses_give_the_same_bits(P, idx):
    c = C.CASES[idx]
    x, g = C.operands(idx, "random", "cuda")
    first = P.linear_param_grads(x, g, bias=True)
    again = P.linear_param_grads(x, g, bias=True)
    pad = torch.full((12345 + 7 * idx,), 3.0, device="cuda")  # an unrelated allocation of another size: what follows lies elsewhere
    x2, g2 = x.clone(), g.clone()
    moved = P.linear_param_grads(x2, g2, bias=True)
    assert c["n"] == 0 or (x2.data_ptr() != x.data_ptr() and g2.data_ptr() != g.data_ptr())
    for a, b, m in zip(first, again, moved):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), m.view(torch.int32))
    del pad


@pytest.mark.parametrize("types", [(C.F32, C.F32), (C.F16, C.F16)], ids=["f32", "f16"])
def test_non_finite_operands_poison_exactly_the_references_elements(P, types):
    n, n_in, n_out = R + 1, 15, 17
    rng = np.random.default_rng(91)
    x = torch.from_numpy(rng.standard_normal((n, n_in)).astype(np.float32)).to(types[0])
    g = torch.from_numpy(rng.standard_normal((n, n_out)).astype(np.float32)).to(types[1])
    x[R, 3] = float("inf")  # row R is the tail chunk: one row, the other three rows of its MFMA step are padding
    g[R, 5] = float("nan")
    want = O.reference(O.widen(x), O.widen(g))
    assert np.isinf(want["dW"][:, 3]).sum() == n_out - 1 and np.isnan(want["dW"][5]).all() and np.isnan(want["db"][5])
    assert (~np.isfinite(want["dW"])).sum() == n_out + n_in - 1 and (~np.isfinite(want["db"])).sum() == 1
    dW, db = (_np(t) for t in P.linear_param_grads(x.cuda(), g.cuda()))
    for got, ref, tol, what in ((dW, want["dW"], want["tol_W"], "grad_weight"), (db, want["db"], want["tol_b"], "grad_bias")):
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN where the reference has none, or none where it has one"
        inf = np.isinf(ref)
        assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf].astype(np.float32))  # (and its sign)
        ok = np.isfinite(ref)
        _within(got[ok], ref[ok], tol[ok], what)


@pytest.mark.parametrize("n", [0, 1, R + 1])
def test_outputs_are_fully_written(P, n):
    """outputs and workspace pre-filled with NaN: none comes back on finite input - through the ABI wrappers, which take the caller's buffers"""
    from stratified_transformer_amd import pointops2_cuda as K
    n_in, n_out = 15, 17
    gen = torch.Generator().manual_seed(n)
    x, g = torch.randn((n, n_in), generator=gen).cuda(), torch.randn((n, n_out), generator=gen).cuda()
    rows = K.linear_grads_partial_rows(n, n_in, n_out)
    assert rows == max(1, -(-n // R))
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    partials, dW, db = nan(rows, n_out, n_in + 1), nan(n_out, n_in), nan(n_out)
    K.linear_grads_partial(n, n_in, n_out, x, g, partials)
    K.linear_grads_reduce(n_in, n_out, partials, dW, db)
    assert torch.isfinite(partials).all() and torch.isfinite(dW).all() and torch.isfinite(db).all()
    if n == 0:
        assert not dW.any() and not db.any()
    want = P.linear_param_grads(x, g)
    assert torch.equal(dW, want[0]) and torch.equal(db, want[1])
    dW2, untouched = nan(n_out, n_in), nan(n_out)
    K.linear_grads_reduce(n_in, n_out, partials, dW2, None)  # without a bias nothing but grad_weight is written
    assert torch.equal(dW2, dW) and torch.isnan(untouched).all()


def test_the_abi_with_caller_allocated_zero_filled_buffers(P):
    """the three entry points through _lib.call the way a C caller uses them; a `partials` of the wrong row count is an error and stays unwritten"""
    from stratified_transformer_amd import _lib
    idx = next(i for i, c in enumerate(C.CASES) if (c["n"], c["in"], c["out"]) == (3 * R + 5, 48, 192))
    c = C.CASES[idx]
    n, n_in, n_out = c["n"], c["in"], c["out"]
    x, g = C.operands(idx, "random", "cuda")
    rows = _lib.lib().pointops2_linear_grads_partial_rows(n, n_in, n_out)
    assert rows == 4
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    partials, dW, db = z(rows, n_out, n_in + 1), z(n_out, n_in), z(n_out)
    ptr, dev = _lib.ptr, x.device
    _lib.call("linear_grads_partial_launcher", n, n_in, n_out, 0, 0, ptr(x), ptr(g), ptr(partials), rows, device=dev)
    _lib.call("linear_grads_reduce_launcher", n_in, n_out, 1, ptr(partials), rows, ptr(dW), ptr(db), device=dev)
    want = P.linear_param_grads(x, g)
    assert torch.equal(dW, want[0]) and torch.equal(db, want[1])
    # the blocks are the chunks' own sums: block 3 holds the last five rows
    tail = O.reference(O.widen(x[3 * R:]), O.widen(g[3 * R:]))
    _within(_np(partials[3, :, :n_in]), tail["dW"], tail["tol_W"], "the last block")
    _within(_np(partials[3, :, n_in]), tail["db"], tail["tol_b"], "the last block's bias column")
    for wrong in (rows - 1, rows + 1):
        buf = z(max(rows, wrong), n_out, n_in + 1)
        with pytest.raises(RuntimeError, match="partial_rows"):
            _lib.call("linear_grads_partial_launcher", n, n_in, n_out, 0, 0, ptr(x), ptr(g), ptr(buf), wrong, device=dev)
        torch.cuda.synchronize()
        assert not buf.any()
    for bad in ((n, 0, n_out, 0, 0), (n, n_in, 1537, 0, 0), (n, n_in, n_out, 3, 0), (n, n_in, n_out, 0, -1), (-1, n_in, n_out, 0, 0)):
        buf = z(rows, n_out, n_in + 1)
        with pytest.raises(RuntimeError):
            _lib.call("linear_grads_partial_launcher", *bad, ptr(x), ptr(g), ptr(buf), rows, device=dev)
        assert not buf.any()
    with pytest.raises(RuntimeError):
        _lib.call("linear_grads_reduce_launcher", n_in, n_out, 1, ptr(partials), 0, ptr(dW), ptr(db), device=dev)
    with pytest.raises(RuntimeError):
        _lib.call("linear_grads_reduce_launcher", n_in, n_out, 1, ptr(partials), rows, ptr(dW), None, device=dev)


def test_the_operator_checks_its_operands(P):
    x, g = torch.zeros(4, 3, device="cuda"), torch.zeros(4, 5, device="cuda")
    with pytest.raises(ValueError):
        P.linear_param_grads(x, g[:3])
    with pytest.raises(ValueError):
        P.linear_param_grads(torch.zeros(4, 1537, device="cuda"), g)
    with pytest.raises(ValueError):
        P.linear_param_grads(x[0], g[0])
    with pytest.raises(TypeError):
        P.linear_param_grads(x.double(), g)
    with pytest.raises(TypeError):
        P.linear_param_grads(x, g.int())
    with pytest.raises(RuntimeError):
        P.linear_param_grads(x, g.cpu())
    dW, db = P.linear_param_grads(x.requires_grad_(True), g)
    assert not dW.requires_grad and not db.requires_grad


# ---- the autograd function and the layer hook ----
def _model(kind, bias):
    torch.manual_seed(11)
    if kind == "bare":
        return nn.Linear(48, 192, bias=bias).cuda()
    return nn.Sequential(nn.Linear(48, 192, bias=bias), nn.GELU(), nn.Linear(192, 48, bias=bias)).cuda()


def _linears(model):
    return [m for m in model.modules() if type(m) is nn.Linear]


def _traced_run(model, x, half):
    """one forward + backward of `model` -> (output, x.grad, per Linear: dict(x, g, dx) as the layer met them)"""
    seen, hooks = [], []
    for m in _linears(model):
        rec = {}
        seen.append(rec)

        def hook(mod, inp, out, rec=rec):
            rec["x"] = inp[0].detach()
            if inp[0].requires_grad:
                inp[0].register_hook(lambda grad, rec=rec: rec.__setitem__("dx", grad.detach()))
            out.register_hook(lambda grad, rec=rec: rec.__setitem__("g", grad.detach()))
        hooks.append(m.register_forward_hook(hook))
    model.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=half):
        out = model(xx)
    gen = torch.Generator(device="cuda").manual_seed(5)
    (out.float() * torch.randn(out.shape, device="cuda", generator=gen)).sum().backward()
    for h in hooks:
        h.remove()
    return out.detach(), xx.grad, seen


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "autocast_f16"])
@pytest.mark.parametrize("n", [65, R + 1])
@pytest.mark.parametrize("kind", ["bare", "mlp"])
def test_the_bound_forward_is_torchs_and_its_parameter_gradients_keep_the_bound(P, monkeypatch, kind, n, half):
    import stratified_transformer_amd as sta
    from stratified_transformer_amd import layers
    monkeypatch.setattr(layers, "linear_grads_worth_it", lambda n, in_features, out_features, row_type: True)
    model = _model(kind, True)
    x = torch.randn((n, 48), device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
    out_ref, dx_ref, seen_ref = _traced_run(model, x, half)
    names = sta.fuse_linear_grads(model)
    assert names == [name for name, m in model.named_modules() if type(m) is nn.Linear] and len(names) == len(_linears(model))
    with torch.autocast("cuda", dtype=torch.float16, enabled=half):
        probe = model(x.clone().requires_grad_(True))
    assert "LinearRows" in type(probe.grad_fn).__name__  # the new path does run
    out, dx, seen = _traced_run(model, x, half)
    assert out.dtype == out_ref.dtype == (torch.float16 if half else torch.float32)
    assert torch.equal(out, out_ref)  # the same torch call on the same operands
    lowp = torch.float16 if half else torch.float32
    for m, rec, rec_ref in zip(_linears(model), seen, seen_ref):
        assert m.weight.grad.dtype == torch.float32 and m.bias.grad.dtype == torch.float32
        xs, g = rec["x"].to(lowp), rec["g"]  # as the GEMM saw them
        assert g.dtype == lowp
        want = O.reference(O.widen(xs), O.widen(g))
        _within(_np(m.weight.grad), want["dW"], want["tol_W"], "weight.grad")
        _within(_np(m.bias.grad), want["db"], want["tol_b"], "bias.grad")
        for side, r in (("bound", rec), ("unbound", rec_ref)):
            ref, tol = O.input_grad_reference(O.widen(r["g"]), O.widen(m.weight.detach().to(lowp)), 2.0 ** -11 if half else 0.0)
            _within(_np(r["dx"]), ref, tol, f"x.grad ({side})")
    assert dx.dtype == torch.float32 and dx.shape == dx_ref.shape
    sta.unfuse_linear_grads(model)
    out_again, _, _ = _traced_run(model, x, half)
    assert torch.equal(out_again, out_ref)


def test_no_bias_no_bias_gradient_and_no_gradient_no_new_path(P, monkeypatch):
    import stratified_transformer_amd as sta
    from stratified_transformer_amd import layers
    calls = []
    monkeypatch.setattr(layers, "linear_grads_worth_it", lambda *a: calls.append(a) or True)
    model = _model("mlp", False)
    sta.fuse_linear_grads(model)
    x = torch.randn((65, 48), device="cuda")
    out = model(x)
    assert "LinearRows" in type(out.grad_fn).__name__ and [a[:3] for a in calls] == [(65, 48, 192), (65, 192, 48)] and calls[0][3] == torch.float32
    out.sum().backward()
    for m in _linears(model):
        assert m.bias is None and m.weight.grad is not None and m.weight.grad.dtype == torch.float32
    # 3-D rows flatten: the rule sees all of them
    calls.clear()
    model(x[:64].reshape(4, 16, 48)).sum().backward()
    assert [a[0] for a in calls] == [64, 64]
    # under no_grad, and with no parameter wanting a gradient, the module runs F.linear and saves nothing extra
    calls.clear()
    with torch.no_grad():
        quiet = model(x)
    assert quiet.grad_fn is None and torch.equal(quiet, out.detach()) and not calls
    for p in model.parameters():
        p.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    plain = model(xr)
    assert plain.grad_fn is not None and "LinearRows" not in type(plain.grad_fn).__name__ and not calls
    assert torch.equal(plain.detach(), out.detach())
    # a view that is not contiguous stays with torch as well
    for p in model.parameters():
        p.requires_grad_(True)
    strided = torch.randn((65, 96), device="cuda")[:, ::2]
    assert "LinearRows" not in type(model[0](strided).grad_fn).__name__


def test_linear_rows_casts_the_parameters_and_returns_their_dtypes(P):
    torch.manual_seed(3)
    w = torch.randn((17, 15), device="cuda", requires_grad=True)
    b = torch.randn((17,), device="cuda", requires_grad=True)
    x = torch.randn((R + 1, 15), device="cuda").half().requires_grad_(True)
    out = P.linear_rows(x, w, b)
    assert out.dtype == torch.float16 and torch.equal(out, F.linear(x, w.half(), b.half()))
    g = torch.randn(out.shape, device="cuda").half()
    out.backward(g)
    assert w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32 and x.grad.dtype == torch.float16
    want = O.reference(O.widen(x), O.widen(g))
    _within(_np(w.grad), want["dW"], want["tol_W"], "weight.grad")  # the fp32 sums, not rounded to half on the way
    _within(_np(b.grad), want["db"], want["tol_b"], "bias.grad")
    assert torch.equal(x.grad, g @ w.detach().half())
    wh = w.detach().half().requires_grad_(True)  # half parameters get half gradients
    P.linear_rows(x.detach(), wh, None).backward(g)
    assert wh.grad.dtype == torch.float16 and torch.equal(wh.grad, P.linear_param_grads(x.detach(), g, bias=False)[0].half())
