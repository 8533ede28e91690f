"""GPU: optim.SGD, and the clip by the global gradient norm of optim.SGD and optim.AdamW (`max_grad_norm`), against the numpy oracle
(tests/optim_sgd_clip_oracle.py, float32 mode) - BIT-IDENTICAL parameters, momentum buffers or moments, step counts and `last_grad_norm`
in every case; the oracle itself is bound to torch.optim.SGD and torch.nn.utils.clip_grad_norm_ in tests/test_optim_sgd_clip_cpu.py."""
import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, optim
from tests import optim_cases as C
from tests import optim_oracle as O
from tests import optim_sgd_clip_cases as K
from tests import optim_sgd_clip_oracle as S

pytestmark = pytest.mark.gpu
CHUNK = S.CHUNK
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 70001, (64, 3, 16, 3), 0]
KINDS = {"sgd": optim.SGD, "adamw": optim.AdamW}
TORCH = {"sgd": torch.optim.SGD, "adamw": torch.optim.AdamW}


def _numel(shape):
    return int(np.prod(shape))


def _place(a, shape=None, offset=None):
    """device tensor with a's values: freshly allocated, or (offset given) a view `offset` elements into a larger buffer"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if offset is not None:
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
        buf[offset:offset + t.numel()] = t
        t = buf[offset:offset + t.numel()]
        assert t.data_ptr() % 16 == (4 * offset) % 16
    return t if shape is None else t.view(shape)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


class Pair:
    """device parameters under optim.SGD / optim.AdamW (or `make`) next to the oracle's state on the same values"""

    def __init__(self, kind, shapes, seed=0, config="momentum", max_norm=None, offsets=None, grad_offsets=None, make=None):
        self.kind, self.shapes = kind, list(shapes)
        n = len(self.shapes)
        self.offsets = offsets or [None] * n
        self.grad_offsets = grad_offsets or self.offsets
        self.rng = np.random.default_rng(seed)
        values = [self.rng.standard_normal(_numel(s)).astype(np.float32) for s in self.shapes]
        self.groups, self.group_of = K.groups_of(kind, config), C.group_of(n)
        self.oracle = S.State(kind, values, self.groups, self.group_of, max_norm=max_norm)
        self.params = [_place(v, s, o).requires_grad_(True) for v, s, o in zip(values, self.shapes, self.offsets)]
        self.opt = (make or KINDS[kind])(K.param_groups(self.params, self.groups))
        if max_norm is not None:
            self.opt.max_grad_norm = max_norm

    def grads(self, scale=1.0):
        return [(self.rng.standard_normal(_numel(s)) * scale).astype(np.float32) for s in self.shapes]

    def set_grads(self, grads):
        for p, g, s, o in zip(self.params, grads, self.shapes, self.grad_offsets):
            p.grad = None if g is None else _place(g, s, o)

    def step(self, grads, scaler=None, scale=None):
        """one step on both sides; scale: the loss scale in force (what the oracle unscales by) -> whether the oracle skipped"""
        self.set_grads(grads)
        if scaler is None:
            self.opt.step()
        else:
            scaler.step(self.opt)
            scaler.update()
        return self.oracle.step(grads, scale)

    def state_bits(self):
        keys = ("momentum_buffer",) if self.kind == "sgd" else ("exp_avg", "exp_avg_sq", "step")
        return [[_bits(p).copy()] + [_bits(self.opt.state[p][k]).copy() for k in keys if k in self.opt.state.get(p, {})] for p in self.params]

    def check(self):
        for i, p in enumerate(self.params):
            st = self.opt.state.get(p, {})
            assert np.array_equal(_bits(p), _bits(self.oracle.p[i])), f"tensor {i} {self.shapes[i]}: params differ"
            if self.kind == "sgd":
                if self.groups[self.group_of[i]]["momentum"] == 0 or self.oracle.t[i] == 0:
                    assert not st, f"tensor {i}: state without a momentum or a step"
                    continue
                assert set(st) == {"momentum_buffer"}
                assert np.array_equal(_bits(st["momentum_buffer"]), _bits(self.oracle.m[i])), f"tensor {i} {self.shapes[i]}: momentum_buffer differs"
                continue
            if not st:
                assert self.oracle.t[i] == 0
                continue
            assert np.array_equal(_bits(st["exp_avg"]), _bits(self.oracle.m[i])), f"tensor {i} {self.shapes[i]}: exp_avg differs"
            assert np.array_equal(_bits(st["exp_avg_sq"]), _bits(self.oracle.v[i])), f"tensor {i} {self.shapes[i]}: exp_avg_sq differs"
            assert float(st["step"]) == self.oracle.t[i], f"tensor {i}: step count"

    def check_norm(self):
        got = self.opt.last_grad_norm
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
        assert np.array_equal(_bits(got), _bits(self.oracle.norm)), f"norm {float(got)!r}, oracle {float(self.oracle.norm)!r}"


def _scaler(init_scale, cls=None, **kw):
    s = (cls or optim.GradScaler)("cuda", init_scale=float(init_scale), **kw)
    s.scale(torch.zeros((), device="cuda"))   # creates the scale tensor, as the first scaler.scale(loss) of a run does
    return s


def _same(a, b):
    return all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q)) and [len(p) for p in a] == [len(q) for q in b]


# ---- SGD ----
@pytest.mark.parametrize("scale", [None, 65536.0, 3000.0])
@pytest.mark.parametrize("config", ["momentum", "nesterov", "plain", "two_groups"])
def test_sgd_sizes(config, scale):
    pair = Pair("sgd", SIZES, seed=1, config=config)
    scaler = None if scale is None else _scaler(scale)
    calls = _lib.CALLS[0]
    for _ in range(5):
        assert pair.step(pair.grads(scale or 1.0), scaler, scale) is False
    assert _lib.CALLS[0] - calls == 5
    pair.check()
    assert pair.oracle.t == [5] * len(SIZES)
    assert float(pair.opt.last_found_inf) == 0.0 and pair.opt.last_grad_norm is None
    if config == "plain":
        assert len(pair.opt.state) == 0
    if scale is not None:
        assert float(scaler.get_scale()) == scale


@pytest.mark.parametrize("kind, max_norm", [("sgd", None), ("sgd", 1.0), ("adamw", 1.0)])
def test_alignment(kind, max_norm):
    shapes = [1000, CHUNK, 2 * CHUNK + 5, 9, CHUNK + 1]
    offsets = [1, 2, 3, 1, None]
    grad_offsets = [1, 2, 3, None, 3]              # the last two: one side aligned, the other not
    moved = Pair(kind, shapes, seed=2, max_norm=max_norm, offsets=offsets, grad_offsets=grad_offsets)
    plain = Pair(kind, shapes, seed=2, max_norm=max_norm)
    for _ in range(3):
        g = moved.grads()
        assert all(np.array_equal(a, b) for a, b in zip(g, plain.grads()))
        moved.step(g)
        plain.step(g)
        if max_norm is not None:
            moved.check_norm()
            plain.check_norm()
            assert np.array_equal(_bits(moved.opt.last_grad_norm), _bits(plain.opt.last_grad_norm)) and moved.oracle.coef < 1
    moved.check()
    plain.check()
    assert _same(moved.state_bits(), plain.state_bits())
    assert [p.data_ptr() % 16 for p in moved.params[:4]] == [4, 8, 12, 4]
    assert [p.grad.data_ptr() % 16 for p in moved.params] == [4, 8, 12, 0, 12]


# ---- clipping ----
@pytest.mark.parametrize("scale", [None, 3000.0])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipping(kind, scale):
    pair = Pair(kind, SIZES, seed=12, max_norm=1.0)
    scaler = None if scale is None else _scaler(scale)
    for _ in range(3):
        calls = _lib.CALLS[0]
        assert pair.step(pair.grads(scale or 1.0), scaler, scale) is False
        assert _lib.CALLS[0] - calls == 1
        pair.check_norm()
        assert 0 < pair.oracle.coef < 1 and 200 < float(pair.opt.last_grad_norm) < 400          # 84 000 N(0, 1) elements: near 290
    pair.check()
    assert pair.oracle.t == [3] * len(SIZES) and float(pair.opt.last_found_inf) == 0.0


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipping_over_many_tensors_and_chunks(kind):
    shapes = [7] * 300 + [1_100_000]                                                            # 300 + 269 chunks: the reduce loop goes round
    pair = Pair(kind, shapes, seed=13, max_norm=2.5)
    assert sum(-(-_numel(s) // CHUNK) for s in shapes) > 2 * S.THREADS
    for _ in range(2):
        calls = _lib.CALLS[0]
        pair.step(pair.grads())
        assert _lib.CALLS[0] - calls == 1
        pair.check_norm()
        assert 0 < pair.oracle.coef < 1
    pair.check()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_a_max_norm_above_the_norm_changes_nothing(kind):
    shapes = [5, 300, CHUNK + 1, 2 * CHUNK]
    loose, free = Pair(kind, shapes, seed=14, max_norm=1e9), Pair(kind, shapes, seed=14)
    for _ in range(3):
        g = loose.grads()
        assert all(np.array_equal(a, b) for a, b in zip(g, free.grads()))
        loose.step(g)
        free.step(g)
        loose.check_norm()
        assert loose.oracle.coef == np.float32(1.0) and free.opt.last_grad_norm is None
    loose.check()
    free.check()
    assert _same(loose.state_bits(), free.state_bits())
    loose.opt.max_grad_norm = None                                                             # disarmed again: no norm is reported
    loose.oracle.max_norm = None
    loose.step(loose.grads())
    loose.check()
    assert loose.opt.last_grad_norm is None


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_parameters_without_gradients_are_left_out_of_the_norm(kind):
    pair = Pair(kind, [50, 6000, 70, 80], seed=15, max_norm=1.0)
    pair.params[3].requires_grad_(False)
    for _ in range(2):
        g = pair.grads()
        g[1] = g[3] = None
        pair.step(g)
        pair.check_norm()
        assert float(pair.opt.last_grad_norm) < 20                                              # 120 elements; with the 6000 it would be near 79
    pair.check()
    assert pair.oracle.t == [2, 0, 2, 0] and pair.params[1] not in pair.opt.state and pair.params[3] not in pair.opt.state
    g = pair.grads()
    g[3] = None
    pair.step(g)
    pair.check_norm()
    pair.check()
    assert float(pair.opt.last_grad_norm) > 60


# ---- overflow ----
@pytest.mark.parametrize("case", ["inf_last", "nan_misaligned"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_overflow_with_clipping(kind, case):
    shapes = [300, 2 * CHUNK, CHUNK + 77]
    pair = Pair(kind, shapes, seed=4, max_norm=1.0, offsets=[None, 1, None], grad_offsets=[None, 1, None])
    scaler = _scaler(65536.0, growth_interval=1000)
    for _ in range(2):
        pair.step(pair.grads(65536.0), scaler, 65536.0)
        pair.check_norm()
    pair.check()
    before = pair.state_bits()
    bad = pair.grads(65536.0)
    which, index, value = {"inf_last": (2, CHUNK + 76, np.inf), "nan_misaligned": (1, CHUNK + 3, np.nan)}[case]
    bad[which][index] = value
    pair.set_grads(bad)
    assert pair.params[1].grad.data_ptr() % 16 == 4
    scaler.step(pair.opt)
    assert float(pair.opt.last_found_inf) == 1.0
    scaler.update()
    assert pair.oracle.step(bad, 65536.0) is True
    assert _same(before, pair.state_bits())
    assert float(scaler.get_scale()) == 32768.0 and int(scaler._growth_tracker) == 0
    assert not np.isfinite(float(pair.opt.last_grad_norm))
    pair.check()
    assert pair.step(pair.grads(32768.0), scaler, 32768.0) is False
    pair.check_norm()
    pair.check()
    assert pair.oracle.t == [3, 3, 3] and float(pair.opt.last_found_inf) == 0.0 and int(scaler._growth_tracker) == 1


def test_overflow_without_a_scaler_skips_too():
    pair = Pair("sgd", [10, CHUNK], seed=5, max_norm=1.0)
    pair.step(pair.grads())
    bad = pair.grads()
    bad[1][CHUNK - 1] = np.inf
    assert pair.step(bad) is True
    assert float(pair.opt.last_found_inf) == 1.0
    pair.check()
    assert pair.oracle.t == [1, 1]


# ---- the scalers ----
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_stock_scaler_gives_the_same_bits(max_norm):
    shapes = [5, 300, CHUNK + 1]
    ours, stock = Pair("sgd", shapes, seed=7, max_norm=max_norm), Pair("sgd", shapes, seed=7, max_norm=max_norm)
    s_ours, s_stock = _scaler(65536.0), _scaler(65536.0, cls=torch.amp.GradScaler)
    scale = 65536.0
    for i in range(4):
        g = ours.grads(scale)
        assert all(np.array_equal(a, b) for a, b in zip(g, stock.grads(scale)))
        if i == 1:
            g[1][17] = np.inf
        calls = _lib.CALLS[0]
        skipped = ours.step(g, s_ours, scale)
        stock.step(g, s_stock, scale)
        assert _lib.CALLS[0] - calls == 2 and skipped == (i == 1)
        scale = scale / 2 if skipped else scale
        assert float(s_ours.get_scale()) == float(s_stock.get_scale()) == scale
        if max_norm is not None and not skipped:
            ours.check_norm()
            stock.check_norm()
    ours.check()
    stock.check()
    assert ours.oracle.t == [3, 3, 3] and _same(ours.state_bits(), stock.state_bits())
    # after unscale_() the stock path: the gradients carry no scale any more, the scaler's verdict is used - and the clip still applies
    g = ours.grads(scale)
    ours.set_grads(g)
    s_ours.unscale_(ours.opt)
    s_ours.step(ours.opt)
    s_ours.update()
    ours.oracle.step([a * O.inv_scale_of(scale) for a in g])
    ours.check()
    if max_norm is not None:
        ours.check_norm()
        assert 0 < ours.oracle.coef < 1


def test_no_host_wait():
    pair = Pair("sgd", [300, CHUNK + 1], seed=8, max_norm=1.0)
    scaler = _scaler(65536.0)
    pair.step(pair.grads(65536.0), scaler, 65536.0)                  # creates the state, the workspace and the norm's tensor
    g = pair.grads(65536.0)
    pair.set_grads(g)
    probe = torch.ones((), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:                                                         # the control: the mode traps a deliberate read-back on this build
            probe.item()
            trapped = False
        except RuntimeError:
            trapped = True
        if trapped:
            scaler.step(pair.opt)
            scaler.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not trapped:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not trap .item() on this build")
    pair.oracle.step(g, 65536.0)
    pair.check()
    pair.check_norm()
    assert 0 < pair.oracle.coef < 1


# ---- state dicts ----
@pytest.mark.parametrize("config", ["momentum", "plain"])
def test_resume(config):
    shapes = [33, CHUNK + 9, 0]
    whole, first = Pair("sgd", shapes, seed=9, config=config, max_norm=1.0), Pair("sgd", shapes, seed=9, config=config, max_norm=1.0)
    grads = [whole.grads() for _ in range(6)]
    for g in grads:
        whole.step(g)
    for g in grads[:3]:
        first.step(g)
    second = Pair("sgd", shapes, seed=9, config=config, max_norm=1.0)
    for p, q in zip(second.params, first.params):
        p.data.copy_(q.data)
    second.opt.load_state_dict(first.opt.state_dict())
    assert second.opt.max_grad_norm == 1.0                           # (not part of the state dict: the fresh optimizer's own)
    second.oracle = first.oracle
    for g in grads[3:]:
        second.step(g)
    second.check()
    second.check_norm()
    whole.check()
    assert _same(second.state_bits(), whole.state_bits())


def test_resume_from_a_torch_state_dict():
    shapes = [33, CHUNK + 9]
    theirs = Pair("sgd", shapes, seed=10, make=lambda groups: torch.optim.SGD(groups, foreach=False))
    for _ in range(3):
        theirs.set_grads(theirs.grads())
        theirs.opt.step()
    sd = theirs.opt.state_dict()
    assert all(s["momentum_buffer"].is_cuda for s in sd["state"].values())
    ours = Pair("sgd", shapes, seed=10)
    for p, q in zip(ours.params, theirs.params):
        p.data.copy_(q.data)
    ours.opt.load_state_dict(sd)
    order = [p for k in range(len(ours.groups)) for p, g in zip(range(len(shapes)), ours.group_of) if g == k]   # state dict ids: group by group
    for sid, i in enumerate(order):
        ours.oracle.p[i] = theirs.params[i].detach().cpu().numpy().reshape(-1).copy()
        ours.oracle.m[i] = sd["state"][sid]["momentum_buffer"].cpu().numpy().reshape(-1).copy()
        ours.oracle.t[i] = 3
    for _ in range(3):
        ours.step(ours.grads())
    ours.check()
    assert ours.oracle.t == [6, 6]


def test_against_torch_on_the_device():
    params, grads = C.params_and_grads(C.SEQUENCE_SIZES, C.SEQUENCE_STEPS, seed=7)
    groups = K.SGD_CONFIGS["momentum"]
    o64, _ = K.oracle_run("sgd", groups, params, grads, np.float64)
    ps = [torch.tensor(a, device="cuda").requires_grad_(True) for a in params]
    opt = optim.SGD(K.param_groups(ps, groups))
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, device="cuda")
        opt.step()
    got = [p.detach().cpu().numpy() for p in ps]
    ours = C.max_abs_errors(got, o64.p)
    torchs = C.max_abs_errors(K.torch_run("sgd", groups, params, grads, torch.float32, device="cuda")[0], o64.p)
    for i, (a, b) in enumerate(zip(ours, torchs)):
        print("tensor", i, "device error", a, "torch (device, foreach=False) error", b, "ratio", a / b if b else float("nan"))
        assert a <= 2 * b
    o32, _ = K.oracle_run("sgd", groups, params, grads, np.float32)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, o32.p))
