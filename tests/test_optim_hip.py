"""GPU: optim.AdamW / optim.GradScaler (csrc/optim.hip) against the numpy oracle (tests/optim_oracle.py, float32 mode) - BIT-IDENTICAL
parameters, both moments and step counts in every case; the oracle itself is bound to torch.optim.AdamW in tests/test_optim_cpu.py, and the
last test here repeats that measurement with the device in the oracle's place."""
import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, optim
from tests import optim_cases as C
from tests import optim_oracle as O

pytestmark = pytest.mark.gpu
CHUNK = 4096   # POINTOPS2_OPTIM_CHUNK (tests/test_optim_cpu.py reads it from the header)
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 70001, (64, 3, 16, 3), 0]


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
    """device parameters under optim.AdamW next to the oracle's state on the same values"""

    def __init__(self, shapes, seed=0, offsets=None, grad_offsets=None, group_of=None, make=optim.AdamW):
        self.shapes = list(shapes)
        n = len(self.shapes)
        self.offsets = offsets or [None] * n
        self.grad_offsets = grad_offsets or self.offsets
        self.rng = np.random.default_rng(seed)
        values = [self.rng.standard_normal(_numel(s)).astype(np.float32) for s in self.shapes]
        self.group_of = group_of or C.group_of(n)
        self.oracle = O.State(values, C.GROUPS, self.group_of)
        self.params = [_place(v, s, o).requires_grad_(True) for v, s, o in zip(values, self.shapes, self.offsets)]
        self.opt = make([dict(params=[p for p, g in zip(self.params, self.group_of) if g == k], **C.GROUPS[k]) for k in range(len(C.GROUPS))])

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

    def check(self):
        for i, p in enumerate(self.params):
            st = self.opt.state.get(p, {})
            assert np.array_equal(_bits(p), _bits(self.oracle.p[i])), f"tensor {i} {self.shapes[i]}: params differ"
            if not st:
                assert self.oracle.t[i] == 0
                continue
            assert np.array_equal(_bits(st["exp_avg"]), _bits(self.oracle.m[i])), f"tensor {i} {self.shapes[i]}: exp_avg differs"
            assert np.array_equal(_bits(st["exp_avg_sq"]), _bits(self.oracle.v[i])), f"tensor {i} {self.shapes[i]}: exp_avg_sq differs"
            assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].is_cuda
            assert float(st["step"]) == self.oracle.t[i], f"tensor {i}: step count"


def _scaler(init_scale, cls=None, **kw):
    s = (cls or optim.GradScaler)("cuda", init_scale=float(init_scale), **kw)
    s.scale(torch.zeros((), device="cuda"))   # creates the scale tensor, as the first scaler.scale(loss) of a run does
    return s


@pytest.mark.parametrize("scale", [None, 65536.0, 3000.0])
def test_sizes(scale):
    pair = Pair(SIZES, seed=1)
    scaler = None if scale is None else _scaler(scale)
    calls = _lib.CALLS[0]
    for _ in range(5):
        assert pair.step(pair.grads(scale or 1.0), scaler, scale) is False
    assert _lib.CALLS[0] - calls == 5
    pair.check()
    assert pair.oracle.t == [5] * len(SIZES)
    assert float(pair.opt.last_found_inf) == 0.0
    if scale is not None:
        assert float(scaler.get_scale()) == scale


def test_alignment():
    shapes = [1000, CHUNK, 2 * CHUNK + 5, 9, CHUNK + 1]
    offsets = [1, 2, 3, 1, None]
    grad_offsets = [1, 2, 3, None, 3]              # the last two: one side aligned, the other not
    moved = Pair(shapes, seed=2, offsets=offsets, grad_offsets=grad_offsets)
    plain = Pair(shapes, seed=2)
    for _ in range(3):
        g = moved.grads()
        assert all(np.array_equal(a, b) for a, b in zip(g, plain.grads()))
        moved.step(g)
        plain.step(g)
    moved.check()
    plain.check()
    for a, b in zip(moved.params, plain.params):
        assert np.array_equal(_bits(a), _bits(b))
    assert [p.data_ptr() % 16 for p in moved.params[:4]] == [4, 8, 12, 4]
    assert all(moved.opt.state[p]["exp_avg"].data_ptr() % 16 == 0 for p in moved.params)


def test_tensor_count():
    pair = Pair([7] * 300 + [200000], seed=3)
    for _ in range(2):
        calls = _lib.CALLS[0]
        pair.step(pair.grads())
        assert _lib.CALLS[0] - calls == 1
    pair.check()


def test_steps_in_flight_keep_their_tables():
    """30 steps enqueued without a wait in between, every one with gradients at other addresses: each step's table must still be the one
    it was given when the device gets to it (a host table is rewritten only after the stream has passed the call that copied it)"""
    pair = Pair([7, CHUNK + 1, 300], seed=11)
    steps = [pair.grads() for _ in range(30)]
    placed = [[_place(g, s) for g, s in zip(gs, pair.shapes)] for gs in steps]
    torch.cuda.synchronize()
    for gs in placed:
        for p, g in zip(pair.params, gs):
            p.grad = g
        pair.opt.step()
    for gs in steps:
        pair.oracle.step(gs)
    pair.check()
    assert pair.oracle.t == [30, 30, 30] and 1 <= len(pair.opt._slots) <= 30


def _poisoned(pair, which, index, value):
    g = pair.grads(65536.0)
    g[which][index] = value
    return g


@pytest.mark.parametrize("case", ["inf_last", "nan_first", "neg_inf_misaligned"])
def test_overflow(case):
    shapes = [300, 2 * CHUNK, CHUNK + 77]
    pair = Pair(shapes, seed=4, offsets=[None, 1, None], grad_offsets=[None, 1, None])
    scaler = _scaler(65536.0, growth_interval=1000)
    for _ in range(2):
        pair.step(pair.grads(65536.0), scaler, 65536.0)
    pair.check()
    assert int(scaler._growth_tracker) == 2
    before = [[_bits(t).copy() for t in (p, pair.opt.state[p]["exp_avg"], pair.opt.state[p]["exp_avg_sq"], pair.opt.state[p]["step"])]
              for p in pair.params]
    bad = {"inf_last": lambda: _poisoned(pair, 2, CHUNK + 76, np.inf), "nan_first": lambda: _poisoned(pair, 0, 0, np.nan),
           "neg_inf_misaligned": lambda: _poisoned(pair, 1, CHUNK + 3, -np.inf)}[case]()
    pair.set_grads(bad)
    scaler.step(pair.opt)
    assert float(pair.opt.last_found_inf) == 1.0
    scaler.update()
    assert pair.oracle.step(bad, 65536.0) is True
    after = [[_bits(t) for t in (p, pair.opt.state[p]["exp_avg"], pair.opt.state[p]["exp_avg_sq"], pair.opt.state[p]["step"])] for p in pair.params]
    assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y))
    assert float(scaler.get_scale()) == 32768.0 and int(scaler._growth_tracker) == 0
    pair.check()
    assert pair.step(pair.grads(32768.0), scaler, 32768.0) is False                       # continues from the unskipped count
    pair.check()
    assert pair.oracle.t == [3, 3, 3] and float(pair.opt.last_found_inf) == 0.0 and int(scaler._growth_tracker) == 1


def test_overflow_without_a_scaler_skips_too():
    pair = Pair([10, CHUNK], seed=5)
    pair.step(pair.grads())
    bad = pair.grads()
    bad[1][CHUNK - 1] = np.inf
    assert pair.step(bad) is True
    assert float(pair.opt.last_found_inf) == 1.0
    pair.check()
    assert pair.oracle.t == [1, 1]


def test_skipped_parameters():
    pair = Pair([50, 60, 70, 80], seed=6)
    pair.params[3].requires_grad_(False)
    for _ in range(2):
        g = pair.grads()
        g[1] = g[3] = None
        pair.step(g)
    pair.check()
    assert pair.oracle.t == [2, 0, 2, 0]
    assert pair.params[1] not in pair.opt.state and pair.params[3] not in pair.opt.state
    g = pair.grads()                                   # the parameter without a gradient gets one later: its own count starts then
    g[3] = None
    pair.step(g)
    pair.check()
    assert pair.oracle.t == [3, 1, 3, 0]


def test_stock_scaler_gives_the_same_bits():
    shapes = [5, 300, CHUNK + 1]
    ours, stock = Pair(shapes, seed=7), Pair(shapes, seed=7)
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
    ours.check()
    stock.check()
    assert ours.oracle.t == [3, 3, 3]
    # after unscale_() the stock path: the gradients carry no scale any more, the scaler's verdict is used
    g = ours.grads(scale)
    ours.set_grads(g)
    s_ours.unscale_(ours.opt)
    s_ours.step(ours.opt)
    s_ours.update()
    ours.oracle.step([a * O.inv_scale_of(scale) for a in g])
    ours.check()


def test_no_host_wait():
    pair = Pair([300, CHUNK + 1], seed=8)
    scaler = _scaler(65536.0)
    pair.step(pair.grads(65536.0), scaler, 65536.0)                  # creates the state
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


def test_resume():
    shapes = [33, CHUNK + 9, 0]
    whole, first = Pair(shapes, seed=9), Pair(shapes, seed=9)
    grads = [whole.grads() for _ in range(6)]
    for g in grads:
        whole.step(g)
    for g in grads[:3]:
        first.step(g)
    second = Pair(shapes, seed=9)
    for p, q in zip(second.params, first.params):
        p.data.copy_(q.data)
    second.opt.load_state_dict(first.opt.state_dict())
    second.oracle = first.oracle
    for g in grads[3:]:
        second.step(g)
    second.check()
    whole.check()
    for a, b in zip(second.params, whole.params):
        assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(second.opt.state[a]["exp_avg_sq"]), _bits(whole.opt.state[b]["exp_avg_sq"]))


def test_resume_from_a_torch_state_dict():
    shapes = [33, CHUNK + 9]
    theirs = Pair(shapes, seed=10, make=lambda groups: torch.optim.AdamW(groups, foreach=False))
    for _ in range(3):
        theirs.set_grads(theirs.grads())
        theirs.opt.step()
    sd = theirs.opt.state_dict()
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values())
    ours = Pair(shapes, seed=10)
    for p, q in zip(ours.params, theirs.params):
        p.data.copy_(q.data)
    ours.opt.load_state_dict(sd)
    order = [p for k in range(len(C.GROUPS)) for p, g in zip(range(len(shapes)), ours.group_of) if g == k]   # state dict ids: group by group
    for sid, i in enumerate(order):
        ours.oracle.p[i] = theirs.params[i].detach().cpu().numpy().reshape(-1).copy()
        ours.oracle.m[i] = sd["state"][sid]["exp_avg"].cpu().numpy().reshape(-1).copy()
        ours.oracle.v[i] = sd["state"][sid]["exp_avg_sq"].cpu().numpy().reshape(-1).copy()
        ours.oracle.t[i] = 3
    for _ in range(3):
        ours.step(ours.grads())
    ours.check()
    assert ours.oracle.t == [6, 6]


def test_against_torch_on_the_device():
    params, grads = C.params_and_grads(C.SEQUENCE_SIZES, C.SEQUENCE_STEPS, seed=7)
    o64 = C.oracle_run(params, grads, np.float64)
    got = C.torch_run(params, grads, torch.float32, device="cuda", make=optim.AdamW)
    ours = C.max_abs_errors(got, o64.p)
    torchs = C.max_abs_errors(C.torch_run(params, grads, torch.float32, device="cuda"), o64.p)
    for i, (a, b) in enumerate(zip(ours, torchs)):
        print("tensor", i, "device error", a, "torch (device, foreach=False) error", b, "ratio", a / b)
        assert b > 0 and a <= 2 * b
    o32 = C.oracle_run(params, grads, np.float32)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, o32.p))
