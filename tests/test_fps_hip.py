"""GPU (-m gpu): furthest point sampling on every kernel path, size boundary, request length and degenerate cloud of
tests/fps_cases.py, against the CPU oracle.

Bar: every index equals the oracle's (np.array_equal; no tolerance, nothing skipped); a resumed chain is compared on both of
its calls, and the shorter result must be the prefix of the longer.  tests/test_fps_cases_cpu.py establishes, without a GPU,
which kernels each case reaches, that the cases are what they claim, and that the oracle follows the 64-bit key where float64 is
exact.  P2_FPS_STEPWISE is read once per process, so its cases run in one child process."""
import multiprocessing
import os

import numpy as np
import pytest
import torch

from oracle import pointops_ref as ref
from tests import fps_cases as C

pytestmark = pytest.mark.gpu

ALL = sorted(C.CASES)
CHILD_SECONDS = 240   # the child's work is a few seconds behind its imports; the limit only ends a hung child
_ORACLE = {}


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()
    return pointops


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")   # (a copy: the cases' arrays are read-only)


def _oracle(name, call):
    """the oracle's samples for one call of a case's chain, computed once and never written to"""
    if (name, call) not in _ORACLE:
        c = C.CASES[name]
        want = ref.furthestsampling(c.xyz, c.offset, c.requests[call])
        want.setflags(write=False)
        _ORACLE[(name, call)] = want
    return _ORACLE[(name, call)]


def _run_chain(pointops, c):
    """every call of the case's chain on one device tensor, from cleared caches -> list of index arrays"""
    pointops.clear_caches()
    x, off = _dev(c.xyz), _dev(c.offset)
    if c.plain:
        from stratified_transformer_amd import pointops2_cuda
        assert len(c.requests) == 1
        new = c.requests[0]
        idx = torch.zeros(int(new[-1]), dtype=torch.int32, device="cuda")
        tmp = torch.full((len(c.xyz),), 1e10, device="cuda")
        pointops2_cuda.furthestsampling_cuda(len(c.offset), C.n_max_of(c), x, off, _dev(new), tmp, idx)   # (no launch options)
        return [idx.cpu().numpy()]
    if c.hint:
        pointops.hint_unordered(x)
    return [pointops.furthestsampling(x, off, _dev(new)).cpu().numpy() for new in c.requests]


def _prefix_of(short, short_new, long, long_new):
    """per batch element: is `short` the head of `long`?"""
    lo_s = lo_l = 0
    for hi_s, hi_l in zip(short_new, long_new):
        if not np.array_equal(short[lo_s:hi_s], long[lo_l: lo_l + (hi_s - lo_s)]):
            return False
        lo_s, lo_l = int(hi_s), int(hi_l)
    return True


def _assert_chain(name, got, stepwise=False):
    c = C.CASES[name]
    for call, g in enumerate(got):
        want = _oracle(name, call)
        d = C.dispatch_of(c, call, stepwise=stepwise)
        bad = np.flatnonzero(g != want) if g.shape == want.shape else None
        assert np.array_equal(g, want), (f"{name} call {call} ({' + '.join(d.kernels)}, G = {d.G}, BSZ = {d.BSZ}): "
                                         f"first differences at {None if bad is None else bad[:8].tolist()}")
    if len(got) == 2:
        assert _prefix_of(got[0], c.requests[0], got[1], c.requests[1]), f"{name}: the first call is not the prefix of the second"


@pytest.mark.parametrize("name", ALL)
def test_fps_case_equals_the_oracle(P, name):
    _assert_chain(name, _run_chain(P, C.CASES[name]))


@pytest.mark.parametrize("n", C.DEGEN_SIZES)
def test_translation_does_not_change_the_samples(P, n):
    """every coordinate, difference and squared distance of the family is exact in fp32 at every T
    (tests/test_fps_cases_cpu.py): the Morton cells and the boxes see T, the samples must not"""
    base = _run_chain(P, C.CASES[f"degen-translate0-{n}"])[0]
    for T in C.TRANSLATIONS[1:]:
        assert np.array_equal(_run_chain(P, C.CASES[f"degen-translate{T}-{n}"])[0], base), T


def _stepwise_child(names, out_path):
    """a fresh process: the switch is set before the library's first call, which reads it once"""
    os.environ["P2_FPS_STEPWISE"] = "1"
    from stratified_transformer_amd import pointops
    res = {}
    for name in names:
        for call, g in enumerate(_run_chain(pointops, C.CASES[name])):
            res[f"{name}|{call}"] = g
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def test_stepwise_switch_returns_the_oracles_samples(tmp_path):
    """P2_FPS_STEPWISE=1 - what the barrier-timeout error tells users to set - on the sizes where it changes the dispatch
    (2048 to 229376 points): the step-by-step kernel alone, resumes and verified prefixes included.  One child process, joined
    under a time limit; if it dies or hangs the test fails and nothing else is started."""
    out_path = os.path.join(str(tmp_path), "stepwise.npz")
    ctx = multiprocessing.get_context("spawn")
    p = ctx.Process(target=_stepwise_child, args=(C.STEPWISE_CASES, out_path))
    p.start()
    p.join(CHILD_SECONDS)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail(f"the P2_FPS_STEPWISE child did not finish within {CHILD_SECONDS} s")
    assert p.exitcode == 0, p.exitcode
    got = np.load(out_path)
    for name in C.STEPWISE_CASES:
        _assert_chain(name, [got[f"{name}|{call}"] for call in range(len(C.CASES[name].requests))], stepwise=True)
