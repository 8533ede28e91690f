"""Inputs the optimizer tests share (tests/test_optim_cpu.py, tests/test_optim_hip.py): the two parameter groups, seeded parameters and
gradients, and the 20-step accuracy measurement of an fp32 implementation against the float64 oracle."""
import numpy as np
import torch

from tests import optim_oracle as O

GROUPS = [dict(lr=6e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=6e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]
SEQUENCE_SIZES = [257, 4097, 48, 1]   # the 20-step sequence: tensors 0, 2 in group 0, tensors 1, 3 in group 1
SEQUENCE_STEPS = 20


def group_of(n_tensors):
    return [i % 2 for i in range(n_tensors)]


def params_and_grads(sizes, steps, seed):
    """N(0,1) fp32 parameters and `steps` lists of N(0,1) fp32 gradients (exactly representable in float64, so every precision sees the
    same inputs)"""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(steps)]
    return params, grads


def torch_groups(tensors):
    """param_groups for a torch-style constructor: the tensors dealt to GROUPS as group_of() says"""
    gof = group_of(len(tensors))
    return [dict(params=[t for t, g in zip(tensors, gof) if g == k], **GROUPS[k]) for k in range(len(GROUPS))]


def oracle_run(params, grads, dtype, scale=None):
    st = O.State(params, GROUPS, group_of(len(params)), dtype)
    for g in grads:
        st.step(g, scale)
    return st


def torch_run(params, grads, dtype, device="cpu", make=None):
    """the final parameters of torch.optim.AdamW(foreach=False) (or make(param_groups)) on tensors of `dtype` -> list of numpy arrays"""
    ps = [torch.tensor(a, dtype=dtype, device=device).requires_grad_(True) for a in params]
    opt = (make or (lambda groups: torch.optim.AdamW(groups, foreach=False)))(torch_groups(ps))
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=dtype, device=device)
        opt.step()
    return [p.detach().cpu().numpy() for p in ps]


def max_abs_errors(got, want64):
    return [float(np.max(np.abs(np.asarray(a, np.float64) - b))) if b.size else 0.0 for a, b in zip(got, want64)]
