"""Inputs and runners the SGD / clipping tests share (tests/test_optim_sgd_clip_cpu.py, tests/test_optim_sgd_clip_hip.py): the SGD
parameter groups, and 20-step runs of the oracle (tests/optim_sgd_clip_oracle.py) and of torch's optimizers with torch's clipping."""
import torch

from tests import optim_cases as C
from tests import optim_sgd_clip_oracle as S

# momentum 0.9 with decay, the same with Nesterov, no momentum; two groups each (tensors alternate, optim_cases.group_of)
SGD_CONFIGS = {
    "momentum": [dict(lr=6e-3, momentum=0.9, weight_decay=1e-4, nesterov=False), dict(lr=6e-4, momentum=0.9, weight_decay=1e-4, nesterov=False)],
    "nesterov": [dict(lr=6e-3, momentum=0.9, weight_decay=1e-4, nesterov=True), dict(lr=6e-4, momentum=0.9, weight_decay=1e-4, nesterov=True)],
    "plain": [dict(lr=6e-3, momentum=0.0, weight_decay=1e-4, nesterov=False), dict(lr=6e-4, momentum=0.0, weight_decay=1e-4, nesterov=False)],
    "two_groups": [dict(lr=6e-3, momentum=0.9, weight_decay=1e-4, nesterov=False), dict(lr=2e-3, momentum=0.5, weight_decay=0.0, nesterov=True)],
}
MAX_NORM = 1.0   # N(0, 1) gradients of the 4403 elements of optim_cases.SEQUENCE_SIZES have a norm near 66: the factor stays near 0.015


def groups_of(kind, config=None):
    return C.GROUPS if kind == "adamw" else SGD_CONFIGS[config]


def param_groups(tensors, groups):
    gof = C.group_of(len(tensors))
    return [dict(params=[t for t, g in zip(tensors, gof) if g == k], **groups[k]) for k in range(len(groups))]


def oracle_run(kind, groups, params, grads, dtype, scale=None, max_norm=None):
    """-> the State after every step of `grads`, and the clip factors it used"""
    st = S.State(kind, params, groups, C.group_of(len(params)), dtype, max_norm)
    coefs = []
    for g in grads:
        assert st.step(g, scale) is False
        coefs.append(st.coef)
    return st, coefs


def torch_run(kind, groups, params, grads, dtype, device="cpu", max_norm=None):
    """the final parameters of torch.optim.AdamW / torch.optim.SGD (foreach=False), with torch.nn.utils.clip_grad_norm_ in front of every
    step when max_norm is given -> (list of numpy arrays, the norms clip_grad_norm_ returned)"""
    ps = [torch.tensor(a, dtype=dtype, device=device).requires_grad_(True) for a in params]
    opt = (torch.optim.AdamW if kind == "adamw" else torch.optim.SGD)(param_groups(ps, groups), foreach=False)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=dtype, device=device)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)))
        opt.step()
    return [p.detach().cpu().numpy() for p in ps], norms
