"""The last two lines of a training step on the device (tool/train.py:350-352, `scaler.step(optimizer)`; `scaler.update()`):

    AdamW       torch.optim.AdamW's update (amsgrad=False, maximize=False) of every parameter in ONE library call on csrc/optim.hip: the
                loss scaler's finite check, the unscale and the update in a fixed number of launches, whatever the number of tensors
    SGD         torch.optim.SGD's update (dampening=0, maximize=False; momentum, Nesterov, weight decay), the reference's other optimizer
                (tool/train.py:127-128), by the same call
    GradScaler  torch.amp.GradScaler whose step() hands the scale to that call and records its verdict where the inherited update() looks
                for it: nothing is read back, the scale is halved or grown by torch's own device op

Both optimizers clip by the global gradient norm inside that call when `optimizer.max_grad_norm` is set (torch's recipe is
`scaler.unscale_(opt)`; `clip_grad_norm_(params, max_norm)`; `scaler.step(opt)`): the squared norm is summed in the finite check's read of
the gradients, the factor is applied in the update's registers, and `optimizer.last_grad_norm` is what clip_grad_norm_ returns.

A driver changes two lines: `optimizer = sta.optim.AdamW(param_dicts, ...)` (or `sta.optim.SGD(...)`) and
`scaler = sta.optim.GradScaler()`.  param_groups carry torch's keys, so util/lr.py's schedulers (LambdaLR on group['lr']) work unchanged;
state_dict() / load_state_dict() round-trip and accept what torch.optim.AdamW / torch.optim.SGD wrote.  No CPU fallback: step() on a CPU
parameter raises.
"""
import math

import numpy as np
import torch
from torch.amp.grad_scaler import OptState

from . import _lib

__all__ = ["AdamW", "SGD", "GradScaler"]

_TENSOR_WORDS = 7   # pointops2_optim_tensor: param, grad, exp_avg, exp_avg_sq, step, numel, (group | first_chunk << 32) as int64 words
_GROUP_WORDS = 5    # pointops2_optim_group: lr, beta1, beta2, eps, weight_decay as doubles
_CHUNK_SHIFT = 12   # POINTOPS2_OPTIM_CHUNK = 4096 elements: one float64 partial of the norm per chunk


class _Slot:
    """One page-locked host table and the event behind the last call that copied from it"""
    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.words = self.buf.numpy().view(np.int64)
        self.event = None


class _TableStep(torch.optim.Optimizer):
    """What AdamW and SGD share: the descriptor table of optim_step_launcher, its page-locked slots, the workspace, the flag and the step.
    A subclass names its kind (_KIND), the state entries whose identity a table row depends on (_STATE_KEYS, three names, None where the
    kernel takes no array), refuses what the kernels do not do (_check_groups), creates and checks a parameter's state (_refresh_state) and
    packs a group's five doubles (_group_row).

    max_grad_norm   None (default), or a positive finite Python number: clip by the global 2-norm of the unscaled gradients of all
                    parameters that have one, across all groups, inside the step's one call; anything else raises at step()
    last_grad_norm  after a step with clipping: that norm before the clip, a 0-dim fp32 device tensor (what clip_grad_norm_ returns);
                    else None
    last_found_inf  the verdict of the last step's own check (or the scaler's found_inf it used), a 0-dim device tensor
    Neither attribute is part of param_groups or of state_dict()."""

    _step_supports_amp_scaling = True
    _KIND = None
    _STATE_KEYS = (None, None, None)

    def _init_table(self):
        self.max_grad_norm = None
        self.last_grad_norm = None
        self.last_found_inf = None   # the verdict of the last step's own check (or the scaler's found_inf it used)
        self._slots = []             # page-locked tables; one is rewritten only after the stream has passed its last copy
        self._workspace = None
        self._flag = None
        self._norm = None
        self._recs, self._static, self._device = None, None, None   # the cached table (see _rows)

    def __setstate__(self, state):
        super().__setstate__(state)
        for name, value in (("max_grad_norm", None), ("last_grad_norm", None), ("last_found_inf", None), ("_slots", []), ("_workspace", None),
                            ("_flag", None), ("_norm", None)):
            self.__dict__.setdefault(name, value)   # (load_state_dict comes through here: tables a copy may still read are kept)
        self._recs, self._static, self._device = None, None, None

    # ---- the table ----
    # One record per parameter, in group order: [param, group, three state entries (_STATE_KEYS), param's address, row of _static].  A step
    # asks every parameter for its gradient, its address and its state; the record's row of the table (_static: the addresses of the
    # parameter and its state, numel, group) is rebuilt - with every check - only when one of them is not the object it was.
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._recs = None

    def _refresh(self, rec, g):
        p, gi, who = rec[0], rec[1], type(self).__name__
        if p.dtype != torch.float32:
            raise TypeError(f"{who}: params: expected torch.float32, got {p.dtype}")
        if g.dtype != torch.float32:
            raise TypeError(f"{who}: grad: expected torch.float32, got {g.dtype}")
        if not p.is_contiguous():
            raise RuntimeError(f"{who}: params: expected contiguous parameters")
        if not p.is_cuda:
            raise RuntimeError(f"{who}: params: expected GPU tensors (the HIP path has no CPU fallback), got {p.device}")
        if self._device is None:
            self._device = p.device
        device = self._device
        if p.device != device or g.device != device:
            raise RuntimeError(f"{who}: params: parameters and gradients must be on one device, got {device} and {p.device} / {g.device}")
        a, b, c = self._refresh_state(rec, p, device)
        rec[5] = p.data_ptr()
        self._static[rec[6]] = (rec[5], 0, a, b, c, p.numel(), gi)

    def _state_array(self, name, t, p, device):
        if t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or t.numel() != p.numel():
            raise RuntimeError(f"{type(self).__name__}: state[{name!r}]: expected a contiguous fp32 tensor of the parameter's size on {device}")
        return t.data_ptr()

    def _rows(self):
        """(table rows [n, 7] without the gradients' column, the gradients' addresses, the gradients) of the parameters this step updates"""
        self._check_groups()
        recs = self._recs
        if recs is None or len(recs) != sum(len(group["params"]) for group in self.param_groups):
            recs = self._recs = [[p, gi, None, None, None, -1, 0] for gi, group in enumerate(self.param_groups) for p in group["params"]]
            for row, rec in enumerate(recs):
                rec[6] = row
            self._static = np.zeros((len(recs), _TENSOR_WORDS), np.int64)
        state, rows, g_ptrs, grads, who = self.state, [], [], [], type(self).__name__
        k0, k1, k2 = self._STATE_KEYS
        absent = {}
        for rec in recs:
            p = rec[0]
            g = p.grad
            if g is None or not p.requires_grad:
                continue
            if g.is_sparse:
                raise RuntimeError(f"{who}: grad: sparse gradients are not supported")
            if not g.is_contiguous():
                g = g.contiguous()   # (freed after the call: the allocator reuses it for later work of this stream only)
            st = state.get(p)
            if st is None:
                st = absent
            if p.data_ptr() != rec[5] or st.get(k0) is not rec[2] or st.get(k1) is not rec[3] or st.get(k2) is not rec[4]:
                self._refresh(rec, g)
            rows.append(rec[6])
            g_ptrs.append(g.data_ptr())
            grads.append(g)
        table = self._static if len(rows) == len(recs) else self._static[rows]
        return table, g_ptrs, grads

    def _slot(self, nbytes):
        for s in self._slots:
            if s.buf.numel() >= nbytes and (s.event is None or s.event.query()):
                return s
        s = _Slot(max(nbytes, 4096))
        self._slots = [x for x in self._slots if x.buf.numel() >= nbytes or not (x.event is None or x.event.query())] + [s]
        return s

    def _max_norm(self):
        m = self.max_grad_norm
        if m is None:
            return 0.0
        if isinstance(m, bool) or not isinstance(m, (int, float)) or not math.isfinite(m) or not m > 0:
            raise ValueError(f"{type(self).__name__}: max_grad_norm: expected None or a positive finite Python number, got {m!r}")
        return float(m)

    @torch.no_grad()
    def step(self, closure=None):
        loss, self.last_found_inf, self.last_grad_norm = None, None, None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        who = type(self).__name__
        max_norm = self._max_norm()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        table, g_ptrs, grads = self._rows()
        if not g_ptrs:
            return loss
        device = self._device
        for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.numel() == 1 and t.dtype == torch.float32):
                    raise TypeError(f"{who}: {name}: expected an fp32 tensor of one element")
                if t.device != device:
                    raise RuntimeError(f"{who}: {name}: is on {t.device}, the parameters on {device}")
        n_t, n_g = len(g_ptrs), len(self.param_groups)
        words = n_t * _TENSOR_WORDS + n_g * _GROUP_WORDS
        slot = self._slot(8 * words)
        rows = slot.words[:n_t * _TENSOR_WORDS].reshape(n_t, _TENSOR_WORDS)
        rows[:] = table
        rows[:, 1] = g_ptrs
        slot.words[n_t * _TENSOR_WORDS:words].view(np.float64).reshape(n_g, _GROUP_WORDS)[:] = [self._group_row(g) for g in self.param_groups]
        if max_norm > 0.0:
            n_chunks = int(((rows[:, 5] + ((1 << _CHUNK_SHIFT) - 1)) >> _CHUNK_SHIFT).sum())
            need = _lib.lib().pointops2_optim_step_workspace_bytes(n_t, n_g, n_chunks)
            if self._norm is None or self._norm.device != device:
                self._norm = torch.zeros((), dtype=torch.float32, device=device)
            norm = self._norm
        else:
            need = _lib.lib().pointops2_optim_workspace_bytes(n_t, n_g)
            norm = None
        if self._workspace is None or self._workspace.device != device or self._workspace.numel() < need:
            self._workspace = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=device)
        if found_inf is None:
            if self._flag is None or self._flag.device != device:
                self._flag = torch.zeros((), dtype=torch.float32, device=device)
            flag, run_check = self._flag, 1
        else:
            flag, run_check = found_inf, 0
        _lib.call("optim_step_launcher", self._KIND, n_t, n_g, slot.buf.data_ptr(), _lib.ptr(self._workspace), self._workspace.numel(),
                  _lib.ptr(grad_scale), _lib.ptr(flag), run_check, max_norm, _lib.ptr(norm), device=device)
        if slot.event is None:
            slot.event = torch.cuda.Event()
        slot.event.record(torch.cuda.current_stream(device))
        self.last_found_inf, self.last_grad_norm = flag, norm
        return loss


class AdamW(_TableStep):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) with amsgrad=False and maximize=False, stepped by one call of
    optim_step_launcher.  Per-parameter state: `step` (0-dim fp32 device tensor), `exp_avg`, `exp_avg_sq`, created on the first step;
    a `step` that load_state_dict() brought as a number or a CPU tensor is moved to the device on the next step.  A parameter without a
    gradient (or with requires_grad=False) is skipped and its count does not advance.  Parameters and gradients are fp32, dense, on one GPU;
    parameters are contiguous.  lr, betas, eps, weight_decay are read from param_groups as Python numbers at every step.

    Without a scaler step() checks the gradients itself and skips the whole step when one holds an infinity or a NaN (`last_found_inf`,
    a 0-dim device tensor, is then 1).  Under a stock torch.amp.GradScaler it reads the `grad_scale` / `found_inf` attributes the scaler
    sets and skips its own check; optim.GradScaler sets `grad_scale` alone, so that the one call checks, unscales and updates.
    `max_grad_norm` / `last_grad_norm`: clipping by the global norm inside the call (_TableStep)."""

    _KIND = _lib.OPTIM_KINDS["adamw"]
    _STATE_KEYS = ("exp_avg", "exp_avg_sq", "step")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, capturable=False,
                 differentiable=False):
        for name, value in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if value:
                raise ValueError(f"AdamW: {name}=True is not supported (csrc/optim.hip implements amsgrad=False, maximize=False; no graph capture)")
        if isinstance(lr, torch.Tensor):
            raise ValueError("AdamW: lr: must be a Python number (it is read on the host at every step)")
        if not 0.0 <= lr:
            raise ValueError(f"AdamW: lr: invalid learning rate {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"AdamW: eps: invalid epsilon {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"AdamW: betas: must be in [0, 1), got {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"AdamW: weight_decay: invalid value {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._init_table()

    def _check_groups(self):
        for gi, group in enumerate(self.param_groups):
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name):
                    raise ValueError(f"AdamW: param_groups[{gi}]: {name}=True is not supported")

    def _group_row(self, g):
        return g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]

    def _refresh_state(self, rec, p, device):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step = st["step"]
        if not (isinstance(step, torch.Tensor) and step.device == device and step.dtype == torch.float32 and step.dim() == 0):
            # written by torch.optim.AdamW: a number, or a tensor on the CPU (no wait: float() of a CPU tensor reads host memory)
            if isinstance(step, torch.Tensor) and step.is_cuda:
                step = step.detach().to(device=device, dtype=torch.float32).reshape(()).clone()
            else:
                step = torch.tensor(float(step), dtype=torch.float32, device=device)
            st["step"] = step
        m, v = st["exp_avg"], st["exp_avg_sq"]
        ptrs = self._state_array("exp_avg", m, p, device), self._state_array("exp_avg_sq", v, p, device), step.data_ptr()
        rec[2:5] = m, v, step
        return ptrs


class SGD(_TableStep):
    """torch.optim.SGD(params, lr, momentum, dampening=0, weight_decay, nesterov) with maximize=False, stepped by one call of
    optim_step_launcher.  Per-parameter state: `momentum_buffer`, created as zeros on the first step (the first update then leaves the
    gradient in it, as torch's clone does); empty when the group's momentum is 0.  A state dict of torch.optim.SGD loads (a buffer of None
    counts as absent) and ours loads into torch's.  A parameter without a gradient (or with requires_grad=False) is skipped.  Parameters and
    gradients are fp32, dense, on one GPU; parameters are contiguous.  lr, momentum, weight_decay and nesterov are read from param_groups as
    Python values at every step; `foreach` and `fused` are accepted and have no meaning here.

    The scaler protocol, the own finite check without a scaler (a step with an infinity or a NaN is skipped) and `max_grad_norm` /
    `last_grad_norm` are AdamW's (_TableStep)."""

    _KIND = _lib.OPTIM_KINDS["sgd"]
    _STATE_KEYS = ("momentum_buffer", None, None)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        for name in ("lr", "momentum", "weight_decay"):
            value = locals()[name]
            if isinstance(value, torch.Tensor):
                raise ValueError(f"SGD: {name}: must be a Python number (it is read on the host at every step)")
            if not 0.0 <= value:
                raise ValueError(f"SGD: {name}: invalid value {value}")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=foreach, differentiable=differentiable, fused=fused)
        self._refuse("SGD", defaults)
        super().__init__(params, defaults)
        self._init_table()
        self._with_momentum = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self._with_momentum = None

    @staticmethod
    def _refuse(where, group):
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError(f"{where}: lr: must be a Python number (it is read on the host at every step)")
        if group.get("dampening", 0) != 0:
            raise ValueError(f"{where}: dampening={group['dampening']} is not supported (csrc/optim.hip implements dampening=0)")
        for name in ("maximize", "differentiable"):
            if group.get(name):
                raise ValueError(f"{where}: {name}=True is not supported")
        if group.get("nesterov") and not group["momentum"] > 0:
            raise ValueError(f"{where}: nesterov=True requires a momentum above 0, got momentum={group['momentum']}")

    def _check_groups(self):
        for gi, group in enumerate(self.param_groups):
            self._refuse(f"SGD: param_groups[{gi}]", group)
        with_momentum = tuple(group["momentum"] != 0 for group in self.param_groups)
        if with_momentum != self._with_momentum:   # a group that gains a momentum needs its buffers: every row is rebuilt
            self._with_momentum, self._recs = with_momentum, None

    def _group_row(self, g):
        return g["lr"], g["momentum"], 1.0 if g["nesterov"] else 0.0, 0.0, g["weight_decay"]

    def _refresh_state(self, rec, p, device):
        st = self.state.get(p)
        buf = None if st is None else st.get("momentum_buffer")
        if buf is None and self.param_groups[rec[1]]["momentum"] != 0:
            buf = self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        rec[2:5] = buf, None, None
        return (0 if buf is None else self._state_array("momentum_buffer", buf, p, device)), 0, 0


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler; step() alone differs, and only for an optim.AdamW or optim.SGD whose gradients are still scaled (no unscale_()
    since the last update()): the optimizer's one call checks, unscales, clips when asked to and updates, and its found_inf is what update()
    then reads on the device."""

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled or not isinstance(optimizer, _TableStep):
            return super().step(optimizer, *args, **kwargs)
        state = self._per_optimizer_states[id(optimizer)]
        if state["stage"] is not OptState.READY or "closure" in kwargs:
            return super().step(optimizer, *args, **kwargs)   # unscaled already, stepped twice, a closure: torch's own handling
        self._check_scale_growth_tracker("step")
        optimizer.grad_scale, optimizer.found_inf = self._get_scale_async(), None
        try:
            retval = optimizer.step(*args, **kwargs)
        finally:
            del optimizer.grad_scale
            del optimizer.found_inf
        if optimizer.last_found_inf is not None:
            state["found_inf_per_device"] = {optimizer.last_found_inf.device: optimizer.last_found_inf}
        else:   # no parameter had a gradient: nothing ran, nothing overflowed
            scale = self._get_scale_async()
            state["found_inf_per_device"] = {scale.device: torch.zeros((), dtype=torch.float32, device=scale.device)}
        state["stage"] = OptState.STEPPED
        return retval
