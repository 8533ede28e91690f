"""The last two lines of a training step on the device (tool/train.py:350-352, `scaler.step(optimizer)`; `scaler.update()`):

    AdamW       torch.optim.AdamW's update (amsgrad=False, maximize=False) of every parameter in ONE library call on csrc/optim.hip: the
                loss scaler's finite check, the unscale and the update in a fixed number of launches, whatever the number of tensors
    GradScaler  torch.amp.GradScaler whose step() hands the scale to that call and records its verdict where the inherited update() looks
                for it: nothing is read back, the scale is halved or grown by torch's own device op

A driver changes two lines: `optimizer = sta.optim.AdamW(param_dicts, ...)` and `scaler = sta.optim.GradScaler()`.
param_groups carry torch's keys, so util/lr.py's schedulers (LambdaLR on group['lr']) work unchanged; state_dict() / load_state_dict()
round-trip and accept what torch.optim.AdamW wrote.  No CPU fallback: step() on a CPU parameter raises.
"""
import numpy as np
import torch
from torch.amp.grad_scaler import OptState

from . import _lib

__all__ = ["AdamW", "GradScaler"]

_TENSOR_WORDS = 7   # pointops2_optim_tensor: param, grad, exp_avg, exp_avg_sq, step, numel, (group | first_chunk << 32) as int64 words
_GROUP_WORDS = 5    # pointops2_optim_group: lr, beta1, beta2, eps, weight_decay as doubles


class _Slot:
    """One page-locked host table and the event behind the last call that copied from it"""
    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.words = self.buf.numpy().view(np.int64)
        self.event = None


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) with amsgrad=False and maximize=False, stepped by one call of
    optim_adamw_step_launcher.  Per-parameter state: `step` (0-dim fp32 device tensor), `exp_avg`, `exp_avg_sq`, created on the first step;
    a `step` that load_state_dict() brought as a number or a CPU tensor is moved to the device on the next step.  A parameter without a
    gradient (or with requires_grad=False) is skipped and its count does not advance.  Parameters and gradients are fp32, dense, on one GPU;
    parameters are contiguous.  lr, betas, eps, weight_decay are read from param_groups as Python numbers at every step.

    Without a scaler step() checks the gradients itself and skips the whole step when one holds an infinity or a NaN (`last_found_inf`,
    a 0-dim device tensor, is then 1).  Under a stock torch.amp.GradScaler it reads the `grad_scale` / `found_inf` attributes the scaler
    sets and skips its own check; optim.GradScaler sets `grad_scale` alone, so that the one call checks, unscales and updates."""

    _step_supports_amp_scaling = True

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
        self.last_found_inf = None   # the verdict of the last step's own check (or the scaler's found_inf it used)
        self._slots = []             # page-locked tables; one is rewritten only after the stream has passed its last copy
        self._workspace = None
        self._flag = None
        self._recs, self._static, self._device = None, None, None   # the cached table (see _rows)

    def __setstate__(self, state):
        super().__setstate__(state)
        for name, value in (("last_found_inf", None), ("_slots", []), ("_workspace", None), ("_flag", None)):
            self.__dict__.setdefault(name, value)   # (load_state_dict comes through here: tables a copy may still read are kept)
        self._recs, self._static, self._device = None, None, None

    # ---- the table ----
    # One record per parameter, in group order: [param, group, exp_avg, exp_avg_sq, step, param's address, row of _static].  A step asks
    # every parameter for its gradient, its address and its state; the record's row of the table (_static: the addresses of the
    # parameter and its state, numel, group) is rebuilt - with every check - only when one of them is not the object it was.
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._recs = None

    def _refresh(self, rec, g):
        p, gi = rec[0], rec[1]
        if p.dtype != torch.float32:
            raise TypeError(f"AdamW: params: expected torch.float32, got {p.dtype}")
        if g.dtype != torch.float32:
            raise TypeError(f"AdamW: grad: expected torch.float32, got {g.dtype}")
        if not p.is_contiguous():
            raise RuntimeError("AdamW: params: expected contiguous parameters")
        if not p.is_cuda:
            raise RuntimeError(f"AdamW: params: expected GPU tensors (the HIP path has no CPU fallback), got {p.device}")
        if self._device is None:
            self._device = p.device
        device = self._device
        if p.device != device or g.device != device:
            raise RuntimeError(f"AdamW: params: parameters and gradients must be on one device, got {device} and {p.device} / {g.device}")
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
        for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
            if t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or t.numel() != p.numel():
                raise RuntimeError(f"AdamW: state[{name!r}]: expected a contiguous fp32 tensor of the parameter's size on {device}")
        rec[2:6] = m, v, step, p.data_ptr()
        self._static[rec[6]] = (rec[5], 0, m.data_ptr(), v.data_ptr(), step.data_ptr(), p.numel(), gi)

    def _rows(self):
        """(table rows [n, 7] without the gradients' column, the gradients' addresses, the gradients) of the parameters this step updates"""
        for gi, group in enumerate(self.param_groups):
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name):
                    raise ValueError(f"AdamW: param_groups[{gi}]: {name}=True is not supported")
        recs = self._recs
        if recs is None or len(recs) != sum(len(group["params"]) for group in self.param_groups):
            recs = self._recs = [[p, gi, None, None, None, -1, 0] for gi, group in enumerate(self.param_groups) for p in group["params"]]
            for row, rec in enumerate(recs):
                rec[6] = row
            self._static = np.zeros((len(recs), _TENSOR_WORDS), np.int64)
        state, rows, g_ptrs, grads = self.state, [], [], []
        for rec in recs:
            p = rec[0]
            g = p.grad
            if g is None or not p.requires_grad:
                continue
            if g.is_sparse:
                raise RuntimeError("AdamW: grad: sparse gradients are not supported")
            if not g.is_contiguous():
                g = g.contiguous()   # (freed after the call: the allocator reuses it for later work of this stream only)
            st = state.get(p)
            if (st is None or p.data_ptr() != rec[5] or st.get("exp_avg") is not rec[2] or st.get("exp_avg_sq") is not rec[3]
                    or st.get("step") is not rec[4]):
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

    @torch.no_grad()
    def step(self, closure=None):
        loss, self.last_found_inf = None, None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        table, g_ptrs, grads = self._rows()
        if not g_ptrs:
            return loss
        device = self._device
        for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.numel() == 1 and t.dtype == torch.float32):
                    raise TypeError(f"AdamW: {name}: expected an fp32 tensor of one element")
                if t.device != device:
                    raise RuntimeError(f"AdamW: {name}: is on {t.device}, the parameters on {device}")
        n_t, n_g = len(g_ptrs), len(self.param_groups)
        words = n_t * _TENSOR_WORDS + n_g * _GROUP_WORDS
        slot = self._slot(8 * words)
        rows = slot.words[:n_t * _TENSOR_WORDS].reshape(n_t, _TENSOR_WORDS)
        rows[:] = table
        rows[:, 1] = g_ptrs
        slot.words[n_t * _TENSOR_WORDS:words].view(np.float64).reshape(n_g, _GROUP_WORDS)[:] = [
            (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in self.param_groups]
        need = _lib.lib().pointops2_optim_workspace_bytes(n_t, n_g)
        if self._workspace is None or self._workspace.device != device or self._workspace.numel() < need:
            self._workspace = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=device)
        if found_inf is None:
            if self._flag is None or self._flag.device != device:
                self._flag = torch.zeros((), dtype=torch.float32, device=device)
            flag, run_check = self._flag, 1
        else:
            flag, run_check = found_inf, 0
        _lib.call("optim_adamw_step_launcher", n_t, n_g, slot.buf.data_ptr(), _lib.ptr(self._workspace), self._workspace.numel(),
                  _lib.ptr(grad_scale), _lib.ptr(flag), run_check, device=device)
        if slot.event is None:
            slot.event = torch.cuda.Event()
        slot.event.record(torch.cuda.current_stream(device))
        self.last_found_inf = flag
        return loss


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler; step() alone differs, and only for an optim.AdamW whose gradients are still scaled (no unscale_() since the
    last update()): the optimizer's one call checks, unscales and updates, and its found_inf is what update() then reads on the device."""

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled or not isinstance(optimizer, AdamW):
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
