"""The optimizer of the train step on libvsr_hip_opt.so (include/vsr_hip_opt.h states the arithmetic operation by operation):
`Adam`, a `torch.optim.Optimizer` whose `state_dict` interchanges with `torch.optim.Adam`'s, with an optional clip of the global
gradient norm that never leaves the device.

    opt = Adam(model.parameters(), lr=1e-3, max_grad_norm=1.0)
    loss.backward(); opt.step()

One library call (one kernel launch) updates every tensor of a parameter group (one per distinct `step` value: normally one); with
`max_grad_norm` one more call (two launches) first takes the norm over every parameter that has a gradient and leaves the coefficient
on the device, where the update reads it.  `launches` counts the KERNEL LAUNCHES of the last `step()`: 1, or 3 with `max_grad_norm`
(2 + one per group and distinct `step` value in general).
`.grad` is never modified (torch.nn.utils.clip_grad_norm_ scales it in place; this step scales the value it reads).  The kernels write
through raw pointers, so after the launches `step()` moves the version counter of every tensor they wrote (`mark_updated`: the parameter,
`exp_avg`, `exp_avg_sq`; on the host), as an in-place operator would: the inference kernels read packed copies keyed by it.  There is no
fallback: a CPU, non-float32, non-contiguous or sparse parameter or gradient raises `VsrHipError`, and so do the variants the
kernels do not implement (amsgrad, maximize, capturable, differentiable, decoupled_weight_decay).

`step()` never synchronises the device.  The tensor table of a launch (a plan: pointers and sizes) is built on the host, cached by
the stream, the pointers and the sizes it holds, and uploaded only when they change, from one of two pinned staging buffers with a non-blocking
copy on the current stream; an event per buffer guards its reuse (the host waits on that event only).  The stream is part
of the cache key: a `step()` on another stream builds and uploads a plan (and a norm workspace) of its own, ordered on that stream."""
from __future__ import annotations

import collections
import ctypes
import math

import torch

from . import _lib
from ._lib import VsrHipError

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")
_PLANS_KEPT = 8   # plans cached per optimizer (a step uses one, or one per group plus the norm's)


def _stock_defaults() -> dict:
    """The group keys and defaults of the installed torch.optim.Adam (they grow with the torch version)."""
    return dict(torch.optim.Adam([torch.zeros(1)]).defaults)


def adam_scalars(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, t: float) -> tuple:
    """The seven float32 scalars of vsr_opt_adam_f32, formed in float64 (Python floats) and rounded once at the call:
    (omb1, b2, omb2, step_size, rs, eps, wd)."""
    return (1.0 - beta1, beta2, 1.0 - beta2, lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), eps, weight_decay)


def mark_updated(tensors) -> None:
    """Tell torch that `tensors` were written through their raw pointers: their version counters move, as after an in-place operator.
    Every packed copy of the weights (the SR net's pack, the trunk executors, the graphs of GraphedVSR) is keyed by (address, version),
    so a write that leaves the version alone would leave those copies stale.  Host only: no launch, no synchronisation, no value read or
    written; under no_grad it takes leaves that require grad."""
    with torch.no_grad():
        for t in tensors:
            torch._C._increment_version(t)


class _Plan:
    __slots__ = ("host", "dev", "bytes", "n_chunks", "ws")

    def __init__(self, host, dev, nbytes, n_chunks):
        self.host, self.dev, self.bytes, self.n_chunks, self.ws = host, dev, nbytes, n_chunks, None


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr must be a number (a tensor lr would be read back from its device at every step)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        defaults = _stock_defaults()
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._reset_buffers()

    # ------------------------------------------------------------------ what is not state: dropped by pickling, rebuilt on demand
    def _reset_buffers(self):
        self.launches = 0               # kernel launches the last step() enqueued (the norm's call makes two, each update one)
        self.last_grad_norm_sq = None   # device float64 (0-dim), written by the last clipped step(); never synchronised here
        self._plans = collections.OrderedDict()   # key (pointers and sizes) -> _Plan
        self._pin = [None, None]        # pinned staging buffers (uint8)
        self._pin_ev = [None, None]     # per buffer: its last upload has finished
        self._pin_next = 0
        self._ctl = None                # device vsr_opt_ctl_t as two float64 ({c, pad}, sumsq)

    def __getstate__(self):
        state = super().__getstate__()
        for k in ("launches", "last_grad_norm_sq", "_plans", "_pin", "_pin_ev", "_pin_next", "_ctl"):
            state.pop(k, None)
        state["max_grad_norm"] = self.max_grad_norm
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self._reset_buffers()

    # ------------------------------------------------------------------ plans
    def _upload(self, host, nbytes: int, device) -> torch.Tensor:
        a = self._pin_next
        self._pin_next = 1 - a
        if self._pin_ev[a] is not None:
            self._pin_ev[a].synchronize()   # the staging buffer is free again (host wait on one event)
        if self._pin[a] is None or self._pin[a].numel() < nbytes:
            self._pin[a] = torch.empty(max(nbytes, 4096) * 2, dtype=torch.uint8, pin_memory=True)
        ctypes.memmove(self._pin[a].data_ptr(), host, nbytes)
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(self._pin[a][:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._pin_ev[a] = ev
        return dev

    def _plan(self, entries) -> _Plan:
        """The plan of `entries` = [(p, g, m, v), ...]: cached by the pointers and sizes it holds, built and uploaded on a miss."""
        device = entries[0][0].device
        # (the stream leads the key: the upload, the launches that read the plan and the norm's workspace are ordered on one stream)
        table_key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, g, m, v in entries)
        key = (_lib.raw_stream(device.index), table_key)
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        L = _lib.load_opt()
        n = len(table_key)
        sizes = (ctypes.c_ulonglong * n)(*(k[4] for k in table_key))
        nbytes = L.vsr_opt_plan_bytes(n, sizes)
        if nbytes == 0:
            _lib.check(-1, "opt_plan_bytes", lib=L)
        table = (_lib.OptTensor * n)(*(_lib.OptTensor(*k) for k in table_key))
        host = ctypes.create_string_buffer(nbytes)
        _lib.check(L.vsr_opt_plan_fill(host, nbytes, n, table), "opt_plan_fill", lib=L)
        plan = _Plan(host, self._upload(host, nbytes, device), nbytes, (nbytes - 32 - 40 * n) // 8)
        self._plans[key] = plan
        while len(self._plans) > _PLANS_KEPT:
            self._plans.popitem(last=False)
        return plan

    # ------------------------------------------------------------------ the step
    @staticmethod
    def _device_f32(t: torch.Tensor, what: str) -> None:
        if t.is_sparse or t.layout is not torch.strided:
            raise VsrHipError(f"{what} is sparse (the device path updates dense tensors only; no fallback exists)")
        if not t.is_cuda:
            raise VsrHipError(f"{what} is a CPU tensor (the update runs on the device; no CPU fallback exists)")
        if t.dtype != torch.float32:
            raise VsrHipError(f"{what}: expected torch.float32, got {t.dtype}")
        if not t.is_contiguous():
            raise VsrHipError(f"{what} must be contiguous")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.launches = 0
        batches = []   # (group, step value, [(p, g, m, v)])
        for gi, group in enumerate(self.param_groups):
            for flag in _UNSUPPORTED:
                if group.get(flag, False):
                    raise VsrHipError(f"param group {gi}: {flag}=True is not implemented by the device update (no fallback exists)")
            if isinstance(group["lr"], torch.Tensor):
                raise VsrHipError(f"param group {gi}: a tensor lr is not supported (it would be read back at every step)")
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._device_f32(p, "a parameter")
                self._device_f32(p.grad, "a gradient")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st = state["step"]
                if not isinstance(st, torch.Tensor):
                    st = state["step"] = torch.tensor(float(st), dtype=torch.float32)
                if st.is_cuda:
                    raise VsrHipError("state['step'] lives on the device (a capturable / fused state): it would be read back at every step")
                self._device_f32(state["exp_avg"], "state['exp_avg']")
                self._device_f32(state["exp_avg_sq"], "state['exp_avg_sq']")
                if state["exp_avg"].numel() != p.numel() or state["exp_avg_sq"].numel() != p.numel() or p.grad.numel() != p.numel():
                    raise VsrHipError("parameter, gradient and state differ in size")
                if p.numel() == 0:
                    continue
                by_step.setdefault(float(st) + 1.0, []).append((p, p.grad, state["exp_avg"], state["exp_avg_sq"]))
            batches += [(group, t, entries) for t, entries in by_step.items()]
        if not batches:
            return loss
        every = [e for _, _, entries in batches for e in entries]
        device = every[0][0].device
        if any(t.device != device for e in every for t in e):
            raise VsrHipError("parameters, gradients and state must live on one device")
        L = _lib.load_opt()
        with torch.cuda.device(device):
            stream = _lib.stream()
            ctl = None
            if self.max_grad_norm is not None:
                plan = self._plan(every)
                if self._ctl is None or self._ctl.device != device:
                    self._ctl = torch.empty(2, dtype=torch.float64, device=device)
                if plan.ws is None:
                    plan.ws = torch.empty(plan.n_chunks, dtype=torch.float64, device=device)
                _lib.check(L.vsr_opt_grad_norm(plan.host, plan.dev.data_ptr(), self.max_grad_norm, self._ctl.data_ptr(),
                                               plan.ws.data_ptr(), stream), "opt_grad_norm", lib=L)
                self.launches += 2
                self.last_grad_norm_sq = self._ctl[1]
                ctl = self._ctl.data_ptr()
            for group, t, entries in batches:
                plan = self._plan(entries)
                b1, b2 = group["betas"]
                sc = adam_scalars(float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), t)
                _lib.check(L.vsr_opt_adam_f32(plan.host, plan.dev.data_ptr(), ctl, *sc, stream), "opt_adam_f32", lib=L)
                self.launches += 1
                for p, _, _, _ in entries:
                    self.state[p]["step"] += 1
        # the kernel wrote p, exp_avg and exp_avg_sq behind torch's back (a parameter without a gradient was not touched: it keeps its version)
        mark_updated(t for p, _, m, v in every for t in (p, m, v))
        return loss
