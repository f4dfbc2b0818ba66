"""``torch.optim.Adam`` with its step as one kernel launch (``reart_adam_groups``, csrc/adam.hip).

``Adam`` is a drop-in for the host loops (``run_robot.OperatorLoop --fused_adam``, ``ik_single(fused_adam=True)``, a user's own
loop): the constructor, ``param_groups``, the state keys (``step``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``) and therefore
``state_dict()`` / ``load_state_dict()`` are torch's; only ``step`` differs.  Where torch walks its groups in Python and issues a
chain of small kernels per group, ``step`` fills one table of per-tensor records on the host and passes it BY VALUE to one
launch for up to ``_lib.ADAM_MAX_TENSORS`` tensors: no device allocation, no copy of a pointer table, no synchronisation.

The native path needs, at the step: every parameter that has a gradient a contiguous float32 tensor on the current GPU with a
contiguous dense float32 gradient of its shape (and, where state exists already, moments laid out likewise); ``capturable``, ``differentiable``, ``fused`` and ``decoupled_weight_decay``
off in every group; ``lr``, the betas, ``eps`` and ``weight_decay`` Python numbers.  Otherwise the WHOLE step is torch's own
(host tensors, float64, non-contiguous or sparse gradients, a tensor-valued ``lr``, any of those switches): same bits as
``torch.optim.Adam``.  ``last_path`` tells which ran (``"native"`` / ``"torch"``), ``last_launches`` how many native calls the
step made (one per ``ADAM_MAX_TENSORS`` tensors that share betas and eps).
"""
import ctypes

import torch

from . import _lib


class AdamTensor(ctypes.Structure):
    """reart_adam_tensor of include/reart_hip.h."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("max_exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int),
                ("step_size", ctypes.c_float), ("bias_correction2_sqrt", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("maximize", ctypes.c_int)]


_SWITCHES = ("capturable", "differentiable", "fused", "decoupled_weight_decay")


class Adam(torch.optim.Adam):
    last_path = None
    last_launches = 0

    def _with_grad(self):
        """[(group, [parameters with a gradient])] if the native path takes this step, else None.  Nothing is modified."""
        out, device = [], None
        for group in self.param_groups:
            if any(group.get(k) for k in _SWITCHES):
                return None
            numbers = (group["lr"], group["eps"], group["weight_decay"]) + tuple(group["betas"])
            if not all(isinstance(x, (int, float)) for x in numbers):
                return None
            params = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and g.layout == torch.strided
                        and g.device == p.device and g.shape == p.shape and p.is_contiguous() and g.is_contiguous()
                        and p.numel() < 2 ** 31):
                    return None
                if device is None:
                    device = p.device
                    if device.index != torch.cuda.current_device():
                        return None
                elif p.device != device:
                    return None
                st = self.state.get(p)
                if st:                                       # state that was loaded or set by hand: the kernel indexes it like p
                    moments = [st.get(k) for k in (("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if group["amsgrad"] else ("exp_avg", "exp_avg_sq"))]
                    if not all(torch.is_tensor(t) and t.dtype == torch.float32 and t.device == p.device and t.shape == p.shape
                               and t.is_contiguous() for t in moments) or not torch.is_tensor(st.get("step")) or st["step"].is_cuda:
                        return None
                params.append(p)
            out.append((group, params))
        return out

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = self._with_grad()
        if work is None:
            self.last_path, self.last_launches = "torch", 0
            plain = torch.optim.Adam.step       # without the step hooks: they run around this method already
            if getattr(plain, "hooked", False):
                plain = plain.__wrapped__
            plain(self)
            return loss
        tables = self.__dict__.setdefault("_tables", {})     # (beta1, beta2, eps) -> [records, filled]
        try:
            launches = self._native_step(work, tables) if any(params for _, params in work) else 0
        finally:
            for table in tables.values():
                table[1] = 0
        self.last_path, self.last_launches = "native", launches
        return loss

    def _native_step(self, work, tables):
        fn, stream, cap = _lib.lib().reart_adam_groups, _lib.stream(), _lib.ADAM_MAX_TENSORS
        launches = 0
        for group, params in work:
            if not params:
                continue
            states = [self.state[p] for p in params]
            for p, st in zip(params, states):
                if len(st) == 0:                             # as torch.optim.Adam._init_group creates it for these options
                    st["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if group["amsgrad"]:
                        st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            torch._foreach_add_([st["step"] for st in states], 1)
            lr, (beta1, beta2), eps = group["lr"], group["betas"], group["eps"]
            wd, amsgrad, maximize = group["weight_decay"], group["amsgrad"], int(bool(group["maximize"]))
            key = (float(beta1), float(beta2), float(eps))
            table = tables.get(key)
            if table is None:
                table = tables[key] = [(AdamTensor * cap)(), 0]
            corrections = {}                                  # step -> (step size, sqrt of the second bias correction), in double
            for p, st in zip(params, states):
                step = st["step"].item()
                c = corrections.get(step)
                if c is None:
                    c = corrections[step] = (lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5)
                r = table[0][table[1]]
                r.param, r.grad, r.n = p.data_ptr(), p.grad.data_ptr(), p.numel()
                r.exp_avg, r.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                r.max_exp_avg_sq = st["max_exp_avg_sq"].data_ptr() if amsgrad else None
                r.step_size, r.bias_correction2_sqrt, r.weight_decay, r.maximize = c[0], c[1], wd, maximize
                table[1] += 1
                if table[1] == cap:
                    _lib.check(fn(table[0], cap, *key, stream), "reart_adam_groups")
                    table[1] = 0
                    launches += 1
        for key, table in tables.items():
            if table[1]:
                _lib.check(fn(table[0], table[1], *key, stream), "reart_adam_groups")
                table[1] = 0
                launches += 1
        return launches
