"""The parameter update of the three training programs as one launch (csrc/optim.hip), two with gradient-norm clipping:

    from recon_amd.optim import SGD, Adam
    opt = SGD(model.parameters(), lr=args.lr)                                     # stage A, GAT/main.py:445-449
    opt = Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)    # ConvKB, GAT/main.py:747-751
    opt = Adam(model.parameters(), lr=lr, weight_decay=wd, max_grad_norm=clip)    # stage B, train.py:234 + :314-315
    loss.backward(); opt.step()

Both are torch.optim.Optimizer subclasses: zero_grad, add_param_group, state_dict, load_state_dict and every lr scheduler are the base
class's, `lr` (and every other hyper-parameter) is read from param_groups at each step.  The arithmetic is torch.optim.SGD's without
momentum and torch.optim.Adam's with L2 weight decay (not AdamW, no amsgrad); Adam's state is torch's (per parameter: `step`, a 0-d CPU
float tensor, `exp_avg`, `exp_avg_sq`), so a state_dict written by either optimizer loads into the other.

max_grad_norm=c fuses `clip_grad_norm_(parameters, c); opt.step()`: one launch leaves the norm over the gradients of ALL groups and the
scale min(1, c / (norm + 1e-6)) on the device, the update launch reads the scale.  One deviation: p.grad keeps its UNCLIPPED values.
`opt.last_grad_norm` is the 0-d device tensor holding the norm (what clip_grad_norm_ returns); nothing here ever synchronises on it.

Parameters are fp32, contiguous GPU tensors on one device (checked at construction).  A parameter without a gradient is left alone (its
Adam step does not advance), a frozen one is ignored, a sparse gradient raises; a gradient that is not contiguous fp32 is copied first.
Once the state exists step() allocates no tensor and issues no torch op: segment lists go to the library as host arrays of pointers.
DESIGN.md section 17.
"""
import ctypes as C

import torch

from . import _lib

__all__ = ["SGD", "Adam"]


def _refuse(name, unsupported):
    if unsupported:
        raise TypeError("recon_amd.optim.%s does not implement %s" % (name, ", ".join(sorted(unsupported))))


class _MultiTensor(torch.optim.Optimizer):
    """What SGD and Adam share: the checks, the global gradient norm, and the host arrays the segment lists travel in."""

    def __init__(self, params, defaults, max_grad_norm):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("Invalid max_grad_norm: %r" % (max_grad_norm,))
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._ws, self._checked, self._cap, self._device = None, set(), 0, None
        self._check_params()
        self._chunk = _lib.lib().recon_optim_chunk_elems()
        if self.max_grad_norm is not None:
            ps = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
            self._workspace(sum(p.numel() for p in ps), len(ps), ps[0].device if ps else None)

    def _check(self, p):
        """A parameter the kernels will write: fp32, contiguous, on the GPU of the others."""
        _lib.require_gpu(p, dtype=torch.float32)
        if not p.is_contiguous():
            raise ValueError("recon_amd.optim: parameters must be contiguous, got strides %s for shape %s" % (p.stride(), tuple(p.shape)))
        if self._device is None:
            self._device = p.device
        elif p.device != self._device:
            raise ValueError("recon_amd.optim: all parameters must be on one device, got %s and %s" % (self._device, p.device))
        self._checked.add(id(p))

    def _check_params(self):
        """Every trainable parameter at construction (a frozen one is ignored; whatever turns up with a gradient later — a group added,
        a parameter unfrozen — is checked at its first step)."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad and id(p) not in self._checked:
                    self._check(p)

    def _arrays(self, n):
        """Host arrays for n segments: [0] parameters [1] gradients [2], [3] state, numel — reused by every launch (the library reads them
        during the call), grown when a group is added."""
        if n > self._cap:
            self._cap = n
            self._ptrs = [(C.c_void_p * n)() for _ in range(4)]
            self._numel = (C.c_int64 * n)()
            self._all_g, self._all_n = (C.c_void_p * n)(), (C.c_int64 * n)()
        return self._ptrs, self._numel

    def _workspace(self, total, n, dev):
        need = 16 + (total // self._chunk + n) * 8                       # recon_optim_workspace_bytes(total, n)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device=dev)     # zero-filled: the kernel's arrival counter
            self.last_grad_norm = self._ws[0]
        return self._ws

    @staticmethod
    def _dense32(g):
        if g.is_sparse:
            raise RuntimeError("recon_amd.optim does not support sparse gradients")
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()                          # the rare path: one more launch
        return g

    def _collect(self):
        """[(group, [(parameter, gradient as the kernels read it), ...]), ...] over the parameters that have a gradient."""
        work, checked = [], self._checked
        for group in self.param_groups:
            act = []
            for p in group["params"]:
                g = p.grad
                if g is None or not p.requires_grad:
                    continue
                if id(p) not in checked:
                    self._check(p)
                act.append((p, self._dense32(g)))
            if act:
                work.append((group, act))
        return work

    def _clip_scale(self, L, work, stream):
        """Launches the norm over every gradient of `work`; returns the device address of the scale (None: no clipping)."""
        if self.max_grad_norm is None:
            return None
        n = sum(len(act) for _, act in work)
        self._arrays(n)
        G, N, k, total = self._all_g, self._all_n, 0, 0
        for _, act in work:
            for p, g in act:
                G[k], N[k] = g.data_ptr(), p.numel()
                total += N[k]
                k += 1
        ws = self._workspace(total, n, self._device)
        _lib.check(L.recon_optim_grad_sumsq(G, N, n, self.max_grad_norm, ws.data_ptr(), ws.numel() * 4, stream), "recon_optim_grad_sumsq")
        return ws.data_ptr() + 4

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = self._collect()
        if not work:
            if self.last_grad_norm is not None:
                self.last_grad_norm.zero_()                               # clip_grad_norm_ over no gradient returns 0
            return loss
        L = _lib.lib()
        with _lib.on_device(self._device):
            stream = _lib.current_stream()
            scale = self._clip_scale(L, work, stream)
            for group, act in work:
                self._update(L, group, act, scale, stream)
        return loss


class SGD(_MultiTensor):
    """torch.optim.SGD(params, lr, weight_decay=weight_decay) without momentum, one launch per param group (module docstring)."""

    def __init__(self, params, lr, weight_decay=0, max_grad_norm=None, **unsupported):
        _refuse("SGD", unsupported)
        if not lr >= 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not weight_decay >= 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        super().__init__(params, {"lr": lr, "weight_decay": weight_decay}, max_grad_norm)

    def _update(self, L, group, act, scale, stream):
        if group.get("momentum") or group.get("nesterov") or group.get("maximize"):
            raise RuntimeError("recon_amd.optim.SGD does not implement momentum, nesterov or maximize (a loaded param group asks for one)")
        n = len(act)
        (P, G, _, _), N = self._arrays(n)
        for k, (p, g) in enumerate(act):
            P[k], G[k], N[k] = p.data_ptr(), g.data_ptr(), p.numel()
        _lib.check(L.recon_optim_sgd(P, G, N, n, float(group["lr"]), float(group["weight_decay"]), scale, stream), "recon_optim_sgd")


class Adam(_MultiTensor):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay), one launch per param group and distinct step count (module docstring)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, **unsupported):
        _refuse("Adam", unsupported)
        if not lr >= 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not eps >= 0.0:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not weight_decay >= 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        self._seen = {}                  # parameter -> (step tensor, its numpy view, exp_avg, exp_avg_sq) as last validated
        super().__init__(params, {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay}, max_grad_norm)

    def _init_state(self, fresh):
        """torch's state for the parameters that have none; exp_avg and exp_avg_sq are views of ONE zero-filled buffer, each at a multiple
        of four floats (16-byte aligned: the wide path of the kernel)."""
        offs, total = [], 0
        for p in fresh:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        flat = torch.zeros(2 * total, dtype=torch.float32, device=fresh[0].device)
        for p, o in zip(fresh, offs):
            st = self.state[p]
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = flat[o:o + p.numel()].view_as(p)
            st["exp_avg_sq"] = flat[total + o:total + o + p.numel()].view_as(p)

    def _validated(self, p, st):
        """State tensors as the kernel needs them, whoever put them there (load_state_dict): step on the CPU, moments fp32 and contiguous."""
        step, m, v = st["step"], st["exp_avg"], st["exp_avg_sq"]
        if not torch.is_tensor(step) or step.device.type != "cpu" or step.dtype != torch.float32 or step.dim() != 0:
            step = st["step"] = torch.tensor(float(step), dtype=torch.float32)
        for key, t in (("exp_avg", m), ("exp_avg_sq", v)):
            _lib.require_gpu(t)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape:
                st[key] = t.to(torch.float32).reshape(p.shape).contiguous()
        seen = self._seen[p] = (step, step.numpy(), st["exp_avg"], st["exp_avg_sq"])
        return seen

    def _update(self, L, group, act, scale, stream):
        if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
            raise RuntimeError("recon_amd.optim.Adam does not implement amsgrad, maximize or decoupled weight decay (a loaded param group asks for one)")
        state, seen_of = self.state, self._seen
        fresh = [p for p, _ in act if len(state[p]) == 0]
        if fresh:
            self._init_state(fresh)
        by_step = {}
        for p, g in act:
            st, seen = state[p], seen_of.get(p)
            if seen is None or seen[0] is not st["step"] or seen[2] is not st["exp_avg"] or seen[3] is not st["exp_avg_sq"]:
                seen = self._validated(p, st)
            count = seen[1]
            count += 1.0                                                  # in place, through the numpy view: the CPU tensor advances without a torch op
            by_step.setdefault(float(count), []).append((p, g, seen[2], seen[3]))
        lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        for t, items in by_step.items():
            n = len(items)
            (P, G, M, V), N = self._arrays(n)
            for k, (p, g, m, v) in enumerate(items):
                P[k], G[k], M[k], V[k], N[k] = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            _lib.check(L.recon_optim_adam(P, G, M, V, N, n, lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t, scale, stream), "recon_optim_adam")
