"""EWC / PI / RW: the weight-space regularisers of the reference's other baselines (utils/regularizer.py), on one HIP launch.

Interface of the reference: ``get_regularizer(model, model_old, device, opts, old_state)`` and the classes :class:`EWC`,
:class:`PI`, :class:`RW` with ``update()``, ``penalty()``, ``state_dict()`` and ``load_state_dict()``.  The reference's
iteration (train.py:139-145) calls ``update()`` after the first backward, back-propagates ``reg_importance * penalty()`` a
second time and synchronises with the host (``if l_reg != 0.``); PI and RW also copy the whole model to the host on every
update.  None of that fits a captured step on the gradient buckets of ``ucd_amd.ddp``, so the train step calls :meth:`step`
instead: on a GPU one ``ucd_reg_step`` (csrc/reg.hip) updates the state, adds the penalty's gradient analytically to the
reduced gradients and leaves ``reg_importance * penalty`` in a device scalar; the update counter that decides PI's and RW's
"first update" and RW's "every ``iterations`` updates" lives in device memory, so a replayed graph advances it.

``update()`` / ``penalty()`` / :meth:`add_penalty_grad` are the plain-torch twin of the same arithmetic, op for op the
reference's: the path on CPU devices (``use_kernel=False``) and the comparison of the GPU tests.

Names: state dictionaries are keyed by the student's ``named_parameters()`` names; the student is wrapped in
``ucd_amd.ddp.DistributedDataParallel`` (``module.`` keys) like the reference's, the teacher is not (the reference wraps both,
run.py:199,204).  Keys of a loaded state and of the teacher are matched with the ``module.`` prefix stripped, so a
``trainer_state`` written by the reference loads here and one written here loads in the reference.

Ranks: the reference updates the state on rank 0 only, from the already averaged gradient.  Here every rank runs the same
launch on the same reduced buckets, so every rank holds rank 0's state.
"""
from __future__ import annotations

import ctypes as C
import warnings

import torch

from . import hip

EPS = 1e-8
METHODS = {"ewc": 0, "pi": 1, "rw": 2}          # UCD_REG_EWC / UCD_REG_PI / UCD_REG_RW


class _RegTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("p_old", C.c_void_p), ("omega", C.c_void_p),
                ("fisher", C.c_void_p), ("score", C.c_void_p), ("temp", C.c_void_p), ("n", C.c_longlong),
                ("penalize", C.c_int), ("pad", C.c_int)]


class _RegHyper(C.Structure):
    _fields_ = [("reg_importance", C.c_double), ("alpha", C.c_float), ("one_minus_alpha", C.c_float),
                ("lambda_f", C.c_float), ("iterations", C.c_int), ("counter", C.c_int), ("pad", C.c_int)]


def normalize_fn(mat):
    return (mat - mat.min()) / (mat.max() - mat.min() + EPS)


def _strip(key):
    return key[len("module."):] if key.startswith("module.") else key


def get_regularizer(model, model_old, device, opts, old_state, use_kernel=None):
    name = opts.regularizer
    resume = old_state is not None
    if resume and name != old_state["name"]:
        warnings.warn(f"the regularizer passed ({name}) differs from the state's ({old_state['name']})")
    if name is None:
        return None
    kw = dict(reg_importance=opts.reg_importance, normalize=not opts.reg_no_normalize, use_kernel=use_kernel)
    if name == "ewc":
        return EWC(model, model_old, device, fisher=old_state["fisher"] if resume else None, alpha=opts.reg_alpha, **kw)
    if name == "pi":
        return PI(model, model_old, device, score=old_state["score"] if resume else None, **kw)
    if name == "rw":
        return RW(model, model_old, device, score=old_state["score"] if resume else None,
                  fisher=old_state["fisher"] if resume else None, alpha=opts.reg_alpha, iterations=opts.reg_iterations, **kw)
    raise NotImplementedError(name)


class _Plan:
    __slots__ = ("signature", "table", "blocks", "n_blocks", "partials", "elements")


class _Regularizer:
    name = None
    bytes_per_element = 0.0

    def __init__(self, model, model_old, device, reg_importance=1.0, alpha=0.9, iterations=1, normalize=True,
                 use_kernel=None):
        self.model, self.device = model, torch.device(device)
        self.reg_importance, self.alpha, self.iterations, self.normalize = float(reg_importance), alpha, iterations, normalize
        self.use_kernel = self.device.type == "cuda" if use_kernel is None else bool(use_kernel)
        self.params = dict(model.named_parameters())
        self._by_stripped = {_strip(n): n for n in self.params}
        self.penalize = model_old is not None
        # theta_old: the teacher's parameter storage itself (a copy only where its layout differs from the student's); at
        # step 0 a copy of the initial parameters (deepcopy(model.state_dict()), regularizer.py:147,228)
        self.old = {}
        if model_old is not None:
            old_sd = {_strip(k): v for k, v in model_old.state_dict().items()}
            for n, p in self.params.items():
                if _strip(n) in old_sd:
                    self.old[n] = self._like(p, old_sd[_strip(n)], share=True)
        self.count = 0                  # the twin's update counter (the kernel's lives in self._hyper_dev)
        self._plan = None
        self._hyper_dev = None
        self._penalty = None

    # -- helpers ---------------------------------------------------------------------------------------------------------
    def _name(self, key):
        return self._by_stripped.get(_strip(key), key)

    def _like(self, p, src=None, fill=None, share=False):
        """A state tensor laid out like parameter ``p`` (reference checkpoints hold contiguous NCHW tensors)."""
        from .optim import _same_layout
        if share and src is not None and src.device == self.device and src.dtype == torch.float32 and _same_layout(src, p):
            return src
        t = torch.empty_like(p, device=self.device, dtype=torch.float32, requires_grad=False)
        if src is not None:
            t.copy_(src.detach())
        else:
            t.fill_(fill)
        return t

    def _load_dict(self, src, normalize=False):
        """{key: tensor} of a loaded state -> {student name: device tensor laid out like its parameter}."""
        out = {}
        for k, v in src.items():
            n = self._name(k)
            v = v.detach().to(self.device)
            if normalize:
                v = normalize_fn(v)
            out[n] = self._like(self.params[n], v) if n in self.params and self.params[n].shape == v.shape else v.clone()
        return out

    def _invalidate(self):
        """After load_state_dict: the kernel's tables and hyper-parameters are rebuilt at the next step (the run loads right
        after construction, before any update, so the device counter restarts at 0 like the reference's fresh objects)."""
        self._plan = None
        self._hyper_dev = None
        self.count = 0

    def _snapshot(self):
        return {n: p.detach().clone() for n, p in self.params.items()}

    # per method: which entries are penalised, their omega, and the state slots of the kernel table
    def _penalized(self, n):
        return self.penalize and n in self.old and self.params[n].requires_grad

    def _omega(self, n):
        raise NotImplementedError

    def _slots(self, n):
        """(fisher, score / delta, temp) tensors of parameter n for the kernel table (None: unused)."""
        raise NotImplementedError

    # -- the torch twin ---------------------------------------------------------------------------------------------------
    def penalty(self):
        if not self.penalize:
            return 0.
        loss = 0.
        for n, p in self.params.items():
            if self._penalized(n):
                loss += (self._omega(n) * (p.detach() - self.old[n]) ** 2).sum()
        return loss

    @torch.no_grad()
    def add_penalty_grad(self):
        """p.grad += the gradient autograd gives reg_importance * penalty(): (lambda * omega) * (2 * (p - p_old))."""
        for n, p in self.params.items():
            if self._penalized(n) and p.grad is not None:
                p.grad.add_((self.reg_importance * self._omega(n)) * (2 * (p - self.old[n])))

    # -- the fused step -------------------------------------------------------------------------------------------------
    def step(self):
        """update() + the penalty's gradient into p.grad; returns reg_importance * penalty as a 0-d tensor on the device."""
        if self.use_kernel:
            return self._kernel_step()
        self.update()
        pen = self.penalty()
        if not torch.is_tensor(pen):
            return torch.zeros((), device=self.device)
        self.add_penalty_grad()
        return self.reg_importance * pen

    def _signature(self):
        sig = []
        for p in self.params.values():
            sig.append(p.data_ptr())
            sig.append(0 if p.grad is None else p.grad.data_ptr())
        return sig

    def plan_is_current(self):
        """True when the next step() launches without rebuilding its tables (nothing may be built under graph capture)."""
        return not self.use_kernel or (self._plan is not None and self._plan.signature == self._signature())

    def _build_plan(self, signature):
        from .optim import _same_layout, block_table
        rows = []
        for n, p in self.params.items():
            g = p.grad
            if g is None:
                # no gradient (a frozen parameter): no update, no penalty.  The reference's EWC.update would raise TypeError
                # at `p.grad ** 2` here; PI and RW skip such parameters.
                continue
            if not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or not _same_layout(g, p):
                raise RuntimeError(f"ucd_amd.regularizer: parameter {n}: needs fp32 CUDA tensors with its gradient laid out "
                                   "like it (the kernel has no other path)")
            fisher, score, temp = self._slots(n)
            pen = self._penalized(n)
            old, omega = (self.old[n], self._omega(n)) if pen else (None, None)
            for t in (fisher, score, temp, old, omega):
                if t is not None and (not _same_layout(t, p) or t.dtype != torch.float32 or t.device != p.device):
                    raise RuntimeError(f"ucd_amd.regularizer: state of {n} is not laid out like the parameter")
            rows.append((p, g, old, omega, fisher, score, temp, pen))
        plan = _Plan()
        plan.signature = signature
        plan.elements = sum(r[0].numel() for r in rows)
        plan.n_blocks = 0
        plan.table = plan.blocks = plan.partials = None
        if not rows:
            return plan
        table = (_RegTensor * len(rows))()
        for e, (p, g, old, omega, fisher, score, temp, pen) in zip(table, rows):
            e.p, e.g, e.p_old, e.omega = p.data_ptr(), g.data_ptr(), hip.ptr(old), hip.ptr(omega)
            e.fisher, e.score, e.temp = hip.ptr(fisher), hip.ptr(score), hip.ptr(temp)
            e.n, e.penalize = p.numel(), 1 if pen else 0
        blocks = block_table([r[0].numel() for r in rows], hip.load().ucd_reg_chunk())
        plan.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        plan.blocks = torch.from_numpy(blocks).to(self.device)
        plan.n_blocks = int(blocks.shape[0])
        plan.partials = torch.empty(plan.n_blocks, dtype=torch.float64, device=self.device)
        return plan

    def _init_device(self):
        hyper = _RegHyper()
        hyper.reg_importance = self.reg_importance
        # the float32 values torch casts the Python doubles to in `alpha * t`, `(1 - alpha) * t`, `reg_importance * t`
        hyper.alpha = float(torch.tensor(self.alpha, dtype=torch.float32))
        hyper.one_minus_alpha = float(torch.tensor(1 - self.alpha, dtype=torch.float32))
        hyper.lambda_f = float(torch.tensor(self.reg_importance, dtype=torch.float32))
        hyper.iterations, hyper.counter = int(self.iterations), 0
        self._hyper_dev = torch.zeros(C.sizeof(_RegHyper), dtype=torch.uint8, device=self.device)
        self._penalty = torch.zeros((), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            hip._check(hip.load().ucd_reg_hyper_store(self._hyper_dev.data_ptr(), C.byref(hyper), hip.stream()),
                       "ucd_reg_hyper_store")

    def device_counter(self):
        """The kernel's update counter (host read: synchronises)."""
        if self._hyper_dev is None:
            return 0
        off = _RegHyper.counter.offset
        return int(self._hyper_dev[off:off + 4].view(torch.int32).item())

    def _kernel_step(self):
        signature = self._signature()
        plan = self._plan
        if plan is None or plan.signature != signature:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ucd_amd.regularizer step under graph capture: parameters or gradients moved since the "
                                   "last eager step")
            if self._hyper_dev is None:
                self._init_device()
            plan = self._plan = self._build_plan(signature)
        if plan.n_blocks:
            with torch.cuda.device(self.device):
                with hip._timed("ucd_reg_step", self.bytes_per_element * plan.elements):
                    hip._check(hip.load().ucd_reg_step(plan.table.data_ptr(), plan.blocks.data_ptr(), plan.n_blocks,
                                                       METHODS[self.name], self._hyper_dev.data_ptr(),
                                                       plan.partials.data_ptr(), self._penalty.data_ptr(), hip.stream()),
                               "ucd_reg_step")
        return self._penalty


class EWC(_Regularizer):
    name = "ewc"
    bytes_per_element = 28.0

    def __init__(self, model, model_old, device, fisher=None, alpha=0.9, normalize=True, reg_importance=1.0, use_kernel=None):
        super().__init__(model, model_old, device, reg_importance=reg_importance, alpha=alpha, normalize=normalize,
                         use_kernel=use_kernel)
        if fisher is not None:
            self.fisher_old = self._load_dict(fisher, normalize=normalize)
            self.fisher = self._load_dict(fisher)                           # un-normalised clone
        else:                                                               # no previous Fisher matrix: nothing to penalise
            self.fisher_old = None
            self.penalize = False
            self.fisher = {}
        for n, p in self.params.items():                                    # keys of the new classes
            if p.requires_grad and n not in self.fisher:
                self.fisher[n] = self._like(p, fill=1.0)

    def _omega(self, n):
        return self.fisher_old[n]

    def _slots(self, n):
        return self.fisher[n], None, None

    @torch.no_grad()
    def update(self):
        for n, p in self.params.items():
            if p.grad is None:          # the reference raises TypeError at `p.grad ** 2`; a frozen parameter has no gradient
                continue
            self.fisher[n].copy_((self.alpha * (p.grad ** 2)) + ((1 - self.alpha) * self.fisher[n]))
        self.count += 1

    def get(self):
        return self.fisher

    def state_dict(self):
        return {"name": "ewc", "fisher": self.fisher, "alpha": self.alpha}

    def load_state_dict(self, state):
        assert state["name"] == "ewc", f"Error, you are trying to restore {state['name']} into ewc"
        self.fisher = self._load_dict(state["fisher"])
        self.alpha = state["alpha"]
        self._invalidate()


class PI(_Regularizer):
    name = "pi"
    bytes_per_element = 36.0

    def __init__(self, model, model_old, device, score=None, normalize=False, reg_importance=1.0, use_kernel=None):
        super().__init__(model, model_old, device, reg_importance=reg_importance, normalize=normalize, use_kernel=use_kernel)
        self.starting_new = {}
        if model_old is not None:
            for n, p in self.params.items():          # keys the teacher lacks: penalised against their starting value
                if n not in self.old:
                    self.starting_new[n] = p.detach().clone().cpu()
                    self.old[n] = self._like(p, p)
        else:
            self.old = self._snapshot()
        if score is not None:
            self.score = {self._name(k): v for k, v in score.items()}
            self.score_actual = self._load_dict(score, normalize=normalize)
        else:
            self.score = None
            self.penalize = False
            self.score_actual = {}
        self.delta = {n: self._like(p, fill=0.0) for n, p in self.params.items()}
        self.temp = {n: self._like(p, fill=0.0) for n, p in self.params.items() if p.requires_grad}

    def _penalized(self, n):
        return self.penalize and n in self.score_actual and self.params[n].requires_grad

    def _omega(self, n):
        return self.score_actual[n]

    def _slots(self, n):
        return None, self.delta[n], self.temp[n]

    @torch.no_grad()
    def update(self):
        if self.count > 0:
            for n, p in self.params.items():
                if p.grad is not None:
                    self.delta[n] += p.grad * (self.temp[n] - p)
        for n, p in self.params.items():
            if p.grad is not None:
                self.temp[n].copy_(p)
        self.count += 1

    @torch.no_grad()
    def get(self):
        score = {}
        for n, p in self.params.items():
            s = self.delta[n] / ((p.detach() - self.old[n]).pow(2) + 1e-20)
            s = torch.where(s > 0, s, torch.tensor(0.).to(s.device))
            if self.score is not None and n in self.score:
                s = self.score[n].to(s.device) + s
            score[n] = s
        return score

    def state_dict(self):
        return {"name": "pi", "score": self.get(), "delta": self.delta, "starting_model": self.starting_new}

    def load_state_dict(self, state):
        assert state["name"] == "pi", f"Error, you are trying to restore {state['name']} into pi"
        self.delta = self._load_dict(state["delta"])
        for k, p in state["starting_model"].items():
            n = self._name(k)
            self.old[n] = self._like(self.params[n], p.to(self.device)) if n in self.params else p.to(self.device)
        self._invalidate()


class RW(_Regularizer):
    name = "rw"
    bytes_per_element = 44.0

    def __init__(self, model, model_old, device, score=None, fisher=None, alpha=0.9, iterations=10, normalize=True,
                 reg_importance=1.0, use_kernel=None):
        super().__init__(model, model_old, device, reg_importance=reg_importance, alpha=alpha, iterations=iterations,
                         normalize=normalize, use_kernel=use_kernel)
        if model_old is None:
            self.old = self._snapshot()
        if fisher is not None and score is not None:
            self.score_plus_fisher = self._load_dict(fisher, normalize=normalize)
            self.fisher = self._load_dict(fisher)
            self.score_old = {self._name(k): v for k, v in score.items()}
            for n, v in self._load_dict(score, normalize=normalize).items():
                self.score_plus_fisher[n] += v
        else:
            self.penalize = False
            self.score_old = None
            self.score_plus_fisher = {}
            self.fisher = {}
        self.score = {n: self._like(p, fill=0.0) for n, p in self.params.items() if p.requires_grad}
        self.temp = {n: self._like(p, fill=0.0) for n, p in self.params.items() if p.requires_grad}
        for n, p in self.params.items():
            if p.requires_grad and n not in self.fisher:
                self.fisher[n] = self._like(p, fill=1.0)

    def _omega(self, n):
        return self.score_plus_fisher[n]

    def _slots(self, n):
        return self.fisher[n], self.score[n], self.temp[n]

    @torch.no_grad()
    def update(self):
        if self.count % self.iterations == 0:
            if self.count > 0:
                for n, p in self.params.items():
                    if p.grad is not None:
                        delta = p.grad * (self.temp[n] - p)
                        den = 0.5 * self.fisher[n] * (p - self.temp[n]).pow(2) + EPS
                        self.score[n] += (delta / den)
            for n, p in self.params.items():
                if p.grad is not None:
                    self.temp[n].copy_(p)
        self.count += 1
        for n, p in self.params.items():
            if p.grad is not None:
                self.fisher[n].copy_((self.alpha * p.grad.pow(2)) + ((1 - self.alpha) * self.fisher[n]))

    @torch.no_grad()
    def get_score(self):
        score = {}
        for n, p in self.score.items():
            s = torch.where(p >= 0, p, torch.tensor(0.).to(p.device))
            if self.score_old is not None and n in self.score_old:
                s = 0.5 * (s + self.score_old[n].to(p.device))
            score[n] = s
        return score

    def state_dict(self):
        return {"name": "rw", "score": self.get_score(), "fisher": self.fisher, "iteration": self.iterations,
                "alpha": self.alpha}

    def load_state_dict(self, state):
        assert state["name"] == "rw", f"Error, you are trying to restore {state['name']} into rw"
        self.iterations = state["iteration"]
        self.alpha = state["alpha"]
        self.fisher = self._load_dict(state["fisher"])
        self.score = self._load_dict(state["score"])
        self._invalidate()
