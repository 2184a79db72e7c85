"""`HipAdam`: gradient clipping, Adam and the EMA of the weights as one stream-ordered, capturable step of libns2hip
(include/ns2hip_optim.h, csrc/optim.hip).  Reference: what follows `accelerator.backward(loss)` in Trainer.train, NS2:1888-1901.

The step reads no device value on the host: the gradient norm, the clip coefficient, the decision to SKIP the step (a non-finite norm, or
a range counter of the mixed arithmetic that moved since `mark()`), the step count and Adam's bias corrections are computed on the device
and consumed by the update kernel, so `mark(); loss.backward(); step()` can be enqueued ahead or captured in a HIP graph
(`GraphedTrainStep(optimizer=)`).  It owns its parameter writes: nothing rewrites a parameter behind a version counter that some cache
trusts -- the weight packs are NOT touched, the next pass's one-launch repack reads the parameters' own storage."""
import ctypes

import torch

from .. import _lib

_C = _lib.ABI["ns2hip_optim.h"].constants
_ADAM_DEFAULTS = torch.optim.Adam([torch.zeros(1)]).defaults       # the keys a torch.optim.Adam param group has in this torch


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam (weight_decay 0, amsgrad off) + `clip_grad_norm_(params, max_grad_norm)` + an optional EMA of the parameters.

    One parameter group; fp32, contiguous parameters on one GPU.  Device tensors of one element each, valid in stream order and never
    read by the optimizer itself: `grad_norm` (the norm BEFORE clipping, what clip_grad_norm_ returns), `skipped` (int32: the last step
    wrote nothing), `steps_taken` (int32), and the two the caller may write between steps or graph replays, `lr` and `ema_decay`.
    (`param_groups[0]["lr"]` is pushed to `lr` by an eager `step()` whenever it changed, so torch's schedulers work on the eager path;
    under a graph write `optimizer.lr.fill_(...)`.)

    `mark()` snapshots the IEEE-half range counters on the device; a later `step()` is skipped if one of them moved -- the counterpart
    of `_Scale.overflowed()` / GradScaler's inf check without the host round trip.  Call it before the forward of a mixed-arithmetic pass.
    `bind(params, grads)` makes `step()` read the given gradient tensors (None: no gradient) instead of `.grad`.
    EMA: a CONSTANT decay by default, applied every `ema_update_every`-th step; `ema_decay` on the device is the hook for a schedule."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=None, ema=False, ema_decay=0.995, ema_update_every=10,
                 weight_decay=0, amsgrad=False, maximize=False):
        if not 0.0 <= lr:
            raise ValueError(f"HipAdam: invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"HipAdam: betas in [0, 1), got {betas}")
        if not 0.0 <= eps:
            raise ValueError(f"HipAdam: invalid eps {eps}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"HipAdam: max_grad_norm is positive or None, got {max_grad_norm}")
        if ema and not (0.0 <= ema_decay <= 1.0 and int(ema_update_every) >= 1):
            raise ValueError("HipAdam: ema_decay in [0, 1] and ema_update_every >= 1")
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError("HipAdam: one parameter group (the kernels take one set of hyperparameters)")
        defaults = dict(_ADAM_DEFAULTS, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("HipAdam: one parameter group (the kernels take one set of hyperparameters)")
        self.max_grad_norm = max_grad_norm
        self.use_ema, self.ema_update_every = bool(ema), int(ema_update_every)
        self._ema_decay0 = float(ema_decay)
        self._check_group()
        self._check_params()
        self._block = None          # the device state block (int32 words); grad_norm / skipped / steps_taken / lr / ema_decay are views
        self._m = self._v = self._ema = None
        self._table = None          # device table + what it was built from
        self._table_key = None
        self._table_grads = None    # the grad pointers the table holds
        self._bound = None          # (params, grads) of bind()
        self._lr_pushed = None
        self._pending_step = 0      # a step count loaded before the state block exists

    # ------------------------------------------------------------------------------------------------------------ refusals
    def _check_group(self):
        g = self.param_groups[0]
        for key, what in (("weight_decay", "weight decay (the kernels implement weight_decay = 0; AdamW / L2 are not covered)"),
                          ("amsgrad", "amsgrad (no max_exp_avg_sq buffer in the kernels)"),
                          ("maximize", "maximize (the kernels descend)")):
            if g.get(key):
                raise ValueError(f"HipAdam does not support {what}")

    def _check_params(self):
        for i, p in enumerate(self._params()):
            if p.dtype != torch.float32:
                raise ValueError(f"HipAdam: parameter {i} is {p.dtype}; the kernels update fp32 parameters only")
            if not p.is_contiguous():
                raise ValueError(f"HipAdam: parameter {i} is not contiguous; the kernels walk dense storage")

    def _params(self):
        return self.param_groups[0]["params"]

    # ------------------------------------------------------------------------------------------------------------ state
    @staticmethod
    def _like(p, fill=None):
        """a dense buffer of p's shape whose address modulo 16 is p's: the update kernel then moves 16 bytes per lane"""
        off = (p.data_ptr() % 16) // 4
        flat = torch.zeros(p.numel() + off, dtype=torch.float32, device=p.device)
        out = flat[off:].view(p.shape)
        if fill is not None:
            out.copy_(fill)
        return out

    def init_state(self):
        """allocate the moments (zeros), the EMA buffers (a copy of the parameters) and the device scalars where the parameters live now.
        Done by the first `step()` / `mark()` / `state_dict()` / `ema_parameters()`; parameters moved to another device afterwards need a new optimizer."""
        if self._block is not None:
            return
        self._check_params()
        ps = self._params()
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise ValueError("HipAdam: the parameters live on more than one device")
        with torch.no_grad():
            self._m = [self._like(p) for p in ps]
            self._v = [self._like(p) for p in ps]
            self._ema = [self._like(p, p.detach()) for p in ps] if self.use_ema else None
            self._block = torch.zeros(_C["NS2_OPTIM_STATE_WORDS"], dtype=torch.int32, device=dev)
        if dev.type == "cuda":
            with torch.cuda.device(dev):
                if torch.cuda.is_current_stream_capturing():
                    self._block = None
                    raise _lib.Ns2Error("HipAdam: the state is set up by a synchronising call; call init_state() before capturing a graph")
                _lib.check(_lib.load().ns2_optim_state_init(self._block.data_ptr(), self._pending_step, float(self.param_groups[0]["lr"]),
                                                            self._ema_decay0, torch.cuda.current_stream().cuda_stream), "ns2_optim_state_init")
        else:                                             # a CPU optimizer holds state (state_dict / load_state_dict work); step() refuses
            self._block[_C["NS2_OPTIM_W_STEP"]] = self._pending_step
            self._word("NS2_OPTIM_W_LR", torch.float32).fill_(float(self.param_groups[0]["lr"]))
            self._word("NS2_OPTIM_W_EMA_DECAY", torch.float32).fill_(self._ema_decay0)
        self._lr_pushed = float(self.param_groups[0]["lr"])
        self.grad_norm = self._word("NS2_OPTIM_W_GRAD_NORM", torch.float32)
        self.skipped = self._word("NS2_OPTIM_W_SKIP")
        self.steps_taken = self._word("NS2_OPTIM_W_STEP")
        self.lr = self._word("NS2_OPTIM_W_LR", torch.float32)
        self.ema_decay = self._word("NS2_OPTIM_W_EMA_DECAY", torch.float32)
        for p, m, v in zip(ps, self._m, self._v):
            self.state[p] = {"step": torch.tensor(float(self._pending_step)), "exp_avg": m, "exp_avg_sq": v}

    def _word(self, name, dtype=torch.int32):
        w = self._block[_C[name]:_C[name] + 1]
        return w if dtype == torch.int32 else w.view(dtype)

    def ema_parameters(self):
        """the EMA tensors, in parameter order (they start as a copy of the parameters)"""
        if not self.use_ema:
            raise ValueError("HipAdam: built with ema=False")
        self.init_state()
        return list(self._ema)

    def bind(self, params, grads):
        """read `grads[i]` (a dense fp32 tensor of params[i]'s shape, or None) as the gradient of `params[i]` from now on instead of
        `.grad`; `params` are this optimizer's parameters, in any order (those left out have no gradient).  `bind(None, None)` undoes it."""
        if params is None:
            self._bound = None
            return
        params, grads = list(params), list(grads)
        mine = {id(p) for p in self._params()}
        if len(params) != len(grads) or any(id(p) not in mine for p in params):
            raise ValueError("HipAdam.bind: one gradient (or None) per parameter, parameters of this optimizer")
        self._bound = {id(p): g for p, g in zip(params, grads)}

    def _grads(self):
        ps = self._params()
        gs = [p.grad for p in ps] if self._bound is None else [self._bound.get(id(p)) for p in ps]
        for i, (p, g) in enumerate(zip(ps, gs)):
            if g is None:
                continue
            if g.dtype != torch.float32 or g.shape != p.shape or not g.is_contiguous() or g.device != p.device or g.is_sparse:
                raise ValueError(f"HipAdam: the gradient of parameter {i} is not a dense contiguous fp32 tensor of its shape on its device")
        return gs

    # ------------------------------------------------------------------------------------------------------------ the device calls
    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _ensure_table(self, grads):
        lib = _lib.load()
        ps = self._params()
        key = tuple(p.data_ptr() for p in ps)
        gptr = [0 if g is None else g.data_ptr() for g in grads]
        if self._table is None or key != self._table_key:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.Ns2Error("HipAdam: the tensor table is built by a synchronising call; run prepare() (or one step) before capturing")
            n = len(ps)
            arr = (_lib.OptimTensor * max(n, 1))()
            for i, (p, m, v) in enumerate(zip(ps, self._m, self._v)):
                arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = p.data_ptr() or None, gptr[i] or None, m.data_ptr() or None, v.data_ptr() or None
                arr[i].ema = (self._ema[i].data_ptr() or None) if self._ema is not None else None
                arr[i].numel = p.numel()
            chunks = lib.ns2_optim_chunks(arr, n)
            if chunks < 0:
                _lib.check(int(chunks), "ns2_optim_chunks")
            nbytes = lib.ns2_optim_table_bytes(n, chunks)
            table = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=ps[0].device)
            _lib.check(lib.ns2_optim_table_build(arr, n, table.data_ptr(), table.numel(), self._stream()), "ns2_optim_table_build")
            self._table, self._table_key, self._table_grads, self._chunks = table, key, list(gptr), int(chunks)
        capturing = torch.cuda.is_current_stream_capturing()
        if gptr != self._table_grads or capturing:        # a backward pass that allocated its gradients anew: stream-ordered, capturable
            n, cap = len(ps), _C["NS2_OPTIM_GRADS_MAX"]
            for first in range(0, n, cap):
                part = gptr[first:first + cap]
                if part == self._table_grads[first:first + cap] and not capturing:     # (a graph carries every pointer: an eager step
                    continue                                                              # between replays may point the table anywhere)
                host = (ctypes.c_void_p * len(part))(*[g or None for g in part])
                _lib.check(lib.ns2_optim_set_grads(self._table.data_ptr(), n, first, len(part), host, self._stream()), "ns2_optim_set_grads")
            self._table_grads = list(gptr)

    def table_grads(self, ptrs=None):
        """the gradient addresses the device table holds, as this object believes; `GraphedTrainStep` sets them after a replay, whose
        captured launches rewrote the table behind this object's back"""
        if ptrs is not None:
            self._table_grads = list(ptrs)
        return list(self._table_grads)

    def _require_gpu(self):
        ps = self._params()
        if not ps[0].is_cuda:
            raise ValueError("HipAdam: the parameters are CPU tensors; the step runs on HIP kernels only (move the model to the GPU before the first step)")

    def prepare(self):
        """everything a captured step needs that cannot be captured: the state and the tensor table (synchronising set-up calls)"""
        self._require_gpu()
        with torch.cuda.device(self._params()[0].device):
            self.init_state()
            self._ensure_table(self._grads())

    def mark(self):
        """snapshot the range counters of the mixed arithmetic on the device (stream-ordered, capturable): a `step()` after it is skipped
        when one of them moved in between"""
        self._require_gpu()
        with torch.cuda.device(self._params()[0].device):
            self.init_state()
            _lib.check(_lib.load().ns2_optim_mark(self._block.data_ptr(), self._stream()), "ns2_optim_mark")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_group()
        self._require_gpu()
        g = self.param_groups[0]
        with torch.cuda.device(self._params()[0].device):
            self.init_state()
            self._ensure_table(self._grads())
            if float(g["lr"]) != self._lr_pushed:         # a scheduler wrote the group's lr (an eager loop); under a graph write `self.lr`
                self._lr_pushed = float(g["lr"])
                self.lr.fill_(self._lr_pushed)
            cfg = _lib.OptimConfig(float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                   float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0,
                                   self.ema_update_every if self.use_ema else 0)
            _lib.check(_lib.load().ns2_optim_step(self._table.data_ptr(), len(self._params()), self._chunks, self._block.data_ptr(),
                                                  ctypes.byref(cfg), self._stream()), "ns2_optim_step")
        return loss

    # ------------------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.Adam's layout: per-parameter `step` / `exp_avg` / `exp_avg_sq`, the usual `param_groups` keys.  Reads the step count
        (a synchronisation, like any checkpoint).  The EMA tensors are the caller's to save (`ema_parameters()`)."""
        if self._block is not None:
            n = float(int(self.steps_taken.item()))
            for st in self.state.values():
                st["step"] = torch.tensor(n)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """accepts a torch.optim.Adam state dict (the `opt` entry of a reference checkpoint) or one of ours; the values are copied into
        this optimizer's own buffers.  The step count becomes the largest per-parameter `step`."""
        steps = [int(float(s["step"])) for s in state_dict["state"].values() if "step" in s]
        self._pending_step = max(steps, default=0)
        self.init_state()
        super().load_state_dict(state_dict)
        self._check_group()
        with torch.no_grad():
            for p, m, v in zip(self._params(), self._m, self._v):
                st = self.state.get(p, {})
                if "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                else:
                    m.zero_()
                    v.zero_()
                self.state[p] = {"step": torch.tensor(float(self._pending_step)), "exp_avg": m, "exp_avg_sq": v}
            self.steps_taken.fill_(self._pending_step)
            self._lr_pushed = float(self.param_groups[0]["lr"])
            self.lr.fill_(self._lr_pushed)
