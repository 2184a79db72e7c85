"""What "the current pass" is, and everything selected by it: the pass state (`_Pass`, set and restored by `training_pass` alone), the
backend of the Function whose forward is running (`backend()`, the registries behind it, the tests' substitute), the frozen-weights flag
(`weights_unchanged`) and the loss scale of the mixed arithmetic (`_Scale`).  The only module of the package with module state."""
import contextlib
from typing import NamedTuple, Optional

import torch

from .._range_guard import RangePeek, moved
from .backend import HipBackend

TRAIN_PRECISIONS = {"exact": 3, "mixed": 4}


# =============================================================================================== loss scaling of the mixed arithmetic
class _Scale:
    """Loss scale of ONE forward / backward pass of the mixed arithmetic.  IEEE half (and its e5m2 companions) stops at 65504 and
    thins out below 6e-5; the gradient of a mean-reduced loss over 1.7e7 elements is ~1e-7.  Every gradient is linear in the
    gradient that enters the graph, so the pass runs on gradients multiplied by a power of two `s` (exact in fp32) -- what the
    reference's accelerate / fp16 training does with its GradScaler (NS2:1710-1711, 1723-1726).  `s` is chosen where the gradient
    enters (`_ScaleIn` at the model output) from its largest magnitude, on the device, without a synchronisation: the scaled maximum
    becomes 2^5 ... 2^6, which leaves 2^10 of head-room before 65504 for growth inside the graph and ~2^19 below for small values.
    Token-sized gradients stay scaled between the Functions; whatever leaves the scaled domain -- parameter gradients, FiLM /
    adaptive-norm conditioning gradients, x.grad -- is multiplied by 1 / s (`unscale`).  Values that still leave the half range are
    COUNTED by the converting kernels: `overflowed()` (below) compares the device's range counters after the pass with their values
    when the pass began and tells a training loop to skip / repeat the step -- the counterpart of GradScaler's inf check
    (`model._last_loss_scale.overflowed()` after `loss.backward()`)."""
    TARGET = 64.0

    def __init__(self, device=None):
        self.s = None
        self.inv = None
        self._before = RangePeek().take(device)      # stream-ordered: the counters of the pass's device as they stand when it is enqueued
                                                     # (None under capture: GraphedTrainStep peeks around the replay instead)

    def overflowed(self) -> bool:
        """did a conversion of this pass (forward activations, scaled gradients) leave the IEEE-half range?  Call after `backward()`;
        waits for the pass (one event synchronisation).  True: the gradients of this step are clamped somewhere -- skip the optimizer
        step (and train on with `train_precision="exact"` if it keeps happening: bf16 planes have the fp32 range)."""
        return moved(self._before)

    def choose(self, g):
        amax = g.detach().abs().amax().clamp_min(1e-30).float()
        self.s = torch.exp2(torch.floor(torch.log2(self.TARGET / amax))).clamp(2.0 ** -60, 2.0 ** 60)
        self.inv = 1.0 / self.s
        return self.s

    def unscale(self, t):
        return t if t is None else t * self.inv


class _ScaleIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, sc):
        ctx.sc = sc
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.sc.choose(g), None


class _ScaleOut(torch.autograd.Function):
    """a tensor entering the scaled domain from outside (x, `null_prompt_tokens`, the resampler's latents ...): its gradient leaves it"""

    @staticmethod
    def forward(ctx, t, sc):
        ctx.sc = sc
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.sc.unscale(g), None


# =============================================================================================== the pass state and the backend it selects
class _Pass(NamedTuple):
    """the training pass whose graph is being BUILT (`training_pass` sets it around the Functions' forwards; a Function keeps what its
    backward needs -- the backend, the scale -- in its ctx)"""
    precision: int = 3                       # the arithmetic of the pass (TRAIN_PRECISIONS)
    scale: Optional[_Scale] = None           # ... and its loss scale (None: exact arithmetic)
    device: Optional[int] = None             # device index of the pass (None: the current device)


_PASS = _Pass()
_BACKEND = None            # a substitute installed by the tests (tests/emu_backend.py)
_HIP = {}                  # (device index, precision) -> HipBackend of the eager passes, each with its own packed-weight cache and re-pack
                           # table (models on two GPUs of one process must not share a device table)
_REGISTRY = _HIP           # the registry backend() consults: _HIP, or a GraphedTrainStep's own while it warms up and captures (`_registry`)
_WEIGHTS_FROZEN = False    # inside `with weights_unchanged():`


def current():
    """the `_Pass` being built (the default one -- exact arithmetic, current device -- outside `training_pass`); every reader of the state,
    in this module too, goes through here -- only `training_pass` touches `_PASS` itself"""
    return _PASS


def backend():
    """the backend the Function whose forward is running should use (it keeps it in ctx for its backward)"""
    if _BACKEND is not None:
        return _BACKEND
    p = current()
    dev = p.device if p.device is not None else (torch.cuda.current_device() if torch.cuda.is_available() else -1)
    key = (dev, p.precision)
    if key not in _REGISTRY:
        _REGISTRY[key] = HipBackend(p.precision)
    return _REGISTRY[key]


def set_backend(b):
    """tests: install a substitute backend (tests/emu_backend.py); returns the previous one"""
    global _BACKEND
    prev, _BACKEND = _BACKEND, b
    return prev


@contextlib.contextmanager
def _registry(reg):
    """`with _registry(reg):` -- backend() takes its HipBackends from `reg` (and creates them there) instead of `_HIP`"""
    global _REGISTRY
    prev, _REGISTRY = _REGISTRY, reg
    try:
        yield
    finally:
        _REGISTRY = prev


class weights_unchanged:
    """`with training.weights_unchanged():` around training passes that follow another pass WITHOUT an optimizer step in between -- the later
    micro-batches of gradient accumulation (NS2:1877-1885), several losses on one set of weights: the per-pass refresh of every packed weight
    (one launch reading all parameters: 1.3 ms at d512 / L12; needed by default because fused optimizers change parameters without bumping the
    version counters a cache could key on) is skipped and the packs of the previous pass are used as they are.  The caller's promise;
    weights changed inside the block the way a fused optimizer changes them (no version bump) are NOT seen until the first pass outside it."""

    def __enter__(self):
        global _WEIGHTS_FROZEN
        self.prev, _WEIGHTS_FROZEN = _WEIGHTS_FROZEN, True

    def __exit__(self, *exc):
        global _WEIGHTS_FROZEN
        _WEIGHTS_FROZEN = self.prev


@contextlib.contextmanager
def training_pass(precision, like):
    """`with training_pass(precision, x) as p:` around the forwards of one pass on the device of the tensor `like`; `p` is its `_Pass`.
    The one place that sets and restores the pass state -- whatever fails after the state is set, the previous one comes back.  Stream
    order: the range-counter peeks of a mixed pass's `_Scale()`, then the one re-pack launch of `begin_pass` (every trainable weight is
    re-packed at its first use of the pass: `_PackedCache`), then the Functions."""
    global _PASS
    prev = _PASS
    try:
        dev = like.device.index if like.is_cuda else None
        _PASS = _Pass(precision, _Scale(dev) if precision == TRAIN_PRECISIONS["mixed"] else None, dev)
        bk = backend()
        if hasattr(bk, "packs"):
            bk.packs.begin_pass(frozen=_WEIGHTS_FROZEN)
        yield _PASS
    finally:
        _PASS = prev


def _enter(t):
    sc = current().scale
    return t if sc is None else _ScaleOut.apply(t, sc)


def _un(ctx, *ts):
    """parameter / conditioning gradients of a Function leave the scaled domain (one multi-tensor launch per Function: the per-tensor
    multiplications were 325 launches of a d512 / L12 step)"""
    sc = ctx.sc
    if sc is None:
        return ts
    live = [t for t in ts if t is not None]
    if not live:
        return ts
    done = iter(torch._foreach_mul(live, sc.inv))
    return tuple(None if t is None else next(done) for t in ts)
