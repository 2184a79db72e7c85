"""The training step (loss + backward) of a fixed shape as one HIP graph"""
import torch

from .._range_guard import RangePeek, moved
from .passes import _registry


class _LossOf(torch.nn.Module):
    """`loss_fn` as the forward of a module that owns `root`: lets torch.func.functional_call run it on substitute parameters"""

    def __init__(self, root, loss_fn):
        super().__init__()
        self.root, self.loss_fn = root, loss_fn

    def forward(self, *inputs):
        return self.loss_fn(*inputs)


class GraphedTrainStep:
    """`loss = loss_fn(*inputs); loss.backward()` of a FIXED shape captured once in a HIP graph and replayed per step.

    Why: a d512 / L12 training pass enqueues ~2 000 launches from Python (the autograd Functions of functions.py are coarse, but each is a
    dozen library calls); on a host whose cores are shared the enqueue, not the GPU, set the step time (98 ms vs 151 ms for the same
    kernels, profiles/README.md), and at BASELINE config 1's size (d128 / L6, 4 x 1024) the GPU waits for Python: 20 ms eager, 12 ms
    replayed.  Everything this package launches is capture-safe after a warm pass -- the weight packs are refreshed by ONE
    `ns2_weights_repack` launch that reads the parameters' own storage (`_PackedCache._repack_all`), the loss scale of the mixed
    arithmetic is chosen on the device (`_Scale.choose`), buffers come from PyTorch's allocator (its graph-private pool during
    capture), random draws (conditioning dropout, times / noise when `loss_fn` draws them) go through PyTorch's graph-aware
    generator -- so the replay runs the same kernels on the same operands: loss and gradients are bit-identical to the eager pass
    (tests/test_round6_gpu.py::test_graphed_training_step).

    The graph owns what its kernels read: the warm passes and the capture take their backends from a registry of this object's own
    (`_registry`), not from `_HIP`, so the packed weights, the repack table and the array of tiled handles the replays read live exactly
    as long as the graph.  Eager passes (a ragged last batch), other graphs and other models may run between replays, and nothing they
    do -- nor `_HIP.clear()` -- frees that state.

        step = GraphedTrainStep(lambda a, t, n: diffusion(a, times=t, noise=n), (audio, times, noise), model)
        loss = step(audio, times, noise)          # .grad of every trainable parameter of `model` is now this batch's gradient
        optimizer.step()                          # any in-place torch optimizer, after the replay (`zero_grad` between replays is
                                                  # unnecessary and harmless) -- or hand the graph a `HipAdam` and drop this line:

        step = GraphedTrainStep(..., model, optimizer=training.HipAdam(model.parameters(), max_grad_norm=1.0, ema=True))
        loss = step(audio, times, noise)          # a whole training step: mark, loss, backward, gradient norm + clip, Adam, EMA

    With `optimizer=` (a `HipAdam` over `module`'s trainable parameters) the captured graph is `optimizer.mark()`, loss and backward,
    then the optimizer's norm and update launches (training/optim.py), bound to the graph's own gradient tensors; leaves the loss does not
    reach have no gradient there either.  A step whose conversions left the IEEE-half range, or whose gradient norm is not finite, is
    skipped ON THE DEVICE (`optimizer.skipped`), so `overflowed()` and its host round trip are not needed on that path.  Constructing the
    object moves neither a parameter nor any optimizer state: the warm passes run no optimizer step and a capture executes nothing.

    `module`: the nn.Module (or a list of them) whose trainable parameters `loss_fn` reaches.  During the warm passes and the capture
    the module runs on SUBSTITUTE leaves over the same storage (torch.func.functional_call): a parameter's own AccumulateGrad node lives
    on the stream it was created on -- the default stream whenever an eager pass's `loss` is still referenced -- and the autograd engine
    would tie that stream into the capture (observed: a crash inside hipStreamEndCapture; tools/exp_graph_crash.py).  The gradients
    come back from torch.autograd.grad as the graph's own tensors and are attached as `.grad` after every replay.

    The parameters must be updated IN PLACE (every torch optimizer does); re-create the object after changing shapes, freezing /
    unfreezing parameters or loading a state dict into NEW storage.  `overflowed()` is `_Scale.overflowed` for the replayed pass.
    Tensor hooks on the parameters do not run during a replay (`distributed.GradientAllReducer` overlaps its all-reduces with an EAGER
    backward through such hooks): a data-parallel loop on the graph all-reduces `step.grads` after the call instead."""

    def __init__(self, loss_fn, example_inputs, module, warmup=2, optimizer=None):
        root = module if isinstance(module, torch.nn.Module) else torch.nn.ModuleList(list(module))
        named = [(k, p) for k, p in root.named_parameters() if p.requires_grad]
        assert named, "GraphedTrainStep: no trainable parameter"
        self.inputs = [t.detach().clone() for t in example_inputs]
        assert self.inputs and self.inputs[0].is_cuda, "GraphedTrainStep captures a HIP graph: inputs live on the GPU"
        self.params = [p for _, p in named]
        self.optimizer = optimizer
        if optimizer is not None:
            from .optim import HipAdam
            assert isinstance(optimizer, HipAdam), "GraphedTrainStep(optimizer=): a training.HipAdam (its step is capturable and reads no device value on the host)"
            mine = {id(p) for p in self.params}
            assert all(id(p) in mine for p in optimizer.param_groups[0]["params"]), "GraphedTrainStep(optimizer=): the optimizer holds a parameter that is not a trainable parameter of `module`"
            optimizer.bind(None, None)
            optimizer.prepare()                           # state block and tensor table: synchronising set-up, before any capture
        self._subs = {"root." + k: p.detach().requires_grad_(True) for k, p in named}
        self._backends = {}                               # the HipBackends of the warm passes and the capture: what the replays read
        leaves = list(self._subs.values())
        fn = _LossOf(root, loss_fn)
        run = lambda: torch.func.functional_call(fn, self._subs, tuple(self.inputs))       # noqa: E731
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with _registry(self._backends), torch.cuda.stream(side):   # warm passes: packs, tile images, split-K plans, function attributes all exist
            for _ in range(max(2, warmup)):               # (two at least: the first packs the substitutes' weights, the second builds the
                torch.autograd.grad(run(), leaves, allow_unused=True)      # one-launch repack table -- a synchronising build, not capturable)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with _registry(self._backends), torch.cuda.graph(self.graph):
            if optimizer is not None:
                optimizer.mark()
            loss = run()
            grads = torch.autograd.grad(loss, leaves, allow_unused=True)
            if optimizer is not None:
                optimizer.bind(self.params, grads)        # the graph's own tensors; their addresses travel as launch arguments
                optimizer.step()
        self.loss = loss.detach()
        self.grads = list(grads)                          # the graph's own tensors: every replay writes them, __call__ attaches them as .grad
        self._opt_grads = None if optimizer is None else optimizer.table_grads()
        self._before = None

    def __call__(self, *inputs):
        assert len(inputs) == len(self.inputs)
        for s, t in zip(self.inputs, inputs):
            if t is not s:
                s.copy_(t)
        self._before = RangePeek().take(self.inputs[0].device)
        self.graph.replay()
        if self.optimizer is not None:                    # (an eager optimizer.step() in between may have pointed the table elsewhere;
            self.optimizer.bind(self.params, self.grads)  # the replay pointed it back at the graph's gradients)
            self.optimizer.table_grads(self._opt_grads)
        for p, g in zip(self.params, self.grads):         # (whatever a zero_grad(set_to_none=True) or an eager pass in between left there)
            p.grad = g
        return self.loss

    def overflowed(self) -> bool:
        return moved(self._before)
