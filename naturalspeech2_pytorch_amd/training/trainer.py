"""`Trainer`: the reference's training loop (Trainer, NS2:1689-1930) over this package's training step -- a thin loop.

What it keeps of the reference: the keyword names that mean something here, `train()`, `save(milestone)` / `load(milestone)` with the
reference's checkpoint keys, the EMA copy to sample from.  What is absent, by name: SoundDataset and folder loading (`folder=`,
`dataset=`: pass a `dataloader=`), accelerate (`amp=`, `mixed_precision_type=`, `split_batches=`: one process, one GPU; the mixed
arithmetic is the model's `train_precision`), audio file writing (samples are saved with `torch.save`).

The loop body is `HipAdam`'s (training/optim.py): with `use_graph=True` and `gradient_accumulate_every == 1` a batch of the first
batch's shapes is ONE graph replay -- mark, loss, backward, gradient norm + clip, Adam, EMA -- and the host reads nothing but the loss
it prints.  Other batches (a ragged last one, gradient accumulation) run the same kernels eagerly."""
import contextlib
import copy
import os

import torch

from .graph import GraphedTrainStep
from .optim import HipAdam
from .passes import weights_unchanged

__version__ = "hip-1"


def _cycle(dl):
    while True:
        for data in dl:
            yield data


def _as_inputs(data):
    """a batch -> (keys or None, tensors): a tensor, a tuple / list of tensors (positional arguments of the diffusion object's forward),
    or a dict of tensors (keyword arguments)"""
    if torch.is_tensor(data):
        return None, [data]
    if isinstance(data, dict):
        return list(data), list(data.values())
    return None, list(data)


class Trainer:
    def __init__(self, diffusion_model, *, dataloader=None, folder=None, dataset=None, amp=False, train_lr=1e-4, train_num_steps=100000,
                 gradient_accumulate_every=1, ema_update_every=10, ema_decay=0.995, adam_betas=(0.9, 0.99), use_ema=True,
                 results_folder="./results", save_and_sample_every=1000, num_samples=1, sample_length=None, max_grad_norm=1.0,
                 use_graph=True, sample_kwargs=None):
        if folder is not None or dataset is not None:
            raise NotImplementedError("Trainer(folder=) / Trainer(dataset=): SoundDataset and folder loading (NS2:1746-1771) are not part of "
                                      "this package; build the DataLoader yourself and pass `dataloader=`")
        if amp:
            raise NotImplementedError("Trainer(amp=True): accelerate and its autocast / GradScaler are absent here; the mixed arithmetic of "
                                      "this package is the model's own (`model.train_precision = 'mixed'`), its overflow check is HipAdam.mark()")
        if dataloader is None:
            raise ValueError("Trainer: `dataloader=` is required (an iterable of batches: a tensor, a tuple / list, or a dict of tensors)")
        assert gradient_accumulate_every >= 1
        self.model = diffusion_model
        self.dl = _cycle(dataloader)
        self.train_num_steps, self.gradient_accumulate_every = train_num_steps, gradient_accumulate_every
        self.use_ema, self.use_graph = use_ema, use_graph
        self.opt = HipAdam([p for p in diffusion_model.parameters() if p.requires_grad], lr=train_lr, betas=adam_betas,
                           max_grad_norm=max_grad_norm, ema=use_ema, ema_decay=ema_decay, ema_update_every=ema_update_every)
        self.sample_length, self.num_samples, self.save_and_sample_every = sample_length, num_samples, save_and_sample_every
        self.sample_kwargs = dict(sample_kwargs or {})     # a conditional model samples from a prompt and a text / cond
        self.results_folder = str(results_folder)
        os.makedirs(self.results_folder, exist_ok=True)
        self.step = 0
        self.last_loss = None                              # device scalar of the latest step (summed over its micro-batches)
        self._graph = None                                 # (signature, GraphedTrainStep) of the first batch's shapes
        self._ema_model = None

    # ------------------------------------------------------------------------------------------------------------ EMA copy
    @property
    def device(self):
        return next(self.model.parameters()).device

    @property
    def ema_model(self):
        """a deep copy of the diffusion object (the codec excluded from the copy and shared, NS2:1781-1797) whose parameters ARE the
        optimizer's EMA tensors; buffers are the copy's own.  Call `refresh_weights()` on it before using it -- `sample()` does."""
        if not self.use_ema:
            raise ValueError("Trainer: built with use_ema=False")
        if self._ema_model is None:
            codec = getattr(self.model, "codec", None)
            self.model.codec = None
            try:
                em = copy.deepcopy(self.model)
            finally:
                self.model.codec = codec
            ema_of = {id(p): e for p, e in zip(self.opt.param_groups[0]["params"], self.opt.ema_parameters())}
            theirs = dict(em.named_parameters())
            for name, p in self.model.named_parameters():
                if name in theirs and id(p) in ema_of:
                    theirs[name].data = ema_of[id(p)]
                    theirs[name].requires_grad_(False)
            em.codec = codec
            self._ema_model = em.eval()
        return self._ema_model

    # ------------------------------------------------------------------------------------------------------------ checkpoints
    def _path(self, milestone):
        return os.path.join(self.results_folder, f"model-{milestone}.pt")

    def _ema_state(self):
        codec, em = self.ema_model.codec, self.ema_model
        em.codec = None
        try:
            return {k: v.detach().clone() for k, v in em.state_dict().items()}
        finally:
            em.codec = codec

    def save(self, milestone):
        data = {"step": self.step, "model": self.model.state_dict(), "opt": self.opt.state_dict(),
                "ema": {"ema_model": self._ema_state()} if self.use_ema else None, "scaler": None, "version": __version__}
        torch.save(data, self._path(milestone))

    def load(self, milestone):
        data = torch.load(self._path(milestone), map_location=self.device)
        self.model.load_state_dict(data["model"])          # in place: a captured graph keeps reading the same storage
        self.step = data["step"]
        self.opt.load_state_dict(data["opt"])
        if self.use_ema:
            ema = data["ema"]["ema_model"] if "ema_model" in data["ema"] else \
                {k[len("ema_model."):]: v for k, v in data["ema"].items() if k.startswith("ema_model.")}   # ema_pytorch's flat layout
            codec, em = self.ema_model.codec, self.ema_model
            em.codec = None
            try:
                em.load_state_dict(ema)
            finally:
                em.codec = codec

    # ------------------------------------------------------------------------------------------------------------ the loop
    def _loss(self, keys, tensors):
        return self.model(*tensors) if keys is None else self.model(**dict(zip(keys, tensors)))

    def train_step(self):
        """one optimizer step: `gradient_accumulate_every` batches.  Returns the loss as a device scalar (no synchronisation)."""
        acc = self.gradient_accumulate_every
        keys, tensors = _as_inputs(next(self.dl))
        tensors = [t.to(self.device, non_blocking=True) for t in tensors]
        sig = (tuple(keys) if keys else None, tuple((tuple(t.shape), t.dtype) for t in tensors))
        if self.use_graph and acc == 1:
            if self._graph is None:
                self._graph = (sig, GraphedTrainStep(lambda *ts: self._loss(keys, ts), tensors, self.model, optimizer=self.opt))
            if self._graph[0] == sig:
                self.last_loss = self._graph[1](*tensors)
                self.step += 1
                return self.last_loss
        # eager: gradient accumulation, a batch of other shapes than the graph's, use_graph=False
        self.opt.bind(None, None)
        self.opt.zero_grad(set_to_none=True)
        self.opt.mark()
        total = 0.
        for i in range(acc):
            if i > 0:
                keys, tensors = _as_inputs(next(self.dl))
                tensors = [t.to(self.device, non_blocking=True) for t in tensors]
            with (weights_unchanged() if i > 0 else contextlib.nullcontext()):      # no optimizer step since the previous micro-batch
                loss = self._loss(keys, tensors) / acc
            loss.backward()
            total = total + loss.detach()
        self.opt.step()
        self.last_loss = total
        self.step += 1
        return total

    def sample_and_save(self):
        """what the reference does every `save_and_sample_every` steps (NS2:1903-1927), samples written with torch.save"""
        milestone = self.step // self.save_and_sample_every
        models = [(self.model, str(self.step))] + ([(self.ema_model, f"{self.step}.ema")] if self.use_ema else [])
        if self.sample_length is not None:
            for model, label in models:
                was_training = model.training
                model.eval()
                with torch.no_grad():
                    generated = model.sample(batch_size=self.num_samples, length=self.sample_length, **self.sample_kwargs)
                model.train(was_training)
                torch.save(generated.detach().cpu(), os.path.join(self.results_folder, f"sample_{label}.pt"))
        self.save(milestone)

    def train(self, log_every=0):
        """until `train_num_steps`.  `log_every` > 0 prints the loss that often (reading it is the loop's only synchronisation)."""
        while self.step < self.train_num_steps:
            loss = self.train_step()
            if log_every and self.step % log_every == 0:
                print(f"{self.step}: loss {float(loss):.4f}  grad norm {float(self.opt.grad_norm):.3f}  skipped {int(self.opt.skipped)}")
            if self.save_and_sample_every and self.step % self.save_and_sample_every == 0:
                self.sample_and_save()
        print("training complete")
