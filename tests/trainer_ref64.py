"""fp64 restatement of the optimizer step of csrc/optim.hip (include/ns2hip_optim.h): clip_grad_norm_ + torch.optim.Adam (weight_decay 0,
amsgrad off) + a constant-decay EMA every `update_every` steps, on lists of tensors.  Plain torch, no library; checked against
torch.optim.Adam in fp64 by tests/test_trainer_step_cpu.py and used as the reference of tests/test_trainer_step_gpu.py."""
import math

import torch


class Ref64:
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=None, ema=False, update_every=10):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.ema = [p.clone() for p in self.p] if ema else None
        self.lr, self.betas, self.eps, self.max_grad_norm, self.update_every = lr, betas, eps, max_grad_norm, update_every
        self.t = 0
        self.grad_norm = None

    def step(self, grads, ema_decay=0.995, lr=None):
        """grads[i]: a tensor or None (no gradient: no part in the norm or in Adam, still in the EMA).  A non-finite norm skips the step."""
        lr = self.lr if lr is None else lr
        gs = [None if g is None else g.detach().double() for g in grads]
        self.grad_norm = math.sqrt(sum(float((g * g).sum()) for g in gs if g is not None))
        if not math.isfinite(self.grad_norm):
            return False
        coef = 1.0 if self.max_grad_norm is None else min(1.0, self.max_grad_norm / (self.grad_norm + 1e-6))
        self.t += 1
        b1, b2 = self.betas
        step_size = lr / (1.0 - b1 ** self.t)
        bc2_sqrt = math.sqrt(1.0 - b2 ** self.t)
        for p, g, m, v in zip(self.p, gs, self.m, self.v):
            if g is None:
                continue
            g = g * coef
            m += (g - m) * (1.0 - b1)
            v.mul_(b2).add_(g * g, alpha=1.0 - b2)
            p -= step_size * m / (v.sqrt() / bc2_sqrt + self.eps)
        if self.ema is not None and self.t % self.update_every == 0:
            w = 1.0 - float(torch.tensor(ema_decay, dtype=torch.float32))      # the decay is an fp32 device scalar
            for e, p in zip(self.ema, self.p):
                e += w * (p - e)
        return True
