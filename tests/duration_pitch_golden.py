"""TEST INFRASTRUCTURE shared by tests/test_duration_pitch_training_cpu.py and tests/test_duration_pitch_training_gpu.py (never imported by
the product):

  * the fixtures of tests/golden/make_golden_duration_pitch_grads.py put back together (`load_cases`) and turned into this package's
    predictor, inputs and reference gradients (`build_case`, `run_case`);
  * `DurationPitchEmuBackend`: tests/encoder_golden.MaskedEmuBackend plus torch restatements of the backend calls the predictor's training
    path adds (GroupNorm + SiLU forward / backward in the kernels' own formulas, the heads), on the CPU.
"""
import os

import torch
import torch.nn.functional as F

from tests.encoder_golden import GOLDEN, MaskedEmuBackend, rel  # noqa: F401  (rel: re-exported for the tests)
from tests.golden.gen import make_input, make_weights


def load_cases():
    """-> {case: meta dict with `grads` = {name: tensor}}"""
    fix = torch.load(os.path.join(GOLDEN, "duration_pitch_grads.pt"), weights_only=False)
    flat = {}
    for part in fix["parts"]:
        flat.update(torch.load(os.path.join(GOLDEN, part), weights_only=False))
    cases = {}
    for name, meta in fix["cases"].items():
        meta = dict(meta)
        meta["grads"] = {k: flat[f"{name}/{k}"] for k in meta["grad_names"]}
        cases[name] = meta
    return cases


def build_case(meta, device="cpu", train_backend="composite", **extra):
    """-> (predictor in train() mode, x, prompts (requires grad), the float input (requires grad) or None, (proj0, proj1))"""
    from naturalspeech2_pytorch_amd import DurationPitchPredictor
    m = DurationPitchPredictor(**dict(meta["kwargs"], **extra), train_backend=train_backend)
    m.load_state_dict(make_weights(meta["shapes"], seed=meta["weight_seed"]))
    m = m.to(device).train()
    seed = meta["input_seed"]
    prompts = make_input("prompt_enc", meta["prompts_shape"], seed=seed).to(device).requires_grad_(True)
    if "ids" in meta:
        x, xf = meta["ids"].to(device), None
    else:
        x = xf = make_input("phoneme_enc", meta["x_shape"], seed=seed).to(device).requires_grad_(True)
    projs = tuple(make_input(f"proj{i}", tuple(meta["duration"].shape), seed=seed).to(device) for i in range(2))
    return m, x, prompts, xf, projs


def run_case(m, fwd, x, prompts, xf, projs):
    """one forward + backward of (dur * proj0).sum() + (pitch * proj1).sum() with (dur, pitch) = fwd(m, x, prompts)
    -> (dur, pitch, {name: grad}) with the gradients of prompts / the float input as "prompts" / "input" """
    for p in m.parameters():
        p.grad = None
    prompts.grad = None
    if xf is not None:
        xf.grad = None
    dur, pitch = fwd(m, x, prompts)
    ((dur * projs[0]).sum() + (pitch * projs[1]).sum()).backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    grads["prompts"] = prompts.grad.detach().clone()
    if xf is not None:
        grads["input"] = xf.grad.detach().clone()
    return dur.detach(), pitch.detach(), grads


class DurationPitchEmuBackend(MaskedEmuBackend):
    name = "emu-duration-pitch"

    @staticmethod
    def _xhat(x, B, n, groups, eps):
        C = x.shape[1]
        xg = x.reshape(B, n, groups, C // groups)
        mean = xg.mean(dim=(1, 3), keepdim=True)
        rstd = (xg.var(dim=(1, 3), unbiased=False, keepdim=True) + eps).rsqrt()
        return ((xg - mean) * rstd).reshape(B * n, C), rstd

    def groupnorm_silu_fwd(self, x, B, n, weight, bias, groups, eps, resid=None):
        self.calls.append("groupnorm_silu_fwd")
        C = weight.shape[0]
        x = x[:, :C]
        assert not torch.isnan(x).any(), "groupnorm_silu_fwd read an unwritten column"
        xh, rstd = self._xhat(x, B, n, groups, eps)
        y = F.silu(xh * weight + bias)
        if resid is not None:
            y = y + resid[:, :C]
        return y, x, torch.empty(0)             # (the kernels keep their statistics slots; the restatement recomputes)

    def groupnorm_silu_bwd(self, dy, x, stats, B, n, weight, bias, groups, eps):
        """include/ns2hip.h, ns2_groupnorm_silu_bwd, formula for formula"""
        self.calls.append("groupnorm_silu_bwd")
        C = weight.shape[0]
        xh, rstd = self._xhat(x, B, n, groups, eps)
        z = xh * weight + bias
        sg = torch.sigmoid(z)
        dz = dy[:, :C] * sg * (1 + z * (1 - sg))
        dxh = (dz * weight).reshape(B, n, groups, C // groups)
        xg = xh.reshape(B, n, groups, C // groups)
        s1 = dxh.mean(dim=(1, 3), keepdim=True)
        s2 = (dxh * xg).mean(dim=(1, 3), keepdim=True)
        dx = (rstd * (dxh - s1 - xg * s2)).reshape(B * n, C)
        return dx, (dz * xh).sum(0), dz.sum(0)

    def row_dot_relu(self, h, w, b):
        self.calls.append("row_dot_relu")
        return F.relu(h[:, :w.numel()] @ w + b)

    def row_dot_relu_bwd(self, dout, out, h, w):
        self.calls.append("row_dot_relu_bwd")
        g = torch.where(out > 0, dout, torch.zeros_like(dout))
        return g[:, None] * w[None], g @ h[:, :w.numel()], g.sum().reshape(1)

    def attention(self, *a, **k):
        self.calls.append("attention")
        return super().attention(*a, **k)

    def attention_bwd(self, *a, **k):
        self.calls.append("attention_bwd")
        return super().attention_bwd(*a, **k)
