"""Generate the gradient goldens at head dims 32 and 128 by executing the UNMODIFIED reference (build container only).

    python tests/golden/make_golden_head_dim_grads.py

Writes tests/golden/grads_uncond_d64_hd32.pt and tests/golden/grads_cond_d64_hd128.pt with make_golden.py's `gen_grad_case`: every
parameter's gradient, dL/dx and the prediction from the reference's own autograd.  The specs are those of the forward goldens of the
same names (make_golden.py MODEL_CASES) -- full-size Wavenet stacks, so 8 and 15 MB of gradients: each fixture is then split like
encoder_grads.pt, grads_<name>.pt keeping everything but the tensors plus the list of its parts grads_<name>.partNN.pt (each below the
size limit of a committed file; a tensor larger than a part is cut along its first axis).  `load_head_dim_grads(name)` puts a fixture
together again; tests/test_head_dim_training_gpu.py reads them through it."""
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle.ref_stub import load_reference                  # noqa: E402
from tests.golden.make_golden import gen_grad_case          # noqa: E402

HEAD_DIM_GRAD_CASES = {
    # name: (ctor kwargs, batch, n, n_prompt, n_cond)
    "uncond_d64_hd32": (dict(dim=64, depth=2, dim_head=32, heads=4), 2, 80, None, None),
    "cond_d64_hd128": (dict(dim=64, depth=2, dim_head=128, heads=2, dim_prompt=48, condition_on_prompt=True, num_latents_m=16), 2, 72, 21, 60),
}

OUT = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900 * 1000


def split_fixture(name):
    """grads_<name>.pt as gen_grad_case wrote it -> an index file of the same name + parts"""
    path = os.path.join(OUT, f"grads_{name}.pt")
    fix = torch.load(path, weights_only=False)
    flat = {"output": fix.pop("output"), "x_grad": fix.pop("x_grad")}
    flat.update({f"grads/{k}": g for k, g in fix.pop("grads").items()})
    pieces = []                                            # (key, piece index, number of pieces, tensor)
    for k, t in flat.items():
        n = max(1, -(-t.numel() * t.element_size() // PART_BYTES))
        chunks = [t] if n == 1 else list(torch.chunk(t, n, dim=0))
        pieces += [(k, i, len(chunks), c.clone()) for i, c in enumerate(chunks)]
    parts, cur, size = [], {}, 0
    for k, i, n, t in pieces:
        nbytes = t.numel() * t.element_size()
        assert nbytes <= PART_BYTES, (k, tuple(t.shape))
        if cur and size + nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[(k, i, n)] = t
        size += nbytes
    parts.append(cur)
    names = [f"grads_{name}.part{i:02d}.pt" for i in range(len(parts))]
    for fn, part in zip(names, parts):
        torch.save(part, os.path.join(OUT, fn))
    torch.save(dict(fix, parts=names), path)
    print("split", name, "into", len(names), "parts")


def load_head_dim_grads(name):
    """the fixture as gen_grad_case made it: kwargs, shapes, seeds, output, x_grad, grads"""
    fix = torch.load(os.path.join(OUT, f"grads_{name}.pt"), weights_only=False)
    got = {}
    for fn in fix.pop("parts"):
        for (k, i, n), t in torch.load(os.path.join(OUT, fn), weights_only=False).items():
            got.setdefault(k, [None] * n)[i] = t
    flat = {k: (v[0] if len(v) == 1 else torch.cat(v, dim=0)) for k, v in got.items()}
    fix["output"], fix["x_grad"] = flat.pop("output"), flat.pop("x_grad")
    fix["grads"] = {k[len("grads/"):]: v for k, v in flat.items()}
    return fix


if __name__ == "__main__":
    ns2 = load_reference()
    for name, spec in HEAD_DIM_GRAD_CASES.items():
        gen_grad_case(ns2, name, spec)
        whole = torch.load(os.path.join(OUT, f"grads_{name}.pt"), weights_only=False)
        split_fixture(name)
        back = load_head_dim_grads(name)
        assert torch.equal(back["output"], whole["output"]) and torch.equal(back["x_grad"], whole["x_grad"])
        assert list(back["grads"]) == list(whole["grads"]) and all(torch.equal(back["grads"][k], v) for k, v in whole["grads"].items())
