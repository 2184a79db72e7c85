"""The optimizer step without a GPU: the optimizer's header of the C ABI and its binding, the refusals of `HipAdam` and `Trainer`, the
state-dict contract with torch.optim.Adam, and the fp64 restatement the GPU tests use as their reference."""
import ctypes
import os
import subprocess

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, training
from naturalspeech2_pytorch_amd.training import HipAdam, Trainer
from tests.trainer_ref64 import Ref64


def test_second_header_parses_by_the_one_rule_and_is_exported():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    consts, structs, sigs = _lib.ABI["ns2hip_optim.h"]
    assert sorted(sigs) == _lib.header_symbols("ns2hip_optim.h")
    assert sorted(structs) == ["ns2_optim_config", "ns2_optim_tensor"]
    assert [n for n, _ in structs["ns2_optim_tensor"]._fields_] == ["param", "grad", "exp_avg", "exp_avg_sq", "ema", "numel"]
    assert [n for n, _ in structs["ns2_optim_config"]._fields_] == ["beta1", "beta2", "eps", "max_grad_norm", "ema_update_every"]
    T, C = _lib.OptimTensor, _lib.OptimConfig
    assert ctypes.sizeof(T) == 48 and ctypes.sizeof(C) == 40
    pinned = {
        "ns2_optim_chunks": (L, [ctypes.POINTER(T), I]),
        "ns2_optim_table_bytes": (L, [I, L]),
        "ns2_optim_table_build": (I, [ctypes.POINTER(T), I, P, L, P]),
        "ns2_optim_set_grads": (I, [P, I, I, I, ctypes.POINTER(P), P]),
        "ns2_optim_state_init": (I, [P, I, F, F, P]),
        "ns2_optim_mark": (I, [P, P]),
        "ns2_optim_step": (I, [P, I, L, P, ctypes.POINTER(C), P]),
    }
    assert sigs == pinned and all(_lib.SIGNATURES[n] == row for n, row in pinned.items())
    assert len(consts) == 14 and consts["NS2_OPTIM_CHUNK"] % 1024 == 0 and consts["NS2_OPTIM_STATE_WORDS"] == 128
    assert (T, C) == (structs["ns2_optim_tensor"], structs["ns2_optim_config"])
    # the tables of the other headers describe them alone (how many entries each holds, that no name is in two headers, and that the
    # library exports and binds every one: test_host_cpu.py::test_library_exports_whole_abi)
    others = [t for h, t in _lib.ABI.items() if h != "ns2hip_optim.h"]
    assert sorted(s for t in others for s in t.structs) == ["ns2_attn_args", "ns2_attn_bwd_args", "ns2_linear_args", "ns2_model_config",
                                                            "ns2_repack_part"]
    assert not any(k.startswith("NS2_OPTIM") for t in others for k in t.constants)


def test_bad_arguments_come_back_as_codes_before_any_device_call():
    """no GPU here: an entry point that reached a device call would fail with NS2_ERR_HIP, not NS2_ERR_ARG"""
    lib = _lib.load()
    T, C = _lib.OptimTensor, _lib.OptimConfig
    err = lambda: lib.ns2_last_error().decode()       # noqa: E731
    one = (T * 1)()
    one[0].numel = -1
    assert lib.ns2_optim_chunks(one, 1) == _lib.NS2_ERR_ARG and "negative numel" in err()
    one[0].numel = 4097
    assert lib.ns2_optim_chunks(one, 1) == 2 and lib.ns2_optim_chunks(one, 0) == 0
    assert lib.ns2_optim_table_bytes(1, 2) == 48 + 2 * 16 + 2 * 4
    assert lib.ns2_optim_table_bytes(-1, 0) == _lib.NS2_ERR_ARG
    assert lib.ns2_optim_table_build(one, 1, None, 1 << 20, None) == _lib.NS2_ERR_ARG and "16-byte aligned" in err()
    assert lib.ns2_optim_table_build(one, 1, 4096, 8, None) == _lib.NS2_ERR_ARG and "smaller than" in err()
    assert lib.ns2_optim_table_build(one, 1, 4096, 1 << 20, None) == _lib.NS2_ERR_ARG and "may not be null" in err()
    one[0].param, one[0].exp_avg, one[0].exp_avg_sq = 4096 + 2, 8192, 12288
    assert lib.ns2_optim_table_build(one, 1, 4096, 1 << 20, None) == _lib.NS2_ERR_ARG and "4-byte aligned" in err()
    host = (ctypes.c_void_p * 1)(4096)
    assert lib.ns2_optim_set_grads(4096, 1, 0, 0, host, None) == _lib.NS2_ERR_ARG and "count" in err()
    assert lib.ns2_optim_set_grads(4096, 1, 1, 1, host, None) == _lib.NS2_ERR_ARG and "first" in err()
    assert lib.ns2_optim_set_grads(4096, 300, 0, 257, host, None) == _lib.NS2_ERR_ARG
    assert lib.ns2_optim_state_init(None, 0, 1e-4, 0.995, None) == _lib.NS2_ERR_ARG
    assert lib.ns2_optim_state_init(4096, -1, 1e-4, 0.995, None) == _lib.NS2_ERR_ARG and "step" in err()
    assert lib.ns2_optim_mark(4100, None) == _lib.NS2_ERR_ARG
    cfg = C(0.9, 0.99, 1e-8, 1.0, 10)
    assert lib.ns2_optim_step(4096, 1, 1, 4096, None, None) == _lib.NS2_ERR_ARG and "config" in err()
    assert lib.ns2_optim_step(4096, 1, 1, None, ctypes.byref(cfg), None) == _lib.NS2_ERR_ARG and "state" in err()
    assert lib.ns2_optim_step(None, 1, 1, 4096, ctypes.byref(cfg), None) == _lib.NS2_ERR_ARG and "table" in err()
    assert lib.ns2_optim_step(4096, 1, -1, 4096, ctypes.byref(cfg), None) == _lib.NS2_ERR_ARG
    cfg.beta2 = 1.0
    assert lib.ns2_optim_step(4096, 1, 1, 4096, ctypes.byref(cfg), None) == _lib.NS2_ERR_ARG and "betas" in err()


def _params(n=3):
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(5, 3), (7,), (2, 2, 2)][:n]]


@pytest.mark.parametrize("kw, word", [(dict(weight_decay=0.01), "weight decay"), (dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize")])
def test_hipadam_refuses_what_the_kernels_do_not_cover(kw, word):
    with pytest.raises(ValueError, match=word):
        HipAdam(_params(), **kw)


def test_hipadam_refuses_parameters_the_kernels_cannot_walk():
    with pytest.raises(ValueError, match="fp32 parameters only"):
        HipAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="not contiguous"):
        HipAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="one parameter group"):
        HipAdam([{"params": _params(1)}, {"params": _params(1), "lr": 1.0}])
    opt = HipAdam(_params())
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="CPU tensors"):
        opt.step()
    with pytest.raises(ValueError, match="CPU tensors"):
        opt.mark()
    opt.param_groups[0]["weight_decay"] = 0.1             # changed behind the constructor's back (a loaded state dict, a scheduler)
    with pytest.raises(ValueError, match="weight decay"):
        opt.step()
    with pytest.raises(ValueError, match="ema=False"):
        HipAdam(_params()).ema_parameters()
    with pytest.raises(ValueError, match="one gradient"):
        HipAdam(_params()).bind(_params(), [None] * 3)    # parameters of another optimizer


def test_trainer_names_what_is_absent():
    m = torch.nn.Linear(2, 2)
    with pytest.raises(NotImplementedError, match="SoundDataset"):
        Trainer(m, folder="/data")
    with pytest.raises(NotImplementedError, match="SoundDataset"):
        Trainer(m, dataset=[torch.zeros(2)])
    with pytest.raises(NotImplementedError, match="accelerate"):
        Trainer(m, dataloader=[torch.zeros(2)], amp=True)
    with pytest.raises(ValueError, match="dataloader"):
        Trainer(m)


def test_state_dict_has_adams_layout_and_loads_both_ways():
    ps = _params()
    ours = HipAdam(ps, lr=3e-4, ema=True)
    ours.init_state()
    # the EMA buffers start as a copy of the parameters, in parameter order
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(ours.ema_parameters(), ps))
    adam = torch.optim.Adam(ps, lr=3e-4, betas=(0.9, 0.99))
    for p in ps:
        p.grad = torch.ones_like(p)
    adam.step()
    adam.step()
    a, o = adam.state_dict(), ours.state_dict()
    assert [sorted(g) for g in o["param_groups"]] == [sorted(g) for g in a["param_groups"]]
    assert o["param_groups"][0]["params"] == a["param_groups"][0]["params"] and o["param_groups"][0]["betas"] == (0.9, 0.99)
    assert sorted(o["state"]) == sorted(a["state"])
    for k in a["state"]:
        assert sorted(o["state"][k]) == sorted(a["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        for name in a["state"][k]:
            assert o["state"][k][name].shape == a["state"][k][name].shape and o["state"][k][name].dtype == a["state"][k][name].dtype, name
    # Adam's state (a reference checkpoint's `opt`) loads into ours, values copied into our own buffers ...
    before = [t.data_ptr() for t in ours._m]
    ours.load_state_dict(a)
    assert int(ours.steps_taken) == 2 and [t.data_ptr() for t in ours._m] == before
    for i, p in enumerate(ps):
        assert torch.equal(ours.state[p]["exp_avg"], adam.state[p]["exp_avg"]) and ours.state[p]["exp_avg"] is ours._m[i]
        assert torch.equal(ours.state[p]["exp_avg_sq"], adam.state[p]["exp_avg_sq"])
    # ... and torch.optim.Adam loads ours
    fresh = torch.optim.Adam(ps)
    fresh.load_state_dict(ours.state_dict())
    assert float(fresh.state[ps[0]]["step"]) == 2.0 and torch.equal(fresh.state[ps[1]]["exp_avg"], adam.state[ps[1]]["exp_avg"])
    assert fresh.param_groups[0]["lr"] == 3e-4


def test_ref64_agrees_with_torch_adam_in_fp64():
    g = torch.Generator().manual_seed(1)
    shapes = [(5,), (33, 7), (257,)]
    p0 = [0.1 * torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    adam = torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.99), eps=1e-8)
    ref = Ref64(p0, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=1.0)
    for s in range(6):
        gs = [(0.5 if s % 2 == 0 else 0.01) * torch.randn(sh, generator=g, dtype=torch.float64) for sh in shapes]
        gs[1] = None if s == 2 else gs[1]                 # a step without a gradient for one tensor
        for p, gr in zip(ps, gs):
            p.grad = None if gr is None else gr.clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, 1.0)
        adam.step()
        assert ref.step(gs)
        assert abs(ref.grad_norm - float(norm)) <= 1e-14 * float(norm)
        assert (ref.grad_norm > 1.0) == (s % 2 == 0)      # clipping active and inactive in turn
    for i, p in enumerate(ps):
        if i == 1:
            continue                                      # torch counts that tensor's steps separately (5 of 6): not the kernels' contract
        assert (ref.p[i] - p.detach()).abs().max() <= 1e-15
        assert (ref.m[i] - adam.state[p]["exp_avg"]).abs().max() <= 1e-15
        assert (ref.v[i] - adam.state[p]["exp_avg_sq"]).abs().max() <= 1e-16


def test_training_exports():
    assert training.HipAdam is HipAdam and training.Trainer is Trainer
    assert os.path.exists(os.path.join(_lib.INCLUDE_DIR, "ns2hip_optim.h")) and "ns2hip_optim.h" in _lib.HEADERS


def test_second_header_is_plain_c_and_a_c_caller_links(tmp_path):
    """include/ns2hip_optim.h compiles as C99 on its own, a C program links against the library, runs the host arithmetic and gets
    argument errors back as codes; the ctypes mirrors of its two structs have the header's layout"""
    import shutil
    if shutil.which("gcc") is None or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs gcc and the built library")
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "ns2hip_optim.h"
int main(void) {
  ns2_optim_tensor t[2] = {{0, 0, 0, 0, 0, 4097}, {0, 0, 0, 0, 0, 0}};
  ns2_optim_config cfg = {0.9, 0.99, 1e-8, 1.0, 10};
  long long chunks = (long long)ns2_optim_chunks(t, 2);
  printf("%lld %lld %d %d\n", chunks, (long long)ns2_optim_table_bytes(2, chunks), ns2_optim_step(0, 2, chunks, 0, &cfg, 0),
         ns2_optim_mark(0, 0));
#define OFF(s, f) (int)offsetof(s, f)
  printf("%d %d %d %d %d %d %d\n", (int)sizeof(ns2_optim_tensor), OFF(ns2_optim_tensor, grad), OFF(ns2_optim_tensor, ema), OFF(ns2_optim_tensor, numel),
         (int)sizeof(ns2_optim_config), OFF(ns2_optim_config, max_grad_norm), OFF(ns2_optim_config, ema_update_every));
  return 0;
}
''')
    exe, libdir = tmp_path / "caller", os.path.dirname(_lib.LIB_PATH)
    inc = _lib.INCLUDE_DIR
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)], check=True)
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lns2hip", "-Wl,-rpath," + libdir], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.split()]
    T, C = _lib.OptimTensor, _lib.OptimConfig
    assert out[:4] == [2, 2 * 48 + 2 * 16 + 2 * 4, _lib.NS2_ERR_ARG, _lib.NS2_ERR_ARG], out
    assert out[4:] == [ctypes.sizeof(T), T.grad.offset, T.ema.offset, T.numel.offset, ctypes.sizeof(C), C.max_grad_norm.offset, C.ema_update_every.offset], out
