"""The chain rule of the denoiser step (csrc/model_exec.cpp chains_by_rule) on the host: when does a forward run its row-dependent
part as two utterance chains?  Only where every product of the step keeps, for each chain's M, the kernel it takes for the whole
batch, none splits K, and each chain is whole 256-row tiles.  ns2_debug_chain_rule evaluates it for a configuration without a device."""
import ctypes
import os
import shutil
import subprocess

import pytest

from naturalspeech2_pytorch_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HYBRID, EXACT = 5, 3


def _rule(B, N, dim=512, depth=12, precision=HYBRID, cond=False):
    cfg = _lib.ModelConfig(dim=dim, depth=depth, dim_head=64, heads=8, ff_mult=4, wavenet_layers=8, wavenet_stacks=4, dim_cond_mult=4,
                           condition_on_prompt=int(cond), dim_prompt=512 if cond else 0, num_latents_m=32, resampler_depth=2,
                           precision=precision)
    n = ctypes.c_int(-1)
    _lib.check(_lib.load().ns2_debug_chain_rule(ctypes.byref(cfg), B, N, ctypes.byref(n)), "ns2_debug_chain_rule")
    return n.value


def test_chain_rule_host_arithmetic():
    assert _rule(32, 1024) == 2                       # the headline: every product stays on its dedicated kernel (narrowest: 512 tiles of 128 x 128)
    assert _rule(32, 1024, precision=EXACT) == 2      # ... and on the 256 x 256 kernel in the exact plan
    assert _rule(32, 1024, cond=True) == 2            # the conditioned model: the cross-attention products too
    assert _rule(33, 1024) == 2                       # uneven chains 17 + 16
    assert _rule(1, 1024) == 1                        # nothing to halve
    assert _rule(4, 1024) == 1                        # the whole batch splits K (one scratch region: not for two chains)
    assert _rule(16, 1024) == 1                       # 8 x 1024 rows x 512 columns = 64 blocks of 256 x 256: a chain would take the 128 x 128 kernel
    assert _rule(32, 1000) == 1                       # M no multiple of 256: a chain boundary would cut a row tile
    assert _rule(2, 1000) == 1
    assert _rule(4, 256, dim=64, depth=2) == 1        # d64: the out-projection (K = 512) of 4 x 256 rows splits K
    assert _rule(32, 1024, dim=128, depth=6) == 1     # d128: the residual updates fuse their norm on the 128 x 128 kernel at full batch ...
    lib = _lib.load()
    cfg = _lib.ModelConfig(dim=64, depth=1, dim_head=48, heads=2, precision=HYBRID)
    n = ctypes.c_int(-1)
    assert lib.ns2_debug_chain_rule(ctypes.byref(cfg), 2, 256, ctypes.byref(n)) != 0          # a configuration ns2_model_create refuses
    assert lib.ns2_debug_chain_rule(None, 2, 256, ctypes.byref(n)) != 0
    assert lib.ns2_debug_force_chains(3) != 0 and b"ns2_debug_force_chains" in lib.ns2_last_error()
    assert lib.ns2_debug_force_chains(0) == 0


def test_chain_rule_follows_the_gemm_hook():
    """small shapes split K by default; with the split switched off (ns2_debug_force_gemm 3 / 5: what the GPU tests of the chains use)
    every product of 2 x 256 and 3 x 256 frames keeps its kernel per chain"""
    lib = _lib.load()
    assert _rule(2, 256, depth=1) == 1
    try:
        for mode in (3, 5):
            _lib.check(lib.ns2_debug_force_gemm(mode), "ns2_debug_force_gemm")
            for prec in (HYBRID, EXACT):
                assert _rule(2, 256, depth=1, precision=prec) == 2
                assert _rule(3, 256, depth=1, precision=prec) == 2
            assert _rule(2, 256, dim=64, depth=2, cond=True) == 2
            assert _rule(2, 200, depth=1) == 1
    finally:
        lib.ns2_debug_force_gemm(0)


def test_a_c_caller_sees_the_chain_entry_points(tmp_path):
    """the additions of ABI 121 from plain C: the header compiles as C99, the entry points link, the rule runs without a device, and a
    bad argument comes back as a code"""
    if shutil.which("gcc") is None or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs gcc and the built library")
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "ns2hip.h"
int main(void) {
  typedef void (*fn_t)(void);
  fn_t fns[] = {(fn_t)ns2_debug_force_chains, (fn_t)ns2_debug_chains_last, (fn_t)ns2_debug_chain_rule};
  int n = 0, two = -1, one = -1;
  ns2_model_config cfg;
  for (unsigned i = 0; i < sizeof fns / sizeof fns[0]; ++i) n += fns[i] != 0;
  memset(&cfg, 0, sizeof cfg);
  cfg.dim = 512; cfg.depth = 12; cfg.dim_head = 64; cfg.heads = 8; cfg.ff_mult = 4; cfg.wavenet_layers = 8; cfg.wavenet_stacks = 4;
  cfg.dim_cond_mult = 4; cfg.num_latents_m = 32; cfg.resampler_depth = 2; cfg.precision = 5;
  if (ns2_debug_chain_rule(&cfg, 32, 1024, &two) != NS2_OK || ns2_debug_chain_rule(&cfg, 4, 1024, &one) != NS2_OK) return 2;
  printf("%d %d %d %d %d %d\n", n, ns2_version(), two, one, ns2_debug_chains_last(), ns2_debug_force_chains(99) != NS2_OK);
  return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)], check=True)
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lns2hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    assert out[0] == "3" and int(out[1]) >= 121 and out[2:] == ["2", "1", "0", "1"], out
