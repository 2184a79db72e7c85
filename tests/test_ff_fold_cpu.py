"""The feed-forward fold (include/ns2hip.h) on the host: the chain rule sees the folded product list, the switch refuses what it does
not know, and the new header is plain C99."""
import ctypes
import os
import shutil
import subprocess

import pytest

from naturalspeech2_pytorch_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HYBRID, EXACT, MIXED, HALF = 5, 3, 4, 2


def _rule(B, N, dim=512, depth=12, precision=HYBRID, cond=False):
    cfg = _lib.ModelConfig(dim=dim, depth=depth, dim_head=64, heads=8, ff_mult=4, wavenet_layers=8, wavenet_stacks=4, dim_cond_mult=4,
                           condition_on_prompt=int(cond), dim_prompt=512 if cond else 0, num_latents_m=32, resampler_depth=2,
                           precision=precision)
    n = ctypes.c_int(-1)
    _lib.check(_lib.load().ns2_debug_chain_rule(ctypes.byref(cfg), B, N, ctypes.byref(n)), "ns2_debug_chain_rule")
    return n.value


def test_header_table_and_exports():
    assert {"ns2_debug_force_fold", "ns2_ff_fold"} <= set(_lib.header_symbols("ns2hip.h"))
    lib = _lib.load()
    assert lib.ns2_version() >= 124
    assert lib.ns2_debug_force_fold(2) != 0 and b"ns2_debug_force_fold" in lib.ns2_last_error()
    assert lib.ns2_ff_fold(None, None, None, None, 64, 170, None, None, None) != 0 and b"ns2_ff_fold" in lib.ns2_last_error()
    assert lib.ns2_debug_force_fold(1) == 0


def test_chain_rule_with_the_fold_on_and_off():
    """32 x 1024 frames at d512 run as two chains with the folded product (each chain's 64 x 2 blocks keep the dedicated conv kernel in the
    half plans, the 256 x 256 kernel in the others), as they do with the two products; the small shapes keep their verdicts"""
    lib = _lib.load()
    try:
        for fold in (1, 0):
            _lib.check(lib.ns2_debug_force_fold(fold), "ns2_debug_force_fold")
            for prec in (HYBRID, EXACT, MIXED, HALF, 6):
                assert _rule(32, 1024, precision=prec) == 2, (fold, prec)
            assert _rule(32, 1024, cond=True) == 2
            assert _rule(4, 1024) == 1                    # the whole batch splits K -- the folded conv too, by K tiles of every tap
            assert _rule(16, 1024) == 1
            assert _rule(32, 1000) == 1
    finally:
        lib.ns2_debug_force_fold(1)


def test_a_c_caller_sees_the_fold_entry_points(tmp_path):
    """the header compiles as C99 with the new declarations, the entry points link, and a bad argument comes back as a code"""
    if shutil.which("gcc") is None or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs gcc and the built library")
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "ns2hip.h"
int main(void) {
  int two = -1;
  ns2_model_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.dim = 512; cfg.depth = 12; cfg.dim_head = 64; cfg.heads = 8; cfg.ff_mult = 4; cfg.wavenet_layers = 8; cfg.wavenet_stacks = 4;
  cfg.dim_cond_mult = 4; cfg.num_latents_m = 32; cfg.resampler_depth = 2; cfg.precision = 5;
  if (ns2_debug_force_fold(1) != NS2_OK || ns2_debug_chain_rule(&cfg, 32, 1024, &two) != NS2_OK) return 2;
  printf("%d %d %d %d\n", ns2_version(), two, ns2_debug_force_fold(7) == NS2_ERR_ARG, ns2_ff_fold(0, 0, 0, 0, 1, 1, 0, 0, 0) == NS2_ERR_ARG);
  return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)], check=True)
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lns2hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    assert int(out[0]) >= 124 and out[1:] == ["2", "1", "1"], out
