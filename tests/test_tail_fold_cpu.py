"""The Wavenet tail fold and the wide RMSNorm kernel (include/ns2hip.h) on the host: the chain rule and the skip rule see the
folded launch list, the switches refuse what they do not know, and the new header is plain C99."""
import ctypes
import os
import shutil
import subprocess

import pytest

from naturalspeech2_pytorch_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HYBRID, EXACT, MIXED, HALF = 5, 3, 4, 2
ENTRIES = ["ns2_debug_force_norm", "ns2_debug_force_tail_fold", "ns2_debug_norm_last", "ns2_tail_fold"]


def _cfg(dim=512, depth=12, precision=HYBRID, cond=False):
    return _lib.ModelConfig(dim=dim, depth=depth, dim_head=64, heads=8, ff_mult=4, wavenet_layers=8, wavenet_stacks=4, dim_cond_mult=4,
                            condition_on_prompt=int(cond), dim_prompt=512 if cond else 0, num_latents_m=32, resampler_depth=2,
                            precision=precision)


def _rule(B, N, **kw):
    cfg, n = _cfg(**kw), ctypes.c_int(-1)
    _lib.check(_lib.load().ns2_debug_chain_rule(ctypes.byref(cfg), B, N, ctypes.byref(n)), "ns2_debug_chain_rule")
    return n.value


def _skip_rule(B, N, **kw):
    cfg, n = _cfg(**kw), ctypes.c_int(-1)
    _lib.check(_lib.load().ns2_debug_skip_rule(ctypes.byref(cfg), B, N, ctypes.byref(n)), "ns2_debug_skip_rule")
    return n.value


def test_header_table_and_exports():
    assert set(ENTRIES) <= set(_lib.header_symbols("ns2hip.h"))
    lib = _lib.load()
    assert lib.ns2_version() >= 125
    assert lib.ns2_debug_force_tail_fold(2) != 0 and b"ns2_debug_force_tail_fold" in lib.ns2_last_error()
    assert lib.ns2_debug_force_norm(-1) != 0 and b"ns2_debug_force_norm" in lib.ns2_last_error()
    assert lib.ns2_tail_fold(None, None, None, None, 64, 8, None, None, None) != 0 and b"ns2_tail_fold" in lib.ns2_last_error()
    assert lib.ns2_debug_force_tail_fold(1) == 0 and lib.ns2_debug_force_norm(0) == 0
    assert lib.ns2_debug_norm_last() in (0, 1, 2)


def test_chain_rule_and_skip_rule_with_the_tail_folded_and_not():
    """32 x 1024 frames at d512 run as two chains with the one tail product (each chain's 64 x 2 blocks keep the lean linear kernel in the
    mixed plans, the 256 x 256 kernel in the others) as they do with the two; the shapes that gave one chain still give one"""
    lib = _lib.load()
    others = [dict(B=32, N=1024, dim=128, depth=6), dict(B=8, N=2048), dict(B=2, N=256, dim=128, depth=2), dict(B=64, N=512, precision=EXACT),
              dict(B=33, N=1024), dict(B=2, N=16384)]
    verdicts = {}
    try:
        for fold in (1, 0):
            _lib.check(lib.ns2_debug_force_tail_fold(fold), "ns2_debug_force_tail_fold")
            for prec in (HYBRID, EXACT, MIXED, HALF, 6):
                assert _rule(32, 1024, precision=prec) == 2, (fold, prec)
            assert _rule(32, 1024, cond=True) == 2
            assert _rule(4, 1024) == 1                    # the whole batch splits K -- the folded tail too
            assert _rule(16, 1024) == 1
            assert _rule(32, 1000) == 1
            assert _rule(1, 1024) == 1
            assert _skip_rule(32, 1024) == 1 and _skip_rule(4, 1024) == 0 and _skip_rule(32, 1000) == 0
            verdicts[fold] = [(_rule(**kw), _skip_rule(**kw)) for kw in others]
    finally:
        lib.ns2_debug_force_tail_fold(1)
    assert verdicts[1] == verdicts[0], verdicts            # one chain where the two products gave one, two where they gave two


def test_a_c_caller_sees_the_entry_points(tmp_path):
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
  if (ns2_debug_force_tail_fold(1) != NS2_OK || ns2_debug_chain_rule(&cfg, 32, 1024, &two) != NS2_OK) return 2;
  printf("%d %d %d %d %d\n", ns2_version(), two, ns2_debug_force_tail_fold(7) == NS2_ERR_ARG, ns2_debug_force_norm(3) == NS2_ERR_ARG,
         ns2_tail_fold(0, 0, 0, 0, 1, 1, 0, 0, 0) == NS2_ERR_ARG);
  return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)], check=True)
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lns2hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    assert int(out[0]) >= 125 and out[1:] == ["2", "1", "1", "1"], out
