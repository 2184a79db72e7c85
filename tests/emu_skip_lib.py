"""A stand-in for the loaded library under Model's inference forward, for the CPU tests of `ragged_skip` (tests/test_ragged_skip_cpu.py):
every entry records its name and returns NS2_OK and writes nothing: the tensor a forward returns is uninitialised, the tests look at the
recorded names alone.  `plumbed(model)` puts it, and stubs of the three device-side helpers of the forward, in place and takes them out again."""
import contextlib
import ctypes
import types

import torch

from naturalspeech2_pytorch_amd import _lib


class RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ns2_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return _lib.NS2_OK
        return entry


@contextlib.contextmanager
def plumbed(m):
    """Model `m` (on the CPU) with its HIP forward reaching a RecordingLib instead of libns2hip; yields the recorder"""
    rec = RecordingLib()
    ns = types.SimpleNamespace(handle=ctypes.c_void_p(1), ws=None, cond_cache={})
    saved = (_lib.load, torch.cuda.current_stream)          # (model.py's `_lib` is this module: one patch serves both)
    m._guards = lambda: None
    m._ensure_native = lambda: ns
    m._workspace = lambda ns_, B, N, n_p, n_c: torch.zeros(16, dtype=torch.uint8)
    m._after_hip_forward = lambda ns_: None
    _lib.load = lambda: rec
    torch.cuda.current_stream = lambda *a, **k: types.SimpleNamespace(cuda_stream=0)
    try:
        yield rec
    finally:
        _lib.load, torch.cuda.current_stream = saved
        for name in ("_guards", "_ensure_native", "_workspace", "_after_hip_forward"):
            m.__dict__.pop(name, None)
