"""The IEEE-half range guard without a GPU: the library's counter registry (every source file that includes csrc/ns2_common.h registers
its counter when the library is loaded) and the host logic on top of `_range_guard.RangePeek`, with the peek substituted."""
import ctypes
import os
import types

import pytest
import torch

from naturalspeech2_pytorch_amd import _lib, _range_guard, training
from naturalspeech2_pytorch_amd.model import HipDenoiserMixin, _NativeState
from naturalspeech2_pytorch_amd.training import passes


def test_library_registry_names_every_guarded_source_file():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs the built library")
    lib = _lib.load()
    n = lib.ns2_saturation_counters()
    names = [lib.ns2_saturation_counter_name(i) for i in range(-1, n + 2)]
    assert names[0] is None and names[-1] is None and names[-2] is None          # outside 0 <= i < n
    names = [s.decode() for s in names if s is not None]
    assert len(names) == n
    assert {"gemm.hip", "gemm2.hip", "attention.hip", "elementwise.hip", "backward.hip", "aligner.hip", "duration_pitch.hip"} <= set(names)
    assert len(set(names)) == n                                                   # one counter per file
    assert not [s for s in names if s.endswith((".cpp", ".h"))]                   # host-only code and headers register nothing
    words = (ctypes.c_uint * n)(*([0xdead] * n))
    rc = lib.ns2_saturation_peek(words, n - 1, None)                              # too few words: refused before anything is enqueued
    assert rc != 0 and rc != _lib.NS2_UNAVAILABLE and b"ns2_saturation_peek" in lib.ns2_last_error()
    with pytest.raises(_lib.Ns2Error):
        _lib.check(rc, "ns2_saturation_peek")
    assert list(words) == [0xdead] * n


def test_training_pass_peeks_on_the_device_of_the_pass(monkeypatch):
    """`training_pass(4, like)` snapshots the counters of `like`'s device, and `overflowed()` asks the same device again -- whatever the
    current device is"""
    asked = []

    class Ev:
        def synchronize(self):
            pass

    def take(self, device=None):
        asked.append(device)
        self.words, self.event, self.device = torch.zeros(3, dtype=torch.int32), Ev(), device
        return self

    monkeypatch.setattr(_range_guard.RangePeek, "take", take)
    prev = training.set_backend(object())
    try:
        like = types.SimpleNamespace(is_cuda=True, device=torch.device("cuda", 1))
        with passes.training_pass(4, like) as p:
            assert asked == [1] and p.device == 1
        assert not p.scale.overflowed() and asked == [1, 1]
        with passes.training_pass(3, like) as p:                                  # exact arithmetic: no loss scale, no peek
            assert p.scale is None
        with passes.training_pass(4, torch.zeros(1)) as p:                        # a CPU tensor: the current device
            assert p.device is None
        assert asked == [1, 1, None]
    finally:
        training.set_backend(prev)


class _FakePeek:
    def __init__(self):
        self.flying, self.tot, self.taken = False, 0, []

    def take(self, device=None):
        self.taken.append(device)
        self.flying = True
        return self

    def in_flight(self):
        return self.flying

    def done(self):
        return True

    def wait(self):
        pass

    def total(self):
        return self.tot

    def drop(self):
        self.flying = False


class _Host(HipDenoiserMixin, torch.nn.Module):
    def __init__(self, precision):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.precision = precision
        self._native = _NativeState()


def test_check_saturation_raises_once_per_new_count():
    m = _Host("half")
    ns = m._native
    ns.sat_peek = pk = _FakePeek()
    m.check_saturation(sync=True)                          # nothing packed: nothing to guard
    assert pk.taken == []
    ns.handle = object()
    try:
        ns.sat_seen, pk.tot = 10, 13
        with pytest.raises(_lib.Ns2Error, match=r"^3 activation conversions left the IEEE-half range .* precision='half'"):
            m.check_saturation(sync=True)
        assert pk.taken == [m.w.device] and not pk.in_flight() and ns.sat_seen == 13
        m.check_saturation(sync=True)                      # the same total again: already accounted for
        assert len(pk.taken) == 2 and not pk.in_flight()
        m.check_saturation(sync=False)                     # no peek in flight: nothing to look at, and none is taken
        assert len(pk.taken) == 2
        pk.tot, pk.flying = 14, True                       # a peek taken behind a forward has arrived
        with pytest.raises(_lib.Ns2Error, match=r"^1 activation conversions"):
            m.check_saturation(sync=False)
        m.precision = "exact"                              # bf16 planes: not guarded
        pk.tot = 99
        m.check_saturation(sync=True)
        assert len(pk.taken) == 2
    finally:
        ns.handle = None
