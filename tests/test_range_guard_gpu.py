"""The IEEE-half range guard on the MI355X: every counter the library registers is read, by `ns2_saturation_count` and by
`ns2_saturation_peek` alike -- including the ones of aligner.hip (`relu_split`) and duration_pitch.hip (GroupNorm + SiLU), whose clamps
nothing read before the counters registered themselves.  Clamping is defined behaviour of the converting kernels, not a fault."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import _lib, ops  # noqa: E402
from naturalspeech2_pytorch_amd._range_guard import RangePeek  # noqa: E402
from naturalspeech2_pytorch_amd.training import passes  # noqa: E402

DEV = torch.device("cuda:0")


def _count():
    return ops.saturation_count(reset=False, device=DEV)


def _big():
    x = torch.zeros(32, 32, device=DEV)
    x[3, 5] = 1e5                                  # beyond 65504 (half) and 57344 (e5m2)
    return x


def _peek_words():
    lib = _lib.load()
    n = lib.ns2_saturation_counters()
    words = torch.full((n,), -1, dtype=torch.int32).pin_memory()
    with torch.cuda.device(DEV):
        _lib.check(lib.ns2_saturation_peek(words.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "ns2_saturation_peek")
        torch.cuda.current_stream().synchronize()
    return words


def test_every_registered_counter_is_read():
    with torch.cuda.device(DEV):
        ops.relu_split(_big(), precision=4)                      # at least one counter is non-zero
    words = _peek_words()
    assert (words >= 0).all() and int(words.sum()) == _count() >= 1
    pk = RangePeek().take(DEV)                                   # the package's own peek sees the same words
    pk.wait()
    assert pk.done() and pk.words.numel() == words.numel() and pk.total() == int(words.sum())
    ops.saturation_count(reset=True, device=DEV)
    assert int(_peek_words().sum()) == 0 and _count() == 0


@pytest.mark.parametrize("p", [2, 4, 3])
def test_relu_split_clamps_are_counted(p):
    with torch.cuda.device(DEV):
        before = _count()
        ops.relu_split(_big(), precision=p)
        new = _count() - before
    print(f"relu_split precision {p}: {new} new")
    assert (new == 0) if p == 3 else (new >= 1)                    # bf16 planes (3) have the fp32 exponent range


@pytest.mark.parametrize("p", [2, 4])
def test_groupnorm_silu_clamps_are_counted(p):
    x = torch.randn(32, 32, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.cuda.device(DEV):
        new = []
        for w in (torch.full((32,), 1e6, device=DEV), torch.ones(32, device=DEV)):
            before = _count()
            ops.groupnorm_silu(x, 1, weight=w, bias=torch.zeros(32, device=DEV), groups=8, want_f32=False, precision=p)
            new.append(_count() - before)
    print(f"groupnorm_silu precision {p}: {new[0]} new with weight 1e6, {new[1]} with weight 1")
    assert new[0] >= 1 and new[1] == 0


def test_training_snapshot_sees_a_clamp():
    with torch.cuda.device(DEV):
        sc = passes._Scale(DEV.index)
        assert sc._before is not None
        ops.relu_split(_big(), precision=4)
        assert sc.overflowed()
        assert not passes._Scale(DEV.index).overflowed()         # a fresh snapshot, nothing in between
