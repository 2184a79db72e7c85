"""rmsnorm_wide_kernel (csrc/elementwise.hip; include/ns2hip.h) against rmsnorm_kernel through ns2_rmsnorm: the same bytes in
the planes and in the fp32 output, the same range-guard counts, nothing written outside the output, and the routing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 256                    # guard bytes in front of and behind every output (a multiple of 16: the outputs stay aligned)
SENTINEL = 0xA5
OLD, WIDE = 1, 2               # ns2_debug_norm_last
BYTES_PER_EL = {4: 4, 3: 4, 2: 2}      # FMT_H8 lines, interleaved bf16 hi | lo, dense IEEE half
GRID_ROWS = 1024 * 16          # the grid is at most 1024 workgroups of 16 rows: beyond, a workgroup strides to a second tile


def _force(k):
    _lib.check(_lib.load().ns2_debug_force_norm(k), "ns2_debug_force_norm")


def _guarded(nbytes):
    return torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)


def _norm(x, M, d, seq_len, gamma, cond, precision, want_f32, ldo=None, cond_ptr=None, cond_ld=None):
    """one ns2_rmsnorm launch into sentinel-filled, guarded buffers -> (plane bytes with guards, fp32 bytes with guards or None, kernel)"""
    ldo = ldo or d
    planes = _guarded(M * ldo * BYTES_PER_EL[precision])
    outf = _guarded(M * d * 4) if want_f32 else None
    hi = planes.data_ptr() + GUARD
    lo = hi + 64 if precision != 2 else None
    cp = cond_ptr if cond_ptr is not None else (cond.data_ptr() if cond is not None else None)
    cl = cond_ld if cond_ld is not None else (cond.shape[1] if cond is not None else 0)
    lib = _lib.load()
    _lib.check(lib.ns2_rmsnorm(x.data_ptr(), d, M, d, seq_len, gamma.data_ptr() if gamma is not None else None, cp, cl, hi, lo, ldo,
                               outf.data_ptr() + GUARD if want_f32 else None, d, precision, torch.cuda.current_stream().cuda_stream),
               "ns2_rmsnorm")
    torch.cuda.synchronize()
    return planes, outf, lib.ns2_debug_norm_last()


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _inputs(M, d, seq_len, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, d, generator=g)
    if M >= 5:
        x[1] = 0.0                           # the 1e-12 floor: every output of the row is 0 (or beta)
        x[2, d // 3] = float("nan")          # the whole row turns NaN: the range guard counts every pair of it
        x[3, 7] = 7e4                        # beyond the half range on the way in; the normalised row is not
    if M > GRID_ROWS + 16:                   # the same rows again in a workgroup's second tile
        x[GRID_ROWS + 6] = 0.0
        x[GRID_ROWS + 7, d // 3] = float("nan")
        x[GRID_ROWS + 9, 7] = 7e4
    B = (M + seq_len - 1) // seq_len
    gamma = torch.randn(d, generator=g) + 1.0
    cond = torch.randn(B, 2 * d, generator=g)
    cond[:, :d] += 1.0
    cond[0, d + 5] = 7e4                     # a beta beyond the half range: every row of utterance 0 clamps column 5
    return x.to(DEV), gamma.to(DEV), cond.to(DEV)


# seq_len: a multiple of the 16 rows a workgroup owns, with an utterance boundary inside every launch that has more than 16 rows
SHAPES = [(1, 16), (5, 16), (259, 16), (512, 256)]


ALL_COMBOS = ((True, False), (False, True), (True, True), (False, False))      # (gamma, cond)


def _compare(M, d, seq_len, precision, combos, seed):
    """hook 0 against hook 1 for one shape: kernels, plane bytes, fp32 bytes, guards, range-guard counts"""
    x, gamma, cond = _inputs(M, d, seq_len, seed=seed)
    for with_gamma, with_cond in combos:
        for want_f32 in (False, True):
            args = (x, M, d, seq_len, gamma if with_gamma else None, cond if with_cond else None, precision, want_f32)
            ops.saturation_count(reset=True)
            _force(0)
            p_new, f_new, k_new = _norm(*args)
            sat_new = ops.saturation_count(reset=True)
            _force(1)
            p_old, f_old, k_old = _norm(*args)
            sat_old = ops.saturation_count(reset=True)
            what = (M, d, precision, with_gamma, with_cond, want_f32)
            assert (k_new, k_old) == (WIDE, OLD), what
            assert torch.equal(p_new, p_old), what              # guards and sentinel-filled output compared as bytes
            assert _guards_intact(p_new) and _guards_intact(p_old), what
            assert not bool((p_new[GUARD:-GUARD] == SENTINEL).all()), what
            if want_f32:
                assert torch.equal(f_new, f_old) and _guards_intact(f_new), what
            assert sat_new == sat_old, (what, sat_new, sat_old)
            if precision != 3 and M >= 5:
                assert sat_old > 0, what                        # the NaN row (and the 7e4 beta) reached the guard


@pytest.mark.parametrize("precision", [4, 2, 3], ids=["h8", "f16", "bf16il"])
@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_wide_kernel_writes_the_old_kernels_bytes(d, precision):
    """d = 768: three 256-column chunks per lane; its dense-half row is 1536 bytes, the second kilobyte stored by half a wave"""
    try:
        for M, seq_len in SHAPES:
            _compare(M, d, seq_len, precision, ALL_COMBOS, seed=1000 + d + M)
    finally:
        _force(0)


@pytest.mark.parametrize("precision", [4, 2, 3], ids=["h8", "f16", "bf16il"])
def test_a_workgroup_that_strides_to_a_second_tile(precision):
    """M = 16384 + 3 * 16 + 5 rows: 1028 tiles on 1024 workgroups, so workgroups 0 ... 3 prefetch and run a second tile -- the last one five
    rows of a 16-row tile -- with its own conditioning row (utterances of 16 frames: every tile is another utterance), through the same LDS
    region.  d = 256 keeps it at 17 MB of input."""
    M = GRID_ROWS + 3 * 16 + 5
    try:
        _compare(M, 256, 16, precision, ((True, True), (False, True), (False, False)), seed=77)
    finally:
        _force(0)


def test_what_is_not_the_hot_case_keeps_the_old_kernel():
    M, d, seq_len = 64, 256, 16
    x, gamma, cond = _inputs(M, d, seq_len, seed=7)
    try:
        _force(0)
        assert _norm(x, M, d, seq_len, gamma, cond, 4, False)[2] == WIDE
        # d = 128
        x128 = torch.randn(M, 128, device=DEV)
        assert _norm(x128, M, 128, seq_len, None, None, 4, False)[2] == OLD
        # ldo > d: zero-padded planes
        p, _, k = _norm(x, M, d, seq_len, gamma, cond, 4, False, ldo=d + 32)
        assert k == OLD and _guards_intact(p)
        # a cond that is not 16-byte aligned
        flat = torch.zeros(cond.numel() + 1, device=DEV)
        flat[1:] = cond.reshape(-1)
        p_mis, _, k = _norm(x, M, d, seq_len, gamma, cond, 4, False, cond_ptr=flat.data_ptr() + 4, cond_ld=2 * d)
        assert k == OLD
        assert torch.equal(p_mis, _norm(x, M, d, seq_len, gamma, cond, 4, False)[0])      # ... and the same bytes from either kernel
        # utterances that are not whole 16-row tiles (with cond: the tile's conditioning row would not be one row)
        cond8 = torch.randn(M // 8, 2 * d, device=DEV)
        assert _norm(x, M, d, 8, gamma, cond8, 4, False)[2] == OLD
        assert _norm(x, M, d, 8, gamma, None, 4, False)[2] == WIDE                        # without cond seq_len is not read
        # dense bf16 planes (precision 1 through the op entry is interleaved; the dense form is reached by a null lo plane)
        planes = _guarded(M * d * 2)
        lib = _lib.load()
        _lib.check(lib.ns2_rmsnorm(x.data_ptr(), d, M, d, seq_len, None, None, 0, planes.data_ptr() + GUARD, None, d, None, d, 1,
                                   torch.cuda.current_stream().cuda_stream), "ns2_rmsnorm")
        torch.cuda.synchronize()
        assert lib.ns2_debug_norm_last() == OLD and _guards_intact(planes)
        _force(1)
        assert _norm(x, M, d, seq_len, gamma, cond, 4, False)[2] == OLD
    finally:
        _force(0)


def test_hook_refuses_what_it_does_not_know():
    lib = _lib.load()
    assert lib.ns2_debug_force_norm(2) != 0 and b"ns2_debug_force_norm" in lib.ns2_last_error()
    assert lib.ns2_debug_force_norm(0) == 0
