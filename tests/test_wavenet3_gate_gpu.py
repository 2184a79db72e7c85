"""The lean Wavenet block kernel's own gate and early phase-2 prologue (csrc/wavenet3_kernel.h: wn3::midgate, wn3::Gate) against
gemm2_kernel<2, EPI_WAVENET, true, 1>, which keeps the generic wavenet_midgate (gemm_epi.h) behind its first K phase: same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, _lib, ops  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402

DEV = torch.device("cuda:0")


def _force(k):
    _lib.check(_lib.load().ns2_debug_force_gemm(k), "ns2_debug_force_gemm")


# B, N, d, dil: one workgroup whose only tile is a first tile | a non-first row tile behind a first one, two utterances with their own FiLM
# rows | two column tiles (the second workgroup's parameters are the upper 256 columns), tap 0's whole first tile in front of the
# utterance | an odd number of row tiles: a tile's utterance is not its parity
@pytest.mark.parametrize("B,N,d,dil", [(1, 256, 256, 1), (2, 512, 256, 2), (2, 256, 512, 128), (3, 256, 256, 64)])
def test_wavenet3_gate_equals_gemm2_bit_for_bit(B, N, d, dil):
    """Biases and FiLM rows of magnitude ~1 and both signs; every fifth row of x scaled by 8, so that h < 0, h > 0 and u = exp(-|h|) -> 0
    all occur.  The packed output buffers of the two kernels are compared with torch.equal."""
    g = torch.Generator().manual_seed(1000 + 7 * d + dil + B)
    M = B * N
    x = torch.randn(M, d, generator=g)
    x[::5] *= 8.0
    wc = torch.randn(d, d, 3, generator=g) * (3 * d) ** -0.5
    wr = torch.randn(d, d, 1, generator=g) * d ** -0.5
    bc, br = torch.randn(d, generator=g), torch.randn(d, generator=g)
    film = torch.randn(B, 2 * d, generator=g)
    a = ops.split(x.to(DEV), precision=4)
    pw = ops.PackedWeight(wc.to(DEV), extra1x1=wr.to(DEV), precision=4).tile_wavenet()
    outs = {}
    try:
        for k in (5, 2):
            _force(k)
            outs[k] = ops.wavenet_block(pw, a, N, dil, bc.to(DEV), br.to(DEV), film.to(DEV), precision=5).buf.clone()
    finally:
        _force(0)
    assert torch.isfinite(ops.join(ops.Planes(outs[2], M, d, True, "h8"), d)).all()
    assert torch.equal(outs[5], outs[2]), "lean Wavenet block kernel differs from gemm2_kernel<2, EPI_WAVENET, true, 1>"
    # the inputs do what the docstring says: the gate's argument takes both signs and reaches |h| where u underflows towards 0
    xh = x.half().double().reshape(B, N, d).transpose(1, 2)
    h = torch.nn.functional.conv1d(torch.nn.functional.pad(xh, (2 * dil, 0)), wc.half().double(), bc.double(), dilation=dil)
    h = h * film.double()[:, :d, None] + film.double()[:, d:, None]
    assert (h < 0).any() and (h > 0).any() and h.abs().max() > 20.0


def test_wavenet3_stack_in_the_model_equals_gemm2_bit_for_bit():
    """A whole hybrid forward at dim 256, 2 x 512 frames: the Wavenet stacks run as grid-z launches with per-layer bias, FiLM and dilation
    strides -- the only path to those.  The lean kernels forced on against the 256 x 256 kernel forced on: the same output bits."""
    m = Model(dim=256, depth=1, precision="hybrid")
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=131))
    m = m.to(DEV).eval()
    x = make_input("x", (2, 512, 256), seed=132).to(DEV)
    t = make_input("times", (2,), seed=132, uniform=True).to(DEV)
    ys = {}
    try:
        with torch.no_grad():
            for k in (5, 2):                     # 5: the dedicated kernels whatever the size, 2: gemm2_kernel for everything; neither splits K
                _force(k)
                ys[k] = m(x, t).clone()
    finally:
        _force(0)
    assert torch.isfinite(ys[5]).all()
    assert torch.equal(ys[5], ys[2])
