"""The Aligner's HIP kernels and forward(text=..., mel=..., pitch=...) on the MI355X: ns2_maximum_path bit for bit against the
reference's recorded paths and the package composite, ns2_align_attn against fp64 torch, the HIP Aligner and the training pass
against the reference's outputs (tests/golden/make_golden_aligner.py).  Reads stored fixtures only."""
import pytest
import torch

from tests.test_aligner_cpu import (_load, aligner_inputs, build_aligner, build_wrapper, check_grads, forward_inputs, lengths_mask,
                                    mp_value, rows_to_path, run_forward)

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)


@pytest.fixture(scope="module")
def cases():
    return _load("aligner_cases.pt")


def test_maximum_path_bit_equal_to_the_reference(cases):
    from naturalspeech2_pytorch_amd import ops
    for c in cases["maximum_path"]:
        t_x = c["shape"][1]
        path, dur = ops.maximum_path(mp_value(c).cuda(), c["text_lens"].cuda(), c["mel_lens"].cuda())
        assert torch.equal(path.cpu(), rows_to_path(c["rows"], t_x)), (c["kind"], c["shape"])
        assert torch.equal(dur.cpu(), c["durations"])


@pytest.mark.parametrize("t_x,t_y", [(256, 1024), (1024, 2048), (512, 8192)])
def test_maximum_path_bit_equal_to_the_composite(t_x, t_y):
    """B = 32, ragged lengths; (256, 1024) keeps the direction bits in LDS, the other two use the scratch buffer"""
    from naturalspeech2_pytorch_amd import ops
    from naturalspeech2_pytorch_amd.autograd_path import maximum_path_composite
    g = torch.Generator().manual_seed(t_x + t_y)
    B = 32
    tl = torch.randint(1, t_x + 1, (B,), generator=g)
    ml = torch.randint(1, t_y + 1, (B,), generator=g)
    tl[0], ml[0], tl[1], ml[1], tl[2] = t_x, t_y, t_x, t_y // 4, 0
    value = torch.rand(B, t_x, t_y, generator=g).softmax(1).cuda()
    path, dur = ops.maximum_path(value, tl.cuda(), ml.cuda())
    ref = maximum_path_composite(value, lengths_mask(tl, ml, t_x, t_y).cuda())
    assert torch.equal(path, ref)
    assert torch.equal(dur, ref.sum(-1).int())


def test_align_attn_against_fp64():
    from naturalspeech2_pytorch_amd import ops
    g = torch.Generator().manual_seed(5)
    B, T, n, C = 3, 150, 37, 80
    q, k = torch.randn(B * T, C, generator=g), torch.randn(B * n, C, generator=g)
    tl = torch.tensor([37, 20, 0])
    log, soft = ops.align_attn(q.cuda(), k.cuda(), tl.cuda(), B)
    d = torch.cdist(q.double().reshape(B, T, C), k.double().reshape(B, n, C))
    live = (torch.arange(n)[None] < tl[:, None])[:, None, :].expand(B, T, n)
    ref_log = d.masked_fill(~live, -torch.finfo(torch.float32).max)
    ref_soft = ref_log.softmax(-1).transpose(1, 2)
    got = log[:, 0].cpu().double()
    assert float((got - ref_log)[live].abs().max()) <= 1e-5 * float(d.abs().max())
    assert torch.equal(got[~live], ref_log[~live])
    assert float((soft.cpu().double() - ref_soft).abs().max()) <= 1e-5
    assert torch.equal(soft[2].cpu(), torch.full((n, T), 1. / n))          # fully masked: uniform


def test_hip_aligner_against_the_reference(cases):
    fx = cases["aligner"]
    m = build_aligner(fx).cuda()
    x, mel = aligner_inputs(fx)
    n, T = fx["x_shape"][1], fx["mel_shape"][2]
    x_mask = (torch.arange(n)[None] < fx["text_lens"][:, None])[:, None].cuda()
    y_mask = (torch.arange(T)[None] < fx["mel_lens"][:, None])[:, None].cuda()
    with torch.no_grad():
        hard, soft, log, path = m(x.cuda(), x_mask, mel.cuda(), y_mask)
    assert torch.equal(path.cpu(), rows_to_path(fx["rows"], n))
    assert torch.equal(hard.cpu(), fx["hard"])
    live = fx["log"] > -1e30
    assert float(((log.cpu() - fx["log"])[live]).abs().max()) <= 1e-3 * float(fx["log"][live].abs().max())
    assert float((soft.cpu() - fx["soft"]).abs().max()) <= 1e-3 * float(fx["soft"].abs().max())


@pytest.mark.parametrize("kind", ["int", "frac"])
def test_average_over_durations_hip(cases, kind):
    from naturalspeech2_pytorch_amd.aligner import average_over_durations
    c = cases["average"][kind]
    got = average_over_durations(c["pitch"].cuda(), c["durs"].cuda()).cpu()
    if kind == "int":
        assert torch.equal(got, c["avg"])
    else:
        assert float((got - c["avg"]).abs().max()) <= 1e-5 * float(c["avg"].abs().max())


def test_expand_backward_against_fp64_and_reproducible():
    from naturalspeech2_pytorch_amd import ops
    from naturalspeech2_pytorch_amd.autograd_path import f0_to_coarse
    g = torch.Generator().manual_seed(9)
    B, n, D, T = 4, 50, 512, 300
    dur = torch.randint(0, 9, (B, n), generator=g).float()
    pitch = 60 + 300 * torch.rand(B, n, generator=g)
    pitch[:, ::5] = 0.
    dc = torch.randn(B, D, T, generator=g)
    outs = [ops.expand_backward(dc.cuda(), dur.cuda(), pitch.cuda(), 256) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # fp64 reference: the 0/1 frame map of the durations, capped at T frames
    ends = dur.long().cumsum(1).clamp(max=T)
    starts = torch.nn.functional.pad(ends[:, :-1], (1, 0))
    f = torch.arange(T)
    m = ((f[None, None] >= starts[..., None]) & (f[None, None] < ends[..., None])).double()     # [B, n, T]
    d_enc = torch.einsum("bnt,bdt->bnd", m, dc.double())
    onehot = torch.nn.functional.one_hot(f0_to_coarse(pitch).long(), 256).double()               # [B, n, 256]
    d_tab = torch.einsum("bnk,bnd->kd", onehot, d_enc)
    assert float((outs[0][0].cpu().double() - d_enc).abs().max()) <= 1e-5 * float(d_enc.abs().max())
    assert float((outs[0][1].cpu().double() - d_tab).abs().max()) <= 1e-5 * float(d_tab.abs().max())


def test_text_forward_hip_against_the_reference():
    fx = _load("aligner_forward_d64.pt")
    d = build_wrapper(fx).cuda()
    loss = run_forward(d, fx, forward_inputs(fx), dev="cuda")
    assert abs(float(loss) - fx["loss"]) <= 1e-3 * abs(fx["loss"])
    loss.backward()
    check_grads(d, fx, 1e-3)
    assert all(p.grad is None for k, p in d.named_parameters() if k.startswith(("aligner.", "duration_pitch.")))


def test_text_training_step_d512():
    """d512 / L12 at 32 x 1024 mel frames, 256 phonemes: finite loss and gradients, the same loss as forward(cond=...) with the
    conditioning the HIP front end produced, and the composite alignment search's path on the same soft alignment"""
    from naturalspeech2_pytorch_amd import Model, NaturalSpeech2
    from naturalspeech2_pytorch_amd.aligner import create_mask
    from naturalspeech2_pytorch_amd.autograd_path import maximum_path_composite
    torch.manual_seed(0)
    B, n_ph, T = 32, 256, 1024
    dev = torch.device("cuda")
    d = NaturalSpeech2(Model(dim=512, depth=12, dim_prompt=512, condition_on_prompt=True, cond_drop_prob=0.), codec=None, target_sample_hz=24000,
                       build_aligner=True).to(dev).train()
    text = torch.randint(0, 150, (B, n_ph), device=dev)
    text_lens = torch.randint(n_ph // 2, n_ph + 1, (B,), device=dev)
    mel_lens = torch.randint(T // 2, T + 1, (B,), device=dev)
    mel = torch.randn(B, 80, T, device=dev)
    pitch = 80 + 300 * torch.rand(B, 1, T, device=dev)
    audio = torch.randn(B, T, 512, device=dev)
    prompt_enc = torch.randn(B, 64, 512, device=dev)
    times, noise = torch.rand(B, device=dev), torch.randn(B, T, 512, device=dev)
    for enc in (d.phoneme_enc,):
        enc.eval()                                   # no dropout: the two calls below must see the same conditioning
        enc.force_autograd = True
    kw = dict(prompt_enc=prompt_enc, times=times, noise=noise)
    cond = d.text_forward_cond(text, text_lens, mel, mel_lens, pitch, prompt_enc)[0].detach()   # the training call's own front end
    with torch.no_grad():
        ph = d.phoneme_enc(text)
        _, soft, _, path = d.aligner.forward_lengths(ph, text_lens.int(), mel, mel_lens.int())
    ref_path = maximum_path_composite(soft, (create_mask(text_lens, n_ph)[:, :, None] & create_mask(mel_lens, T)[:, None]).float())
    assert torch.equal(path, ref_path)
    loss = d(audio, text=text, text_lens=text_lens, mel=mel, mel_lens=mel_lens, pitch=pitch, **kw)
    loss_cond = d(audio, cond=cond, **kw)                 # the same HIP training path, conditioning handed over
    assert torch.isfinite(loss) and float(loss) == float(loss_cond)
    loss.backward()
    for k, p in d.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k
    assert d.pitch_emb.weight.grad is not None and d.phoneme_enc.transformer.layers[0][1].to_q.weight.grad is not None
