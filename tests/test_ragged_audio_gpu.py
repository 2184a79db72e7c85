"""Ragged RAW AUDIO on the MI355X (include/ns2hip_audio.h, include/ns2hip_train.h): ns2_audio_to_mel_lens, ns2_pitch_yin_lens and ns2_rvq_ce_lens against the
entries without lengths on each utterance alone, the frozen codec's encode of a padded batch, and `NaturalSpeech2(ragged_audio=True)` end
to end -- eager, captured, and in the Trainer.  The definition under test: what utterance i yields in the padded batch is what it yields
alone, cut to its length; what lies at or behind a length (NaN included) reaches no value and no gradient before it; what is returned at
or behind a length is an exact 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import AudioToMel, EncodecWrapperHIP, Model, NaturalSpeech2, PitchExtractor, ops, training  # noqa: E402
from naturalspeech2_pytorch_amd.training import Trainer  # noqa: E402
from tests import pitch_ref64 as PR  # noqa: E402
from tests import rvq_ce_ref64 as R  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402
from tests.test_ragged_training_gpu import YARDSTICK  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300)).item()


def _behind(x, lens, value=NAN):
    y = x.clone()
    for i, s in enumerate(lens):
        y[i, s:] = value
    return y


def _lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- 8. ns2_audio_to_mel_lens
SMALL = dict(n_mels=40, n_fft=256, win_length=256, hop_length=64)


@pytest.mark.parametrize("cfg,L,lens", [(SMALL, 1024, [1024, 640, 192]), (dict(), 4096, [4096, 2400, 1024]), (SMALL, 4096, [4096, 1600, 2048])],
                         ids=["n_fft256", "default", "n_fft256_blocks"])
def test_audio_to_mel_lens_is_the_utterance_alone_bit_for_bit(cfg, L, lens):
    """n_fft 256 / hop 64, L 1024: 192 is just above n_fft / 2 (the clamp's floor is 129), and utterances 1 and 2 end inside the block
    (a block owns 32 frames; there are 17).  The default configuration at L 4096 likewise.  L 4096 at n_fft 256 makes 65 frames, three
    blocks: utterance 1 (26 frames) ends inside the first and leaves two blocks that only store zeros, utterance 2 (33 frames) has
    one frame in the second block"""
    mod = AudioToMel(**cfg)
    hop = mod.hop_length
    x = make_input("ragged_audio:mel", (3, L), seed=21).to(DEV)
    got = mod(x, lens=_lens(lens))
    assert got.shape == (3, mod.n_mels, 1 + L // hop) and torch.isfinite(got).all()
    for i, s in enumerate(lens):
        T = 1 + s // hop
        assert torch.equal(got[i, :, :T], mod(x[i:i + 1, :s].contiguous())[0]), f"utterance {i} ({s} samples)"
        assert torch.count_nonzero(got[i, :, T:]) == 0
    assert not torch.equal(got[1], mod(x)[1])               # the lengths are seen
    assert torch.equal(mod(_behind(x, lens), lens=_lens(lens)), got)
    assert torch.equal(mod(x, lens=lens), got)              # a list goes to the device


# ---- 9. ns2_pitch_yin_lens
def test_pitch_yin_lens_is_the_utterance_alone_bit_for_bit():
    fs, hop, L, lens = 24000, 160, 8000, [8000, 4800, 1600]
    mod = PitchExtractor(sample_rate=fs, hop_length=hop)
    x = torch.stack([PR.tone(f, fs, L) for f in (150., 220., 330.)])
    for i, s in enumerate(lens):                            # the condition on the inputs: not an equality of zeros
        assert int((PR.yin_ref64(x[i, :s], fs, hop, mod.threshold)["tau"] > 0).sum()) >= 1, i
    x = x.to(DEV)
    got = mod(x, lens=_lens(lens))
    assert got.shape == (3, 1 + L // hop)
    for i, s in enumerate(lens):
        T = 1 + s // hop
        alone = mod(x[i:i + 1, :s].contiguous())[0]
        assert torch.equal(got[i, :T], alone) and int((alone > 0).sum()) >= 1, f"utterance {i} ({s} samples)"
        assert torch.count_nonzero(got[i, T:]) == 0
    assert not torch.equal(got[1], mod(x)[1])
    assert torch.equal(mod(_behind(x, lens), lens=_lens(lens)), got)


# ---- 10. ns2_rvq_ce_lens
CE_B, CE_N, CE_LENS, CE_Q, CE_C = 3, 272, [272, 130, 5], 8, 128


@pytest.fixture(scope="module")
def ce_case():
    """inputs made as tests/rvq_ce_ref64.case makes them (noise 0.5, targets = the fp64 nearest codes of the clean latents), and the fp64
    reference of each utterance alone.  816 rows = 7 workgroups of 128: rows 256 .. 383 straddle the boundary of utterances 0 and 1,
    rows 384 .. 511 the length of utterance 1 (row 402), rows 640 .. 767 lie wholly behind the length of utterance 2 (row 549)"""
    M = CE_B * CE_N
    cb = make_input("rvq_ce:lens:codebooks", (CE_Q, CE_C, R.D), seed=R.SEED) * (0.5 ** torch.arange(CE_Q, dtype=torch.float32))[:, None, None]
    lat = make_input("rvq_ce:lens:latents", (M, R.D), seed=R.SEED)
    x = lat + 0.5 * make_input("rvq_ce:lens:noise", (M, R.D), seed=R.SEED)
    idx, r = torch.zeros(M, CE_Q, dtype=torch.int64), lat.clone()
    for q in range(CE_Q):
        _, idx[:, q], _ = R.nearest64(r, cb[q])
        r = r - cb[q][idx[:, q]]
    x, idx = x.reshape(CE_B, CE_N, R.D), idx.reshape(CE_B, CE_N, CE_Q)
    refs = [R.reference(x[b, :n], cb, idx[b, :n]) for b, n in enumerate(CE_LENS)]
    return x, cb, idx, refs


def _ce(x, cb, idx, lens=None, need_grad=True, need_quantized=True):
    M = idx[..., 0].numel()
    cbd = cb.to(DEV).contiguous()
    kw = {} if lens is None else dict(lens=_lens(lens))
    out = ops.rvq_cross_entropy(x.reshape(M, -1).to(DEV).contiguous(), cbd, ops.rvq_prepare(cbd), idx.reshape(M, -1).to(DEV).contiguous(),
                                need_grad, need_quantized=need_quantized, **kw)
    return tuple(None if t is None else t.cpu() for t in out)


def test_rvq_ce_lens_rows_are_the_utterance_alone_and_the_padding_is_zero(ce_case):
    x, cb, idx, _ = ce_case
    loss, rows, quant, G = _ce(x, cb, idx, CE_LENS)
    rows, quant, G = rows.reshape(CE_B, CE_N, CE_Q), quant.reshape(CE_B, CE_N, R.D), G.reshape(CE_B, CE_N, R.D)
    assert torch.isfinite(loss)
    for b, n in enumerate(CE_LENS):
        _, rows_b, quant_b, _ = _ce(x[b:b + 1, :n], cb, idx[b:b + 1, :n])
        assert torch.equal(rows[b, :n], rows_b) and torch.equal(quant[b, :n], quant_b), b
        assert all(torch.count_nonzero(t[b, n:]) == 0 for t in (rows, quant, G)), b
        assert bool((G[b, :n].abs().sum(-1) > 0).all())
    # two launches are bit-identical; the loss does not depend on whether the gradient is asked for
    again = _ce(x, cb, idx, CE_LENS)
    assert all(torch.equal(a, b) for a, b in zip(again, (loss, rows.reshape(-1, CE_Q), quant.reshape(-1, R.D), G.reshape(-1, R.D))))
    loss3, rows3, quant3, G3 = _ce(x, cb, idx, CE_LENS, need_grad=False, need_quantized=False)
    assert G3 is None and quant3 is None and torch.equal(loss3, loss) and torch.equal(rows3, rows.reshape(-1, CE_Q))
    # -1 and NaN behind the lengths: the same bits
    got_n = _ce(_behind(x, CE_LENS), cb, _behind(idx, CE_LENS, -1), CE_LENS)
    assert all(torch.equal(a, b) for a, b in zip(got_n, again))
    # -1 before a length keeps the loud NaN, in that row alone
    bad = idx.clone()
    bad[1, 129, 2] = -1
    loss_b, rows_b, _, G_b = _ce(x, cb, bad, CE_LENS)
    rows_b, G_b = rows_b.reshape(CE_B, CE_N, CE_Q), G_b.reshape(CE_B, CE_N, R.D)
    assert torch.isnan(loss_b) and torch.isnan(rows_b[1, 129, 2]) and torch.isnan(G_b[1, 129]).all()
    ok = torch.ones(CE_B, CE_N, dtype=torch.bool)
    ok[1, 129] = False
    assert torch.isfinite(rows_b[ok]).all() and torch.isfinite(G_b[ok]).all()
    # full lengths: the rows of the entry without lengths, and its loss up to the order of the sum
    loss_f, rows_f, quant_f, G_f = _ce(x, cb, idx, [CE_N] * CE_B)
    loss_0, rows_0, quant_0, G_0 = _ce(x, cb, idx)
    assert torch.equal(rows_f, rows_0) and torch.equal(quant_f, quant_0) and torch.equal(G_f, G_0) and rel(loss_f, loss_0) < 1e-6


def test_rvq_ce_lens_against_fp64(ce_case):
    """tests/rvq_ce_ref64.py restated with the per-utterance means: loss = mean_b loss_b, G[b] = G_b / B (the reference of utterance b alone
    divides by its own row count), the magnitudes A likewise; the bounds are the ones tests/test_rvq_ce_gpu.py asserts"""
    x, cb, idx, refs = ce_case
    loss, rows, _, G = _ce(x, cb, idx, CE_LENS)
    rows, G = rows.reshape(CE_B, CE_N, CE_Q), G.reshape(CE_B, CE_N, R.D)
    k = dict(row_loss=0., G=0.)
    ref_loss = A_loss = 0.
    for b, (n, ref) in enumerate(zip(CE_LENS, refs)):
        pairs, rows_G, _ = R.compared(ref)
        k["row_loss"] = max(k["row_loss"], R.k_of(rows[b, :n], ref["row_loss"], ref["A_row"], pairs))
        k["G"] = max(k["G"], R.k_of(G[b, :n], ref["G"] / CE_B, ref["A_G"] / CE_B, rows_G[:, None].expand(n, R.D)))
        ref_loss = ref_loss + R.mixed_loss(ref, rows[b, :n]) / CE_B
        A_loss = A_loss + ref["A_loss"] / CE_B
    k["loss"] = R.k_of(loss, ref_loss, A_loss)
    print("ns2_rvq_ce_lens: K of the kernel: " + ", ".join(f"{n} {v:.2f} (allowed {R.k_gpu(n)})" for n, v in k.items()))
    for n, v in k.items():
        assert v <= R.k_gpu(n), (n, v)


# ---- 11. the codec
@pytest.fixture(scope="module")
def codec():
    """built as tests/test_ragged_front_gpu.py::test_raw_audio_prompt_frames_do_not_see_the_padding_samples builds it.  A freshly
    initialised EnCodec has all-zero codebooks -- every code 0, every quantized latent 0 -- so the quantizer gets codebooks of the
    encoder's own scale (halving per stage), or the codes, the latents and the RVQ term compared below would be constants"""
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    hf = tf.EncodecModel(tf.EncodecConfig()).eval().to(DEV)
    with torch.no_grad():
        c = EncodecWrapperHIP.from_hf(hf, hip_seanet=True).to(DEV).eval()
        scale = c.encoder(_wav()[:, None]).std()
        assert float(scale) > 0
        cb = make_input("ragged_audio:codebooks", (8, 1024, 128), seed=22) * (0.5 ** torch.arange(8, dtype=torch.float32))[:, None, None]
        return EncodecWrapperHIP(cb.to(DEV) * scale, encoder=c.encoder, decoder=c.decoder).to(DEV).eval()


HOP = EncodecWrapperHIP.seq_len_multiple_of
RAW_LENS = [8 * HOP, 7 * HOP]


def _wav():
    return make_input("wav", (2, 8 * HOP), seed=14).to(DEV) * 0.1


def test_codec_encode_of_a_padded_batch_is_the_utterance_alone(codec):
    """what `forward(raw, audio_lens=)` relies on: the causal SEANet encoder keeps an utterance's padding out of its frames"""
    wav = _wav()
    with torch.no_grad():
        enc = codec.encoder(_behind(wav, RAW_LENS)[:, None]).transpose(1, 2).clone()
        lat, codes, _ = codec(_behind(wav, RAW_LENS), return_encoded=True)
        for i, s in enumerate(RAW_LENS):
            f = s // HOP
            enc_i = codec.encoder(wav[i:i + 1, None, :s].contiguous()).transpose(1, 2).clone()
            lat_i, codes_i, _ = codec(wav[i:i + 1, :s].contiguous(), return_encoded=True)
            assert lat_i.shape[1] == f and lat_i.abs().sum() > 0 and codes_i.unique().numel() > 8
            assert torch.equal(enc[i, :f], enc_i[0]), f"encoder latents of utterance {i} ({f} frames)"
            assert torch.equal(lat[i, :f], lat_i[0]) and torch.equal(codes[i, :f], codes_i[0]), f"utterance {i} ({f} frames)"


# ---- 12. the wrapper end to end
def _diffusion(codec, **kw):
    m = Model(dim=128, depth=1, ragged_training=True)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=71))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", "exact"
    return m, NaturalSpeech2(m, codec=codec, timesteps=2, objective="eps", min_snr_loss_weight=False, ragged_audio=True, rvq_ce_backend="hip",
                             rvq_cross_entropy_loss_weight=0.1, **kw).to(DEV)


def _loss_and_grads(m, d, *a, **kw):
    for p in m.parameters():
        p.grad = None
    loss = d(*a, **kw)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_wrapper_raw_audio_with_audio_lens_is_the_mean_of_the_solo_losses(codec):
    """the bar: twice the equal-length batch-against-solo yardstick of tests/test_ragged_training_gpu.py (exact arithmetic)"""
    m, d = _diffusion(codec)
    wav = _wav()
    t, noise = make_input("times", (2,), seed=72, uniform=True).to(DEV), make_input("noise", (2, 8, 128), seed=73).to(DEV)
    loss, g = _loss_and_grads(m, d, wav, audio_lens=_lens(RAW_LENS), times=t, noise=noise)
    solo, gs = [], None
    for i, s in enumerate(RAW_LENS):
        l, gi = _loss_and_grads(m, d, wav[i:i + 1, :s].contiguous(), times=t[i:i + 1], noise=noise[i:i + 1, :s // HOP].contiguous())
        solo.append(l)
        gs = gi if gs is None else {k: gs[k] + gi[k] for k in gs}
    worst = ("loss", rel(loss, torch.stack(solo).mean()))
    for k in gs:
        worst = max(worst, (k, rel(g[k], gs[k] / 2)), key=lambda z: z[1])
    bound = 2 * YARDSTICK[("uncond", "exact")]
    print(f"raw audio_lens + RVQ term, loss and gradients vs the mean of the solos: worst {worst[0]} {worst[1]:.3e} (bound {bound:.3e})")
    assert torch.isfinite(loss) and set(g) == set(gs)
    loss_n, g_n = _loss_and_grads(m, d, _behind(wav, RAW_LENS), audio_lens=_lens(RAW_LENS), times=t, noise=_behind(noise, [8, 7]))
    assert torch.equal(loss_n, loss) and all(torch.equal(g_n[k], g[k]) for k in g)
    assert rel(_loss_and_grads(m, d, wav, times=t, noise=noise)[0], torch.stack(solo).mean()) > 1e-6      # the lengths are seen
    assert worst[1] <= bound, worst


# ---- 13. capture
def test_graphed_train_step_with_the_rvq_term_follows_rewritten_lengths(codec):
    """The frozen codec encodes OUTSIDE the graph: its SEANet encoder reads the LSTM's abort counter once per run (seanet.py), a host
    synchronisation that no capture admits -- with or without lengths.  What is captured is the step over the latents, the codec's codes
    and the frame counts, RVQ term on ns2_rvq_ce_lens included: the replay follows lengths rewritten in place, bit for bit."""
    m, d = _diffusion(codec)
    wav = _wav()
    with torch.no_grad():
        lat, codes, _ = codec(wav, return_encoded=True)
    t, noise = make_input("times", (2,), seed=72, uniform=True).to(DEV), make_input("noise", (2, 8, 128), seed=73).to(DEV)
    captured, other = _lens([8, 7]), _lens([7, 8])
    step = training.GraphedTrainStep(lambda au, co, ln, ts, no: d(au, codes=co, audio_lens=ln, times=ts, noise=no), (lat, codes, captured, t, noise), m)
    seen = []
    for lens in (other, captured):
        loss = step(lat, codes, lens, t, noise).detach().clone()
        grads = [None if gr is None else gr.detach().clone() for gr in step.grads]
        for p in m.parameters():
            p.grad = None
        loss_e = d(lat, codes=codes, audio_lens=lens, times=t, noise=noise)
        loss_e.backward()
        assert torch.isfinite(loss) and torch.equal(loss, loss_e.detach())
        for p, gr in zip(step.params, grads):
            assert (gr is None and p.grad is None) or torch.equal(gr, p.grad)
        seen.append(float(loss))
    assert seen[0] != seen[1]                               # the lengths do reach the loss
    # ... and it is the loss of the raw-audio call at the same lengths
    assert torch.equal(d(wav, audio_lens=_lens([8 * HOP, 7 * HOP]), times=t, noise=noise).detach(), loss)


def test_trainer_takes_dict_batches_of_raw_audio_with_audio_lens(codec, tmp_path):
    """the real optimizer on the batches of tests/test_ragged_audio_cpu.py's Trainer test: two eager steps"""
    m, d = _diffusion(codec)
    batches = [{"audio": make_input("wav", (2, 8 * HOP), seed=s) * 0.1, "audio_lens": torch.tensor(lens)}
               for s, lens in ((84, [8 * HOP, 7 * HOP]), (85, [7 * HOP, 8 * HOP]))]
    tr = Trainer(d, dataloader=batches, train_lr=1e-3, train_num_steps=2, use_ema=False, save_and_sample_every=0, results_folder=tmp_path,
                 use_graph=False)
    before = [p.detach().clone() for p in m.parameters()]
    losses = [float(tr.train_step()) for _ in range(2)]
    assert tr.step == 2 and all(l == l and abs(l) < float("inf") for l in losses)
    assert any(not torch.equal(a, p) for a, p in zip(before, m.parameters()))
