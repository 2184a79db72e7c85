"""`NaturalSpeech2` — the diffusion wrapper around `Model` for the denoising hot path (NS2:1160-1684), with the
reference's own call signatures:

    NaturalSpeech2(model, codec=None, *, timesteps=1000, use_ddim=True, noise_schedule='sigmoid', objective='v', ...)   NS2:1163-1197
    .sample(*, length, prompt=None, batch_size=1, cond_scale=1., text=None, text_lens=None)                              NS2:1457-1466
            (`length` may also be one frame count per utterance, or None with `text`: a ragged batch, see `sample`)
    .forward(audio, text=None, text_lens=None, mel=None, mel_lens=None, codes=None, prompt=None, pitch=None, ...)       NS2:1503-1515
    .ddim_sample(shape, prompt=None, time_difference=None, cond_scale=1., cond=None)                                     NS2:1380

What runs where.  The per-step path (Model + DDIM update), the codec's RVQ encode/decode, the two conditioning encoders
built from the plain Transformer (`prompt_enc` = SpeechPromptEncoder, `phoneme_enc` = PhonemeEncoder) and, with
`build_duration_pitch=True`, the DurationPitchPredictor and the length regulator behind `sample(text=...)` (NS2:1476-1483;
duration_pitch.py) and, with `build_aligner=True`, the Aligner and the expansion behind `forward(text=..., mel=..., pitch=...)`
(NS2:1524-1602; aligner.py) are HIP, and so is AudioToMel (audio_to_mel.py), which turns raw audio into the Aligner's mel
frames when `forward` gets no `mel`.  With `build_pitch_extractor=True`, PitchExtractor (pitch.py: an own YIN estimator on a HIP
kernel, no parity with pyworld / Kaldi claimed) gives the F0 of those frames when `forward` gets no `pitch`.  The rest of the
conditioning front-end — the tokenizer (OUT OF SCOPE) — is not rebuilt.  By default (no predictor: the state_dict
has no `duration_pitch.*` keys) and for `forward`, a caller hands over what those modules would have produced through two extra keyword arguments that the reference
signature tolerates (`forward` takes **kwargs):

    cond        [b, dim_prompt, n_c]   the frame-aligned phoneme+pitch conditioning (reference: `expand_encodings`, NS2:1449-1455)
    prompt_enc  [b, n_p, dim_prompt]   the encoded prompt (reference: `self.prompt_enc(prompt)`, NS2:1475 / 1543)

`text`, `text_lens`, `mel`, `mel_lens`, `pitch` are accepted as in the reference; only the branch that would need a module
that is not built (no `cond` given) raises, with a NotImplementedError naming it.  One difference from the reference: when
every predicted duration truncates to 0 frames, `sample(text=...)` raises a ValueError (the reference fails with a shape
error inside `cond_to_model_dim`).  `phoneme_enc`, `prompt_enc` and
`pitch_emb` are constructed like upstream (same state_dict keys; load reference checkpoints of a conditional wrapper with
`strict=False`, the out-of-scope members have no counterpart here).

MI355X-first: the per-step elementwise chain of the reference (NS2:1396-1430, ~10 passes over the latents) is ONE fused HIP
kernel (`ns2_ddim_step`), the step-invariant conditioning is computed once per `sample()`, and one denoising step (model +
update) can be captured into a HIP graph and replayed (`use_graph=True`).
"""
import math
import numbers
from functools import partial

import torch
from torch import nn
import torch.nn.functional as F

from . import ops
from .resample import Resample


def sigmoid_schedule(t, start=-3, end=3, tau=1, clamp_min=1e-9):      # NS2:1144-1148
    v_start = torch.tensor(start / tau).sigmoid()
    v_end = torch.tensor(end / tau).sigmoid()
    gamma = (-((t * (end - start) + start) / tau).sigmoid() + v_end) / (v_end - v_start)
    return gamma.clamp(min=clamp_min, max=1.)


def cosine_schedule(t, start=0, end=1, tau=1, clip_min=1e-9):
    """NS2:1136-1142.  Upstream applies `math.cos` to the tensor `t`, which raises for a batch of times (and returns a float
    without `.clamp` for a single one): the schedule cannot run there.  Evaluated with torch.cos, the evident intent."""
    power = 2 * tau
    v_start = math.cos(start * math.pi / 2) ** power
    v_end = math.cos(end * math.pi / 2) ** power
    output = torch.cos((t * (end - start) + start) * math.pi / 2) ** power
    output = (v_end - output) / (v_end - v_start)
    return output.clamp(min=clip_min)


def simple_linear_schedule(t, clip_min=1e-9):                           # NS2:1133-1134
    return (1 - t).clamp(min=clip_min)


_SCHEDULES = {"sigmoid": sigmoid_schedule, "cosine": cosine_schedule, "linear": simple_linear_schedule}


def _safe_div(numer, denom, eps=1e-10):                                  # NS2:1122-1123
    return numer / denom.clamp(min=eps)


def _is_denoiser(m):
    return all(hasattr(m, a) for a in ("forward_with_cond_scale", "dim", "condition_on_prompt")) and isinstance(m, nn.Module)


def _check_raw_sample_lens(codec, hop, lens, total, what, noun):
    """the one check of per-utterance SAMPLE counts of raw audio that the codec encodes as a padded batch (a raw-audio prompt of
    `sample(prompt_lens=)`, raw audio of `forward(audio_lens=)` with `ragged_audio=True`): every length, and the padded length, a
    positive multiple of the codec's hop, and at least `min_causal_prompt_frames` frames.  One host read."""
    ok = (total > 0 and total % hop == 0 and bool(((lens > 0) & (lens % hop == 0) & (lens <= total)).all().item()))
    if not ok:
        raise ValueError(f"{what}: every length, and the padded length {total}, must be a "
                         f"positive multiple of the codec's seq_len_multiple_of ({hop}) samples")
    least = int(getattr(codec, "min_causal_prompt_frames", 1))
    if least > 1 and not bool((lens >= least * hop).all().item()):
        raise ValueError(f"{what}: every {noun} must be at least {least} codec frames ({least * hop} "
                         f"samples) long -- the encoder's reflect padding mirrors that many of an utterance's first frames, and "
                         f"would read a shorter {noun}'s padding")


class NaturalSpeech2(nn.Module):
    def __init__(self, model, codec=None, *, tokenizer=None, target_sample_hz=None, timesteps=1000, use_ddim=True,
                 noise_schedule="sigmoid", objective="v", schedule_kwargs: dict = dict(), time_difference=0.,
                 min_snr_loss_weight=True, min_snr_gamma=5, train_prob_self_cond=0.9, rvq_cross_entropy_loss_weight=0.,
                 dim_codebook: int = 128, duration_pitch_dim: int = 512, aligner_dim_in: int = 80, aligner_dim_hidden: int = 512,
                 aligner_attn_channels: int = 80, num_phoneme_tokens: int = 150, pitch_emb_dim: int = 256,
                 pitch_emb_pp_hidden_dim: int = 512, calc_pitch_with_pyworld=True, mel_hop_length=160,
                 audio_to_mel_kwargs: dict = dict(), scale=1., duration_loss_weight=1., pitch_loss_weight=1.,
                 aligner_loss_weight=1., aligner_bin_loss_weight=0.,
                 encoder_precision="exact",            # not in the reference: precision mode of the HIP encoders (and predictor)
                 build_duration_pitch: bool = False,   # not in the reference: build the DurationPitchPredictor (sample(text=...))
                 build_aligner: bool = False,          # not in the reference: build the Aligner (forward(text=..., mel=..., pitch=...))
                 build_pitch_extractor: bool = False,  # not in the reference: build the PitchExtractor (forward(text=...) without pitch=; pitch.py, own YIN estimator)
                 encoder_train_backend="composite",    # not in the reference: "hip" trains phoneme_enc / prompt_enc on the HIP kernels (training/encoder_pass.py)
                 duration_pitch_train_backend="composite",    # not in the reference: "hip" trains the DurationPitchPredictor on them (training/duration_pitch_pass.py)
                 aligner_train_backend="composite",    # not in the reference: "hip" trains the Aligner and runs its two losses on them (training/aligner_pass.py)
                 rvq_ce_backend=None,                  # not in the reference: "composite" / "hip" sets codec.rq.backend, the RVQ cross-entropy term (csrc/rvq_ce.hip); None leaves the codec's own
                 ragged_audio: bool = False,           # not in the reference: forward(raw audio, audio_lens=samples) and audio_lens with the RVQ term (include/ns2hip_audio.h, include/ns2hip_train.h)
                 ragged_conditioning: bool = False):   # not in the reference: forward(text_lens=, prompt_lens=) trains on ragged text and prompts (include/ns2hip_train.h)
        super().__init__()
        assert _is_denoiser(model), "model must be a Model (this package's, or compat.HipBackedModel over the reference's class)"
        self.conditional = model.condition_on_prompt
        self.model = model
        self.codec = codec
        assert codec is not None or target_sample_hz is not None                      # NS2:1207
        self.target_sample_hz = codec.target_sample_hz if codec is not None else target_sample_hz
        self.seq_len_multiple_of = codec.seq_len_multiple_of if codec is not None else None

        if self.conditional:                                                          # NS2:1218-1240, in-scope members only
            from .encoders import PhonemeEncoder, SpeechPromptEncoder
            self.mel_hop_length = mel_hop_length
            from .audio_to_mel import AudioToMel                                       # NS2:1221-1230 (no parameters, no buffers)
            audio_to_mel_kwargs = dict(audio_to_mel_kwargs)                           # the caller's dict is not updated
            if self.target_sample_hz is not None:
                audio_to_mel_kwargs.update(sampling_rate=self.target_sample_hz)
            self.audio_to_mel = AudioToMel(n_mels=aligner_dim_in, hop_length=mel_hop_length, **audio_to_mel_kwargs)
            self.calc_pitch_with_pyworld = calc_pitch_with_pyworld                    # accepted and stored; selects nothing
            if build_pitch_extractor:                                                 # no parameters, no buffers
                from .pitch import PitchExtractor
                self.pitch_extractor = PitchExtractor(sample_rate=self.target_sample_hz, hop_length=mel_hop_length)
            self.phoneme_enc = PhonemeEncoder(tokenizer=tokenizer, num_tokens=num_phoneme_tokens, precision=encoder_precision,
                                              train_backend=encoder_train_backend)
            self.prompt_enc = SpeechPromptEncoder(dim_codebook=dim_codebook, precision=encoder_precision, train_backend=encoder_train_backend)
            self.pitch_emb = nn.Embedding(pitch_emb_dim, pitch_emb_pp_hidden_dim)
            self.aligner_bin_loss_weight = aligner_bin_loss_weight
            if build_duration_pitch:                                                  # NS2:1234
                from .duration_pitch import DurationPitchPredictor
                self.duration_pitch = DurationPitchPredictor(dim=duration_pitch_dim, precision=encoder_precision,
                                                             train_backend=duration_pitch_train_backend)
            if build_aligner:                                                         # NS2:1235, 1238-1239
                from .aligner import Aligner, BinLoss, ForwardSumLoss
                self.aligner = Aligner(dim_in=aligner_dim_in, dim_hidden=aligner_dim_hidden, attn_channels=aligner_attn_channels,
                                       precision=encoder_precision, train_backend=aligner_train_backend)
                self.aligner_loss = ForwardSumLoss(backend=aligner_train_backend)
                self.bin_loss = BinLoss(backend=aligner_train_backend)
        else:
            assert not build_aligner, "the Aligner belongs to a conditional model (condition_on_prompt=True)"
            assert not build_pitch_extractor, "the PitchExtractor belongs to a conditional model (condition_on_prompt=True)"

        assert codec is None or model.dim == codec.codebook_dim, \
            f"transformer model dimension {model.dim} must be equal to codec dimension {codec.codebook_dim}"   # NS2:1244
        self.dim = codec.codebook_dim if codec is not None else model.dim
        assert objective in {"x0", "eps", "v"}, "objective must be either predict x0 or noise"
        if noise_schedule not in _SCHEDULES:
            raise ValueError(f"invalid noise schedule {noise_schedule}")
        assert scale <= 1, "scale must be less than or equal to 1"
        assert use_ddim, "ddpm_sample is unrunnable in the reference (NS2:1361 NameError, NS2:1370 shape); only DDIM is provided"
        self.objective, self.noise_schedule, self.scale = objective, noise_schedule, scale
        self.schedule_kwargs = dict(schedule_kwargs)
        self.gamma_schedule = partial(_SCHEDULES[noise_schedule], **schedule_kwargs)
        self.timesteps, self.use_ddim, self.time_difference = timesteps, use_ddim, time_difference
        self.train_prob_self_cond = train_prob_self_cond
        self.min_snr_loss_weight, self.min_snr_gamma = min_snr_loss_weight, min_snr_gamma
        self.rvq_cross_entropy_loss_weight = rvq_cross_entropy_loss_weight
        self.ragged_audio = ragged_audio
        self.ragged_conditioning = ragged_conditioning
        if ragged_conditioning:                                                       # the switch goes on the members that take lengths under autograd
            for mod in (self.model, getattr(self, "prompt_enc", None), getattr(self, "phoneme_enc", None), getattr(self, "duration_pitch", None)):
                if mod is not None:
                    mod.ragged_conditioning = True
        if rvq_ce_backend is not None:
            assert codec is not None and hasattr(codec, "rq") and hasattr(codec.rq, "backend"), "rvq_ce_backend needs a codec whose rq has a backend (codec.py)"
            assert rvq_ce_backend in ("composite", "hip"), "rvq_ce_backend must be 'composite' or 'hip'"
            codec.rq.backend = rvq_ce_backend
        self.duration_loss_weight, self.pitch_loss_weight, self.aligner_loss_weight = \
            duration_loss_weight, pitch_loss_weight, aligner_loss_weight

    @property
    def device(self):
        return next(self.model.parameters()).device

    def get_sampling_timesteps(self, batch, *, device):                               # NS2:1303-1308
        times = torch.linspace(1., 0., self.timesteps + 1, device=device)
        times = times[None].expand(batch, -1)
        return [(times[:, i].contiguous(), times[:, i + 1].contiguous()) for i in range(self.timesteps)]

    def _fused_ddim_ok(self):
        """the fused HIP update evaluates the schedule on the device with the reference's default schedule parameters"""
        return not self.schedule_kwargs

    # ------------------------------------------------------------------ sampling (NS2:1379-1431)
    @torch.no_grad()
    def ddim_sample(self, shape, prompt=None, time_difference=None, cond_scale=1., cond=None, noise=None, use_graph=False,
                    on_saturation="demote", lens=None, prompt_lens=None):
        """`prompt` here is what the reference passes at NS2:1486-1491: the ENCODED prompt [b, n_p, dim_prompt].

        lens (not in the reference): frames per utterance of a ragged batch, integer [b], each in [1, shape[1]].  Every step hands
        them to the model (`Model.forward(lens=)`: the self-attention kernels read them on the device), so utterance i is denoised as
        it would be alone at lens[i] frames; latent frames at or beyond lens[i] come back as exactly 0.  A model with `ragged_skip = True`
        also skips the 256-row tiles wholly behind a length in every product of the step (model.py `Model`), eager and captured alike.

        prompt_lens (not in the reference): rows per utterance of the encoded prompt, integer [b], each in [1, n_p]; handed to the model
        (`Model.forward(prompt_lens=)`), whose conditioning then sees rows [0, prompt_lens[i]) of prompt i alone.

        on_saturation (not in the reference): what to do when a checkpoint's activations leave the IEEE-half range in one of the
        fast precisions (half / mixed / hybrid: conversions clamp at 65504 -- finite but wrong; the model counts them on the
        device).  "demote" (default): the run is REPEATED from the same initial latents with `model.precision = "exact"` (bf16
        planes keep the fp32 exponent range) and the model stays there -- a fast mode never returns clamped audio and never
        needs a hand-picked precision per checkpoint; "raise": Ns2Error, as rounds 2-3 did."""
        assert on_saturation in ("demote", "raise")
        from ._lib import Ns2Error
        batch, device = shape[0], self.device
        start = torch.randn(shape, device=device) if noise is None else noise.to(device).float().clone()
        if lens is not None:                             # one device buffer for the run: what a captured step keeps reading
            lens = torch.as_tensor(lens).to(device=device, dtype=torch.int32).contiguous()
            assert lens.shape == (batch,), f"lens must hold one frame count per utterance: [{batch}]"
        if prompt_lens is not None:                      # likewise: one tensor for the run, so the model's conditioning cache holds
            prompt_lens = torch.as_tensor(prompt_lens).to(device=device, dtype=torch.int32).contiguous()
            assert prompt_lens.shape == (batch,), f"prompt_lens must hold one prompt length per utterance: [{batch}]"
        for attempt in (0, 1):
            if hasattr(self.model, "refresh_weights"):
                self.model.refresh_weights()        # parameters rewritten through `.data` since the last pack (EMA) -> re-pack
            if hasattr(self.model, "clear_cond_cache"):
                self.model.clear_cond_cache()
            try:
                audio = self._ddim_loop(start.clone(), prompt, cond, cond_scale, use_graph, lens, prompt_lens)
                if lens is not None:
                    audio = audio.masked_fill(torch.arange(audio.shape[1], device=audio.device)[None, :, None] >= lens[:, None, None], 0.)
                if hasattr(self.model, "check_saturation") and audio.is_cuda:
                    # the model polls the device counters every few forwards on its own (any caller); the end of a run takes one
                    # synchronous look (Ns2Error on a new count)
                    self.model.check_saturation(sync=True)
                return audio
            except Ns2Error as e:
                guarded = getattr(self.model, "precision", "exact") in ("half", "mixed", "hybrid", "hybrid_ff")
                if on_saturation == "raise" or attempt == 1 or not guarded or "IEEE-half range" not in str(e):
                    raise
                import warnings
                warnings.warn(f"precision='{self.model.precision}': activations of this checkpoint leave the IEEE-half range; repeating "
                              f"the sampling run with precision='exact' and keeping the model there ({e})")
                self.model.precision = "exact"

    @staticmethod
    def _ragged_kw(lens, prompt_lens):
        """the lengths a step hands to the model: each keyword only when it was given, so a model without it is called as before"""
        kw = {} if lens is None else dict(lens=lens)
        if prompt_lens is not None:
            kw["prompt_lens"] = prompt_lens
        return kw

    def _ddim_loop(self, audio, prompt, cond, cond_scale, use_graph, lens=None, prompt_lens=None):
        batch, device = audio.shape[0], audio.device
        pairs = self.get_sampling_timesteps(batch, device=device)
        # `time_difference` only shifts times_next AFTER gamma_next was taken (NS2:1396-1406): it has no effect upstream either
        if not self._fused_ddim_ok():
            return self._ddim_sample_unfused(audio, pairs, prompt, cond, cond_scale, lens, prompt_lens)
        # the run's times are known here and shared by the batch, so every time-conditioning projection of the run is
        # computed once, ahead of the loop; step i reads row i (Model.time_table)
        table = None
        if hasattr(self.model, "time_table") and audio.is_cuda:
            table = self.model.time_table(torch.stack([p[0][0] for p in pairs]), batch)
        if use_graph:
            return self._ddim_sample_graph(audio, pairs, prompt, cond, cond_scale, table, lens, prompt_lens)
        ragged = self._ragged_kw(lens, prompt_lens)
        for i, (times, times_next) in enumerate(pairs):
            kw = dict(ragged) if table is None else dict(ragged, cond_row=table[i])
            out = self.model.forward_with_cond_scale(audio, times, prompt=prompt, cond_scale=cond_scale, cond=cond, **kw)
            ops.ddim_step(audio, out, times, times_next, self.objective, self.noise_schedule, self.scale, out=audio)
        return audio

    def _ddim_sample_unfused(self, audio, pairs, prompt, cond, cond_scale, lens=None, prompt_lens=None):
        """non-default `schedule_kwargs`: the schedule is evaluated by the host-side functions above, the model step is HIP"""
        ragged = self._ragged_kw(lens, prompt_lens)
        for times, times_next in pairs:
            g, gn = self.gamma_schedule(times)[:, None, None], self.gamma_schedule(times_next)[:, None, None]
            alpha, sigma = torch.sqrt(g) * self.scale, torch.sqrt(1 - g)
            alpha_n, sigma_n = torch.sqrt(gn) * self.scale, torch.sqrt(1 - gn)
            out = self.model.forward_with_cond_scale(audio, times, prompt=prompt, cond_scale=cond_scale, cond=cond, **ragged)
            x0 = {"x0": lambda: out, "eps": lambda: _safe_div(audio - sigma * out, alpha),
                  "v": lambda: alpha * audio - sigma * out}[self.objective]()
            eps = _safe_div(audio - alpha * x0, sigma)
            audio = x0 * alpha_n + eps * sigma_n
        return audio

    def _ddim_sample_graph(self, audio, pairs, prompt, cond, cond_scale, table=None, lens=None, prompt_lens=None):
        """one (model + DDIM update) step captured in a HIP graph; times (and the step's row of the conditioning table) are device
        buffers rewritten per step.  The lengths of a ragged batch are a device buffer the captured kernels read: nothing of the
        step reads them on the host.  The conditioning (prompt_lens included) is computed by the warm-up step, before the capture, and
        the captured step finds it in the model's cache."""
        t_buf, tn_buf = pairs[0][0].clone(), pairs[0][1].clone()
        row = table[0].clone() if table is not None else None
        kw = {} if row is None else dict(cond_row=row)
        kw.update(self._ragged_kw(lens, prompt_lens))
        step = lambda: ops.ddim_step(                                                   # noqa: E731
            audio, self.model.forward_with_cond_scale(audio, t_buf, prompt=prompt, cond_scale=cond_scale, cond=cond, **kw),
            t_buf, tn_buf, self.objective, self.noise_schedule, self.scale, out=audio)
        keep = audio.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                    # warm-up outside capture: packs weights, sizes workspaces
            step()
        torch.cuda.current_stream().wait_stream(side)
        audio.copy_(keep)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        audio.copy_(keep)
        for i, (times, times_next) in enumerate(pairs):
            t_buf.copy_(times)
            tn_buf.copy_(times_next)
            if row is not None:
                row.copy_(table[i])
            g.replay()
        return audio

    # ------------------------------------------------------------------ conditioning (NS2:1433-1455, 1474-1483)
    def process_prompt(self, prompt=None):                                            # NS2:1433-1447
        if prompt is None:
            return None
        assert self.model.condition_on_prompt
        is_raw_prompt = prompt.ndim == 2
        assert not (is_raw_prompt and self.codec is None), "codec must be passed in if one were to train on raw prompt"
        if is_raw_prompt:
            with torch.no_grad():
                self.codec.eval()
                prompt, _, _ = self.codec(prompt, curtail_from_left=True, return_encoded=True)
        return prompt

    def _prompt_frame_lens(self, prompt_lens, prompt, prompt_enc, trust_device=False):
        """sample(prompt_lens=) -> the lengths in rows of the encoded prompt, an integer tensor [b] on the model's device.  They count
        rows of `prompt_enc=`, frames of prompt latents [b, n_p, dim_codebook], samples of a raw-audio prompt [b, samples]: there the
        codec makes one frame of every `seq_len_multiple_of` samples, so each length and the padded length must be a positive multiple
        of it (one host read, before the loop).  trust_device (the training pass): lengths that arrive as a CUDA tensor are not read on
        the host, as `forward(audio_lens=)` trusts them."""
        lens = torch.as_tensor(prompt_lens)
        given = prompt_enc if prompt_enc is not None else prompt
        if lens.ndim != 1 or lens.dtype.is_floating_point or lens.shape[0] != given.shape[0]:
            raise ValueError(f"prompt_lens must hold one integer prompt length per utterance: [{given.shape[0]}]")
        lens = lens.to(self.device).long()
        if prompt_enc is None and prompt.ndim == 2:
            assert self.codec is not None, "codec must be passed in if one were to sample from a raw prompt"
            hop = int(self.seq_len_multiple_of)
            if not (trust_device and torch.as_tensor(prompt_lens).is_cuda):
                _check_raw_sample_lens(self.codec, hop, lens, prompt.shape[-1], "a raw-audio prompt with prompt_lens", "prompt")
            lens = lens // hop
        return lens

    def _resampler(self, sample_hz):
        """input_sample_hz= / prompt_sample_hz= -> the Resample to the codec's rate; None when there is nothing to convert"""
        if sample_hz is None or int(sample_hz) == int(self.target_sample_hz):
            return None
        return Resample(int(sample_hz), int(self.target_sample_hz))

    def _resample_raw(self, rs, x, lens=None):
        """raw audio [b, S] at another rate -> (the audio at the codec's rate, the lengths there).  Without lengths that is `rs(x)`.
        With `lens` (samples of the INPUT per utterance) utterance i is resampled as it is alone (Resample(lens=)), its length becomes
        out_lens(lens[i]) // hop * hop -- whole codec frames, formed where the lengths live, no host read -- and the batch is cut to
        whole frames too, so the values can go through _check_raw_sample_lens as lengths given at the codec's rate do."""
        if lens is None:
            return rs(x), None
        hop = int(self.seq_len_multiple_of)
        y = rs(x, lens=lens)
        return y[..., :y.shape[-1] // hop * hop], rs.out_lens(lens) // hop * hop

    def _encode_prompt(self, prompt, prompt_enc):
        if prompt_enc is not None:
            return prompt_enc
        assert prompt is not None, "conditional model: pass `prompt` (raw audio or codec latents) or `prompt_enc`"
        return self.prompt_enc(self.process_prompt(prompt))                            # NS2:1474-1475 / 1542-1543 (HIP encoder)

    def refresh_weights(self):
        """run boundary: every HIP module re-checks its packed weights against the parameters' CONTENT (writes through `.data` --
        what ema_pytorch does to the copy of this whole object it samples from, NS2:1793-1801 -- bump no version counter)"""
        for name in ("model", "prompt_enc", "phoneme_enc", "duration_pitch", "aligner", "codec"):
            mod = getattr(self, name, None)
            if mod is not None and hasattr(mod, "refresh_weights"):
                mod.refresh_weights()

    @torch.no_grad()
    def text_to_cond(self, text, prompt_enc, text_lens=None, return_lens=False, prompt_lens=None):
        """NS2:1476-1483: phoneme_enc(text) -> DurationPitchPredictor -> the length regulator (durations truncated to whole
        frames, pitch embedded through f0_to_coarse) -> the frame-aligned conditioning [b, dim_prompt, n_frames], n_frames = the
        longest utterance (one host read, the reference's `.item()`).  Every duration truncating to 0 frames leaves nothing to
        condition on: the reference fails there inside cond_to_model_dim; here it is a ValueError.
        Not in the reference (the ragged mode of `sample`): `text_lens` [b] -- phonemes at or beyond text_lens[i] contribute no
        frames (their predicted durations count as 0); `return_lens=True` -> (cond, the utterances' own frame totals, integer [b]).
        `prompt_lens` [b] (rows of prompt_enc per utterance) switches the ragged front-end on: the phoneme encoder gets the key mask of
        `text_lens` (missing: full) and the predictor both length vectors, so the durations and pitches of utterance i are what it
        gives alone with its text cut to text_lens[i] and its prompt to prompt_lens[i].  Without it, today's calls."""
        assert hasattr(self, "duration_pitch"), "construct NaturalSpeech2 with build_duration_pitch=True"
        if prompt_lens is not None:
            from .aligner import create_mask
            b, n = text.shape[0], text.shape[-1]
            text_lens = torch.full((b,), n, dtype=torch.long, device=text.device) if text_lens is None else \
                torch.as_tensor(text_lens).to(device=text.device).long().clamp(1, n)
            phoneme_enc = self.phoneme_enc(text, mask=create_mask(text_lens, n))
            duration, pitch = self.duration_pitch(phoneme_enc, prompt_enc, text_lens=text_lens,
                                                  prompt_lens=torch.as_tensor(prompt_lens).to(text.device))
        else:
            phoneme_enc = self.phoneme_enc(text)
            duration, pitch = self.duration_pitch(phoneme_enc, prompt_enc)
        if text_lens is not None:
            pad = torch.arange(duration.shape[1], device=duration.device)[None] >= torch.as_tensor(text_lens, device=duration.device)[:, None]
            duration = duration.masked_fill(pad, 0.)
        table = self.pitch_emb.weight
        if phoneme_enc.is_cuda:
            cond, totals = ops.length_regulate(duration.float().contiguous(), pitch.float().contiguous(),
                                               phoneme_enc.float().contiguous(), table.detach().float().contiguous(), return_totals=True)
        else:
            from .autograd_path import length_regulate
            cond, totals = length_regulate(duration, pitch, phoneme_enc, table, return_totals=True)
        if cond.shape[-1] == 0:
            raise ValueError("every predicted duration truncates to 0 frames: there is no aligned conditioning to sample from")
        return (cond, totals) if return_lens else cond

    @torch.no_grad()
    def sample(self, *, length=None, prompt=None, batch_size=1, cond_scale=1., text=None, text_lens=None,
               cond=None, prompt_enc=None, noise=None, use_graph=False, return_lens=False, prompt_lens=None, prompt_sample_hz=None):
        """NS2:1457-1501.  Extra keywords (not in the reference): `cond` / `prompt_enc` = pre-computed conditioning (module
        docstring), `noise` = injected initial latents (parity tests), `use_graph` = HIP-graph replay of the step.

        Ragged batches (not in the reference, which accepts `text_lens` and ignores it).  `length` an int: every utterance has that
        many frames, as upstream.  `length` a 1-D integer tensor / sequence of one frame count per utterance, or `length=None` with
        `text=` (the counts are then the utterances' own totals of predicted durations, and phonemes at or beyond `text_lens[i]`
        contribute no frames): the batch is denoised at max(length) frames with the counts handed to the self-attention kernels, so
        utterance i is what `sample` gives for it alone at its own length; its frames (samples, with a codec) past its end come back
        as exactly 0.  `return_lens=True` -> (audio, lens): integer [b], in frames without a codec, in samples with one.

        Ragged prompts and text (not in the reference): `prompt_lens`, integer [b], switches the ragged front-end on -- prompt i counts
        up to prompt_lens[i] and text i up to text_lens[i] (missing: full) in `prompt_enc`, `phoneme_enc`, the DurationPitchPredictor and
        the model's conditioning, so the whole result of utterance i is what `sample` gives for it alone with its own prompt and text; a
        batch whose prompts are all full but whose texts are ragged passes `prompt_lens` full.  The lengths count rows of `prompt_enc=`
        when that is given, frames of prompt latents [b, n_p, dim_codebook], and samples of a raw-audio prompt [b, samples] -- there
        each length, and the padded length, must be a positive multiple of the codec's `seq_len_multiple_of`, and at least the codec's
        `min_causal_prompt_frames` frames (7 for the 24 kHz SEANet: its reflect padding mirrors frames 1 .. 6) -- ValueError otherwise,
        one host check before the loop; the encoder being causal then keeps the padding out of an utterance's frames.
        Without `prompt_lens`, `text_lens` does exactly what it did: it zeroes the padding phonemes' durations.

        `prompt_sample_hz` (not in the reference): the rate of a raw-audio prompt.  Another rate than the codec's is resampled first
        (resample.py), before `process_prompt`; `prompt_lens` then count samples of the INPUT and become
        out_lens(prompt_lens) // seq_len_multiple_of * seq_len_multiple_of before the check above.  A prompt that is not raw audio
        has no rate: ValueError."""
        rs = self._resampler(prompt_sample_hz)
        if rs is not None:
            if prompt is None or prompt.ndim != 2 or prompt_enc is not None:
                raise ValueError(f"prompt_sample_hz={prompt_sample_hz}: only a raw-audio prompt [b, samples] has a sample rate to convert")
            prompt, prompt_lens = self._resample_raw(rs, prompt, prompt_lens)
        if length is None and (text is None or cond is not None):
            raise ValueError("sample(length=None) takes the utterances' lengths from the predicted durations: it needs text= (and no cond=)")
        lens = None
        if length is not None and not isinstance(length, numbers.Integral):
            lens = torch.as_tensor(length)
            if lens.ndim != 1 or lens.dtype.is_floating_point or lens.numel() == 0:
                raise ValueError("length must be an int or a 1-D integer tensor / sequence of one frame count per utterance")
            lens = lens.long()
        if prompt_lens is not None:
            if not self.conditional or (prompt is None and prompt_enc is None):
                raise ValueError("prompt_lens needs a prompt: a conditional model called with prompt= or prompt_enc=")
            prompt_lens = self._prompt_frame_lens(prompt_lens, prompt, prompt_enc)
        self.refresh_weights()
        p_enc = None
        front = {} if prompt_lens is None else dict(prompt_lens=prompt_lens)
        if self.conditional:
            assert (prompt is not None or prompt_enc is not None) and (text is not None or cond is not None)   # NS2:1473
            if prompt_lens is None or prompt_enc is not None:
                p_enc = self._encode_prompt(prompt, prompt_enc)
            else:
                p_enc = self.prompt_enc(self.process_prompt(prompt), lens=prompt_lens)
            if cond is None and not hasattr(self, "duration_pitch"):
                raise NotImplementedError(
                    "sample(text=...) derives the aligned conditioning with the DurationPitchPredictor (NS2:1478-1483), which is "
                    "not built by default: construct with `build_duration_pitch=True`, or pass the aligned conditioning as "
                    "`cond=` [b, dim_prompt, n_frames]")
            if cond is None and length is None:
                cond, lens = self.text_to_cond(text, p_enc, text_lens=text_lens, return_lens=True, **front)
                lens = lens.long()
            elif cond is None:
                cond = self.text_to_cond(text, p_enc, **(dict(front, text_lens=text_lens) if front else {}))
            batch_size = p_enc.shape[0]
        elif length is None:
            raise ValueError("sample(length=None) needs a conditional model: the lengths come from the predicted durations of text=")
        elif prompt is not None:
            batch_size = prompt.shape[0]                                               # NS2:1485-1486
        if lens is not None:
            if lens.shape[0] != batch_size:
                raise ValueError(f"length holds {lens.shape[0]} frame counts for a batch of {batch_size}")
            lens = lens.to(self.device)
            length = int(lens.max().item())                                           # one host read, before the loop (length_regulate has the same)
            if length < 1:
                raise ValueError("every utterance has 0 frames")
        audio = self.ddim_sample((batch_size, length, self.dim), prompt=p_enc, cond=cond, cond_scale=cond_scale, noise=noise,
                                 use_graph=use_graph, **({} if lens is None else dict(lens=lens)), **front)
        ragged = lens is not None
        if return_lens and not ragged:
            lens = torch.full((batch_size,), length, dtype=torch.long, device=audio.device)
        if self.codec is not None:
            # the 24 kHz SEANet decoder is causal: the padded batch decodes in one pass, an utterance's samples do not see its padding
            audio = self.codec.decode(audio)
            if audio.ndim == 3:
                audio = audio[:, 0]
            if lens is not None:
                lens = lens.to(audio.device) * self.seq_len_multiple_of
            if ragged:
                audio = audio.masked_fill(torch.arange(audio.shape[-1], device=audio.device)[None] >= lens[:, None], 0.)
        return (audio, lens) if return_lens else audio

    # ------------------------------------------------------------------ training loss (NS2:1503-1684)
    def text_forward_cond(self, text, text_lens, mel, mel_lens, pitch, prompt_enc, return_aux_losses=False, prompt_lens=None, ragged=False):
        """NS2:1524-1602 up to the conditioning: masks from the lengths, the Aligner, average_over_durations and the expansion
        of the phoneme encodings + pitch embeddings into exactly T_mel = mel.shape[-1] frames.  Unlike the reference, the
        caller's `text_lens` / `mel_lens` are not clamped in place: clamped copies are used.  On CUDA the Aligner runs its HIP
        path under no_grad (the returned loss depends on it only through the hard path) and the lengths go straight to the
        kernels: no host read.  With return_aux_losses the Aligner runs its differentiable composite (or, built with
        `aligner_train_backend="hip"`, its HIP training pass on the lengths: still no host read) and the auxiliary terms
        of NS2:1587-1602 are returned as a dict.  -> (cond, aux or None)
        ragged (`ragged_conditioning`, with `text_lens` and / or `prompt_lens`): the phoneme encoder runs under the key mask of text_lens
        and its rows from text_lens[i] on are selected to 0, the predictor gets both length vectors, and the duration / pitch terms are the
        mean over the utterances of each one's own mean absolute error over its phonemes [0, text_lens[i]) -- mask and divisor formed on the
        device with a select, the convention of `codec.rq(..., lens=)`."""
        from .aligner import average_over_durations, create_mask, expand_encodings
        b, n = text.shape[0], text.shape[-1]
        dev = text.device
        text_lens_given = text_lens is not None
        text_lens = torch.full((b,), n, device=dev, dtype=torch.long) if text_lens is None else (text_lens if torch.is_tensor(text_lens) else torch.as_tensor(text_lens, device=dev)).clamp(max=n)
        T = mel.shape[-1]
        mel_lens_given = mel_lens is not None
        mel_lens = torch.full((b,), T, device=dev, dtype=torch.long) if mel_lens is None else mel_lens.clamp(max=T)
        ragged = ragged and (text_lens_given or prompt_lens is not None)
        if ragged and mel_lens_given:
            # mel and pitch frames behind mel_lens are selected to 0, what AudioToMel / PitchExtractor leave there with lens=: the Aligner's
            # k = 3 convolutions then read behind an utterance's last frame what they read behind the end of the utterance alone
            frame_keep = (torch.arange(T, device=dev)[None] < mel_lens.clamp(min=1)[:, None])[:, None]
            mel = torch.where(frame_keep, mel, torch.zeros((), dtype=mel.dtype, device=dev))
            pitch = torch.where(frame_keep, pitch, torch.zeros((), dtype=pitch.dtype, device=dev))
        if ragged:
            tl = text_lens.clamp(1, n)
            text_keep = torch.arange(n, device=dev)[None] < tl[:, None]                  # [b, n]
            phoneme_enc = self.phoneme_enc(text, lens=tl)
            phoneme_enc = torch.where(text_keep[..., None], phoneme_enc, torch.zeros((), dtype=phoneme_enc.dtype, device=dev))
        else:
            phoneme_enc = self.phoneme_enc(text)                                       # [b, n, dim_hidden]
        if return_aux_losses and torch.is_grad_enabled() and self.aligner.train_ready(phoneme_enc, mel):
            # aligner_train_backend="hip": the clamped lengths go straight to the kernels -- no masks, no host read
            aln_hard, aln_soft, aln_log, aln_mask = self.aligner.forward_lengths_train(phoneme_enc, text_lens, mel, mel_lens)
        elif return_aux_losses or not phoneme_enc.is_cuda:
            text_mask, mel_mask = create_mask(text_lens, n)[:, None], create_mask(mel_lens, T)[:, None]
            with torch.set_grad_enabled(return_aux_losses and torch.is_grad_enabled()):
                aln_hard, aln_soft, aln_log, aln_mask = self.aligner._forward_composite(phoneme_enc, text_mask, mel, mel_mask)
        else:
            with torch.no_grad():
                aln_hard, aln_soft, aln_log, aln_mask = self.aligner.forward_lengths(phoneme_enc.detach(), text_lens, mel, mel_lens)
        pitch = average_over_durations(pitch, aln_hard)                                # [b, 1, n]
        cond = expand_encodings(phoneme_enc, aln_hard, aln_mask, pitch[:, 0], self.pitch_emb.weight)
        if not return_aux_losses:
            return cond, None
        assert hasattr(self, "duration_pitch"), "return_aux_losses needs the predictor: construct with build_duration_pitch=True"
        if ragged:
            duration_pred, pitch_pred = self.duration_pitch(phoneme_enc, prompt_enc, text_lens=tl if text_lens_given else None,
                                                            prompt_lens=prompt_lens)

            def own_l1(target, pred):                                                  # the mean over utterances of each one's own mean
                err = torch.where(text_keep, (target - pred).abs(), torch.zeros((), dtype=pred.dtype, device=dev))
                return (err.sum(dim=1) / tl.to(err.dtype)).mean()
            duration_loss, pitch_loss = own_l1(aln_hard, duration_pred), own_l1(pitch[:, 0], pitch_pred)
        else:
            duration_pred, pitch_pred = self.duration_pitch(phoneme_enc, prompt_enc)
            duration_loss = F.l1_loss(aln_hard, duration_pred)
            pitch_loss = F.l1_loss(pitch[:, 0], pitch_pred)
        align_loss = self.aligner_loss(aln_log, text_lens, mel_lens)
        bin_loss = None
        if self.aligner_bin_loss_weight > 0.:
            bin_loss = self.bin_loss(aln_mask, aln_log, text_lens) * self.aligner_bin_loss_weight
            align_loss = align_loss + bin_loss
        aux = duration_loss * self.duration_loss_weight + pitch_loss * self.pitch_loss_weight + align_loss * self.aligner_loss_weight
        return cond, dict(duration=duration_loss, pitch=pitch_loss, align=align_loss, bin=bin_loss, aux=aux)

    def forward(self, audio, text=None, text_lens=None, mel=None, mel_lens=None, codes=None, prompt=None, pitch=None,
                *args, cond=None, prompt_enc=None, times=None, noise=None, return_aux_losses=False, audio_lens=None,
                input_sample_hz=None, **kwargs):
        """Reference signature; `cond`, `prompt_enc` (module docstring) and `times`, `noise` (deterministic parity tests) are
        the keyword-only extras.  The model call runs the autograd composite when gradients are required.

        With `build_aligner=True` and no `cond`, `text`, `mel` [b, aligner_dim_in, T_mel] and `pitch` [b, 1, T_mel] derive the
        conditioning as NS2:1524-1602 does (text_forward_cond).  The value returned is the reference's: its auxiliary duration /
        pitch / alignment losses are computed and dropped upstream, so they are not computed here.  Without `mel`, raw audio
        goes through AudioToMel; without `pitch`, a wrapper built with `build_pitch_extractor=True` runs its PitchExtractor on
        the raw audio (without one, the missing `pitch` raises as before).  `return_aux_losses=True`
        (not in the reference, needs build_duration_pitch=True) returns (loss, dict(duration=, pitch=, align=, bin=, aux=)),
        the only way to train the Aligner and the predictor.

        `audio_lens` (not in the reference; needs a model built with `ragged_training=True`): latent frames per utterance of a padded
        batch, integer [b].  The lengths go to the model as `lens=`, and the loss of utterance i is the mean of the squared error over
        its own frames [0, audio_lens[i]) x dim -- what it is for the utterance alone -- before the reference's (loss * weight).mean().
        Mask and divisor are formed on the device from the lengths (no host read: a captured step follows rewritten lengths); what
        audio, noise and cond hold from a length on never reaches the loss or a gradient.  Latents only: raw audio, the RVQ
        cross-entropy term and `prompt_lens` are not taken together with it (NotImplementedError; `ragged_audio` / `ragged_conditioning` below).

        Built with `ragged_audio=True` (not in the reference; also a plain attribute), the first two are taken:
          * raw audio [b, S] with `audio_lens` counting SAMPLES.  Each length and S must be a positive multiple of the codec's
            `seq_len_multiple_of` and at least its `min_causal_prompt_frames` frames (ValueError; the check of sample(prompt_lens=) with a
            raw-audio prompt, for the same reason: the SEANet encoder is causal and its reflect padding is a left prefix, so an
            utterance's frames do not see its padding).  The check is one host read: it is made only when the lengths arrive as a list
            or a CPU tensor, and never while the stream is capturing; a CUDA tensor is TRUSTED and stays on the device.  The padded
            batch is encoded in one pass and the frame counts audio_lens // hop go on as above;
          * the RVQ cross-entropy term: the frame counts go to `codec.rq(x_start, codes, lens=)`, the mean over the utterances of each
            one's own term (codec.py);
          * with `text=` and the Aligner: `mel` (when not given) is `audio_to_mel(audio, lens=audio_lens)`, `pitch` (when not given)
            `pitch_extractor(audio, lens=audio_lens)`, and `mel_lens` defaults to 1 + audio_lens // mel_hop_length, formed on the device;
            the Aligner and its losses run on lengths already.  The phoneme encoder, the prompt encoder and the predictor see lengths
            under `ragged_conditioning=True` (below); without it they see none, and `prompt_lens` with `audio_lens` keeps raising.
        The model still needs `ragged_training=True` for `audio_lens`.

        Built with `ragged_conditioning=True` (not in the reference; also a plain attribute; include/ns2hip_train.h), `text_lens` and
        `prompt_lens` (a keyword the reference signature tolerates) reach the conditioning under autograd: `prompt_lens` -- rows of
        `prompt_enc=`, frames of prompt latents or samples of a raw-audio prompt (`_prompt_frame_lens`; a CUDA tensor is trusted) -- goes to
        `prompt_enc`, the predictor and the model, together with `audio_lens` or without it; `text_lens` goes to the phoneme encoder's key
        mask and the predictor; and with `return_aux_losses=True` the duration and pitch terms are the mean over the utterances of each one's
        own mean absolute error over its phonemes [0, text_lens[i]) (text_forward_cond).  What ids, prompt rows, mel and pitch frames hold
        behind their lengths reaches no term of the loss and no gradient.

        `input_sample_hz` (keyword-only; the keyword of audiolm_pytorch's EncodecWrapper.forward): the rate of the raw `audio` and of a
        raw `prompt`.  Another rate than the codec's is resampled first (resample.py), so mel, pitch and codec all see the target rate.
        With `ragged_audio=True` and `audio_lens`, the lengths count samples of the INPUT: utterance i is resampled as it is alone, its
        length becomes out_lens(audio_lens[i]) // hop * hop (formed on the device) and the resampled batch is cut to whole codec frames;
        the check above then applies to the converted values (a list or a CPU tensor only, never during capture), so the padded
        input length need not be a multiple of hop.  `prompt_lens` of a raw prompt are converted the same way.  Latents have no
        rate: a foreign rate with neither raw audio nor a raw prompt is a ValueError."""
        is_raw = audio.ndim == 2
        rs = self._resampler(input_sample_hz)
        if rs is not None:
            raw_prompt = prompt is not None and prompt.ndim == 2 and prompt_enc is None
            if not is_raw and not raw_prompt:
                raise ValueError(f"input_sample_hz={input_sample_hz}: neither `audio` nor `prompt` is raw audio [b, samples]; latents have no "
                                 f"sample rate to convert")
            if raw_prompt:
                # (without ragged_conditioning `prompt_lens` is tolerated and unused, as it is at the codec's rate: the whole prompt counts)
                prompt, p_lens = self._resample_raw(rs, prompt, kwargs.get("prompt_lens") if getattr(self, "ragged_conditioning", False) else None)
                if p_lens is not None:
                    kwargs = dict(kwargs, prompt_lens=p_lens)
            if is_raw and audio_lens is None:
                audio = rs(audio)
        ragged_audio = bool(getattr(self, "ragged_audio", False))
        ragged_cond = bool(getattr(self, "ragged_conditioning", False))
        sample_lens = None                                                            # ragged raw audio: the sample counts, on the device
        if audio_lens is not None:
            if is_raw and not ragged_audio:
                raise NotImplementedError("audio_lens with raw audio: the frozen codec's encode of a padded batch is not shown to equal the "
                                          "utterance alone -- pass the latents [b, n, dim] and their frame counts")
            if self.rvq_cross_entropy_loss_weight > 0 and codes is not None and not ragged_audio:
                raise NotImplementedError("audio_lens with the RVQ cross-entropy term (rvq_cross_entropy_loss_weight > 0 and codes=): "
                                          "ns2_rvq_ce averages over all frames, it takes no per-utterance lengths")
            if kwargs.get("prompt_lens") is not None and not ragged_cond:
                raise NotImplementedError("prompt_lens in training: per-utterance prompt lengths are a sampling feature; audio_lens "
                                          "shortens the utterances, not their prompts (a wrapper built with ragged_conditioning=True takes both)")
            audio_lens = torch.as_tensor(audio_lens)
            if audio_lens.dtype.is_floating_point or audio_lens.dtype == torch.bool:
                raise ValueError(f"audio_lens must be integers (frame counts), got {audio_lens.dtype}")
            if audio_lens.shape != (audio.shape[0],):
                raise ValueError(f"audio_lens must hold one frame count per utterance: [{audio.shape[0]}], got {list(audio_lens.shape)}")
            if is_raw:
                assert self.codec is not None, "codec must be passed in if one were to train on raw audio"
                if rs is not None:                                                    # the lengths count input samples
                    audio, audio_lens = self._resample_raw(rs, audio, audio_lens)
                if not audio_lens.is_cuda and not (audio.is_cuda and torch.cuda.is_current_stream_capturing()):
                    _check_raw_sample_lens(self.codec, int(self.seq_len_multiple_of), audio_lens.long(), audio.shape[-1],
                                           "raw audio with audio_lens", "utterance")
                sample_lens = audio_lens.to(audio.device)
                audio_lens = sample_lens // int(self.seq_len_multiple_of)             # frames, as the latent path counts
        p_enc = None
        aux = None
        if return_aux_losses and (not self.conditional or cond is not None):
            raise ValueError("return_aux_losses needs the text-conditioned path: text=, mel=, pitch= and no cond=")
        prompt_lens = None                                                            # ragged_conditioning: rows of the encoded prompt, on the device
        if self.conditional:
            if ragged_cond and kwargs.get("prompt_lens") is not None:
                if prompt is None and prompt_enc is None:
                    raise ValueError("prompt_lens needs a prompt: a conditional model called with prompt= or prompt_enc=")
                prompt_lens = self._prompt_frame_lens(kwargs["prompt_lens"], prompt, prompt_enc, trust_device=True)
                p_enc = prompt_enc if prompt_enc is not None else self.prompt_enc(self.process_prompt(prompt), lens=prompt_lens)
            else:
                p_enc = self._encode_prompt(prompt, prompt_enc)
            if cond is None and hasattr(self, "aligner"):
                assert text is not None, "forward(text=...) needs the phoneme ids"
                if mel is None and not is_raw:
                    raise NotImplementedError("forward(text=...) without `mel` computes it with AudioToMel (NS2:1561-1567), which "
                                              "needs raw audio [b, samples], not latents: pass the raw audio, or the mel frames as "
                                              "`mel=` [b, aligner_dim_in, T_mel]")
                if pitch is None and hasattr(self, "pitch_extractor"):
                    if not is_raw:
                        raise NotImplementedError("forward(text=...) without `pitch` computes it with PitchExtractor, which needs raw "
                                                  "audio [b, samples], not latents: pass the raw audio, or `pitch=` [b, 1, T_mel]")
                    with torch.no_grad():                                             # one value per AudioToMel frame, Hz, 0 unvoiced
                        pitch = self.pitch_extractor(audio, **({} if sample_lens is None else dict(lens=sample_lens)))[:, None]
                if pitch is None:
                    raise NotImplementedError("forward(text=...) without `pitch` needs the pyworld / kaldi pitch extraction "
                                              "(NS2:1546-1559), which is outside the HIP hot path: pass `pitch=` [b, 1, T_mel]")
                if mel is None:                                                       # NS2:1561-1567; mel_lens default to full
                    with torch.no_grad():
                        mel = self.audio_to_mel(audio, **({} if sample_lens is None else dict(lens=sample_lens)))[..., :pitch.shape[-1]]
                if mel_lens is None and sample_lens is not None:                      # the utterances' own frames (no host read)
                    mel_lens = 1 + sample_lens.long() // self.mel_hop_length
                front = dict(prompt_lens=prompt_lens, ragged=True) if ragged_cond else {}
                cond, aux = self.text_forward_cond(text, text_lens, mel, mel_lens, pitch, p_enc, return_aux_losses, **front)
            if cond is None:
                raise NotImplementedError(
                    "forward(text=..., mel=..., pitch=...) derives the aligned conditioning with the Aligner, the "
                    "DurationPitchPredictor and mel / pitch extraction (NS2:1524-1602), which are outside the HIP hot path: pass "
                    "the aligned conditioning as `cond=` [b, dim_prompt, n_frames]")
        assert not (is_raw and self.codec is None), "codec must be passed in if one were to train on raw audio"
        if is_raw:
            with torch.no_grad():
                self.codec.eval()
                audio, codes, _ = self.codec(audio, return_encoded=True)             # NS2:1608-1611 (RVQ encode in HIP)
        batch, n, d = audio.shape
        assert d == self.dim, f"codec codebook dimension {d} must match model dimensions {self.dim}"
        device = audio.device
        times = torch.zeros((batch,), device=device).float().uniform_(0, 1.) if times is None else times
        noise = torch.randn_like(audio) if noise is None else noise
        gamma = self.gamma_schedule(times)[:, None, None]
        alpha, sigma = torch.sqrt(gamma) * self.scale, torch.sqrt(1 - gamma)         # NS2:1152-1153
        noised = alpha * audio + sigma * noise
        target = {"eps": noise, "x0": audio, "v": alpha * noise - sigma * audio}[self.objective]
        pl_kw = {} if prompt_lens is None else dict(prompt_lens=prompt_lens)
        if audio_lens is None:
            pred = self.model(noised, times, prompt=p_enc, cond=cond, **pl_kw)        # NS2:1635
            loss = F.mse_loss(pred, target, reduction="none").flatten(1).mean(dim=1)  # [b]
        else:
            lens = audio_lens.to(device=device, dtype=torch.int32)                    # (an int32 device tensor stays the caller's buffer)
            pred = self.model(noised, times, prompt=p_enc, cond=cond, lens=lens, **pl_kw)
            ln = lens.clamp(1, n)                                                     # as the kernels clamp
            keep = (torch.arange(n, device=device)[None] < ln[:, None])[..., None]
            # a select, not a product (NaN may lie beyond a length), on the difference: the padding's cotangent is an exact 0
            err = torch.where(keep, pred - target, torch.zeros((), dtype=pred.dtype, device=device))
            loss = (err * err).flatten(1).sum(dim=1) / (ln * d).to(err.dtype)         # [b]: the mean over the utterance's own frames x dim
        snr = (alpha * alpha) / (sigma * sigma)                                       # [b, 1, 1]
        clipped = snr.clamp(max=self.min_snr_gamma) if self.min_snr_loss_weight else snr
        weight = {"eps": clipped / snr, "x0": clipped, "v": clipped / (snr + 1)}[self.objective]
        # NS2:1668 as written upstream: `loss` is [b] and `loss_weight` is [b, 1, 1], so the product broadcasts to
        # [b, 1, b] and the mean equals mean(loss) * mean(weight) -- kept bit-compatible with the reference.
        loss = (loss * weight).mean()
        if self.rvq_cross_entropy_loss_weight == 0 or codes is None:                  # NS2:1672-1673
            return loss if aux is None else (loss, aux)
        x_start = {"x0": lambda: pred, "eps": lambda: _safe_div(audio - sigma * pred, alpha),
                   "v": lambda: alpha * audio - sigma * pred}[self.objective]()
        assert self.codec is not None and hasattr(self.codec, "rq"), "the RVQ cross-entropy term needs codec.rq (NS2:1682)"
        _, ce_loss = self.codec.rq(x_start, codes, **({} if audio_lens is None else dict(lens=audio_lens)))
        loss = loss + self.rvq_cross_entropy_loss_weight * ce_loss                    # NS2:1684 (duration_pitch_loss is 0 upstream)
        return loss if aux is None else (loss, aux)
