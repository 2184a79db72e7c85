"""The small text-conditioned wrapper of tests/test_ragged_front_gpu.py's end-to-end sampling test, and its CPU precondition: importable
without a GPU, so the seeds and the duration head's bias below were chosen on the CPU composite (python -m tests.ragged_front_sample
prints the figures the test asserts on)."""
import torch
from torch import nn

from naturalspeech2_pytorch_amd import DurationPitchPredictor, Model, NaturalSpeech2, PhonemeEncoder, SpeechPromptEncoder
from tests.golden.gen import make_input, make_weights

TEXT_LENS, PROMPT_LENS = [12, 7, 3], [24, 9, 1]
DURATION_BIAS = 2.79         # to_duration_pred's head bias: durations of a few frames per phoneme instead of the ReLU's zeros
MARGIN = 0.05                # every predicted duration stays this far from an integer: int(duration) cannot flip inside the kernels' tolerance


def _seeded(module, seed):
    module.load_state_dict(make_weights({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed=seed))
    return module


def tiny_wrapper(precision="exact"):
    """dim-64 conditional model, 2 DDIM steps, every front-end module at width 64 (on the CPU; move it with .to(device))"""
    m = _seeded(Model(dim=64, depth=2, dim_prompt=64, condition_on_prompt=True, num_latents_m=16, precision=precision), 1)
    d = NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2, build_duration_pitch=True, duration_pitch_dim=64,
                       pitch_emb_pp_hidden_dim=64, dim_codebook=64)
    d.phoneme_enc = _seeded(PhonemeEncoder(num_tokens=150, dim=64, dim_hidden=64, depth=1), 2)
    d.prompt_enc = _seeded(SpeechPromptEncoder(64, dims=(64, 128, 64), depth=1), 3)
    d.duration_pitch = _seeded(DurationPitchPredictor(dim=64, dim_hidden=64, depth=2, heads=2), 4)
    d.pitch_emb = _seeded(nn.Embedding(256, 64), 5)
    with torch.no_grad():
        d.duration_pitch.to_duration_pred.to_pred[0].bias.fill_(DURATION_BIAS)
        d.duration_pitch.to_pitch_pred.to_pred[0].bias.fill_(150.)          # Hz: inside f0_to_coarse's range
    return d.eval()


def inputs():
    g = torch.Generator().manual_seed(11)
    text = torch.randint(0, 150, (3, 12), generator=g)
    latents = make_input("prompt_latents", (3, 24, 64), seed=12)
    return text, latents


def alone_durations(d):
    """the CPU composite's durations of every utterance alone, its text and prompt cut to their lengths"""
    from naturalspeech2_pytorch_amd.autograd_path import (duration_pitch_autograd, phoneme_encoder_autograd,
                                                         speech_prompt_encoder_autograd)
    text, latents = inputs()
    out = []
    with torch.no_grad():
        for i, (tl, pl) in enumerate(zip(TEXT_LENS, PROMPT_LENS)):
            p_enc = speech_prompt_encoder_autograd(d.prompt_enc, latents[i:i + 1, :pl])
            ph = phoneme_encoder_autograd(d.phoneme_enc, text[i:i + 1, :tl])
            out.append(duration_pitch_autograd(d.duration_pitch, ph, p_enc)[0][0])
    return out


def precondition(durations):
    """(smallest distance of a duration from an integer, the utterances' frame totals)"""
    dist = min(float((t - t.round()).abs().min()) for t in durations)
    return dist, [int(t.int().clamp(min=0).sum()) for t in durations]


if __name__ == "__main__":
    durs = alone_durations(tiny_wrapper())
    for t in durs:
        print([round(v, 3) for v in t.tolist()])
    print(precondition(durs))
