"""fp64 restatement of the YIN formula of naturalspeech2_pytorch_amd/pitch.py (its docstring is the specification), the seeded
test signals, and the tolerance the CPU and GPU tests share.

The restatement is a plain loop over frames and lags in numpy fp64 on the fp32 audio the code under test reads.  Per frame it
returns F0, the integer lag `tau` (0: unvoiced), the interpolation offset `delta`, and a DECISION MARGIN: the smallest absolute
gap of any comparison the decision evaluated --
    |d'(tau) - threshold|     for every tau the threshold search looked at,
    |d'(tau + 1) - d'(tau)|   for every step of the descent and for the comparison that stopped it,
    |den|                     when its sign decided (tau + 1 <= tau_max).
A frame whose margin is below MARGIN_MIN may legitimately come out differently in fp32; the tests compare the others and assert
that at most EXCLUDED_MAX of the frames are set aside (the restatement alone sets aside 0.9 %, 1.7 %, 1.3 % and 0 % of `mixture`
at the four CONFIGS: the cap tests the inputs, not the code under test; the shares depend on the noise drawn, that is on the
seeds and the generator of the signal builders below, so another implementation of the same recipe gives other small shares).
"""
import functools
import math

import numpy as np
import torch

MARGIN_MIN = 1e-4
EXCLUDED_MAX = 0.05
# worst relative F0 difference of the fp32 composite (pitch.yin_composite, CPU) from this restatement on the frames of `mixture`
# with margin >= MARGIN_MIN, over CONFIGS: measured 1.06e-7, 1.25e-7, 1.16e-7, 1.08e-7, pinned at the worst rounded up.  (The last
# three fp32 operations alone -- tau + delta, the division, the stored result -- can give 3 x 6e-8.)
K_EMU_PITCH = 1.3e-7
# the composite's own bound: 2 x the pinned figure, the allowance for another torch build summing a row in another order
COMPOSITE_F0_RTOL = 2 * K_EMU_PITCH
GPU_F0_RTOL = max(8 * K_EMU_PITCH, 1e-6)          # the kernel's bound: 8 x the pinned figure, and not below 1e-6
CONFIGS = ((24000, 160, 0.1), (16000, 200, 0.1), (24000, 160, 0.15), (22050, 256, 0.1))   # (sample_rate, hop_length, threshold)
F0_FLOOR, F0_CEIL = 71.0, 640.0


def lags(fs, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    return int(math.floor(fs / f0_ceil)), int(math.ceil(fs / f0_floor))


def yin_frame64(span, fs, tau_min, tau_max, threshold):
    """one frame: span [3 tau_max] fp64 -> (f0, tau, delta, margin)"""
    W = 2 * tau_max
    d = np.zeros(tau_max + 2)
    for tau in range(1, tau_max + 1):
        e = span[:W] - span[tau:tau + W]
        d[tau] = np.sum(e * e)
    dp = np.ones(tau_max + 2)
    c = 0.0
    for tau in range(1, tau_max + 1):
        c += d[tau]
        dp[tau] = d[tau] * tau / c if c > 0 else 1.0
    margin, found = math.inf, 0
    for tau in range(tau_min, tau_max + 1):
        margin = min(margin, abs(dp[tau] - threshold))
        if dp[tau] < threshold:
            found = tau
            break
    if not found:
        return 0.0, 0, 0.0, margin
    tau = found
    while tau < tau_max:
        margin = min(margin, abs(dp[tau + 1] - dp[tau]))
        if not dp[tau + 1] < dp[tau]:
            break
        tau += 1
    delta = 0.0
    if tau + 1 <= tau_max:
        y0, y1, y2 = dp[tau - 1], dp[tau], dp[tau + 1]
        den = y0 - 2 * y1 + y2
        margin = min(margin, abs(den))
        if den > 0:
            delta = min(max(0.5 * (y0 - y2) / den, -1.0), 1.0)
    return fs / (tau + delta), tau, delta, margin


def yin_ref64(audio, fs, hop, threshold, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    """audio [L] fp32 tensor -> dict of numpy arrays over the 1 + L // hop frames: f0 (fp64), tau (int), delta, margin"""
    x = audio.detach().cpu().to(torch.float64).numpy()
    tau_min, tau_max = lags(fs, f0_floor, f0_ceil)
    L, S = x.shape[0], 3 * tau_max
    T = 1 + L // hop
    out = dict(f0=np.zeros(T), tau=np.zeros(T, dtype=np.int64), delta=np.zeros(T), margin=np.zeros(T))
    for i in range(T):
        s = i * hop - S // 2
        span = np.zeros(S)
        lo, hi = max(s, 0), min(s + S, L)
        if hi > lo:
            span[lo - s:hi - s] = x[lo:hi]
        out["f0"][i], out["tau"][i], out["delta"][i], out["margin"][i] = yin_frame64(span, fs, tau_min, tau_max, threshold)
    return out


def compare(f0, ref, fs, rtol, tau=None):
    """the rule of the issue, on one utterance: on every frame with margin >= MARGIN_MIN the voiced decision and the integer lag
    equal the restatement's and F0 is within rtol; at most EXCLUDED_MAX of the frames are set aside.  `f0`: fp32 tensor [T];
    `tau`: the code's own integer lags where it reports them (the composite), else the lag is read off F0 with the restatement's
    own delta: round(fs / f0 - delta_ref).  Returns (excluded share, worst relative F0 difference)."""
    f0 = f0.detach().cpu().to(torch.float64).numpy()
    assert f0.shape == ref["f0"].shape and np.isfinite(f0).all()
    keep = ref["margin"] >= MARGIN_MIN
    excluded = 1.0 - keep.mean()
    voiced = ref["tau"] > 0
    assert ((f0 > 0) == voiced)[keep].all(), "voiced decision differs on a frame with margin"
    k = keep & voiced
    if tau is None:
        got_tau = np.zeros_like(ref["tau"])
        got_tau[k] = np.rint(fs / f0[k] - ref["delta"][k]).astype(np.int64)
    else:
        got_tau = tau.detach().cpu().numpy()
        assert (got_tau[keep & ~voiced] == 0).all()
    assert (got_tau[k] == ref["tau"][k]).all(), "integer lag differs on a frame with margin"
    worst = float(np.max(np.abs(f0[k] - ref["f0"][k]) / ref["f0"][k])) if k.any() else 0.0
    print(f"pitch compare: frames {f0.size}, excluded {excluded:.4f}, worst relative F0 difference {worst:.3e} (bound {rtol:.1e})")
    assert excluded <= EXCLUDED_MAX, f"{excluded:.3f} of the frames have a decision margin below {MARGIN_MIN}"
    assert worst <= rtol, f"F0 differs by {worst:.3e} relative, bound {rtol:.1e}"
    return excluded, worst


# ---------------------------------------------------------------- signals
HARMONICS = (1.0, 0.5, 0.3, 0.2)


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def tone(f0, fs, n, noise=0.0, seed=0):
    """0.3 (sum_k a_k sin((k + 1) phi + 0.7 k) + noise randn), a = HARMONICS, phi the running phase of a constant or per-sample
    F0 (Hz): phi[m] = 2 pi sum_{i <= m} f0[i] / fs.  fp64 arithmetic, returned in fp32 [n]"""
    f = torch.as_tensor(f0, dtype=torch.float64).expand(n)
    phi = 2 * math.pi * torch.cumsum(f / fs, 0)
    x = sum(a * torch.sin((k + 1) * phi + 0.7 * k) for k, a in enumerate(HARMONICS))
    return (0.3 * (x + noise * _randn(n, seed))).float()


def chirp_f0(fs, n, f_start=100.0, f_end=400.0):
    """the per-sample instantaneous frequency of the linear chirp"""
    return torch.linspace(f_start, f_end, n, dtype=torch.float64)


def chirp(fs, n, noise=0.0, seed=0):
    return tone(chirp_f0(fs, n), fs, n, noise, seed)


def mixture(fs):
    """1/3 s of a 130 Hz tone (noise 0.03) | 1/12 s of zeros | 1/2 s of a 100 -> 400 Hz chirp (noise 0.1) | 1/4 s of 0.1 randn
    | 1/3 s + 7 samples of a 333 Hz tone (noise 0.3)"""
    return torch.cat((tone(130.0, fs, fs // 3, 0.03, seed=1),
                      torch.zeros(fs // 12),
                      chirp(fs, fs // 2, 0.1, seed=2),
                      (0.1 * _randn(fs // 4, 3)).float(),
                      tone(333.0, fs, fs // 3 + 7, 0.3, seed=4)))


@functools.lru_cache(maxsize=None)
def mixture_case(fs, hop, threshold):
    """(audio, restatement) of `mixture` at one of CONFIGS: computed once, shared by the tests, not to be modified"""
    x = mixture(fs)
    return x, yin_ref64(x, fs, hop, threshold)
