"""The resampling formula of naturalspeech2_pytorch_amd/resample.py restated in fp64 numpy, written from the formula and not from the
module: the yardstick of tests/test_resample_cpu.py and tests/test_resample_gpu.py.

    g = gcd(orig_hz, new_hz); down = orig_hz / g; up = new_hz / g; lpw = 6; rolloff = 0.99
    base = min(down, up) rolloff;  w = ceil(lpw down / base);  T = 2 w + down
    t = clamp((-p / up + (i - w) / down) base, -lpw, lpw)
    k[p][i] = (1 if t == 0 else sin(pi t) / (pi t)) cos(pi t / (2 lpw))^2 base / down
    out[b, f up + p] = sum_i k[p][i] x[b, f down + i - w],  x = 0 outside [0, L);  L_out = ceil(up L / down)

The error bound (derived, not measured).  The code under test rounds k once to fp32 (relative error <= 2^-24 per tap) and sums T
products in one fp32 fma chain (each fma rounds once: after n steps the running sum is within n 2^-24 (1 + O(2^-24)) of the exact sum of
the rounded-tap products, relative to the sum of their magnitudes).  With S[q] = sum_i |k[p][i] x[.]| in fp64 that is at most
(1 + T) 2^-24 S[q] to first order; (T + 2) 2^-24 S[q] covers the second-order terms for every T <= 1024.  Outputs whose S is 0 must be 0:
1e-45 is added so that the comparison is `<=` against a positive number.  A reduction that is not one chain (a convolution library's
blocked sum) has the same first-order bound per partial chain plus the additions that join them, which the same argument bounds by
the same figure again: such code is held to twice the bound.
"""
import functools
import math

import numpy as np

LPW, ROLLOFF = 6, 0.99
PAIRS = ((48000, 24000), (16000, 24000), (24000, 16000), (8000, 24000), (44100, 24000), (22050, 24000))


def ratio(orig_hz, new_hz):
    g = math.gcd(orig_hz, new_hz)
    return new_hz // g, orig_hz // g                                # up, down


@functools.lru_cache(maxsize=None)
def table64(orig_hz, new_hz, lpw=LPW, rolloff=ROLLOFF):
    """(up, down, w, k [up, T] fp64); cached: treat k as read-only"""
    up, down = ratio(orig_hz, new_hz)
    base = min(down, up) * rolloff
    w = int(math.ceil(lpw * down / base))
    T = 2 * w + down
    k = np.empty((up, T), dtype=np.float64)
    for p in range(up):
        for i in range(T):
            t = min(max((-p / up + (i - w) / down) * base, -lpw), lpw)
            sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
            k[p, i] = sinc * math.cos(math.pi * t / (2 * lpw)) ** 2 * base / down
    return up, down, w, k


def out_len(L, up, down):
    return -(-up * L // down)


def resample64(x, orig_hz, new_hz, lpw=LPW, rolloff=ROLLOFF):
    """x [B, L] (any float dtype, taken to fp64) -> (out [B, L_out] fp64, S [B, L_out] fp64 = sum_i |k x|)"""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] >= 1
    up, down, w, k = table64(orig_hz, new_hz, lpw, rolloff)
    B, L = x.shape
    L_out = out_len(L, up, down)
    nf = -(-L_out // up)
    need = (nf - 1) * down + k.shape[1]                             # samples from -w on
    xp = np.zeros((B, max(need, w + L)), dtype=np.float64)
    xp[:, w:w + L] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, k.shape[1], axis=1)[:, :(nf - 1) * down + 1:down]     # [B, nf, T]
    out = (win @ k.T).reshape(B, nf * up)[:, :L_out]
    S = (np.abs(win) @ np.abs(k).T).reshape(B, nf * up)[:, :L_out]
    return out, S


def bound(S, T):
    """the per-output bound of the module docstring for one fp32 fma chain"""
    return (T + 2) * 2.0 ** -24 * S + 1e-45


def taps_per_phase(orig_hz, new_hz, lpw=LPW, rolloff=ROLLOFF):
    up, down = ratio(orig_hz, new_hz)
    return 2 * int(math.ceil(lpw * down / (min(down, up) * rolloff))) + down


# ---- signals (fp32 values, as the code under test receives them)
def noise(seed, *shape):
    """white noise, uniform in [-1, 1)"""
    return (np.random.default_rng(seed).random(shape) * 2 - 1).astype(np.float32)


def tone(freq_hz, sample_hz, L, amp=0.5):
    return (amp * np.sin(2 * np.pi * freq_hz * np.arange(L, dtype=np.float64) / sample_hz)).astype(np.float32)[None]


def edge(orig_hz, new_hz):
    """output samples at either end that see the zero padding: 2 ceil(w up / down) + 2"""
    up, down, w, _ = table64(orig_hz, new_hz)
    return 2 * -(-w * up // down) + 2
