"""TEST INFRASTRUCTURE: `tests/emu_backend.EmuBackend` plus the two backend calls that take per-utterance lengths
(`HipBackend.attention(..., lens=)` / `attention_bwd(..., lens=)`, include/ns2hip_train.h), restated in plain torch from the kernels'
contract -- so that the host logic of a ragged training pass (functions.py AttnFn, model_pass.py) is checked against torch autograd
without a GPU (tests/test_ragged_training_cpu.py).  Never imported by the product.

The contract restated: len_b = clamp(lens[b], 1, N).  Rows of q, k, v, dO from len_b on are read as zeros whatever they hold (here:
selected to 0, NaN included), their lse as +inf and delta as 0; keys from len_b on have P = 0; rows of o, dq, dk, dv from len_b on are
written as exact zeros and the lse of such a row is +inf."""
import math

import torch

from tests.emu_backend import EmuBackend


def _zero():
    return torch.zeros(())


class EmuBackendRagged(EmuBackend):
    name = "emu-ragged"

    @staticmethod
    def _row_mask(lens, B, N):
        """[B, N] bool: True on the rows the utterance owns"""
        return torch.arange(N)[None] < lens.long().clamp(1, N)[:, None]

    def attention(self, q, q_col0, k, k_col0, vt, B, H, Nq, Nk, lens=None):
        if lens is None:
            return super().attention(q, q_col0, k, k_col0, vt, B, H, Nq, Nk)
        assert Nq == Nk and lens.dtype == torch.int32 and lens.shape == (B,)
        self.calls.append(("attention_lens", lens))
        a = H * 64
        own = self._row_mask(lens, B, Nq)                                              # [B, N]
        hd = lambda t: torch.where(own[:, :, None, None], t.reshape(B, Nq, H, 64), _zero()).transpose(1, 2)      # noqa: E731
        qq, kk = hd(q.t[:, q_col0:q_col0 + a]), hd(k.t[:, k_col0:k_col0 + a])
        vv = vt.t.reshape(B, H, 64, -1)[..., :Nk].transpose(2, 3)
        vv = torch.where(own[:, None, :, None], vv, _zero())
        s = (qq @ kk.transpose(2, 3) * 0.125).masked_fill(~own[:, None, None, :], float("-inf"))
        lse = torch.logsumexp(s, dim=-1) / math.log(2.0)
        o = s.softmax(-1) @ vv
        o = torch.where(own[:, None, :, None], o, _zero()).transpose(1, 2).reshape(B * Nq, a)
        return self.split(o), torch.where(own[:, None, :], lse, torch.full((), float("inf")))

    def attention_bwd(self, q, q_col0, k, k_col0, v, v_col0, do_row, lse, delta, B, H, Nq, Nk, dq=None, dkv=None, planes=None, lens=None):
        if lens is None:
            return super().attention_bwd(q, q_col0, k, k_col0, v, v_col0, do_row, lse, delta, B, H, Nq, Nk, dq=dq, dkv=dkv, planes=planes)
        assert Nq == Nk and lens.dtype == torch.int32 and lens.shape == (B,)
        self.calls.append(("attention_bwd_lens", lens))
        a = H * 64
        if planes is not None:
            dq, dkv = (planes[0].t, planes[1]), (planes[0].t, planes[2], planes[3])
        own = self._row_mask(lens, B, Nq)
        hd = lambda t, c0: torch.where(own[:, :, None, None], t[:, c0:c0 + a].reshape(B, Nq, H, 64), _zero()).transpose(1, 2)      # noqa: E731
        qq, kk, vv, dO = hd(q.t, q_col0), hd(k.t, k_col0), hd(v.t, v_col0), hd(do_row.t, 0)
        lse = torch.where(own[:, None, :], lse, torch.full((), float("inf")))
        delta = torch.where(own[:, None, :], delta, _zero())
        s = qq @ kk.transpose(2, 3) * 0.125
        P = torch.exp2(s / math.log(2.0) - lse[..., None])
        P = torch.where(own[:, None, None, :], P, _zero())
        dS = P * (dO @ vv.transpose(2, 3) - delta[..., None])
        unhd = lambda t: torch.where(own[:, None, :, None], t, _zero()).transpose(1, 2).reshape(B * Nq, a)      # noqa: E731
        if dq is not None:
            dq[0][:, dq[1]:dq[1] + a] = unhd(dS @ kk * 0.125)
        if dkv is not None:
            dkv[0][:, dkv[1]:dkv[1] + a] = unhd(dS.transpose(2, 3) @ qq * 0.125)
            dkv[0][:, dkv[2]:dkv[2] + a] = unhd(P.transpose(2, 3) @ dO)
