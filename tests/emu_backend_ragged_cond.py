"""TEST INFRASTRUCTURE: `tests/duration_pitch_golden.DurationPitchEmuBackend` plus the backend calls that ragged text and prompts add to
the training pass (include/ns2hip_train.h), restated in plain torch from the kernels' contract -- so that the host logic of
the conditioning passes with lengths (training/encoder_pass.py, duration_pitch_pass.py, model_pass.py) is checked against torch
autograd without a GPU (tests/test_ragged_conditioning_cpu.py).  Never imported by the product.

The contract restated: len_b = clamp(row_lens[b], 1, n).
  keep_rows           a fresh copy whose rows from len_b on are exact zeros, whatever they held (a select: NaN included).
  groupnorm_silu_fwd  with row_lens: mean and biased variance of (utterance, group) over rows [0, len_b) x the group's columns; rows of x
                      and resid from len_b on are not read (here: selected to 0 first); rows of y from len_b on are exact zeros.
  groupnorm_silu_bwd  with row_lens: s1, s2 and N = len_b * C / groups over rows [0, len_b); rows of x and dy from len_b on are not read;
                      rows of dx from len_b on are exact zeros; dweight | dbias sum the rows before a length of every utterance."""
import torch
import torch.nn.functional as F

from tests.duration_pitch_golden import DurationPitchEmuBackend


def _zero():
    return torch.zeros(())


class RaggedCondEmuBackend(DurationPitchEmuBackend):
    name = "emu-ragged-cond"

    @staticmethod
    def _own(lens, B, n):
        """[B, n] bool: True on the rows the utterance owns"""
        assert lens.dtype == torch.int32 and lens.shape == (B,)
        return torch.arange(n)[None] < lens.long().clamp(1, n)[:, None]

    def keep_rows(self, t, B, n, lens):
        self.calls.append("keep_rows")
        return torch.where(self._own(lens, B, n).reshape(B * n, 1), t, _zero()).contiguous()

    def _xhat_lens(self, x, B, n, groups, eps, own):
        C = x.shape[1]
        cg = C // groups
        m = own[:, :, None, None]
        xg = torch.where(m, x.reshape(B, n, groups, cg), _zero())
        cnt = (own.sum(dim=1) * cg).to(x.dtype)[:, None, None, None]
        mean = xg.sum(dim=(1, 3), keepdim=True) / cnt
        var = torch.where(m, (xg - mean) ** 2, _zero()).sum(dim=(1, 3), keepdim=True) / cnt
        rstd = (var + eps).rsqrt()
        return torch.where(m, (xg - mean) * rstd, _zero()).reshape(B * n, C), rstd, cnt

    def groupnorm_silu_fwd(self, x, B, n, weight, bias, groups, eps, resid=None, row_lens=None):
        if row_lens is None:
            return super().groupnorm_silu_fwd(x, B, n, weight, bias, groups, eps, resid=resid)
        self.calls.append("groupnorm_silu_fwd_lens")
        C = weight.shape[0]
        x = x[:, :C]
        own = self._own(row_lens, B, n)
        xh, _, _ = self._xhat_lens(x, B, n, groups, eps, own)
        y = F.silu(xh * weight + bias)
        if resid is not None:
            y = y + resid[:, :C]
        return torch.where(own.reshape(B * n, 1), y, _zero()), x, torch.empty(0)

    def groupnorm_silu_bwd(self, dy, x, stats, B, n, weight, bias, groups, eps, row_lens=None):
        if row_lens is None:
            return super().groupnorm_silu_bwd(dy, x, stats, B, n, weight, bias, groups, eps)
        self.calls.append("groupnorm_silu_bwd_lens")
        C = weight.shape[0]
        cg = C // groups
        own = self._own(row_lens, B, n)
        rows = own.reshape(B * n, 1)
        xh, rstd, cnt = self._xhat_lens(x, B, n, groups, eps, own)
        z = xh * weight + bias
        sg = torch.sigmoid(z)
        dz = torch.where(rows, dy[:, :C], _zero()) * sg * (1 + z * (1 - sg))
        dz = torch.where(rows, dz, _zero())
        dxh = (dz * weight).reshape(B, n, groups, cg)
        xg = xh.reshape(B, n, groups, cg)
        s1 = dxh.sum(dim=(1, 3), keepdim=True) / cnt
        s2 = (dxh * xg).sum(dim=(1, 3), keepdim=True) / cnt
        dx = (rstd * (dxh - s1 - xg * s2)).reshape(B * n, C)
        return torch.where(rows, dx, _zero()), (dz * xh).sum(0), dz.sum(0)
