"""TEST INFRASTRUCTURE: `tests/emu_backend.EmuBackend` plus the `head_dim` keyword of the four attention calls
(`HipBackend.attention` / `attention_masked` / `attention_delta` / `attention_bwd`, include/ns2hip_train.h), restated in plain
torch from the kernels' contract -- so that the host logic of a training pass at head dims 32 and 128 (functions.py AttnFn, model_pass.py:
column offsets heads * head_dim, scale head_dim ** -0.5) is checked against torch autograd without a GPU
(tests/test_head_dim_training_cpu.py).  Never imported by the product.

The contract restated: head h lies at columns col0 + head_dim * h of q, k, v, o, dO and the gradients, V^T has H * head_dim rows per
utterance, and the scores are scaled by head_dim ** -0.5.  Without the keyword every call is EmuBackend's own (heads of 64)."""
import math

import torch

from tests.emu_backend import EmuBackend


class EmuBackendHeadDim(EmuBackend):
    name = "emu-head-dim"

    def attention(self, q, q_col0, k, k_col0, vt, B, H, Nq, Nk, head_dim=None):
        if head_dim is None:
            return super().attention(q, q_col0, k, k_col0, vt, B, H, Nq, Nk)
        assert head_dim in (32, 128), "64 is not handed over"
        self.calls.append(("attention_hd", head_dim, H, Nq, Nk))
        D, a = head_dim, H * head_dim
        assert vt.t.shape[0] == B * a
        qq = q.t[:, q_col0:q_col0 + a].reshape(B, Nq, H, D).transpose(1, 2)
        kk = k.t[:, k_col0:k_col0 + a].reshape(B, Nk, H, D).transpose(1, 2)
        vv = vt.t.reshape(B, H, D, -1)[..., :Nk].transpose(2, 3)
        s = qq @ kk.transpose(2, 3) * D ** -0.5
        lse = torch.logsumexp(s, dim=-1) / math.log(2.0)
        o = (s.softmax(-1) @ vv).transpose(1, 2).reshape(B * Nq, a)
        return self.split(o), lse

    def attention_delta(self, do, o, B, H, Nq, head_dim=None):
        if head_dim is None:
            return super().attention_delta(do, o, B, H, Nq)
        self.calls.append(("attention_delta_hd", head_dim, H, Nq))
        a = H * head_dim
        return (do[:, :a] * o.t[:, :a]).reshape(B, Nq, H, head_dim).sum(-1).transpose(1, 2).contiguous()

    def attention_bwd(self, q, q_col0, k, k_col0, v, v_col0, do_row, lse, delta, B, H, Nq, Nk, dq=None, dkv=None, planes=None, head_dim=None):
        if head_dim is None:
            return super().attention_bwd(q, q_col0, k, k_col0, v, v_col0, do_row, lse, delta, B, H, Nq, Nk, dq=dq, dkv=dkv, planes=planes)
        self.calls.append(("attention_bwd_hd", head_dim, H, Nq, Nk))
        D, a, scale = head_dim, H * head_dim, head_dim ** -0.5
        if planes is not None:
            dq, dkv = (planes[0].t, planes[1]), (planes[0].t, planes[2], planes[3])
        hd = lambda t, c0, n: t[:, c0:c0 + a].reshape(B, n, H, D).transpose(1, 2)      # noqa: E731
        qq, kk, vv = hd(q.t, q_col0, Nq), hd(k.t, k_col0, Nk), hd(v.t, v_col0, Nk)
        dO = hd(do_row.t, 0, Nq)
        s = qq @ kk.transpose(2, 3) * scale
        P = torch.exp2(s / math.log(2.0) - lse[..., None])
        dS = P * (dO @ vv.transpose(2, 3) - delta[..., None])
        unhd = lambda t, n: t.transpose(1, 2).reshape(B * n, a)                         # noqa: E731
        if dq is not None:
            dq[0][:, dq[1]:dq[1] + a] = unhd(dS @ kk * scale, Nq)
        if dkv is not None:
            dkv[0][:, dkv[1]:dkv[1] + a] = unhd(dS.transpose(2, 3) @ qq * scale, Nk)
            dkv[0][:, dkv[2]:dkv[2] + a] = unhd(P.transpose(2, 3) @ dO, Nk)
