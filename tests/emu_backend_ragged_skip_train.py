"""TEST INFRASTRUCTURE: `tests/emu_backend_ragged.EmuBackendRagged` plus the `row_lens=` keyword of the three product calls
(`HipBackend.gemm_f32` / `gemm_split` / `wgrad_rows`; include/ns2hip_train.h), restated in plain torch from the two
contracts -- so that the host logic of a skipping training pass (which product of functions.py / model_pass.py is handed the lengths,
and what the others then read) is checked against torch autograd without a GPU (tests/test_ragged_skip_training_cpu.py).  Never imported
by the product.

The contracts restated, with H_b = min(n, 256 ceil(clamp(lens[b], 1, n) / 256)):
  * a skipping product writes ZEROS into rows >= H_b of every output it has (fp32 with or without a residual, planes); rows before H_b
    are what the product without lengths gives.  Its operand's hidden rows are not read from a visible row of a causal or plain product
    (here: replaced by NaN before the product, so a read would show); an anticausal product REQUIRES zeros there (asserted);
  * a skipping weight gradient neither fetches nor multiplies the tokens >= H_b (here: selected to 0 in both operands, NaN included).

`frame_rows` = b * n of the pass under test.  The backend ASSERTS that every product over that many rows arrives with the lengths and
that no product over another row count does (the resampler, cond_to_model_dim with n_c != n, the cross attention's k | v)."""
import torch

from tests.emu_backend import EP
from tests.emu_backend_ragged import EmuBackendRagged


def extent(lens, n):
    return ((lens.long().clamp(1, n) + 255) // 256 * 256).clamp(max=n)


class EmuBackendRaggedSkipTrain(EmuBackendRagged):
    name = "emu-ragged-skip-train"

    def __init__(self, frame_rows=None):
        super().__init__()
        self.frame_rows = frame_rows          # None: a pass that must not skip -- any row_lens is an error
        self.skipped = []                     # (call, rows) of every product that took the lengths

    def _hidden(self, row_lens, M, what):
        """bool [M]: rows at or behind their utterance's extent; checks the hand-over"""
        if row_lens is None:
            assert self.frame_rows is None or M != self.frame_rows, f"{what}: a frame-row product of a skipping pass arrived without lengths"
            return None
        lens, n = row_lens
        assert self.frame_rows is not None and M == self.frame_rows, f"{what}: a product over {M} rows arrived with lengths"
        assert lens.dtype == torch.int32 and n % 256 == 0 and lens.numel() * n == M
        self.skipped.append((what, M))
        return (torch.arange(n)[None] >= extent(lens, n)[:, None]).reshape(M)

    def _operand(self, a, hidden, taps, pad_left, what):
        anticausal = taps > 1 and 0 <= pad_left < taps - 1
        if anticausal:
            assert torch.count_nonzero(a.t[hidden]) == 0, f"{what}: an anticausal product needs zeros in its operand's hidden rows"
            return a
        return EP(torch.where(hidden[:, None], torch.full((), float("nan")), a.t))      # a visible row must not read them

    def gemm_f32(self, pw, a, bias=None, resid=None, taps=0, dil=1, seq_len=0, pad_left=-1, row_lens=None):
        hidden = self._hidden(row_lens, a.rows, "gemm_f32")
        if hidden is None:
            return super().gemm_f32(pw, a, bias=bias, resid=resid, taps=taps, dil=dil, seq_len=seq_len, pad_left=pad_left)
        if resid is not None:
            resid = torch.where(hidden[:, None], torch.zeros(()), resid)                # (not read either)
        out = super().gemm_f32(pw, self._operand(a, hidden, taps, pad_left, "gemm_f32"), bias=bias, resid=resid, taps=taps, dil=dil,
                               seq_len=seq_len, pad_left=pad_left)
        N = pw.w.shape[0]
        assert not torch.isnan(out[~hidden][:, :N]).any(), "a visible row read a hidden one"
        out[:, :N] = torch.where(hidden[:, None], torch.zeros(()), out[:, :N])
        return out

    def gemm_split(self, pw, a, bias=None, taps=0, dil=1, seq_len=0, attn=False, row_lens=None):
        hidden = self._hidden(row_lens, a.rows, "gemm_split")
        if hidden is None:
            return super().gemm_split(pw, a, bias=bias, taps=taps, dil=dil, seq_len=seq_len, attn=attn)
        out = super().gemm_split(pw, self._operand(a, hidden, taps, -1, "gemm_split"), bias=bias, taps=taps, dil=dil, seq_len=seq_len, attn=attn)
        assert not torch.isnan(out.t[~hidden]).any(), "a visible row read a hidden one"
        return EP(torch.where(hidden[:, None], torch.zeros(()), out.t))

    def wgrad_rows(self, dy, x, R, T, K, dil=1, seq_len=0, row_lens=None):
        hidden = self._hidden(row_lens, dy.rows, "wgrad_rows")
        if hidden is None:
            return super().wgrad_rows(dy, x, R, T, K, dil, seq_len)
        z = torch.zeros(())
        return super().wgrad_rows(EP(torch.where(hidden[:, None], z, dy.t)), EP(torch.where(hidden[:, None], z, x.t)), R, T, K, dil, seq_len)
