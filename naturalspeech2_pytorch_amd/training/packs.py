"""The packed-weight cache of a training run: one `_Pack` per weight, refreshed in place, all of them in one launch per pass"""
import ctypes
import weakref

import torch

from .. import _lib, ops
from .._lib import check
from ..ops import _p, _stream


class _Pack:
    """one entry of `_PackedCache.map`"""
    __slots__ = ("pw", "sig", "shapes", "src", "refs", "pass_id", "parts")

    def __init__(self, pw, sig, shapes, src, refs, pass_id, parts):
        self.pw = pw                # the PackedWeight
        self.sig = sig              # ((data_ptr, _version) of every parameter) when the pack was last refreshed
        self.shapes = shapes        # shapes of the source matrices: a refresh in place needs the same ones
        self.src = src              # the source tensors, kept alive until the stream has consumed them
        self.refs = refs            # weak references to the parameters
        self.pass_id = pass_id      # the pass that last refreshed the pack
        self.parts = parts          # where the pack's values live in the parameters' storage (`get`), or None


class _RepackTable:
    """the one launch per pass (ns2_weights_repack, then ns2_weights_retile for packs with tile images): this object holds everything
    the two launches read -- the device descriptor table and the array of tiled handles"""
    __slots__ = ("sig", "table", "n", "total", "keys", "tiled", "nt")

    def __init__(self, sig, table, n, total, keys, tiled):
        self.sig, self.table, self.n, self.total, self.keys = sig, table, n, total, keys
        self.nt = len(tiled)
        self.tiled = (ctypes.c_void_p * self.nt)(*tiled) if tiled else None


class _PackedCache:
    """Packed weights of a training run: packed once, refreshed IN PLACE (`ns2_weight_update`: no allocation, no
    synchronisation).  When: the first request of every training PASS (`begin_pass`, called by `passes.training_pass`) for a weight
    that requires grad -- and whenever a version counter moved.  The version counter alone is not enough: PyTorch's fused optimizers
    (`torch.optim.Adam(fused=True)`, what `accelerate` picks on GPUs) update the parameters in place WITHOUT bumping it, and the
    forward would go on multiplying the weights of step 0 (round 5: found through bench.py's `loss_mixed` / `loss_composite` of the
    same iteration, 0.3700 against 0.3630; tests/test_round5_gpu.py::test_fused_optimizer_steps_reach_the_packed_weights).
    A frozen weight is re-packed only when its version moves."""

    LEAN = False        # tile images of the lean mixed linear kernel for the training packs: measured 100.1 vs 98.8 ms per d512 / L12 step WITH them
                        # (the per-pass re-tiling launches cost more than the eligible products gain; tools/exp_graphed_train.py --lean): off

    def __init__(self, precision=3):
        self.map = {}
        self.precision = precision
        self.pass_id = 0
        self._table = None          # _RepackTable: every trainable pack, one launch per pass
        self.lean = self.LEAN       # give mixed linear packs the tile images of the lean kernel (class attribute: the A/B of tools/exp_graphed_train.py)

    # ---- one launch per pass (ns2_weights_repack): possible once every entry has told where its values live (`parts`)
    @staticmethod
    def _part(lib_part, pw, p, mode, row0, col0):
        """`mode`: "n" = the pack's rows / columns / taps are the parameter's; "t" = transposed ([C, R(, T)] from [R, C(, T)]);
        "tf" = transposed with the taps flipped (the dgrad weight of a causal conv)"""
        R, C = p.shape[0], p.shape[1]
        T = p.shape[2] if p.ndim == 3 else 1
        assert p.is_contiguous() and p.dtype == torch.float32
        base = p.data_ptr()
        if mode == "n":
            sr, sc, st, rows, cols = C * T, T, 1, R, C
        elif mode == "t":
            sr, sc, st, rows, cols = T, C * T, 1, C, R
        else:
            sr, sc, st, rows, cols = T, C * T, -1, C, R
            base += 4 * (T - 1)
        return lib_part(pw.handle, base, sr, sc, st, row0, rows, col0, cols)

    def _signature(self):
        # (storage and trainability of every parameter: a re-allocated, frozen or unfrozen parameter rebuilds the table)
        return tuple((k, tuple((p.data_ptr(), p.requires_grad) for p in (r() for r in v.refs) if p is not None)) for k, v in self.map.items())

    def _repack_all(self):
        """every trainable entry with a `parts` description in one launch; False when some entry cannot be described"""
        if not self.map or any(v.parts is None or any(r() is None for r in v.refs) for v in self.map.values()):
            return False
        lib = _lib.load()
        sig = self._signature()
        if self._table is None or self._table.sig != sig:
            parts, keys = [], set()
            for k, v in self.map.items():
                params = [r() for r in v.refs]
                if any(p is None for p in params):                     # (collected since the check above: a cycle freed in between)
                    return False
                if not any(p.requires_grad for p in params):
                    continue
                keys.add(k)
                dev = params[0].device
                for (idx, mode, row0, col0) in v.parts:
                    parts.append(self._part(_lib.RepackPart, v.pw, params[idx], mode, row0, col0))
            if not parts:
                return False
            arr = (_lib.RepackPart * len(parts))(*parts)
            nbytes = lib.ns2_weights_repack_table_bytes(len(parts))
            table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            total = ctypes.c_int64(0)
            check(lib.ns2_weights_repack_build(arr, len(parts), table.data_ptr(), nbytes, ctypes.byref(total), _stream()), "ns2_weights_repack_build")
            tiled = [self.map[k].pw.handle.value for k in keys if getattr(self.map[k].pw, "tiled", False)]
            self._table = _RepackTable(sig, table, len(parts), total.value, keys, tiled)
        t = self._table
        check(lib.ns2_weights_repack(t.table.data_ptr(), t.n, t.total, _stream()), "ns2_weights_repack")
        if t.nt:                              # the lean kernels' tile images follow their packs (one small launch per tiled weight)
            check(lib.ns2_weights_retile(t.tiled, t.nt, _stream()), "ns2_weights_retile")
        return True

    def begin_pass(self, frozen=False):
        self.pass_id += 1
        if frozen:                           # `with training.weights_unchanged():` -- the packs of the last pass are these weights' (stamp them fresh)
            for v in self.map.values():
                v.pass_id = self.pass_id
            return
        if self.pass_id > 1 and self._repack_all():
            for k in self._table.keys:                                       # what the launch re-packed is fresh for this pass
                v = self.map[k]                                              # (a frozen weight is not in the table: its version rule stands)
                v.sig, v.pass_id = tuple((p.data_ptr(), p._version) for p in (r() for r in v.refs)), self.pass_id

    def _purge(self):
        dead = [k for k, v in self.map.items() if any(r() is None for r in v.refs)]
        for k in dead:
            del self.map[k]
        if dead:
            self._table = None

    def get(self, key, params, make_src, parts=None, **pack_kw):
        """`key` carries id()s of `params`: an entry is only a hit while those very objects are alive (weak references), so a
        recycled id can never return another model's weights.  `parts`: [(index into params, mode, row0, col0)] -- where the pack's
        values live in the parameters' own storage (`_part`), which lets begin_pass refresh every pack of the model in one launch;
        `make_src` builds the same matrix as a tensor for the first pack (and for entries without `parts`)."""
        sig = tuple((p.data_ptr(), p._version) for p in params)
        hit = self.map.get(key)
        if hit is not None and any(r() is not p for r, p in zip(hit.refs, params)):
            hit = None
        if hit is None:
            self._purge()                    # a miss is rare (first step of a model): drop the packs of models that no longer exist
            self._table = None
        if hit is not None and hit.sig == sig and (hit.pass_id == self.pass_id or not any(p.requires_grad for p in params)):
            return hit.pw
        src = make_src()
        src = src if isinstance(src, tuple) else (src, None)
        w, extra = (t.detach().float().contiguous() if t is not None else None for t in src)
        shapes = (tuple(w.shape), None if extra is None else tuple(extra.shape))
        if hit is not None and hit.shapes == shapes:
            check(_lib.load().ns2_weight_update(hit.pw.handle, w.data_ptr(), _p(extra), _stream()), "ns2_weight_update")
            hit.sig, hit.src, hit.pass_id, hit.parts = sig, (w, extra), self.pass_id, parts
            return hit.pw
        pw = ops.PackedWeight(w, extra1x1=extra, precision=self.precision, **pack_kw)
        if self.precision == 4 and w.ndim == 2 and extra is None and not pack_kw.get("geglu") and w.shape[1] >= 96 and self.lean:
            pw.tile_linear()                 # round 6: the lean mixed linear kernel (csrc/gemm3_kernel.h) for the forward and dgrad products
            pw.tiled = True                  # on whole 256-row tiles -- bit-identical to gemm2_kernel<2, *>, 10-15 % faster
        self._table = None                   # (a hit whose source changed shape gets a NEW pack: the re-pack table still names the old one's storage)
        self.map[key] = _Pack(pw, sig, shapes, (w, extra), tuple(weakref.ref(p) for p in params), self.pass_id, parts)
        return pw
