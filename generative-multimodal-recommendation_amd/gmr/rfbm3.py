"""RFBM3 on MI355X — drop-in for models/rfbm3.py of the reference: BM3 with the rectified-flow embedding generator
(gmr/rf.py) trained next to it and mixed into the evaluation's user rows.

  training    BM3's step unchanged (the reference mixes nothing in training, rf_modules.py:1070-1072), then one
              RFGenerator.train_step on that step's tables:
                X1    = mean(E_0..E_n) without the item residual (all_embeddings_ori, rfbm3.py:98)
                cond  = [image_trs(image) | text_trs(text)] on the item rows, zeros on the user rows (:114-127: BM3
                        has no R)
                prior = [0; Z - mean_items(Z)], Z = image_trs(image) + text_trs(text) (:146-175; the user half is
                        Z_u - mean(Z_u) of an all-zero Z_u), added to the velocity as (1 - t)^2 0.2 prior
              All three are constants of the RF step, so BM3's ten gradients are BM3's.  The item rows of cond and
              prior are one entry point (gmr_rf_item_inputs) on the projected table tv of the step; the user rows of
              both are zeroed at construction and never written.  The reference also runs its sampler there and
              discards the result; it is not run here.
  evaluation  BM3's tables; from rf_warmup_epochs on, the user rows + rf_inference_mix_ratio * generate(0): the
              reference mixes all N rows and then overwrites the item rows with i_g_embeddings_ori + h
              (rfbm3.py:233), so only the user rows keep the mix, and their conditions are zero: the sampler runs on
              the U user rows alone (a row's result does not depend on the rows around it).

use_rf: False is BM3.  use_denoise / use_2rf: True and rf_hidden_dim != 128 raise NotImplementedError.
"""
import torch

from . import _lib
from . import kernels as K
from .bm3 import BM3
from .kernels import ptr, stream
from .rf import D, RFBackbone


class RFBM3(RFBackbone, BM3):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        if not self.use_rf:
            return
        N, U = self.N, self.n_users
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._x1, self._gen = f(N, D), f(max(U, 1), D)
        # the user rows of both stay zero: gmr_rf_item_inputs writes the item rows only
        self._cond, self._prior = f(N, self.rf_generator.C), f(N, D)
        self._inws = f(int(_lib.load().gmr_rf_item_inputs_ws_floats(self.n_items)))

    def rf_step_inputs(self):
        """cond (N x C, image then text) and prior (N x 64) from the projected table tv of the last step, then X1 =
        mean(E_0..E_n) of its _forward."""
        T, V = self._tables()
        ld = self.tv.stride(0)
        _lib.call("gmr_rf_item_inputs", self.n_items, self.n_users, ptr(T), ld, ptr(V), ld, ptr(self._cond),
                  self._cond.stride(0), ptr(self._prior), self._prior.stride(0), ptr(self._inws), stream())
        return self.rf_layer_mean(self.n_layers), self._cond, self._prior

    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: (P(ua), P(ib)); from rf_warmup_epochs on ua += rf_inference_mix_ratio *
        generate(0) (z0: injected start noise, the first U rows are used)."""
        if not self.rf_warm() or self.n_users == 0:
            return super().forward_embeddings()
        g, s, U = self.rf_generator, self.slab, self.n_users
        self._forward(self._eval)
        g.generate(self._cond[:U], z0=None if z0 is None else z0[:U], out=self._gen[:U])
        _lib.call("gmr_axpy_dev_f32", U * D, ptr(g._ratio), ptr(self._gen), ptr(self._eval), stream())
        K.gemm(self._eval, s.view("Wp"), self._pred, trans_b=True, epi=K.EPI_BIAS, bias=s.view("bp"))
        return self._pred[:U], self._pred[U:]
