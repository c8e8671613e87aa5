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
import ctypes

import torch

from . import _lib
from . import kernels as K
from .bm3 import BM3
from .kernels import ptr, stream
from .rf import D, RFGenerator, check_config


def _get(config, key, default):
    return config[key] if key in config and config[key] is not None else default


class RFBM3(BM3):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        self.use_rf = bool(_get(config, "use_rf", True))
        self.rf_generator = None
        if not self.use_rf:
            return
        check_config(config)
        C = 64 * len(self.mods)
        self.rf_generator = RFGenerator(
            self.n_users, self.n_items, C, self.device, n_layers=_get(config, "rf_n_layers", 2),
            dropout=_get(config, "rf_dropout", 0.1), learning_rate=_get(config, "rf_learning_rate", 0.0001),
            sampling_steps=_get(config, "rf_sampling_steps", 10), warmup_epochs=_get(config, "rf_warmup_epochs", 5),
            inference_mix_ratio=_get(config, "rf_inference_mix_ratio", 0.2),
            contrast_temp=_get(config, "rf_contrast_temp", 0.2), contrast_weight=_get(config, "rf_loss_weight", 1.0),
            n_negatives=_get(config, "rf_infonce_negatives", 1024), seed=self.seed)
        self._training_epoch = -1  # incremented to 0 by the first pre_epoch_processing
        N, U = self.N, self.n_users
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._x1, self._gen = f(N, D), f(max(U, 1), D)
        # the user rows of both stay zero: gmr_rf_item_inputs writes the item rows only
        self._cond, self._prior = f(N, C), f(N, D)
        self._inws = f(int(_lib.load().gmr_rf_item_inputs_ws_floats(self.n_items)))

    # ------------------------------------------------------------------ state
    def extra_state(self):
        st = super().extra_state()
        if self.use_rf:
            st.update({"rf_epoch": int(self._training_epoch), "rf_step": int(self.rf_generator.step_ctr)})
        return st

    def load_extra_state(self, st):
        super().load_extra_state(st)
        if self.use_rf:
            self._training_epoch = int(st["rf_epoch"])
            self.rf_generator.step_ctr = int(st["rf_step"])
            self.rf_generator.set_epoch(self._training_epoch)

    def pre_epoch_processing(self):
        super().pre_epoch_processing()
        if self.use_rf:
            self._training_epoch += 1
            self.rf_generator.set_epoch(self._training_epoch)

    # ------------------------------------------------------------------ RF inputs
    def rf_inputs(self):
        """(cond N x C, prior N x 64) from the projected table tv (after _project): image then text."""
        T, V = self._tables()
        ld = self.tv.stride(0)
        _lib.call("gmr_rf_item_inputs", self.n_items, self.n_users, ptr(T), ld, ptr(V), ld, ptr(self._cond),
                  self._cond.stride(0), ptr(self._prior), self._prior.stride(0), ptr(self._inws), stream())
        return self._cond, self._prior

    def rf_target(self):
        """X1 = mean(E_0..E_n) of the last _forward, without the item residual (all_embeddings_ori)."""
        tabs = [self.slab.view("E")] + self._layers[:self.n_layers]
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", self.N, self.n_users, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(self._x1), self._x1.stride(0),
                  stream())
        return self._x1

    # ------------------------------------------------------------------ training
    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, keep=None,
                 rf_draws=None):
        """BM3's step, then the RF step on the tables of that step (the reference detaches all three, so nothing
        flows back; BM3's backward leaves E, the layer tables and tv as the forward wrote them).  rf_draws: injected
        draws for RFGenerator.train_step.  rf_loss_terms() reads the RF losses."""
        loss = super().rec_step(users, pos, neg, plan_bpr, plan_cl, norm_rows, reg_share, keep=keep)
        if self.use_rf:
            cond, prior = self.rf_inputs()
            self.rf_generator.train_step(self.rf_target(), cond, users, pos, prior=prior, **(rf_draws or {}))
        return loss

    def rf_loss_terms(self):
        """[rf_loss, cl_loss, total] of the last RF step (device tensor)."""
        return self.rf_generator._w["loss"]

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: (P(ua), P(ib)); from rf_warmup_epochs on ua += rf_inference_mix_ratio *
        generate(0) (z0: injected start noise, the first U rows are used)."""
        if not self.use_rf or not self.rf_generator.warmed_up() or self.n_users == 0:
            return super().forward_embeddings()
        g, s, U = self.rf_generator, self.slab, self.n_users
        self._forward(self._eval)
        g.generate(self._cond[:U], z0=None if z0 is None else z0[:U], out=self._gen[:U])
        _lib.call("gmr_axpy_dev_f32", U * D, ptr(g._ratio), ptr(self._gen), ptr(self._eval), stream())
        K.gemm(self._eval, s.view("Wp"), self._pred, trans_b=True, epi=K.EPI_BIAS, bias=s.view("bp"))
        return self._pred[:U], self._pred[U:]

    @torch.no_grad()
    def full_sort_predict(self, interaction, z0=None):
        if z0 is None:
            return super().full_sort_predict(interaction)
        fe = self.forward_embeddings
        self.forward_embeddings = lambda: fe(z0)
        try:
            return super().full_sort_predict(interaction)
        finally:
            del self.forward_embeddings
