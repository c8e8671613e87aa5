"""RFFREEDOM on MI355X — drop-in for models/rffreedom.py of the reference: FREEDOM with the rectified-flow
embedding generator (gmr/rf.py) trained next to it and mixed into the evaluation embeddings.

  training    FREEDOM's step unchanged (the reference mixes nothing in training, rf_modules.py:1070-1072), then one
              RFGenerator.train_step on that step's tables: X1 = the mean of E_0..E_L without the item-item term,
              conditions = [image_trs(image) | text_trs(text)] on the item rows and zeros on the user rows
              (rffreedom.py:106-120: FREEDOM has no R).  Both are constants of the RF step, so FREEDOM's gradients are
              FREEDOM's.  The reference also runs its sampler there and discards the result; it is not run here.
  evaluation  FREEDOM's tables on norm_adj; from rf_warmup_epochs on, + rf_inference_mix_ratio * generate(cond).

use_rf: False is FREEDOM.  use_denoise / use_2rf: True and rf_hidden_dim != 128 raise NotImplementedError.
"""
import ctypes

import torch

from . import _lib
from .freedom import FREEDOM
from .kernels import ptr, stream
from .rf import D, RFGenerator, check_config


def _get(config, key, default):
    return config[key] if key in config and config[key] is not None else default


class RFFREEDOM(FREEDOM):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        self.use_rf = bool(_get(config, "use_rf", True))
        self.rf_generator = None
        if not self.use_rf:
            return
        check_config(config)
        self.rf_generator = RFGenerator(
            self.n_users, self.n_items, 64 * len(self.mods), self.device, n_layers=_get(config, "rf_n_layers", 2),
            dropout=_get(config, "rf_dropout", 0.1), learning_rate=_get(config, "rf_learning_rate", 0.0001),
            sampling_steps=_get(config, "rf_sampling_steps", 10), warmup_epochs=_get(config, "rf_warmup_epochs", 5),
            inference_mix_ratio=_get(config, "rf_inference_mix_ratio", 0.2),
            contrast_temp=_get(config, "rf_contrast_temp", 0.2), contrast_weight=_get(config, "rf_loss_weight", 1.0),
            n_negatives=_get(config, "rf_infonce_negatives", 1024), seed=self.seed)
        self._training_epoch = -1  # incremented to 0 by the first pre_epoch_processing
        N = self.N
        self._x1 = torch.zeros((N, D), dtype=torch.float32, device=self.device)
        self._gen = torch.zeros((N, D), dtype=torch.float32, device=self.device)
        self._cond = torch.zeros((N, 128), dtype=torch.float32, device=self.device) if len(self.mods) == 2 else None

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
    def rf_conditions(self):
        """N x C conditions from the work table (after _project): image then text (rffreedom.py:110-120); the
        table holds text in columns 64:128 and image in 128:192, and its user rows of both are zero."""
        if self._cond is None:
            blk = self.mods[0][2]
            return self.tab[:, 64 * blk:64 * blk + 64]
        self._copy64(self.tab[:, 128:192], self._cond[:, 0:64])
        self._copy64(self.tab[:, 64:128], self._cond[:, 64:128])
        return self._cond

    def rf_target(self):
        """X1 = mean(E_0..E_L) of the last _forward, without the item-item term (all_embeddings_ori)."""
        tabs = [self.slab.view("E")] + self._layers[:self.n_ui_layers]
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", self.N, self.n_users, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(self._x1), self._x1.stride(0),
                  stream())
        return self._x1

    # ------------------------------------------------------------------ training
    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, rf_draws=None):
        """FREEDOM's step, then the RF step on the tables of that step (their reference detaches both, so nothing
        flows back).  rf_draws: injected draws for RFGenerator.train_step.  rf_loss_terms() reads the RF losses."""
        loss = super().rec_step(users, pos, neg, plan_bpr, plan_cl, norm_rows, reg_share)
        if self.use_rf:
            self.rf_generator.train_step(self.rf_target(), self.rf_conditions(), users, pos, **(rf_draws or {}))
        return loss

    def rf_loss_terms(self):
        """[rf_loss, cl_loss, total] of the last RF step (device tensor)."""
        return self.rf_generator._w["loss"]

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: FREEDOM's on norm_adj, + rf_inference_mix_ratio * generate(cond) from
        rf_warmup_epochs on (z0: injected start noise)."""
        usr, itm = super().forward_embeddings()
        if not self.use_rf or not self.rf_generator.warmed_up():
            return usr, itm
        g = self.rf_generator
        self._project()
        g.generate(self.rf_conditions(), z0=z0, out=self._gen)
        # (mean + h) + ratio * gen: the reference adds h last; the two orders differ by one rounding
        _lib.call("gmr_axpy_dev_f32", self.N * D, ptr(g._ratio), ptr(self._gen), ptr(self._eval), stream())
        return usr, itm

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
