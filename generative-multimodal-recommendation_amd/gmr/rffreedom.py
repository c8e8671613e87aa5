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
import torch

from . import _lib
from .abstract_recommender import copy64
from .freedom import FREEDOM
from .kernels import ptr, stream
from .rf import D, RFBackbone


class RFFREEDOM(RFBackbone, FREEDOM):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        if not self.use_rf:
            return
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._x1, self._gen = f(self.N, D), f(self.N, D)
        self._cond = f(self.N, 128) if len(self.mods) == 2 else None

    def rf_conditions(self):
        """N x C conditions from the work table (after _project): image then text (rffreedom.py:110-120); the
        table holds text in columns 64:128 and image in 128:192, and its user rows of both are zero."""
        if self._cond is None:
            blk = self.mods[0][2]
            return self.tab[:, 64 * blk:64 * blk + 64]
        copy64(self.tab[:, 128:192], self._cond[:, 0:64])
        copy64(self.tab[:, 64:128], self._cond[:, 64:128])
        return self._cond

    def rf_step_inputs(self):
        """X1 = mean(E_0..E_L) of the last _forward, the conditions, no prior."""
        return self.rf_layer_mean(self.n_ui_layers), self.rf_conditions(), None

    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: FREEDOM's on norm_adj, + rf_inference_mix_ratio * generate(cond) from
        rf_warmup_epochs on (z0: injected start noise)."""
        usr, itm = super().forward_embeddings()
        if not self.rf_warm():
            return usr, itm
        g = self.rf_generator
        self._project()
        g.generate(self.rf_conditions(), z0=z0, out=self._gen)
        # (mean + h) + ratio * gen: the reference adds h last; the two orders differ by one rounding
        _lib.call("gmr_axpy_dev_f32", self.N * D, ptr(g._ratio), ptr(self._gen), ptr(self._eval), stream())
        return usr, itm
