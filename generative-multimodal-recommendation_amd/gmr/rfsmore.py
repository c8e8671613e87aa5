"""RFSMORE on MI355X — drop-in for models/rfsmore.py of the reference: SMORE with the rectified-flow embedding
generator (gmr/rf.py) trained next to it and mixed into every row of the evaluation table.

SMORE has three views, so the generator takes three conditions, N x 192, dense over all N = U + I rows.  With a, b, f,
c, side, all = c + side and the preference gates gi, gt, gf (dropout mask and 1 / (1 - p) included) as in gmr/smore.py:

  training    SMORE's step unchanged (the reference mixes nothing in training, rf_modules.py:1070-1072), then one
              RFGenerator.train_step on that step's tables, all detached in the reference (rfsmore.py:152-206):
                X1    = all
                cond  = [a | b | gf f]: the image view, the text view and the *gated* fusion view.  The reference
                        reassigns fusion_embeds = fusion_prefer * fusion_embeds (:143) before it collects the
                        conditions (:176), so the third block carries that step's keep mask and scale; a and b are the
                        plain views
                prior = [Z_u - mean_users(Z_u); Z_i - mean_items(Z_i)], Z = (a + b + gf f) / 3 (:179-195), added to
                        the velocity as (1 - t)^2 0.2 prior
              cond and prior come from one entry point (gmr_rf_view3_inputs, csrc/rf_prior.hip) on the three column
              blocks of abf and on saved[:, 384:448] (gf) of the last _forward.  All three are constants of the RF
              step, so SMORE's 29 gradients are SMORE's.  SMORE's step_backward reads abf and saved and writes none of
              abf, saved, all (its outputs are dabf, dc, zf, dpur, zp, dvt and the slab gradient), so they are as the
              forward wrote them when the RF step reads them.  The reference also runs its sampler there and discards
              the result (:217); it is not run here.
  evaluation  SMORE's tables; from rf_warmup_epochs on, all N rows + rf_inference_mix_ratio * generate(cond) (:228-246)
              with cond from the evaluation forward (no dropout: gf is the bare sigmoid gate).  The mix is written
              into a table of its own (_mix), so all stays SMORE's.  Before warm-up the sampler is not run and the
              tables are SMORE's bit for bit.

Draws: SMORE's keep masks are its own Philox stream (its step counter travels in extra_state next to rf_epoch /
rf_step); the generator's are keyed on (seed, RF step counter, site).  The evaluation's start noise is drawn once per
evaluation pass, as in RFMGCN.

use_denoise: the reference's YAML ships True, but the reference hands the model the train data loader, which has no df,
so CausalDenoiser.load_treatment_labels leaves treatment_matrix None and its forward returns (None, 0.0): as shipped,
rf_target is all_embeds and ps_loss is 0, which is use_denoise: False.  The YAML here says False, and True raises
NotImplementedError, as do use_2rf: True and rf_hidden_dim != 128.  use_rf: False is SMORE and allocates nothing.  A
world size above 1 raises, as SMORE does.
"""
import torch

from . import _lib
from .abstract_recommender import copy64
from .kernels import ptr, stream
from .rf import D, RFBackbone
from .smore import SMORE


class RFSMORE(RFBackbone, SMORE):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        if not self.use_rf:
            return
        N = self.N
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._cond, self._prior, self._gen, self._mix = f(N, 3 * D), f(N, D), f(N, D), f(N, D)
        self._pws = f(int(_lib.load().gmr_rf_view3_inputs_ws_floats(self.n_users, self.n_items)))

    def rf_condition_dim(self):
        return 3 * D  # image, text and fusion views

    def _rf_inputs(self):
        """_cond = [a | b | gf f] and _prior from the views and the fusion gate of the last _forward."""
        abf, sv = self.abf, self.saved
        _lib.call("gmr_rf_view3_inputs", self.n_users, self.n_items, ptr(abf), abf.stride(0), ptr(abf[:, D:]),
                  abf.stride(0), ptr(abf[:, 2 * D:]), abf.stride(0), ptr(sv[:, 6 * D:]), sv.stride(0), ptr(self._cond),
                  self._cond.stride(0), ptr(self._prior), self._prior.stride(0), ptr(self._pws), stream())

    def rf_step_inputs(self):
        """X1 = all, cond = [a | b | gf f] and the N x 64 prior.  SMORE's step_backward writes none of abf, saved,
        all, so they are intact after the step."""
        self._rf_inputs()
        return self.all, self._cond, self._prior

    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: SMORE's, and from rf_warmup_epochs on all + rf_inference_mix_ratio *
        generate(cond) over all N rows, in a table of its own (z0: injected start noise)."""
        usr, itm = super().forward_embeddings()
        if not self.rf_warm():
            return usr, itm
        g, U = self.rf_generator, self.n_users
        self._rf_inputs()
        g.generate(self._cond, z0=z0, out=self._gen)
        copy64(self.all, self._mix)
        _lib.call("gmr_axpy_dev_f32", self.N * D, ptr(g._ratio), ptr(self._gen), ptr(self._mix), stream())
        return self._mix[:U], self._mix[U:]
