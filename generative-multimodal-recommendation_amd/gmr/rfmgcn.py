"""RFMGCN on MI355X — drop-in for models/rfmgcn.py of the reference: MGCN with the rectified-flow embedding generator
(gmr/rf.py) trained next to it and mixed into every row of the evaluation table.

MGCN carries both modal views to the users over R, so (unlike RFFREEDOM and RFBM3, whose user conditions are zero) the
RF inputs are dense over all N = U + I rows.  With a, b, c, side and all = c + side as in gmr/mgcn.py:

  training    MGCN's step unchanged (the reference mixes nothing in training, rf_modules.py:1070-1072), then one
              RFGenerator.train_step on that step's tables, all detached in the reference (rfmgcn.py:129-204):
                X1    = all (use_denoise is off, so rf_target = all_embeds.detach())
                cond  = [a | b], N x 128, the image view then the text view: the table ab itself, no copy
                prior = [Z_u - mean_users(Z_u); Z_i - mean_items(Z_i)], Z = (a + b) / 2 (:156-172), one entry point
                        (gmr_rf_view_prior, csrc/rf_prior.hip), added to the velocity as (1 - t)^2 0.2 prior
              All three are constants of the RF step, so MGCN's nineteen gradients are MGCN's.  MGCN's backward reads
              ab and never writes ab or all (mgcn.py step_backward), so both are as the forward wrote them when the RF
              step reads them.  The reference also runs its sampler there and discards the result; it is not run here.
  evaluation  MGCN's tables; from rf_warmup_epochs on, all N rows + rf_inference_mix_ratio * generate([a | b])
              (:205-222).  The mix is written into a table of its own (_mix), so all stays MGCN's; the next training
              step's _forward rewrites all in full anyway.  Before warm-up the sampler is not run and the tables are
              MGCN's bit for bit.

Draws: MGCN draws nothing; the generator's are Philox streams keyed on (seed, RF step counter, site).  The reference
draws the evaluation's start noise inside every full_sort_predict; here it is drawn once per evaluation pass
(Trainer calls forward_embeddings once), as in RFFREEDOM.

use_rf: False is MGCN and allocates no generator.  use_denoise / use_2rf: True and rf_hidden_dim != 128 raise
NotImplementedError.  A world size above 1 raises, as MGCN does.
"""
import torch

from . import _lib
from .abstract_recommender import copy64
from .kernels import ptr, stream
from .mgcn import MGCN
from .rf import D, RFBackbone


class RFMGCN(RFBackbone, MGCN):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        if not self.use_rf:
            return
        N = self.N
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._prior, self._gen, self._mix = f(N, D), f(N, D), f(N, D)
        self._pws = f(int(_lib.load().gmr_rf_view_prior_ws_floats(self.n_users, self.n_items)))

    def rf_step_inputs(self):
        """X1 = all, cond = ab, and the N x 64 prior from the two views of the last _forward (the column blocks of ab).
        MGCN's step_backward reads ab and writes neither ab nor all, so both are intact after the step."""
        ab = self.ab
        _lib.call("gmr_rf_view_prior", self.n_users, self.n_items, ptr(ab), ab.stride(0), ptr(ab[:, D:]), ab.stride(0),
                  ptr(self._prior), self._prior.stride(0), ptr(self._pws), stream())
        return self.all, ab, self._prior

    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: MGCN's, and from rf_warmup_epochs on all + rf_inference_mix_ratio *
        generate(ab) over all N rows, in a table of its own (z0: injected start noise)."""
        usr, itm = super().forward_embeddings()
        if not self.rf_warm():
            return usr, itm
        g, U = self.rf_generator, self.n_users
        g.generate(self.ab, z0=z0, out=self._gen)
        copy64(self.all, self._mix)
        _lib.call("gmr_axpy_dev_f32", self.N * D, ptr(g._ratio), ptr(self._gen), ptr(self._mix), stream())
        return self._mix[:U], self._mix[U:]
