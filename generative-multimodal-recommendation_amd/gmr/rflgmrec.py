"""RFLGMRec on MI355X — drop-in for models/rflgmrec.py of the reference: LGMRec with the rectified-flow embedding
generator (gmr/rf.py) trained on its collaborative view and, in evaluation, mixed into that view *before* the
hypergraph block.

Unlike the other RF models, the generated rows do not end in all + r * gen: they enter cge, and everything LGMRec
computes after cge reads the mixed table.  With cge, mge = [mge_v | mge_t], hi, hu, lat, ghe and all as in
gmr/lgmrec.py:

  training    LGMRec's step unchanged (mix_embeddings(training=True) returns the original cge, rf_modules.py:1066-1072,
              and every RF input is detached), and one RFGenerator.train_step on the tables of that step's forward
              (rflgmrec.py:98-154):
                X1    = cge, the mean of the LightGCN layers (cf_model 'mf': the table E itself)
                cond  = [mge_v | mge_t], N x 128, the propagated modal views, not normalised: the table self.mge
                        itself, no copy
                prior = [Z_u - mean_users(Z_u); Z_i - mean_items(Z_i)], Z = mge_v + mge_t: a sum, no mean of the
                        views (:125-143), one entry point (gmr_rf_view_sum_prior, csrc/rf_prior.hip), added to the
                        velocity as (1 - t)^2 0.2 prior
              LGMRec.step_backward reuses the _mm hop buffers for the backward hops, and self.mge is one of them, so
              the conditions do not survive LGMRec's step: the RF step runs at the head of step_backward, after the
              forward and the loss kernels and before the first backward launch.  It reads cge and mge and writes the
              generator's own buffers and slab and _prior alone, so its place on the stream changes no LGMRec value:
              the six gradients, the loss terms, the draws and the Philox counters are the LGMRec class's bit for
              bit.  The reference also runs its sampler in the training forward and discards the result (:165-169); it
              is not run here.
  evaluation  before rf_warmup_epochs: LGMRec's tables bit for bit for the same Gumbel noise; the sampler is not run.
              From warm-up on (:178-191): cge' = cge + rf_inference_mix_ratio * generate([mge_v | mge_t]) over all N
              rows in one launch (gmr_rf_sample_mix: the mix is the sampler's epilogue) into a table of its own,
              _mixc (at cf_model 'mf' cge is a view of the parameter slab and must not be written), then LGMRec's
              forward from the hypergraph block on with cge' in place of cge: lat from cge'[U:], the layer loop, and
              all = cge' + n(mge_v) + n(mge_t) + alpha n(ghe).  LGMRec._forward asks _cge_for_hyper(cge) for the table
              that block reads; it is the identity in LGMRec and in training.

Draws: the Gumbel draws come from LGMRec's evaluation-pass counter; the start noise z0 is drawn once per
forward_embeddings call, keyed on the generator's (seed, step_ctr, SITE_Z0), as in RFMGCN.  Both may be injected:
forward_embeddings(noise=None, z0=None).  extra_state carries LGMRec's counters next to rf_epoch / rf_step.

use_denoise: the reference's YAML ships True, but the reference hands the model the train data loader, which has no df,
so CausalDenoiser.load_treatment_labels leaves treatment_matrix None and its forward returns (None, 0.0): as shipped,
rf_target is cge and ps_loss is 0, which is use_denoise: False (the reason gmr/rfsmore.py gives).  The YAML here says
False, and True raises NotImplementedError, as do use_2rf: True and rf_hidden_dim != 128.  use_rf: False is LGMRec and
allocates nothing.  A world size above 1 raises, as LGMRec does.
"""
import torch

from . import _lib
from .kernels import ptr, stream
from .lgmrec import LGMRec
from .rf import D, RFBackbone


class RFLGMRec(RFBackbone, LGMRec):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        self._rf_batch = None   # (users, pos, rf_draws) of the rec_step in flight
        self._mixing = False    # inside a warmed-up forward_embeddings
        self._z0 = None
        if not self.use_rf:
            return
        N = self.N
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._prior, self._mixc = f(N, D), f(N, D)
        self._pws = f(int(_lib.load().gmr_rf_view_sum_prior_ws_floats(self.n_users, self.n_items)))

    def rf_condition_dim(self):
        return 2 * D  # the two propagated modal views

    def rf_step_inputs(self, cge):
        """X1 = cge, cond = mge (the table of the last _forward itself) and the N x 64 prior of Z = mge_v + mge_t.
        Valid between that _forward and LGMRec.step_backward, which reuses mge's buffer."""
        mge = self.mge
        _lib.call("gmr_rf_view_sum_prior", self.n_users, self.n_items, ptr(mge), mge.stride(0), ptr(mge[:, D:]),
                  mge.stride(0), ptr(self._prior), self._prior.stride(0), ptr(self._pws), stream())
        return cge, mge, self._prior

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, rf_draws=None,
                 **backbone_kw):
        """LGMRec's step (backbone_kw: g, keep) with the RF step on that step's cge and mge at the head of its
        backward (step_backward).  rf_draws: injected draws for RFGenerator.train_step.  rf_loss_terms() reads the RF
        losses."""
        self._rf_batch = (users, pos, rf_draws) if self.use_rf else None
        try:
            return LGMRec.rec_step(self, users, pos, neg, plan_bpr, plan_cl, norm_rows, reg_share, **backbone_kw)
        finally:
            self._rf_batch = None

    def step_backward(self, cge):
        if self._rf_batch is not None:   # before the backward hops overwrite mge
            users, pos, rf_draws = self._rf_batch
            X1, cond, prior = self.rf_step_inputs(cge)
            self.rf_generator.train_step(X1, cond, users, pos, prior=prior, **(rf_draws or {}))
        super().step_backward(cge)

    def _cge_for_hyper(self, cge):
        """cge in training and before warm-up; in a warmed-up evaluation cge' = cge + ratio * generate(mge) in _mixc."""
        if not self._mixing:
            return cge
        self.rf_generator.generate(self.mge, z0=self._z0, out=self._mixc, base=cge)
        return self._mixc

    @torch.no_grad()
    def forward_embeddings(self, noise=None, z0=None):
        """full_sort_predict's tables: LGMRec's, and from rf_warmup_epochs on LGMRec's forward re-run from the
        hypergraph block on cge' (noise: injected Gumbel draws, z0: injected start noise)."""
        self._mixing, self._z0 = self.rf_warm(), z0
        try:
            return super().forward_embeddings(noise)
        finally:
            self._mixing, self._z0 = False, None
