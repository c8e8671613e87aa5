"""RFMGCN on MI355X — drop-in for models/rfmgcn.py of the reference: MGCN with the rectified-flow embedding generator
(gmr/rf.py) trained next to it and mixed into every row of the evaluation table.

MGCN carries both modal views to the users over R, so (unlike RFFREEDOM and RFBM3, whose user conditions are zero) the
RF inputs are dense over all N = U + I rows.  With a, b, c, side and all = c + side as in gmr/mgcn.py:

  training    MGCN's step unchanged (the reference mixes nothing in training, rf_modules.py:1070-1072), then one
              RFGenerator.train_step on that step's tables, all detached in the reference (rfmgcn.py:129-204):
                X1    = all (use_denoise is off, so rf_target = all_embeds.detach())
                cond  = [a | b], N x 128, the image view then the text view: the table ab itself, no copy
                prior = [Z_u - mean_users(Z_u); Z_i - mean_items(Z_i)], Z = (a + b) / 2 (:156-172), one entry point
                        (gmr_rf_view_prior, csrc/rfmgcn.hip), added to the velocity as (1 - t)^2 0.2 prior
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
from .kernels import ptr, stream
from .mgcn import MGCN
from .rf import D, RFGenerator, check_config

C = 2 * D  # the condition width: both modal views


def _get(config, key, default):
    return config[key] if key in config and config[key] is not None else default


class RFMGCN(MGCN):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        self.use_rf = bool(_get(config, "use_rf", True))
        self.rf_generator = None
        if not self.use_rf:
            return
        check_config(config)
        c = config
        self.seed = int((c["seed"][0] if isinstance(c["seed"], (list, tuple)) else c["seed"]) or 0)
        self.rf_generator = RFGenerator(
            self.n_users, self.n_items, C, self.device, n_layers=_get(config, "rf_n_layers", 2),
            dropout=_get(config, "rf_dropout", 0.1), learning_rate=_get(config, "rf_learning_rate", 0.0001),
            sampling_steps=_get(config, "rf_sampling_steps", 10), warmup_epochs=_get(config, "rf_warmup_epochs", 5),
            inference_mix_ratio=_get(config, "rf_inference_mix_ratio", 0.2),
            contrast_temp=_get(config, "rf_contrast_temp", 0.2), contrast_weight=_get(config, "rf_loss_weight", 1.0),
            n_negatives=_get(config, "rf_infonce_negatives", 1024), seed=self.seed)
        g = self.rf_generator
        assert g.slab.numel == int(_lib.load().gmr_rf_param_floats(C, g.L)), "the velocity slab is the kernels' layout"
        self._training_epoch = -1  # incremented to 0 by the first pre_epoch_processing
        N = self.N
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._prior, self._gen, self._mix = f(N, D), f(N, D), f(N, D)
        self._pws = f(int(_lib.load().gmr_rf_view_prior_ws_floats(self.n_users, self.n_items)))

    # ------------------------------------------------------------------ state
    def extra_state(self):
        """MGCN has no state of its own outside the slab; the RF counters are all there is."""
        if not self.use_rf:
            return {}
        return {"rf_epoch": int(self._training_epoch), "rf_step": int(self.rf_generator.step_ctr)}

    def load_extra_state(self, st):
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
    def rf_prior(self):
        """The N x 64 prior from the two views of the last _forward (the column blocks of ab)."""
        ab = self.ab
        _lib.call("gmr_rf_view_prior", self.n_users, self.n_items, ptr(ab), ab.stride(0), ptr(ab[:, D:]), ab.stride(0),
                  ptr(self._prior), self._prior.stride(0), ptr(self._pws), stream())
        return self._prior

    # ------------------------------------------------------------------ training
    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, rf_draws=None):
        """MGCN's step, then the RF step on the tables of that step: X1 = all, cond = ab, the prior from ab.  The
        reference detaches all three, so nothing flows back; MGCN's step_backward reads ab and writes neither ab nor
        all, so both are intact here.  rf_draws: injected draws for RFGenerator.train_step.  rf_loss_terms() reads
        the RF losses."""
        loss = super().rec_step(users, pos, neg, plan_bpr, plan_cl, norm_rows, reg_share)
        if self.use_rf:
            self.rf_generator.train_step(self.all, self.ab, users, pos, prior=self.rf_prior(), **(rf_draws or {}))
        return loss

    def rf_loss_terms(self):
        """[rf_loss, cl_loss, total] of the last RF step (device tensor)."""
        return self.rf_generator._w["loss"]

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables: MGCN's, and from rf_warmup_epochs on all + rf_inference_mix_ratio *
        generate(ab) over all N rows, in a table of its own (z0: injected start noise)."""
        usr, itm = super().forward_embeddings()
        if not self.use_rf or not self.rf_generator.warmed_up():
            return usr, itm
        g, U = self.rf_generator, self.n_users
        g.generate(self.ab, z0=z0, out=self._gen)
        self._copy64(self.all, self._mix)
        _lib.call("gmr_axpy_dev_f32", self.N * D, ptr(g._ratio), ptr(self._gen), ptr(self._mix), stream())
        return self._mix[:U], self._mix[U:]

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
