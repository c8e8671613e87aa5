"""RFGRCN on MI355X — drop-in for models/rfgrcn.py of the reference: GRCN with the rectified-flow embedding generator
(gmr/rf.py) trained on its concatenated table.

GRCN fuses by concatenation, so this is the one RF model whose generated rows are not 64 wide: the generator's
embedding_dim is embedding_size + latent_embedding * modalities = GRCN's width, 192 with image and text and 128 with
image features alone, and so is its condition_dim.  The generator runs at that width on the gmr_rf_*_w entry points
(csrc/rf.hip).  With result = [id_rep | rep_v | rep_t] (N x width) as in gmr/grcn.py:

  training    GRCN's step unchanged (mix_embeddings(training=True) returns the original table, rf_modules.py:1066-1072,
              and everything handed to the generator is detached), then one RFGenerator.train_step on that step's
              table (rfgrcn.py:141-201):
                X1    = result (use_denoise is off, so rf_target = representation.detach(), :153)
                cond  = [id_rep, rep_v, rep_t] (:156-167), which concatenated is result again: X1 and cond are the one
                        buffer self.result, no copy
                prior = every 64-wide block minus its own segment's column mean, user rows against the users' mean and
                        item rows against the items' (:171-190), which is result minus its segment column means over
                        the whole row: one launch (gmr_rf_center_segments, csrc/rf_prior.hip) into _prior, added to the
                        velocity as (1 - t)^2 0.2 prior
              GRCN's backward (block_backward / step_backward in gmr/grcn.py) reads the rows the forward saved (P, F,
              alpha, x, x1) and G, and writes the gradient tables and the slab's gradient twin alone; it never writes
              self.result, so the table is as _forward wrote it when the RF step reads it after GRCN's step, and GRCN's
              loss and eight gradients are the GRCN class's bit for bit.  The reference also runs its sampler in the
              training forward and discards the result (:212-220); it is not run here.
  evaluation  config key rf_eval:
                cached (default, the reference as written)  full_sort_predict (:294-305) reads self.result, which
                  GRCN's constructor sets to a random table, so it is never None and forward() is never called in
                  evaluation: the scores are the last training forward's unmixed table (the init table before any
                  step), and the generator never reaches the reference's evaluation, whatever the warm-up state.
                  forward_embeddings is GRCN's, bit for bit.
                mixed (not a reference setting)  what the reference's forward() computes in eval mode (:223-241) if it
                  is called: _forward() re-run with the current parameters and, once rf_warm(), result +
                  rf_inference_mix_ratio * generate(result) over all N rows in one launch (gmr_rf_sample_mix_w with
                  cond = base = result) into a table of its own, _mix.  Before warm-up the recomputed result.

Draws: GRCN draws nothing (edge dropout 0); the generator's are Philox streams keyed on (seed, RF step counter, site).
The start noise of a mixed evaluation is drawn once per forward_embeddings call and may be injected (z0).

use_rf: False is GRCN and allocates no generator.  use_denoise / use_2rf: True and rf_hidden_dim != 128 raise
NotImplementedError, an rf_eval other than cached / mixed a ValueError that names the key.  A world size above 1
raises, as GRCN does.
"""
import torch

from . import _lib
from . import rf
from .grcn import GRCN
from .kernels import ptr, stream
from .rf import RFBackbone

RF_EVAL = ("cached", "mixed")


def check_config(config):
    """rf_eval, after raising for the RF settings this package does not run (rf.check_config) and for an unknown
    rf_eval: a ValueError that names the key."""
    rf.check_config(config)
    mode = str(rf._get(config, "rf_eval", "cached"))
    if mode not in RF_EVAL:
        raise ValueError(f"rf_eval = {mode}: 'cached' (the last training forward's table, as the reference's "
                         f"full_sort_predict reads it) or 'mixed' (recomputed and mixed with the generated rows)")
    return mode


class RFGRCN(RFBackbone, GRCN):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        self.rf_eval = "cached"
        if not self.use_rf:
            return
        self.rf_eval = check_config(config)
        N, W = self.N, self.width
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)  # noqa: E731
        self._prior = f(N, W)
        self._mix = f(N, W) if self.rf_eval == "mixed" else None
        self._pws = f(int(_lib.load().gmr_rf_center_segments_ws_floats(self.n_users, self.n_items, W)))

    def rf_condition_dim(self):
        return self.width  # [id_rep | rep_v | rep_t]

    def rf_embedding_dim(self):
        return self.width  # the generated rows are as wide as the concatenated table

    def rf_step_inputs(self):
        """X1 = cond = self.result, the table of the last _forward itself (GRCN's backward never writes it), and the
        N x width prior: result minus its segment's column means."""
        res, W = self.result, self.width
        _lib.call("gmr_rf_center_segments", self.n_users, self.n_items, W, ptr(res), res.stride(0), ptr(self._prior),
                  self._prior.stride(0), ptr(self._pws), stream())
        return res, res, self._prior

    @torch.no_grad()
    def forward_embeddings(self, z0=None):
        """full_sort_predict's tables.  rf_eval 'cached': GRCN's (the table the last forward wrote).  'mixed': the
        table recomputed from the current parameters and, once rf_warm(), result + rf_inference_mix_ratio *
        generate(result) in _mix (z0: injected start noise)."""
        if not self.use_rf or self.rf_eval == "cached":
            return super().forward_embeddings()
        U = self.n_users
        self._forward()
        if not self.rf_warm():
            return self.result[:U], self.result[U:]
        self.rf_generator.generate(self.result, z0=z0, out=self._mix, base=self.result)
        return self._mix[:U], self._mix[U:]
