"""Generate tests/golden/rflgmrec_tiny{,_param,_grad,_step}.npz by running the reference RFLGMRec (models/rflgmrec.py,
models/rf_modules.py) on CPU, on the data, under the seed and with case B of lgmrec_tiny{,_B}.npz (U = 37, I = 41,
B = 16, n_hyper_layer 2, hyper_num 5, keep_rate 0.5; the two embedding tables times 8 and the two hyperedge weights
times 2), first step, under the stand-in of make_golden_lgmrec.py (scipy's removed dok_matrix._update).

LGMRec's draws are replayed from lgmrec_tiny_B.npz: F.gumbel_softmax is replaced by softmax((x + g) / tau) with that
file's recorded g (B_g[0] in training, B_g_eval in evaluation), the module's dropout by one that multiplies by the
recorded keep masks B_keep[0] and 1 / keep_rate.  So LGMRec's part is LGMRec's: the reference's own LGMRec class is run
next to it under the same replays, and the fp32 loss, the six gradients and the scores before warm-up are asserted
equal to that class's bit for bit.  Against lgmrec_tiny_B.npz the fp32 loss is asserted within one fp32 rounding (it
is bit-equal where torch's CPU kernels are those of that file's run; rerunning make_golden_lgmrec.py itself elsewhere
moved B_loss32 by one unit in the last place, 1.9021541 against the stored 1.9021542, the fp64 loss 1.90215415 lying
between the two: B_loss32_bits_equal records which it was), the six gradients against the file's fp64 gradients at the
bar of tests/lgmrec_fixture.py (rtol 1e-5, atol twice the stored fp32 distance), the scores before warm-up against the
file's at its score bar.  None of it is stored again.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  One record, "B_": the two propagated modal views as conditions (C = 128), rf_n_layers = 2, rf_dropout 0,
rf_sampling_steps 3, 7 negatives per row, rf_learning_rate 1e-3, no gradient checkpointing, through
RFLGMRec.calculate_loss / full_sort_predict (before and after warm-up), with the draws recorded (X0, t, the negatives
after the collision rule, the eval z0).

The RNG order of RFLGMRec.calculate_loss is: the four Gumbel draws (iv, uv, it, ut) -> compute_loss_and_step (X0, t,
item negatives, user negatives) -> generate() (its z0, the result is discarded: mix_embeddings(training=True) returns
the original cge) -> LGMRec's four dropout masks.  The replayed Gumbel draws and masks draw nothing, so the stream the
RF step sees starts at its own first draw, which is what make_golden_rffreedom.record replays; the replay is asserted:
the generator's losses from the captured draws (the restatement of tests/rfbm3_fixture.py) equal the reference's.

Stored next to the record, the evaluation: before warm-up LGMRec's table (B_all_pre) and scores; after warm-up, from
the recorded z0 and Gumbel draws, cge (B_cge_eval), the conditions (B_cond_eval), the sampler's rows (B_gen_eval), the
mixed collaborative view cge' (B_cgemix_eval), and the final table and scores (B_eval, B_scores_mix), which are
LGMRec's forward from the hypergraph block on cge', not B_all_pre + ratio * B_gen_eval (asserted).

Usage:  python tests/golden/make_golden_rflgmrec.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import Cfg, MockLoader, OUT, _import_reference  # noqa: E402
from make_golden_lgmrec import rec_order  # noqa: E402
from make_golden_rffreedom import N_NEG, STEPS, record  # noqa: E402
from make_golden_rfbm3 import LR, finish  # noqa: E402
import lgmrec_fixture as F  # noqa: E402
import rf_fixture as R  # noqa: E402

RATIO = 0.2
N_PARAMS = 125760  # C = 128, two layers


def gen_rflgmrec():
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn
    import scipy.sparse as sp
    sp.dok_matrix._update = lambda self, d: self._dict.update(d)  # removed from scipy; lgmrec.py:76 calls it
    _import_reference()
    import models.lgmrec as lgmrec
    import models.rflgmrec as rflgmrec

    f = dict(np.load(os.path.join(OUT, "lgmrec_tiny.npz")))
    f.update(np.load(os.path.join(OUT, "lgmrec_tiny_B.npz")))
    U, I, B = int(f["U"]), int(f["I"]), 16
    N = U + I
    rows, cols, users, pos, neg = f["train_rows"], f["train_cols"], f["users"], f["pos"], f["neg"]
    cs = F.CASES["B"]
    replay = {"g": [], "i": 0}

    def replay_gumbel(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        gg = replay["g"][replay["i"] % 4]
        replay["i"] += 1
        assert gg.shape == logits.shape
        return ((logits + gg) / tau).softmax(dim)

    class Replay(nn.Module):
        """Dropout with the recorded masks of one forward (iv, uv, it, ut), nn.Dropout's arithmetic at p = 0.5 (the
        kept entries times 2, exact); the identity in evaluation."""

        def __init__(self, masks, keep_rate):
            super().__init__()
            self.masks, self.keep_rate, self.i = masks, keep_rate, 0

        def forward(self, x):
            if not self.training:
                return x
            k = torch.as_tensor(self.masks[self.i % 4]).to(x.dtype)
            self.i += 1
            return x * k * (1.0 / self.keep_rate)

    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=True, is_multimodal_model=True, embedding_size=64, feat_embed_dim=64,
              cf_model="lightgcn", n_ui_layers=F.N_UI_LAYERS, n_mm_layers=F.N_MM_LAYERS, alpha=F.ALPHA,
              cl_weight=F.CL_WEIGHT, reg_weight=F.REG_WEIGHT, use_rf=True, use_denoise=False, use_2rf=False,
              rf_hidden_dim=128, rf_n_layers=2, rf_dropout=0.0, rf_learning_rate=LR, rf_sampling_steps=STEPS,
              rf_warmup_epochs=0, rf_mix_ratio=0.1, rf_inference_mix_ratio=RATIO, rf_contrast_temp=0.2,
              rf_loss_weight=1.0, use_gradient_checkpointing=False, **cs)
    # end2end: the base class loads no feature file; the features are set before the constructor reads them
    base = lgmrec.GeneralRecommender.__init__

    def init(self, config, dataset):
        base(self, config, dataset)
        self.v_feat, self.t_feat = torch.as_tensor(f["v_feat"]), torch.as_tensor(f["t_feat"])

    lgmrec.GeneralRecommender.__init__ = init
    try:
        torch.manual_seed(3)
        m = rflgmrec.RFLGMRec(cfg, MockLoader(U, I, rows, cols))
        torch.manual_seed(3)
        plain = lgmrec.LGMRec(cfg, MockLoader(U, I, rows, cols))  # the reference's own LGMRec, same replays
    finally:
        lgmrec.GeneralRecommender.__init__ = base
    params = dict(m.named_parameters())
    assert list(params) == F.STATE_KEYS, "the velocity net is created lazily: LGMRec's parameters alone"
    names = {k: params[s] for k, s in zip(F.PARAMS, F.STATE_KEYS)}
    pnames = {k: dict(plain.named_parameters())[s] for k, s in zip(F.PARAMS, F.STATE_KEYS)}
    want = F.case_params(f, "B")
    with torch.no_grad():
        for k, q in names.items():
            assert np.array_equal(q.numpy(), f["B_init_" + k]), k  # lgmrec_tiny_B's init
            assert np.array_equal(pnames[k].numpy(), f["B_init_" + k]), k
            q.copy_(torch.as_tensor(want[k]))
            pnames[k].copy_(torch.as_tensor(want[k]))
    assert m.drop.p == 0.5
    m.drop = Replay(rec_order(f["B_keep"][0]), cs["keep_rate"])
    plain.drop = Replay(rec_order(f["B_keep"][0]), cs["keep_rate"])
    Fn.gumbel_softmax = replay_gumbel  # rflgmrec.F is torch.nn.functional
    m.pre_epoch_processing()  # the RF epoch counter becomes 0
    gen = m.rf_generator
    gen.infonce_negative_samples = N_NEG
    out = {"U": np.int64(U), "I": np.int64(I), "n_neg": np.int64(N_NEG), "steps": np.int64(STEPS), "lr": np.float64(LR),
           "ratio": np.float64(RATIO)}

    # ---- the RF inputs, which forward does not return: cge and the two propagated modal views
    m.train()
    with torch.no_grad():
        cge = m.cge()
        views = [m.mge("v"), m.mge("t")]
    cap = {}
    step = gen.compute_loss_and_step

    def spy(**kw):
        cap["X1"] = kw["target_embeds"].detach().clone()
        cap["cond"] = torch.cat([c.detach() for c in kw["conditions"]], dim=-1)
        cap["prior"] = kw["user_prior"].detach().clone()
        cap["loss"] = step(**kw)
        return cap["loss"]

    gen.compute_loss_and_step = spy
    # the net is created (and its init drawn) before the draws, which need the shapes only
    seed, X0, t, ni, nu, seen, hook = record(torch, gen, out, "B_", torch.zeros(N, 64), views, users, pos, U, I, 2)
    assert sum(q.numel() for q in gen.velocity_net.parameters()) == N_PARAMS
    m.zero_grad()
    replay["g"], replay["i"] = [torch.as_tensor(a) for a in rec_order(f["B_g"][0])], 0
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    loss = m.calculate_loss(inter)
    loss.backward()
    hook.remove()
    gen.compute_loss_and_step = step
    assert replay["i"] == 4 and m.drop.i == 4, "one forward: four Gumbel draws, four masks"
    # LGMRec's step is the reference LGMRec class's under the same replayed draws, bit for bit: the fp32 loss and the
    # six gradients.  Against lgmrec_tiny_B.npz: the fp32 loss within one fp32 rounding (bit for bit where the CPU
    # kernels are those of that file's run; its own maker rerun elsewhere may differ in the last bit, the fp64 loss
    # lying between the two), the gradients at the fixture's bar against the file's fp64 run
    plain.train()
    plain.zero_grad()
    replay["i"] = 0
    ploss = plain.calculate_loss(inter)
    ploss.backward()
    assert replay["i"] == 4 and plain.drop.i == 4
    assert loss.item() == ploss.item(), (loss.item(), ploss.item())
    for k in F.PARAMS:
        assert torch.equal(names[k].grad, pnames[k].grad), k
    l32, w32 = np.float32(loss.item()), np.float32(f["B_loss32"])
    assert abs(float(l32) - float(w32)) <= float(np.spacing(w32)), (loss.item(), f["B_loss32"])
    assert abs(loss.item() - float(f["B_loss"])) <= 1e-5 * float(f["B_loss"])
    out["B_loss32_bits_equal"] = np.bool_(l32 == w32)
    for k in F.PARAMS:
        g64 = f["B_g_" + k]
        err = np.abs(names[k].grad.numpy().astype(np.float64) - g64)
        assert (err <= 1e-5 * np.abs(g64) + 2 * float(f["B_own_" + k])).all(), (k, err.max(), f["B_own_" + k])
    # the RF inputs: X1 = cge; cond = [mge_v | mge_t], not normalised; prior = the two-segment centred mge_v + mge_t
    assert torch.equal(cap["X1"], cge), "X1 = cge"
    assert torch.equal(cap["cond"], torch.cat(views, dim=-1)), "conditions: the image view then the text view"
    nrm = cap["cond"][:, :64].norm(dim=1)
    assert float((nrm - 1).abs().min()) > 1e-3, "the views are not normalised"
    Z = 0 + views[0] + views[1]
    wantp = torch.cat([Z[:U] - Z[:U].mean(dim=0, keepdim=True), Z[U:] - Z[U:].mean(dim=0, keepdim=True)])
    assert torch.equal(cap["prior"], wantp), "prior: Z - its own segment's mean, Z the sum of the views"
    assert float((cap["prior"] - 0.5 * wantp).abs().max()) > 1e-3
    assert float(cap["prior"][:U].abs().max()) > 0 and float(cap["cond"][:U].abs().max()) > 0, "dense user rows"
    finish(torch, gen, out, "B_", cap["X1"], cap["cond"], cap["prior"], users, pos, U, 2, X0, t, ni, nu, seen,
           cap["loss"])
    out["B_seed"] = np.int64(seed)

    # ---- evaluation before and after warm-up (the velocity parameters are the stepped ones, p1): no dropout
    m.eval()
    g_eval = [torch.as_tensor(a) for a in rec_order(f["B_g_eval"])]
    sample, mix = gen.generate, gen.mix_embeddings

    def gspy(conditions, *a_, **kw):
        cap["cond_eval"] = torch.cat(conditions, dim=-1).clone()
        cap["gen_eval"] = sample(conditions, *a_, **kw)
        return cap["gen_eval"]

    def mspy(original_embeds, generated_embeds, *a_, **kw):
        cap["cge_eval"] = original_embeds.clone()
        cap["cgemix_eval"] = mix(original_embeds, generated_embeds, *a_, **kw)
        return cap["cgemix_eval"]

    with torch.no_grad():
        gen.warmup_epochs = 5
        replay["g"], replay["i"] = g_eval, 0
        out["B_scores_pre"] = m.full_sort_predict([torch.arange(U)]).numpy()
        ua, ia, _, _ = m.forward()
        out["B_all_pre"] = torch.cat([ua, ia]).numpy().copy()
        gen.warmup_epochs = 0
        torch.manual_seed(23)  # the Gumbel draws are replayed, so generate()'s z0 is the first draw: B_z0
        out["B_scores_mix"] = m.full_sort_predict([torch.arange(U)]).numpy()
        gen.generate, gen.mix_embeddings = gspy, mspy
        torch.manual_seed(23)
        eu, ei, _, _ = m.forward()
        gen.generate, gen.mix_embeddings = sample, mix
        out["B_eval"] = torch.cat([eu, ei]).numpy().copy()
        plain.eval()
        replay["i"] = 0
        pscores = plain.full_sort_predict([torch.arange(U)]).numpy()
    assert m.drop.i == 4, "no mask is drawn in evaluation"
    # before warm-up: the reference LGMRec class's scores bit for bit; lgmrec_tiny_B's at the fixture's score bar
    assert np.array_equal(out["B_scores_pre"], pscores), "before warm-up: LGMRec's scores"
    np.testing.assert_allclose(out["B_scores_pre"], f["B_scores"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(out["B_scores_pre"], f["B_scores32"], rtol=1e-5, atol=1e-4)
    for k in ("cge_eval", "cond_eval", "gen_eval", "cgemix_eval"):
        out["B_" + k] = cap[k].numpy().copy()
    assert np.array_equal(out["B_cge_eval"], cge.numpy()) and np.array_equal(out["B_cond_eval"], out["B_cond"])
    np.testing.assert_allclose(out["B_cgemix_eval"], out["B_cge_eval"] + RATIO * out["B_gen_eval"], rtol=0, atol=1e-6)
    # the restatement's sampler on the evaluation conditions from the recorded z0, within the stored spread's bar
    P1 = {n: torch.tensor(out["B_p1_" + R.key(n)], dtype=torch.float64) for n in R.param_names(2)}
    z64 = R.generate(P1, cap["cond_eval"].double(), torch.tensor(out["B_z0"]).double(), STEPS, 2)
    out["B_err_sample_eval"] = np.float64(np.abs(out["B_gen_eval"].astype(np.float64) - z64.numpy()).max())
    assert out["B_err_sample_eval"] <= 4 * out["B_err_sample"] + 1e-6, "the eval z0 is not the recorded one"
    # the final table is the forward from the hypergraph block on cge', not all + ratio * gen
    ev = out["B_eval"].astype(np.float64)
    np.testing.assert_allclose(ev[:U] @ ev[U:].T, out["B_scores_mix"], rtol=1e-5, atol=1e-4)
    late = out["B_all_pre"] + RATIO * out["B_gen_eval"]
    out["B_late_mix_gap"] = np.float64(np.abs(out["B_eval"] - late).max())
    assert out["B_late_mix_gap"] > 1e-3, out["B_late_mix_gap"]
    out["B_score_shift"] = np.float64(np.abs(out["B_scores_mix"] - out["B_scores_pre"]).max())
    return out


def main():
    out = gen_rflgmrec()
    # four files, each under the size limit of a committed file, split as make_golden_rfsmore.py splits: the
    # velocity parameters, their gradients and the stepped parameters are ~0.5 MB each
    parts = {"rflgmrec_tiny_param": {k: v for k, v in out.items() if k[2:5] == "p0_"},
             "rflgmrec_tiny_grad": {k: v for k, v in out.items() if k[2:4] == "g_"},
             "rflgmrec_tiny_step": {k: v for k, v in out.items() if k[2:5] == "p1_"}}
    parts["rflgmrec_tiny"] = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    for name, d in parts.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20) * 9 // 10, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    print("rf", out["B_rf_loss"], "cl", out["B_cl_loss"], "err_grad", out["B_err_grad"], "err_sample",
          out["B_err_sample"], "err_sample_eval", out["B_err_sample_eval"], "prior max", np.abs(out["B_prior"]).max(),
          "largest score", np.abs(out["B_scores_pre"]).max(), "shift by the mix", out["B_score_shift"],
          "gap to the late mix", out["B_late_mix_gap"])


if __name__ == "__main__":
    main()
