"""Generate tests/golden/rfbm3_tiny{,_param,_grad,_step}.npz by running the reference RFBM3 (models/rfbm3.py,
models/rf_modules.py) on CPU, on the data and under the seed of bm3_tiny.npz (U = 37, I = 41, B = 16; case A of
make_golden_bm3.py: n_layers 1, dropout 0.3).  The BM3 parameters are asserted equal to bm3_tiny.npz's.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  Record "A_": both modalities (C = 128), rf_n_layers = 2, through RFBM3.calculate_loss / full_sort_predict
(before and after warm-up).  Record "B_": the text condition and the text prior alone (C = 64), rf_n_layers = 1,
through the generator with user_prior.  Both: rf_dropout 0, rf_sampling_steps 3, 7 negatives per row, with the draws
recorded (X0, t, the negatives after the collision rule, the eval z0).

The RNG order of RFBM3.calculate_loss is: forward() -> compute_loss_and_step (X0, t, item negatives, user negatives)
-> generate() (its z0, the result is discarded) -> the four dropout masks (u, i, t, v).  The draws are captured by
replaying the generator in that order; the replay is asserted: the generator's losses from the captured draws
(the restatement of tests/rfbm3_fixture.py) and BM3's loss from the captured masks equal the reference's.

The fp32-vs-fp64 spread of the sampler output and of the velocity gradients (the restatement run in both precisions on
the same inputs) is stored as A_err_sample / A_err_grad (and B_): the GPU tests allow 4x that.

Usage:  python tests/golden/make_golden_rfbm3.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_freedom import Cfg, MockLoader, OUT, _import_reference  # noqa: E402
from make_golden_bm3 import CASES, PARAMS  # noqa: E402
from make_golden_rffreedom import N_NEG, STEPS, record  # noqa: E402
import rf_fixture as R  # noqa: E402
import rfbm3_fixture as RB  # noqa: E402

LR = 0.001


def finish(torch, gen, out, tag, X1, cond, prior, users, pos, U, n_layers, X0, t, ni, nu, seen, loss_dict):
    """Store one compute_loss_and_step: inputs, draws, v, pred, losses, gradients, stepped parameters; assert the
    replay; measure the fp32 spread; then one generate() with a recorded z0 on the stepped parameters."""
    net = gen.velocity_net
    out[tag + "X1"], out[tag + "X0"], out[tag + "t"] = X1.numpy(), X0.numpy(), t.numpy()
    out[tag + "cond"], out[tag + "prior"] = cond.numpy(), prior.numpy()
    out[tag + "users"], out[tag + "pos"] = users, pos
    out[tag + "neg_items"], out[tag + "neg_users"] = ni, nu
    v = seen["v"]
    out[tag + "v"] = v.numpy()
    out[tag + "pred"] = ((t * X1 + (1 - t) * X0) + (1 - t) * v).numpy()
    out[tag + "rf_loss"] = np.float32(loss_dict["rf_loss"])
    out[tag + "cl_loss"] = np.float32(loss_dict["cl_loss"])
    for n, p in net.named_parameters():
        out[tag + "g_" + R.key(n)] = p.grad.numpy().copy()
        out[tag + "p1_" + R.key(n)] = p.detach().numpy().copy()
    res = {}
    for dt in (torch.float32, torch.float64):
        P = {n: torch.tensor(out[tag + "p0_" + R.key(n)], dtype=dt, requires_grad=True) for n in R.param_names(n_layers)}
        r = RB.train_losses(P, X1.to(dt), X0.to(dt), t.to(dt), cond.to(dt), prior.to(dt), torch.as_tensor(users),
                            torch.as_tensor(pos), torch.as_tensor(ni), torch.as_tensor(nu), U, n_layers)
        res[dt] = (r, R.grads_of(P, r["total"]))
    r32, _ = res[torch.float32]
    _, g64 = res[torch.float64]
    assert abs(r32["rf_loss"].item() - loss_dict["rf_loss"]) <= 1e-5 * abs(loss_dict["rf_loss"]), "draws out of step"
    assert abs(r32["cl_loss"].item() - loss_dict["cl_loss"]) <= 1e-5 * abs(loss_dict["cl_loss"]), "draws out of step"
    assert float((r32["v"].detach() - v).abs().max()) <= 1e-5, "the prior term is out of step"
    err = max(R.rel_to_max(out[tag + "g_" + R.key(n)], g64[n].detach().numpy()) for n in g64)
    out[tag + "err_grad"] = np.float64(err)
    torch.manual_seed(23)
    z0 = torch.randn(X1.shape[0], 64)
    with torch.no_grad():
        net.eval()
        z = gen.generate([cond], n_steps=STEPS, start_noise=z0)
        net.train()
        P1 = {n: torch.tensor(out[tag + "p1_" + R.key(n)], dtype=torch.float64) for n in R.param_names(n_layers)}
        z64 = R.generate(P1, cond.double(), z0.double(), STEPS, n_layers)
    out[tag + "z0"], out[tag + "gen"] = z0.numpy(), z.numpy()
    out[tag + "err_sample"] = np.float64(np.abs(z.numpy().astype(np.float64) - z64.numpy()).max())
    return z0


def gen_rfbm3(tmp):
    import scipy.sparse as sp
    import torch
    import torch.nn.functional as F
    sp.dok_matrix._update = lambda self, d: self._dict.update(d)  # removed from scipy; bm3.py:67 calls it
    _import_reference()
    import models.bm3 as bm3
    import models.rf_modules as rfm
    import models.rfbm3 as rfbm3

    f = dict(np.load(os.path.join(OUT, "bm3_tiny.npz")))
    U, I, B = int(f["U"]), int(f["I"]), 16
    N = U + I
    rows, cols, users, pos = f["train_rows"], f["train_cols"], f["users"], f["items"]
    os.makedirs(os.path.join(tmp, "tf"), exist_ok=True)
    np.save(os.path.join(tmp, "tf", "image_feat.npy"), f["v_feat"])
    np.save(os.path.join(tmp, "tf", "text_feat.npy"), f["t_feat"])
    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset="tf",
              vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64,
              feat_embed_dim=64, reg_weight=0.1, cl_weight=2.0, use_rf=True, use_denoise=False, use_2rf=False,
              rf_hidden_dim=128, rf_n_layers=2, rf_dropout=0.0, rf_learning_rate=LR, rf_sampling_steps=STEPS,
              rf_warmup_epochs=0, rf_mix_ratio=0.1, rf_inference_mix_ratio=0.2, rf_contrast_temp=0.2,
              rf_loss_weight=1.0, use_gradient_checkpointing=False, **CASES["A"])
    torch.manual_seed(3)
    m = rfbm3.RFBM3(cfg, MockLoader(U, I, rows, cols))
    params = dict(m.named_parameters())
    assert list(params) == PARAMS and not hasattr(m, "R")
    for n in PARAMS:
        assert np.array_equal(params[n].detach().numpy(), f["p_" + n.replace(".", "_")]), n  # bm3_tiny's parameters
    m.pre_epoch_processing()  # the RF epoch counter becomes 0
    gen = m.rf_generator
    gen.infonce_negative_samples = N_NEG
    out = {"U": np.int64(U), "I": np.int64(I), "n_neg": np.int64(N_NEG), "steps": np.int64(STEPS), "lr": np.float64(LR)}

    # ---- record A through RFBM3.calculate_loss
    m.train()
    with torch.no_grad():
        vf, tf_ = m.image_trs(m.image_embedding.weight), m.text_trs(m.text_embedding.weight)
        zu = torch.zeros(U, 64)
        conds = [torch.cat([zu, vf]), torch.cat([zu, tf_])]
    cap = {}
    step = gen.compute_loss_and_step

    def spy(**kw):
        cap["X1"] = kw["target_embeds"].detach().clone()
        cap["cond"] = torch.cat([c.detach() for c in kw["conditions"]], dim=-1)
        cap["prior"] = kw["user_prior"].detach().clone()
        cap["loss"] = step(**kw)
        return cap["loss"]

    gen.compute_loss_and_step = spy
    # the net is created (and its init drawn) before the draws, which need X1's shape only
    seed, X0, t, ni, nu, seen, hook = record(torch, gen, out, "A_", torch.zeros(N, 64), conds, users, pos, U, I, 2)
    # the same stream once more: past the RF step's draws and generate()'s z0, the four dropout masks
    torch.manual_seed(seed)
    torch.randn(N, 64), torch.rand(N, 1), torch.randint(0, I, (B, N_NEG)), torch.randint(0, U, (B, N_NEG))
    torch.randn(N, 64)
    p = m.dropout
    keep = [(F.dropout(torch.ones(n, 64), p) != 0) for n in (U, I, I, I)]
    for name, k in zip("uitv", keep):
        out["A_keep_" + name] = k.numpy().astype(np.uint8)
    m.zero_grad()
    torch.manual_seed(seed)
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos)])
    loss = m.calculate_loss(inter)
    loss.backward()
    hook.remove()
    gen.compute_loss_and_step = step
    assert torch.equal(cap["cond"], torch.cat(conds, dim=-1)), "conditions: image then text, zero user rows"
    assert not cap["prior"][:U].any(), "the user half of the prior is zero"
    zi = torch.zeros(I, 64) + vf + tf_
    assert torch.equal(cap["prior"][U:], zi - zi.mean(dim=0, keepdim=True)), "item prior: Z_i - mean_items(Z_i)"
    out["A_prior_colmean"] = np.float64(np.abs(cap["prior"][U:].mean(0).numpy()).max())

    # BM3's loss from the captured masks (make_golden_bm3.py's replay), on BM3's own forward: no second RF step
    with torch.no_grad():
        cos = F.cosine_similarity
        sc = 1.0 / (1.0 - p)
        ua, ib = bm3.BM3.forward(m)
        us, it = inter[0], inter[1]
        kf = [k.float() for k in keep]
        tu, ti = (ua * kf[0] * sc)[us], (ib * kf[1] * sc)[it]
        tt, tvv = (tf_ * kf[2] * sc)[it], (vf * kf[3] * sc)[it]
        pu, pi, pt, pv = (m.predictor(x) for x in (ua, ib, tf_, vf))
        terms = [1 - cos(pu[us], ti, dim=-1).mean(), 1 - cos(pi[it], tu, dim=-1).mean(),
                 1 - cos(pt[it], ti, dim=-1).mean(), 1 - cos(pv[it], ti, dim=-1).mean(),
                 1 - cos(pt[it], tt, dim=-1).mean(), 1 - cos(pv[it], tvv, dim=-1).mean()]
        reg = m.reg_loss(ua, ib)
        again = (terms[0] + terms[1]).mean() + m.reg_weight * reg + m.cl_weight * (terms[2] + terms[3] + terms[4] +
                                                                                  terms[5]).mean()
    assert float((again - loss.detach()).abs().max()) == 0.0, (float(again), float(loss.detach()))
    x1_again = torch.cat([ua, ib - m.item_id_embedding.weight.detach()])
    assert float((cap["X1"] - x1_again).abs().max()) < 1e-6, "X1: the layer mean without the item residual"
    out["A_loss"] = np.float32(loss.item())
    out["A_loss_terms"] = np.asarray([x.item() for x in terms], np.float32)  # ui, iu, t, v, tv, vt
    out["A_reg"] = np.float32(reg.item())
    for n in PARAMS:
        out["A_g_" + n.replace(".", "_")] = params[n].grad.numpy().copy()
    finish(torch, gen, out, "A_", cap["X1"], cap["cond"], cap["prior"], users, pos, U, 2, X0, t, ni, nu, seen,
           cap["loss"])
    out["A_seed"] = np.int64(seed)

    # evaluation before and after warm-up (the velocity parameters are the stepped ones, p1)
    m.eval()
    with torch.no_grad():
        gen.warmup_epochs = 5
        out["A_scores_pre"] = m.full_sort_predict([torch.arange(U)]).numpy()
        gen.warmup_epochs = 0
        torch.manual_seed(23)  # generate() draws z0 first: A_z0
        out["A_scores_mix"] = m.full_sort_predict([torch.arange(U)]).numpy()
        torch.manual_seed(23)
        eu, ei, _ = m.forward()
        out["A_eval_u"], out["A_eval_i"] = eu.numpy().copy(), ei.numpy().copy()
    np.testing.assert_allclose(out["A_scores_pre"], f["A_scores"], rtol=1e-6, atol=1e-7)  # before warm-up: BM3's
    assert np.array_equal(out["A_eval_i"], ib.numpy()), "the item rows are never mixed (rfbm3.py:233)"
    assert np.abs(out["A_eval_u"] - ua.numpy()).max() > 1e-2
    assert np.abs(out["A_scores_mix"] - out["A_scores_pre"]).max() > 1e-3
    np.testing.assert_allclose(out["A_eval_u"], ua.numpy() + 0.2 * out["A_gen"][:U], rtol=0, atol=1e-6)

    # ---- record B: the text condition and the text prior alone, one residual block, through the generator
    g2 = rfm.RFEmbeddingGenerator(embedding_dim=64, hidden_dim=128, n_layers=1, dropout=0.0, learning_rate=LR,
                                  sampling_steps=STEPS, warmup_epochs=0, contrast_temp=0.2, contrast_weight=1.0,
                                  n_users=U, n_items=I, use_2rf=False, use_gradient_checkpointing=False)
    g2.infonce_negative_samples = N_NEG
    zi = torch.zeros(I, 64) + tf_
    prior_b = torch.cat([zu - zu.mean(dim=0, keepdim=True), zi - zi.mean(dim=0, keepdim=True)])
    seed, X0, t, ni, nu, seen, hook = record(torch, g2, out, "B_", cap["X1"], conds[1:], users, pos, U, I, 1)
    ld = g2.compute_loss_and_step(target_embeds=cap["X1"], conditions=conds[1:], user_prior=prior_b,
                                  batch_users=torch.as_tensor(users), batch_pos_items=torch.as_tensor(pos))
    hook.remove()
    finish(torch, g2, out, "B_", cap["X1"], conds[1], prior_b, users, pos, U, 1, X0, t, ni, nu, seen, ld)
    out["B_seed"] = np.int64(seed)
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_rfbm3(tmp)
    # four files, each under the size limit of a committed file, split as make_golden_rffreedom.py splits: the
    # velocity parameters, their gradients and the stepped parameters are ~0.8 MB each
    bm3_grads = {"A_g_" + n.replace(".", "_") for n in PARAMS}
    parts = {"rfbm3_tiny_param": {k: v for k, v in out.items() if k[2:5] == "p0_"},
             "rfbm3_tiny_grad": {k: v for k, v in out.items() if k[2:4] == "g_" and k not in bm3_grads},
             "rfbm3_tiny_step": {k: v for k, v in out.items() if k[2:5] == "p1_"}}
    parts["rfbm3_tiny"] = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    for name, d in parts.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20) * 9 // 10, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    for tag in ("A_", "B_"):
        print(tag, "rf", out[tag + "rf_loss"], "cl", out[tag + "cl_loss"], "err_grad", out[tag + "err_grad"],
              "err_sample", out[tag + "err_sample"])
    print("A loss", out["A_loss"], "prior max", np.abs(out["A_prior"]).max(), "col mean", out["A_prior_colmean"])


if __name__ == "__main__":
    main()
