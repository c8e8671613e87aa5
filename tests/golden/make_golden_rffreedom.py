"""Generate tests/golden/rffreedom_tiny{,_param,_grad,_step}.npz by running the reference RFFREEDOM (models/rffreedom.py,
models/rf_modules.py) on CPU, on the data of freedom_tiny.npz (case A: U = 37, I = 41, B = 16, its pruned graph).

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  Record "A_": both modalities (C = 128), rf_n_layers = 2, through RFFREEDOM.calculate_loss /
full_sort_predict.  Record "B_": the text condition alone (C = 64), rf_n_layers = 1, through the generator.
Both: rf_dropout 0, rf_sampling_steps 3, rf_warmup_epochs 0, 7 negatives per row, with the draws recorded
(X0, t, the negatives after the collision rule, the eval z0).

The fp32-vs-fp64 spread of the sampler output and of the velocity gradients (tests/rf_fixture.py run in both
precisions on the same inputs) is stored as A_err_sample / A_err_grad (and B_): the GPU tests allow 4x that.

Usage:  python tests/golden/make_golden_rffreedom.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import Cfg, MockLoader, OUT, _import_reference  # noqa: E402
import rf_fixture as R  # noqa: E402

N_NEG, STEPS = 7, 3


def _draws(torch, seed, N, U, I, B):
    torch.manual_seed(seed)
    X0 = torch.randn(N, 64)
    t = torch.rand(N, 1)
    ni = torch.randint(0, I, (B, N_NEG))
    nu = torch.randint(0, U, (B, N_NEG))
    return X0, t, ni.numpy(), nu.numpy()


def _pick_seed(torch, N, U, I, B, users, pos):
    """The first seed whose raw negatives hit a positive in some row and repeat within some row."""
    for seed in range(100, 400):
        _, _, ni, nu = _draws(torch, seed, N, U, I, B)
        hit = (ni == pos[:, None]).any() and (nu == users[:, None]).any()
        dup = any(len(set(r.tolist())) < N_NEG for r in R.collide(ni, pos, I))
        if hit and dup:
            return seed
    raise AssertionError("no seed with a drawn positive and a duplicate negative")


def record(torch, gen, out, tag, X1, conds, users, pos, U, I, n_layers):
    """One compute_loss_and_step and one generate of the reference generator with recorded draws."""
    N, B = X1.shape[0], len(users)
    cond = torch.cat(conds, dim=-1)
    torch.manual_seed(5)
    gen._init_velocity_net(cond.shape[-1], torch.device("cpu"))
    net = gen.velocity_net
    names = [n for n, _ in net.named_parameters()]
    assert names == R.param_names(n_layers), names
    for n, p in net.named_parameters():
        out[tag + "p0_" + R.key(n)] = p.detach().numpy().copy()
    seed = _pick_seed(torch, N, U, I, B, users, pos)
    X0, t, ni, nu = _draws(torch, seed, N, U, I, B)
    assert (ni == pos[:, None]).any() and (nu == users[:, None]).any(), "a row must have drawn its positive"
    ni, nu = R.collide(ni, pos, I), R.collide(nu, users, U)
    assert any(len(set(r.tolist())) < N_NEG for r in ni), "a row must hold a duplicate negative"
    seen = {}

    def keep_first(mod, args, o):  # returns None: a hook's return value would replace the output
        seen.setdefault("v", o.detach().clone())

    h = net.register_forward_hook(keep_first)
    torch.manual_seed(seed)
    return seed, X0, t, ni, nu, seen, h


def finish(torch, gen, out, tag, X1, cond, users, pos, U, I, n_layers, X0, t, ni, nu, seen, loss_dict):
    net = gen.velocity_net
    out[tag + "X1"], out[tag + "X0"], out[tag + "t"] = X1.numpy(), X0.numpy(), t.numpy()
    out[tag + "cond"] = cond.numpy()
    out[tag + "users"], out[tag + "pos"] = users, pos
    out[tag + "neg_items"], out[tag + "neg_users"] = ni, nu
    out[tag + "v"] = seen["v"].numpy()
    out[tag + "rf_loss"] = np.float32(loss_dict["rf_loss"])
    out[tag + "cl_loss"] = np.float32(loss_dict["cl_loss"])
    for n, p in net.named_parameters():
        out[tag + "g_" + R.key(n)] = p.grad.numpy().copy()
        out[tag + "p1_" + R.key(n)] = p.detach().numpy().copy()
    # the restatement on the same inputs: it must see the reference's draws (else the record is wrong), and its
    # fp64 run measures the fp32 spread
    res = {}
    for dt in (torch.float32, torch.float64):
        P = {n: torch.tensor(out[tag + "p0_" + R.key(n)], dtype=dt, requires_grad=True) for n in R.param_names(n_layers)}
        r = R.train_losses(P, X1.to(dt), X0.to(dt), t.to(dt), cond.to(dt), torch.as_tensor(users), torch.as_tensor(pos),
                           torch.as_tensor(ni), torch.as_tensor(nu), U, n_layers)
        res[dt] = (r, R.grads_of(P, r["total"]))
    r32, g32 = res[torch.float32]
    r64, g64 = res[torch.float64]
    assert abs(r32["rf_loss"].item() - loss_dict["rf_loss"]) <= 1e-5 * abs(loss_dict["rf_loss"]), "draws out of step"
    assert abs(r32["cl_loss"].item() - loss_dict["cl_loss"]) <= 1e-5 * abs(loss_dict["cl_loss"]), "draws out of step"
    err = max(R.rel_to_max(out[tag + "g_" + R.key(n)], g64[n].detach().numpy()) for n in g64)
    out[tag + "err_grad"] = np.float64(err)
    # generate with a recorded z0 on the stepped parameters
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


def gen_rffreedom(tmp):
    import scipy.sparse as sp
    import torch
    sp.dok_matrix._update = lambda self, d: self._dict.update(d)  # removed from scipy; freedom.py:111 calls it
    _import_reference()
    import models.rf_modules as rfm
    import models.rffreedom as rff

    f = dict(np.load(os.path.join(OUT, "freedom_tiny.npz")))
    U, I, B, k = int(f["U"]), int(f["I"]), 16, 5
    N = U + I
    rows, cols, users, pos, neg = f["train_rows"], f["train_cols"], f["users"], f["pos"], f["neg"]
    os.makedirs(os.path.join(tmp, "tf"), exist_ok=True)
    np.save(os.path.join(tmp, "tf", "image_feat.npy"), f["v_feat"])
    np.save(os.path.join(tmp, "tf", "text_feat.npy"), f["t_feat"])
    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset="tf",
              vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64,
              feat_embed_dim=64, knn_k=k, lambda_coeff=0.9, cf_model="lightgcn", mm_image_weight=0.1, degree_ratio=1.0,
              reg_weight=0.001, n_mm_layers=1, n_ui_layers=2, dropout=0.8, use_rf=True, use_denoise=False,
              use_2rf=False, rf_hidden_dim=128, rf_n_layers=2, rf_dropout=0.0, rf_learning_rate=0.001,
              rf_sampling_steps=STEPS, rf_warmup_epochs=0, rf_mix_ratio=0.1, rf_inference_mix_ratio=0.2,
              rf_contrast_temp=0.2, rf_loss_weight=1.0, use_gradient_checkpointing=False)
    torch.manual_seed(3)
    m = rff.RFFREEDOM(cfg, MockLoader(U, I, rows, cols))
    for n, p in m.named_parameters():
        assert np.array_equal(p.detach().numpy(), f["p_" + n.replace(".", "_")]), n  # freedom_tiny's parameters
    torch.manual_seed(17)
    m.pre_epoch_processing()  # freedom_tiny's pruned graph (degree_idx); the RF epoch counter becomes 0
    gen = m.rf_generator
    gen.infonce_negative_samples = N_NEG
    out = {"n_neg": np.int64(N_NEG), "steps": np.int64(STEPS), "lr": np.float64(0.001)}

    # ---- record A through RFFREEDOM.calculate_loss
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
        cap["loss"] = step(**kw)
        return cap["loss"]

    gen.compute_loss_and_step = spy
    # the draws need X1's shape only; the net is created (and its init drawn) before them
    seed, X0, t, ni, nu, seen, hook = record(torch, gen, out, "A_", torch.zeros(N, 64), conds, users, pos, U, I, 2)
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    loss = m.calculate_loss(inter)
    hook.remove()
    gen.compute_loss_and_step = step
    assert abs(loss.item() - float(f["A_loss"])) <= 1e-6 * abs(float(f["A_loss"])), "the main loss is FREEDOM's"
    assert torch.equal(cap["cond"], torch.cat(conds, dim=-1)), "conditions: image then text, zero user rows"
    z0 = finish(torch, gen, out, "A_", cap["X1"], cap["cond"], users, pos, U, I, 2, X0, t, ni, nu, seen, cap["loss"])
    out["A_seed"] = np.int64(seed)
    m.eval()
    with torch.no_grad():
        gen.warmup_epochs = 5
        out["A_scores_pre"] = m.full_sort_predict([torch.arange(U)]).numpy()
        gen.warmup_epochs = 0
        torch.manual_seed(23)  # generate() draws z0 first
        out["A_scores_mix"] = m.full_sort_predict([torch.arange(U)]).numpy()
    assert np.abs(out["A_scores_mix"] - out["A_scores_pre"]).max() > 1e-3

    # ---- record B: the text condition alone, one residual block, through the generator
    g2 = rfm.RFEmbeddingGenerator(embedding_dim=64, hidden_dim=128, n_layers=1, dropout=0.0, learning_rate=0.001,
                                  sampling_steps=STEPS, warmup_epochs=0, contrast_temp=0.2, contrast_weight=1.0,
                                  n_users=U, n_items=I, use_2rf=False, use_gradient_checkpointing=False)
    g2.infonce_negative_samples = N_NEG
    seed, X0, t, ni, nu, seen, hook = record(torch, g2, out, "B_", cap["X1"], conds[1:], users, pos, U, I, 1)
    ld = g2.compute_loss_and_step(target_embeds=cap["X1"], conditions=conds[1:], batch_users=torch.as_tensor(users),
                                  batch_pos_items=torch.as_tensor(pos))
    hook.remove()
    finish(torch, g2, out, "B_", cap["X1"], conds[1], users, pos, U, I, 1, X0, t, ni, nu, seen, ld)
    out["B_seed"] = np.int64(seed)
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_rffreedom(tmp)
    # four files, each under the 1 MiB limit of a committed file: the velocity parameters, their gradients and
    # the stepped parameters are ~0.8 MB each (random floats do not compress)
    parts = {"rffreedom_tiny_param": {k: v for k, v in out.items() if k[2:5] == "p0_"},
             "rffreedom_tiny_grad": {k: v for k, v in out.items() if k[2:4] == "g_"},
             "rffreedom_tiny_step": {k: v for k, v in out.items() if k[2:5] == "p1_"}}
    parts["rffreedom_tiny"] = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    for name, d in parts.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20) * 9 // 10, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    for tag in ("A_", "B_"):
        print(tag, "rf", out[tag + "rf_loss"], "cl", out[tag + "cl_loss"], "err_grad", out[tag + "err_grad"],
              "err_sample", out[tag + "err_sample"])


if __name__ == "__main__":
    main()
