"""Generate tests/golden/rfmgcn_tiny{,_param,_grad,_step}.npz by running the reference RFMGCN (models/rfmgcn.py,
models/rf_modules.py) on CPU, on the data, under the seed and with case A of mgcn_tiny.npz (U = 37, I = 41, B = 16,
n_layers 1, cl_loss 0.001), under the stand-ins of make_golden_mgcn.py (torch_scatter, Tensor.cuda, a temporary
data_path).  MGCN's part is asserted against mgcn_tiny.npz bit for bit (the 19 parameters, case A's loss and its 19
gradients, the scores before warm-up) and not stored again.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  One record, "A_": both views as conditions (C = 128), rf_n_layers = 2, rf_dropout 0, rf_sampling_steps 3,
7 negatives per row, rf_learning_rate 1e-3, no gradient checkpointing, through RFMGCN.calculate_loss /
full_sort_predict (before and after warm-up), with the draws recorded (X0, t, the negatives after the collision rule,
the eval z0).

The RNG order of RFMGCN.calculate_loss is: the lazy velocity-net init (first call only; here it is made beforehand,
as make_golden_rffreedom.record does) -> compute_loss_and_step (X0, t, item negatives, user negatives) -> generate()
(its z0, the result is discarded).  MGCN draws nothing.  The draws are captured by replaying the generator in that
order; the replay is asserted: the generator's losses from the captured draws (the restatement of
tests/rfbm3_fixture.py) equal the reference's.

The fp32-vs-fp64 spread of the sampler output and of the velocity gradients (the restatement run in both precisions on
the same inputs) is stored as A_err_sample / A_err_grad: the GPU tests allow 4x that.

Usage:  python tests/golden/make_golden_rfmgcn.py
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import Cfg, MockLoader, OUT, _import_reference  # noqa: E402
from make_golden_mgcn import CASES, PARAMS  # noqa: E402
from make_golden_rffreedom import N_NEG, STEPS, record  # noqa: E402
from make_golden_rfbm3 import LR, finish  # noqa: E402

RATIO = 0.2


def gen_rfmgcn(tmp):
    import torch
    ts = types.ModuleType("torch_scatter")

    def scatter_add(src, index, dim=0, dim_size=None):
        return torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, src)

    ts.scatter_add = scatter_add
    sys.modules["torch_scatter"] = ts
    _import_reference()
    torch.Tensor.cuda = lambda self, *a, **kw: self
    import models.rfmgcn as rfmgcn

    f = dict(np.load(os.path.join(OUT, "mgcn_tiny.npz")))
    U, I, B = int(f["U"]), int(f["I"]), 16
    N = U + I
    rows, cols, users, pos, neg = f["train_rows"], f["train_cols"], f["users"], f["pos"], f["neg"]
    os.makedirs(os.path.join(tmp, "tm"), exist_ok=True)
    np.save(os.path.join(tmp, "tm", "image_feat.npy"), f["v_feat"])
    np.save(os.path.join(tmp, "tm", "text_feat.npy"), f["t_feat"])
    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset="tm",
              vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64, knn_k=5,
              n_ui_layers=2, reg_weight=1e-4, lambda_coeff=0.9, use_rf=True, use_denoise=False, use_2rf=False,
              rf_hidden_dim=128, rf_n_layers=2, rf_dropout=0.0, rf_learning_rate=LR, rf_sampling_steps=STEPS,
              rf_warmup_epochs=0, rf_mix_ratio=0.1, rf_inference_mix_ratio=RATIO, rf_contrast_temp=0.2,
              rf_loss_weight=1.0, use_gradient_checkpointing=False, **CASES["A"])
    torch.manual_seed(3)
    m = rfmgcn.RFMGCN(cfg, MockLoader(U, I, rows, cols))
    params = dict(m.named_parameters())
    assert list(params) == PARAMS, "the velocity net is created lazily: MGCN's 19 parameters alone"
    for n in PARAMS:
        assert np.array_equal(params[n].detach().numpy(), f["init_" + n.replace(".", "_")]), n  # mgcn_tiny's
    m.pre_epoch_processing()  # the RF epoch counter becomes 0
    gen = m.rf_generator
    gen.infonce_negative_samples = N_NEG
    out = {"U": np.int64(U), "I": np.int64(I), "n_neg": np.int64(N_NEG), "steps": np.int64(STEPS), "lr": np.float64(LR),
           "ratio": np.float64(RATIO)}

    # ---- the two modal views (mgcn.py:148-185), which forward does not return: the conditions
    m.train()
    with torch.no_grad():
        views = []
        for emb, trs, gate, adj in ((m.image_embedding, m.image_trs, m.gate_v, m.image_original_adj),
                                    (m.text_embedding, m.text_trs, m.gate_t, m.text_original_adj)):
            h = m.item_id_embedding.weight * gate(trs(emb.weight))
            for _ in range(m.n_layers):
                h = torch.sparse.mm(adj, h)
            views.append(torch.cat([torch.sparse.mm(m.R, h), h]))
    assert np.array_equal(views[0].numpy(), f["A_a"]) and np.array_equal(views[1].numpy(), f["A_b"])
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
    seed, X0, t, ni, nu, seen, hook = record(torch, gen, out, "A_", torch.zeros(N, 64), views, users, pos, U, I, 2)
    assert sum(p.numel() for p in gen.velocity_net.parameters()) == 125760
    m.zero_grad()
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    loss = m.calculate_loss(inter)
    loss.backward()
    hook.remove()
    gen.compute_loss_and_step = step
    # MGCN's step is mgcn_tiny's case A bit for bit: the RF part changes nothing in it
    assert np.float32(loss.item()) == f["A_loss"], (loss.item(), f["A_loss"])
    for n in PARAMS:
        assert np.array_equal(params[n].grad.numpy(), f["A_g_" + n.replace(".", "_")]), n
    # the RF inputs: X1 = all = c + side, cond = [a | b], prior = the two-segment centred (a + b) / 2
    assert np.array_equal(cap["X1"].numpy(), f["A_c"] + f["A_side"]), "X1 = all"
    assert torch.equal(cap["cond"], torch.cat(views, dim=-1)), "conditions: the image view then the text view"
    Z = (0 + views[0] + views[1]) / 2
    assert torch.equal(Z, 0.5 * (views[0] + views[1]))
    want = torch.cat([Z[:U] - Z[:U].mean(dim=0, keepdim=True), Z[U:] - Z[U:].mean(dim=0, keepdim=True)])
    assert torch.equal(cap["prior"], want), "prior: Z - its own segment's mean"
    assert float(cap["prior"][:U].abs().max()) > 0 and float(cap["cond"][:U].abs().max()) > 0, "dense user rows"
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
        eu, ei = m.forward(m.norm_adj)
        out["A_eval"] = torch.cat([eu, ei]).numpy().copy()
    assert np.array_equal(out["A_scores_pre"], f["A_scores"]), "before warm-up: MGCN's scores"
    al = f["A_c"] + f["A_side"]
    np.testing.assert_allclose(out["A_eval"], al + RATIO * out["A_gen"], rtol=0, atol=1e-6)
    assert np.abs(out["A_eval"][:U] - al[:U]).max() > 1e-2 and np.abs(out["A_eval"][U:] - al[U:]).max() > 1e-2
    out["A_score_shift"] = np.float64(np.abs(out["A_scores_mix"] - out["A_scores_pre"]).max())
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_rfmgcn(tmp)
    # four files, each under the size limit of a committed file, split as make_golden_rfbm3.py splits: the
    # velocity parameters, their gradients and the stepped parameters are ~0.5 MB each
    parts = {"rfmgcn_tiny_param": {k: v for k, v in out.items() if k[2:5] == "p0_"},
             "rfmgcn_tiny_grad": {k: v for k, v in out.items() if k[2:4] == "g_"},
             "rfmgcn_tiny_step": {k: v for k, v in out.items() if k[2:5] == "p1_"}}
    parts["rfmgcn_tiny"] = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    for name, d in parts.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20) * 9 // 10, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    print("rf", out["A_rf_loss"], "cl", out["A_cl_loss"], "err_grad", out["A_err_grad"], "err_sample",
          out["A_err_sample"], "prior max", np.abs(out["A_prior"]).max(), "largest score",
          np.abs(out["A_scores_pre"]).max(), "shift by the mix", out["A_score_shift"])


if __name__ == "__main__":
    main()
