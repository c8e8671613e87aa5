"""Generate tests/golden/rfsmore_tiny{,_param,_grad,_step}.npz by running the reference RFSMORE (models/rfsmore.py,
models/rf_modules.py) on CPU, on the data, under the seed and with case B of smore_tiny{,_B}.npz (U = 37, I = 41,
B = 16, n_layers 2, dropout 0.1, cl_loss 0.1; the two embedding tables times 8 and the 64-input weights times sqrt(8)),
first step, under the stand-ins of make_golden_smore.py (torch_scatter, Tensor.cuda, a temporary data_path).

The reference's nn.Dropout is replaced by one that replays that step's recorded keep masks B_keep[0] with F.dropout's
arithmetic (kept entries times the fp32 1 / (1 - p)), so the third condition block carries a real mask and scale, and
SMORE's part is smore_tiny_B.npz's: the fp32 loss is asserted bit for bit, the 29 gradients against the file's fp64
gradients at the bar that file's maker uses, the scores before warm-up bit for bit.  None of it is stored again.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  One record, "B_": three views as conditions (C = 192), rf_n_layers = 2, rf_dropout 0, rf_sampling_steps 3,
7 negatives per row, rf_learning_rate 1e-3, no gradient checkpointing, through RFSMORE.calculate_loss /
full_sort_predict (before and after warm-up), with the draws recorded (X0, t, the negatives after the collision rule,
the eval z0).

The RNG order of RFSMORE.calculate_loss is: the lazy velocity-net init (made beforehand, as
make_golden_rffreedom.record does) -> compute_loss_and_step (X0, t, item negatives, user negatives) -> generate()
(its z0, the result is discarded).  The replayed dropout draws nothing.  The replay of the draws is asserted: the
generator's losses from the captured draws (the restatement of tests/rfbm3_fixture.py) equal the reference's.

Stored next to the record: the plain fusion view f and the gate gf of the step (the third condition block is gf * f,
not f), and the evaluation after warm-up, where the forward runs without dropout: its conditions (B_cond_eval), SMORE's
table (B_all_eval), the sampler's rows from the recorded z0 (B_gen_eval) and the mixed table (B_eval).  B_gen is
generate() on the training step's conditions, which the spread B_err_sample is measured on.

Usage:  python tests/golden/make_golden_rfsmore.py
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
from make_golden_rffreedom import N_NEG, STEPS, record  # noqa: E402
from make_golden_rfbm3 import LR, finish  # noqa: E402
import rf_fixture as R  # noqa: E402
import smore_fixture as F  # noqa: E402

RATIO = 0.2
N_PARAMS = 125760 + 128 * 64  # C = 192, two layers


def gen_rfsmore(tmp):
    import torch
    import torch.nn as nn
    ts = types.ModuleType("torch_scatter")
    ts.scatter_add = lambda src, index, dim=0, dim_size=None: torch.zeros(dim_size, dtype=src.dtype).index_add_(
        0, index, src)
    sys.modules["torch_scatter"] = ts
    _import_reference()
    torch.Tensor.cuda = lambda self, *a, **kw: self
    import models.rfsmore as rfsmore

    f = dict(np.load(os.path.join(OUT, "smore_tiny.npz")))
    f.update(np.load(os.path.join(OUT, "smore_tiny_B.npz")))
    U, I, B = int(f["U"]), int(f["I"]), 16
    N = U + I
    rows, cols, users, pos, neg = f["train_rows"], f["train_cols"], f["users"], f["pos"], f["neg"]
    cs = F.CASES["B"]
    p = cs["dropout_rate"]
    keep = F.golden_keep(f, 0)
    assert keep.shape == (N, 192) and 0.85 < keep.mean() < 0.95

    class Replay(nn.Module):
        """Dropout with the recorded masks of one forward (image, text, fusion gate, in that order), F.dropout's
        arithmetic; the identity in evaluation."""

        def __init__(self):
            super().__init__()
            self.i = 0
            self.scale = float(np.float32(1.0) / np.float32(1.0 - p))

        def forward(self, x):
            if not self.training:
                return x
            k = torch.as_tensor(keep[:, 64 * (self.i % 3):64 * (self.i % 3) + 64]).to(x.dtype)
            self.i += 1
            return x * (k * self.scale)

    os.makedirs(os.path.join(tmp, "tm"), exist_ok=True)
    np.save(os.path.join(tmp, "tm", "image_feat.npy"), f["v_feat"])
    np.save(os.path.join(tmp, "tm", "text_feat.npy"), f["t_feat"])
    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset="tm",
              vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64,
              image_knn_k=F.IMAGE_K, text_knn_k=F.TEXT_K, n_ui_layers=F.N_UI_LAYERS, reg_weight=F.REG_WEIGHT,
              lambda_coeff=0.9, temperature=0.2, use_rf=True, use_denoise=False, use_2rf=False, rf_hidden_dim=128,
              rf_n_layers=2, rf_dropout=0.0, rf_learning_rate=LR, rf_sampling_steps=STEPS, rf_warmup_epochs=0,
              rf_mix_ratio=0.1, rf_inference_mix_ratio=RATIO, rf_contrast_temp=0.2, rf_loss_weight=1.0,
              use_gradient_checkpointing=False, **cs)
    torch.manual_seed(3)
    m = rfsmore.RFSMORE(cfg, MockLoader(U, I, rows, cols))
    m.dropout = Replay()
    params = dict(m.named_parameters())
    assert list(params) == F.STATE_KEYS, "the velocity net is created lazily: SMORE's 29 parameters alone"
    names = dict(zip(F.PARAMS, params.values()))
    want = F.case_params(f, "B")
    with torch.no_grad():
        for k, q in names.items():
            assert np.array_equal(q.numpy(), f["init_" + k]), k  # smore_tiny's init
            q.copy_(torch.as_tensor(want[k]))
    m.pre_epoch_processing()  # the RF epoch counter becomes 0
    gen = m.rf_generator
    gen.infonce_negative_samples = N_NEG
    out = {"U": np.int64(U), "I": np.int64(I), "n_neg": np.int64(N_NEG), "steps": np.int64(STEPS), "lr": np.float64(LR),
           "ratio": np.float64(RATIO)}

    # ---- the three views (smore.py:208-291), which forward does not return, and the fusion gate of the step
    m.train()
    with torch.no_grad():
        ic, tc, fc = m.spectrum_convolution(m.image_trs(m.image_embedding.weight), m.text_trs(m.text_embedding.weight))
        views = []
        for conv, gate, adj in ((ic, m.gate_v, m.image_original_adj), (tc, m.gate_t, m.text_original_adj),
                                (fc, m.gate_f, m.fusion_adj)):
            h = m.item_id_embedding.weight * gate(conv)
            for _ in range(m.n_layers):
                h = torch.sparse.mm(adj, h)
            views.append(torch.cat([torch.sparse.mm(m.R, h), h]))
        ego = torch.cat([m.user_embedding.weight, m.item_id_embedding.weight])
        layers = [ego]
        for _ in range(m.n_ui_layers):
            ego = torch.sparse.mm(m.norm_adj, ego)
            layers.append(ego)
        content = torch.stack(layers, dim=1).mean(dim=1)
        gf = m.gate_fusion_prefer(content) * (torch.as_tensor(keep[:, 128:]).float() * m.dropout.scale)
    a, b, fv = views
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
    seed, X0, t, ni, nu, seen, hook = record(torch, gen, out, "B_", torch.zeros(N, 64), [torch.zeros(N, 192)], users,
                                             pos, U, I, 2)
    assert sum(q.numel() for q in gen.velocity_net.parameters()) == N_PARAMS
    m.zero_grad()
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    loss = m.calculate_loss(inter)
    loss.backward()
    hook.remove()
    gen.compute_loss_and_step = step
    assert m.dropout.i == 3, "one forward, three masks"
    # SMORE's step is smore_tiny_B's: the fp32 loss bit for bit, the gradients at that maker's bar against its fp64 run
    assert np.float32(loss.item()) == f["B_loss32"], (loss.item(), f["B_loss32"])
    for k in F.PARAMS:
        g64 = f["B_g_" + k]
        own = np.abs(names[k].grad.numpy().astype(np.float64) - g64).max()
        assert 2 * own < 1e-3 * np.abs(g64).max(), (k, own)
    # the RF inputs: X1 = all = c + side; cond = [a | b | gf f]; prior = the two-segment centred (a + b + gf f) / 3
    np.testing.assert_allclose(cap["X1"].numpy(), f["B_c"] + f["B_side"], rtol=1e-5, atol=2e-6)
    gff = gf * fv
    assert torch.equal(cap["cond"], torch.cat([a, b, gff], dim=-1)), "conditions: image, text, the gated fusion view"
    assert not torch.equal(cap["cond"][:, 128:], fv) and float((cap["cond"][:, 128:] - fv).abs().max()) > 1e-2
    dropped = keep[:, 128:] == 0
    assert dropped.any() and not cap["cond"][:, 128:][torch.as_tensor(dropped)].any(), "the mask is in the condition"
    Z = (0 + a + b + gff) / 3
    wantp = torch.cat([Z[:U] - Z[:U].mean(dim=0, keepdim=True), Z[U:] - Z[U:].mean(dim=0, keepdim=True)])
    assert torch.equal(cap["prior"], wantp), "prior: Z - its own segment's mean"
    assert float(cap["prior"][:U].abs().max()) > 0 and float(cap["cond"][:U].abs().max()) > 0, "dense user rows"
    out["B_f"], out["B_gf"] = fv.numpy().copy(), gf.numpy().copy()
    finish(torch, gen, out, "B_", cap["X1"], cap["cond"], cap["prior"], users, pos, U, 2, X0, t, ni, nu, seen,
           cap["loss"])
    out["B_seed"] = np.int64(seed)

    # evaluation before and after warm-up (the velocity parameters are the stepped ones, p1): no dropout
    m.eval()
    with torch.no_grad():
        gen.warmup_epochs = 5
        out["B_scores_pre"] = m.full_sort_predict([torch.arange(U)]).numpy()
        gen.warmup_epochs = 0
        torch.manual_seed(23)  # generate() draws z0 first: B_z0
        out["B_scores_mix"] = m.full_sort_predict([torch.arange(U)]).numpy()
        sample = gen.generate

        def gspy(conditions, *a_, **kw):
            cap["cond_eval"] = torch.cat(conditions, dim=-1).clone()
            cap["gen_eval"] = sample(conditions, *a_, **kw)
            return cap["gen_eval"]

        gen.generate = gspy
        torch.manual_seed(23)
        eu, ei = m.forward(m.norm_adj)
        gen.generate = sample
        out["B_eval"] = torch.cat([eu, ei]).numpy().copy()
        gen.warmup_epochs = 5
        au, ai = m.forward(m.norm_adj)
        gen.warmup_epochs = 0
        out["B_all_eval"] = torch.cat([au, ai]).numpy().copy()
        gate_eval = m.gate_fusion_prefer(content)
    assert m.dropout.i == 3, "no mask is drawn in evaluation"
    assert np.array_equal(out["B_scores_pre"], f["B_scores32"]), "before warm-up: SMORE's scores"
    out["B_cond_eval"], out["B_gen_eval"] = cap["cond_eval"].numpy().copy(), cap["gen_eval"].numpy().copy()
    assert torch.equal(cap["cond_eval"], torch.cat([a, b, gate_eval * fv], dim=-1)), "evaluation: the bare gate"
    assert not np.array_equal(out["B_cond_eval"], out["B_cond"])
    np.testing.assert_allclose(out["B_eval"], out["B_all_eval"] + RATIO * out["B_gen_eval"], rtol=0, atol=1e-6)
    d = np.abs(out["B_eval"] - out["B_all_eval"])
    assert d[:U].max() > 1e-2 and d[U:].max() > 1e-2
    np.testing.assert_allclose(out["B_eval"][:U] @ out["B_eval"][U:].T, out["B_scores_mix"], rtol=1e-5, atol=1e-4)
    # the restatement's sampler on the evaluation conditions, within the stored spread's bar
    P1 = {n: torch.tensor(out["B_p1_" + R.key(n)], dtype=torch.float64) for n in R.param_names(2)}
    z64 = R.generate(P1, cap["cond_eval"].double(), torch.tensor(out["B_z0"]).double(), STEPS, 2)
    out["B_err_sample_eval"] = np.float64(np.abs(out["B_gen_eval"].astype(np.float64) - z64.numpy()).max())
    out["B_score_shift"] = np.float64(np.abs(out["B_scores_mix"] - out["B_scores_pre"]).max())
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_rfsmore(tmp)
    # four files, each under the size limit of a committed file, split as make_golden_rfmgcn.py splits: the
    # velocity parameters, their gradients and the stepped parameters are ~0.5 MB each
    parts = {"rfsmore_tiny_param": {k: v for k, v in out.items() if k[2:5] == "p0_"},
             "rfsmore_tiny_grad": {k: v for k, v in out.items() if k[2:4] == "g_"},
             "rfsmore_tiny_step": {k: v for k, v in out.items() if k[2:5] == "p1_"}}
    parts["rfsmore_tiny"] = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    for name, d in parts.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20) * 9 // 10, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    print("rf", out["B_rf_loss"], "cl", out["B_cl_loss"], "err_grad", out["B_err_grad"], "err_sample",
          out["B_err_sample"], "err_sample_eval", out["B_err_sample_eval"], "prior max", np.abs(out["B_prior"]).max(),
          "largest score", np.abs(out["B_scores_pre"]).max(), "shift by the mix", out["B_score_shift"])


if __name__ == "__main__":
    main()
