"""Generate tests/golden/rfgrcn_tiny{,_param,_grad,_step}.npz by running the reference RFGRCN (models/rfgrcn.py,
models/rf_modules.py) on CPU, on the data, under the seed and with the scaled parameters of case A of grcn_tiny.npz
(U = 37, I = 41, B = 16, both modalities, n_layers 3), first step, under the torch_geometric stand-ins of
make_golden_grcn.py.

GRCN's part is GRCN's: the reference's own GRCN class is run next to it, and the fp32 loss and the eight gradients are
asserted equal to that class's bit for bit, and against grcn_tiny.npz at the bars of tests/grcn_fixture.py (the loss
within one fp32 rounding and rtol 1e-5 of the fp64 loss, the gradients at rtol 1e-5 with an atol of twice the stored
fp32 distance).  None of it is stored again.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  One record, "A_": the generated rows and the conditions are the concatenated table, 192 wide (embedding_dim =
condition_dim = 192, 166,848 velocity parameters), rf_n_layers = 2, rf_dropout 0, rf_sampling_steps 3, 7 negatives per
row, rf_learning_rate 1e-3, no gradient checkpointing, rf_warmup_epochs 0, through RFGRCN.calculate_loss /
full_sort_predict / forward, with the draws recorded (X0, t, the negatives after the collision rule, the z0 of the
sampler).  make_golden_rffreedom.record and make_golden_rfbm3.finish draw 64 columns; record_w / finish_w here are
the same at the width of X1.

The RNG order of RFGRCN.calculate_loss is: GRCN draws nothing (edge dropout 0) -> compute_loss_and_step (X0, t, item
negatives, user negatives) -> generate() (its z0, the result is discarded: mix_embeddings(training=True) returns the
original table).  The replay is asserted: the generator's losses from the captured draws (the restatement of
tests/rf_fixture.py with the prior term of tests/rfbm3_fixture.py, whose formulas take their widths from the tensors)
equal the reference's.

Stored next to the record, the evaluation.  A_scores_cached: full_sort_predict after calculate_loss, which reads
self.result, the training forward's unmixed table (asserted, with the warm-up at 5 and at 0: the generator never
reaches the reference's evaluation).  From m.eval(); m.forward() under torch.manual_seed(23): the start noise
(A_z0_eval), the sampler's rows (A_gen_eval), the mixed table A_eval = result + 0.2 gen_eval and its scores
(A_scores_mix), what the port's rf_eval: mixed computes.

Usage:  python tests/golden/make_golden_rfgrcn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import Cfg, MockLoader, OUT, _import_reference  # noqa: E402
from make_golden_grcn import stand_ins  # noqa: E402
from make_golden_rffreedom import N_NEG, STEPS  # noqa: E402
import grcn_fixture as F  # noqa: E402
import rf_fixture as R  # noqa: E402
import rfbm3_fixture as RB  # noqa: E402

LR, RATIO = 0.001, 0.2
N_PARAMS = 166848  # D = C = 192, two layers
WIDTH = 192


def _draws(torch, seed, N, D, U, I, B):
    torch.manual_seed(seed)
    X0 = torch.randn(N, D)
    t = torch.rand(N, 1)
    ni = torch.randint(0, I, (B, N_NEG))
    nu = torch.randint(0, U, (B, N_NEG))
    return X0, t, ni.numpy(), nu.numpy()


def record_w(torch, gen, out, tag, D, C, users, pos, U, I, n_layers):
    """make_golden_rffreedom.record at target width D: the net created (its init drawn under seed 5 and stored as
    p0_*), the first seed whose raw negatives hit a positive and repeat within a row, the draws of that seed."""
    N, B = U + I, len(users)
    torch.manual_seed(5)
    gen._init_velocity_net(C, torch.device("cpu"))
    net = gen.velocity_net
    assert [n for n, _ in net.named_parameters()] == R.param_names(n_layers)
    for n, p in net.named_parameters():
        out[tag + "p0_" + R.key(n)] = p.detach().numpy().copy()
    for seed in range(100, 400):
        _, _, ni, nu = _draws(torch, seed, N, D, U, I, B)
        hit = (ni == pos[:, None]).any() and (nu == users[:, None]).any()
        if hit and any(len(set(r.tolist())) < N_NEG for r in R.collide(ni, pos, I)):
            break
    else:
        raise AssertionError("no seed with a drawn positive and a duplicate negative")
    X0, t, ni, nu = _draws(torch, seed, N, D, U, I, B)
    ni, nu = R.collide(ni, pos, I), R.collide(nu, users, U)
    seen = {}

    def keep_first(mod, args, o):  # returns None: a hook's return value would replace the output
        seen.setdefault("v", o.detach().clone())

    h = net.register_forward_hook(keep_first)
    torch.manual_seed(seed)
    return seed, X0, t, ni, nu, seen, h


def finish_w(torch, gen, out, tag, X1, cond, prior, users, pos, U, n_layers, X0, t, ni, nu, seen, loss_dict):
    """make_golden_rfbm3.finish at the width of X1: the step's inputs, draws, v, pred, losses, gradients and stepped
    parameters; the replay asserted; the fp32 spread measured; one generate() with a recorded z0 on the stepped
    parameters."""
    net = gen.velocity_net
    out[tag + "X1"], out[tag + "X0"], out[tag + "t"] = X1.numpy(), X0.numpy(), t.numpy()
    out[tag + "prior"] = prior.numpy()  # cond is X1 (asserted by the caller): not stored twice
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
    z0 = torch.randn(X1.shape[0], X1.shape[1])
    with torch.no_grad():
        net.eval()
        z = gen.generate([cond], n_steps=STEPS, start_noise=z0)
        net.train()
        P1 = {n: torch.tensor(out[tag + "p1_" + R.key(n)], dtype=torch.float64) for n in R.param_names(n_layers)}
        z64 = R.generate(P1, cond.double(), z0.double(), STEPS, n_layers)
    out[tag + "z0"], out[tag + "gen"] = z0.numpy(), z.numpy()
    out[tag + "err_sample"] = np.float64(np.abs(z.numpy().astype(np.float64) - z64.numpy()).max())
    return z0


def gen_rfgrcn():
    import torch
    stand_ins()
    _import_reference()
    import models.grcn as grcn
    import models.rfgrcn as rfgrcn

    f = dict(np.load(os.path.join(OUT, "grcn_tiny.npz")))
    U, I, B = int(f["U"]), int(f["I"]), 16
    N = U + I
    rows, cols, users, pos, neg = f["train_rows"], f["train_cols"], f["users"], f["pos"], f["neg"]
    cs = F.CASES["A"]
    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=True, is_multimodal_model=True, embedding_size=64,
              latent_embedding=64, n_layers=cs["n_layers"], reg_weight=cs["reg_weight"], use_rf=True, use_denoise=False,
              use_2rf=False, rf_hidden_dim=128, rf_n_layers=2, rf_dropout=0.0, rf_learning_rate=LR,
              rf_sampling_steps=STEPS, rf_warmup_epochs=0, rf_mix_ratio=0.1, rf_inference_mix_ratio=RATIO,
              rf_contrast_temp=0.2, rf_loss_weight=1.0, use_gradient_checkpointing=False)
    # end2end: the base class loads no feature file; the features are set before the constructor reads them
    base = grcn.GeneralRecommender.__init__

    def init(self, config, dataset):
        base(self, config, dataset)
        self.v_feat, self.t_feat = torch.as_tensor(f["v_feat"]), torch.as_tensor(f["t_feat"])

    grcn.GeneralRecommender.__init__ = init
    try:
        torch.manual_seed(3)
        m = rfgrcn.RFGRCN(cfg, MockLoader(U, I, rows, cols))
        torch.manual_seed(3)
        plain = grcn.GRCN(cfg, MockLoader(U, I, rows, cols))  # the reference's own GRCN
    finally:
        grcn.GeneralRecommender.__init__ = base
    params = dict(m.named_parameters())
    assert list(params) == F.STATE_KEYS, "the velocity net is created lazily: GRCN's eight parameters alone"
    names = {k: params[s] for k, s in zip(F.PARAMS, F.STATE_KEYS)}
    pnames = {k: dict(plain.named_parameters())[s] for k, s in zip(F.PARAMS, F.STATE_KEYS)}
    assert np.array_equal(m.result.numpy(), f["A_result0"]), "the init table full_sort_predict reads before any step"
    want = F.case_params(f, "A")
    with torch.no_grad():
        for k, q in names.items():
            assert np.array_equal(q.numpy(), f["A_init_" + k]), k  # grcn_tiny's init
            assert np.array_equal(pnames[k].numpy(), f["A_init_" + k]), k
            q.copy_(torch.as_tensor(want[k]))
            pnames[k].copy_(torch.as_tensor(want[k]))
    m.pre_epoch_processing()  # the RF epoch counter becomes 0
    gen = m.rf_generator
    assert gen.embedding_dim == WIDTH
    gen.infonce_negative_samples = N_NEG
    out = {"U": np.int64(U), "I": np.int64(I), "n_neg": np.int64(N_NEG), "steps": np.int64(STEPS), "lr": np.float64(LR),
           "ratio": np.float64(RATIO)}

    m.train()
    cap = {}
    step = gen.compute_loss_and_step

    def spy(**kw):
        cap["X1"] = kw["target_embeds"].detach().clone()
        cap["cond"] = torch.cat([c.detach() for c in kw["conditions"]], dim=-1)
        cap["prior"] = kw["user_prior"].detach().clone()
        cap["loss"] = step(**kw)
        return cap["loss"]

    gen.compute_loss_and_step = spy
    seed, X0, t, ni, nu, seen, hook = record_w(torch, gen, out, "A_", WIDTH, WIDTH, users, pos, U, I, 2)
    assert sum(q.numel() for q in gen.velocity_net.parameters()) == N_PARAMS
    m.zero_grad()
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    loss = m.calculate_loss(inter)
    loss.backward()
    hook.remove()
    gen.compute_loss_and_step = step
    result = m.result.detach().clone()  # the training forward's table
    # GRCN's step is the reference GRCN class's, bit for bit; against grcn_tiny.npz at the fixture's bars
    plain.train()
    plain.zero_grad()
    ploss = plain.calculate_loss(inter)
    ploss.backward()
    assert loss.item() == ploss.item(), (loss.item(), ploss.item())
    for k in F.PARAMS:
        assert torch.equal(names[k].grad, pnames[k].grad), k
    assert torch.equal(result, plain.result.detach())
    l32, w32 = np.float32(loss.item()), np.float32(f["A_loss32"])
    assert abs(float(l32) - float(w32)) <= float(np.spacing(w32)), (loss.item(), f["A_loss32"])
    assert abs(loss.item() - float(f["A_loss"])) <= 1e-5 * abs(float(f["A_loss"]))
    out["A_loss32_bits_equal"] = np.bool_(l32 == w32)
    for k in F.PARAMS:
        g64 = f["A_g_" + k]
        err = np.abs(names[k].grad.numpy().astype(np.float64) - g64)
        assert (err <= 1e-5 * np.abs(g64) + 2 * float(f["A_own_" + k])).all(), (k, err.max(), f["A_own_" + k])
    # the RF inputs: X1 = result = the concatenated conditions; prior = the per-segment centred table
    assert tuple(cap["X1"].shape) == (N, WIDTH)
    assert torch.equal(cap["X1"], result), "X1 = representation.detach()"
    assert torch.equal(cap["X1"], cap["cond"]), "the concatenated conditions are the target table"
    wantp = torch.cat([result[:U] - result[:U].mean(dim=0, keepdim=True),
                       result[U:] - result[U:].mean(dim=0, keepdim=True)])
    assert torch.equal(cap["prior"], wantp), "prior: every column minus its own segment's mean"
    assert float(cap["prior"][:U].abs().max()) > 0 and float(cap["prior"][U:].abs().max()) > 0
    finish_w(torch, gen, out, "A_", cap["X1"], cap["cond"], cap["prior"], users, pos, U, 2, X0, t, ni, nu, seen,
             cap["loss"])
    out["A_seed"] = np.int64(seed)

    # ---- evaluation as written: full_sort_predict reads the cached training table, whatever the warm-up state
    with torch.no_grad():
        r64 = result.numpy().astype(np.float64)
        for warm in (5, 0):
            gen.warmup_epochs = warm
            sc = m.full_sort_predict([torch.arange(U)]).numpy()
            assert np.array_equal(sc, (result[:U] @ result[U:].t()).numpy()), warm
            assert torch.equal(m.result.detach(), result), "full_sort_predict recomputes nothing"
        out["A_scores_cached"] = sc
        np.testing.assert_allclose(sc, r64[:U] @ r64[U:].T, rtol=1e-5, atol=1e-4)
        # ---- what forward() computes in eval mode (never reached by the reference's evaluation): the mix
        m.eval()
        sample = gen.generate

        def gspy(conditions, *a_, **kw):
            cap["cond_eval"] = torch.cat(conditions, dim=-1).clone()
            cap["gen_eval"] = sample(conditions, *a_, **kw)
            return cap["gen_eval"]

        gen.generate = gspy
        torch.manual_seed(23)  # GRCN draws nothing, so generate()'s z0 is the first draw
        ev = m.forward()
        gen.generate = sample
        torch.manual_seed(23)
        z0 = torch.randn(N, WIDTH)
    out["A_z0_eval"], out["A_gen_eval"], out["A_eval"] = z0.numpy(), cap["gen_eval"].numpy().copy(), ev.numpy().copy()
    # the parameters moved by no step of GRCN's (no optimiser here), so the eval table under the mix is result again
    assert torch.equal(cap["cond_eval"], result), "the evaluation's conditions: the recomputed table"
    np.testing.assert_allclose(out["A_eval"], result.numpy() + RATIO * out["A_gen_eval"], rtol=0, atol=1e-6)
    assert np.abs(out["A_eval"] - result.numpy()).max() > 1e-3
    P1 = {n: torch.tensor(out["A_p1_" + R.key(n)], dtype=torch.float64) for n in R.param_names(2)}
    z64 = R.generate(P1, result.double(), z0.double(), STEPS, 2)
    out["A_err_sample_eval"] = np.float64(np.abs(out["A_gen_eval"].astype(np.float64) - z64.numpy()).max())
    assert out["A_err_sample_eval"] <= 4 * out["A_err_sample"] + 1e-6, "the eval z0 is not the recorded one"
    e64 = out["A_eval"].astype(np.float64)
    out["A_scores_mix"] = (ev[:U] @ ev[U:].t()).numpy()
    np.testing.assert_allclose(out["A_scores_mix"], e64[:U] @ e64[U:].T, rtol=1e-5, atol=1e-4)
    out["A_score_shift"] = np.float64(np.abs(out["A_scores_mix"] - out["A_scores_cached"]).max())
    assert out["A_score_shift"] > 1e-3
    return out


def main():
    out = gen_rfgrcn()
    # four files, each under the size limit of a committed file, split as the sibling makers split: the velocity
    # parameters, their gradients and the stepped parameters are ~0.67 MB each
    parts = {"rfgrcn_tiny_param": {k: v for k, v in out.items() if k[2:5] == "p0_"},
             "rfgrcn_tiny_grad": {k: v for k, v in out.items() if k[2:4] == "g_"},
             "rfgrcn_tiny_step": {k: v for k, v in out.items() if k[2:5] == "p1_"}}
    parts["rfgrcn_tiny"] = {k: v for k, v in out.items() if not any(k in p for p in parts.values())}
    for name, d in parts.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20) * 9 // 10, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    print("rf", out["A_rf_loss"], "cl", out["A_cl_loss"], "err_grad", out["A_err_grad"], "err_sample",
          out["A_err_sample"], "err_sample_eval", out["A_err_sample_eval"], "prior max", np.abs(out["A_prior"]).max(),
          "largest score", np.abs(out["A_scores_cached"]).max(), "shift by the mix", out["A_score_shift"])


if __name__ == "__main__":
    main()
