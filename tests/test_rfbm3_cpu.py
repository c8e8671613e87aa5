"""The plain torch restatement of RFBM3 (tests/rfbm3_fixture.py: the RF inputs, the generator's losses with the
user-prior term, BM3's step from tests/bm3_fixture.py) pinned to the reference's golden values
(tests/golden/make_golden_rfbm3.py): with it pinned, the GPU tests may use its fp64 run where the reference recorded
nothing.  Also what the reference's evaluation does to the two halves of the table."""
import numpy as np
import pytest
import torch

import bm3_fixture as B
import rf_fixture as R
import rfbm3_fixture as RB

RECORDS = [("A_", 2, 128), ("B_", 1, 64)]
U, I = 37, 41


@pytest.fixture(autouse=True)
def _feature():
    from gmr.utils import get_model
    get_model("RFBM3")  # the feature under test: raises ValueError without it


@pytest.fixture(scope="module")
def g(golden):
    return RB.load_golden(golden)


@pytest.fixture(scope="module")
def b(golden):
    return golden("bm3_tiny")


@pytest.mark.parametrize("tag,L,C", RECORDS)
def test_train_step_pinned(g, tag, L, C):
    assert g[tag + "cond"].shape == (U + I, C) and not g[tag + "cond"][:U].any()  # zero user rows
    assert g[tag + "prior"].shape == (U + I, 64) and not g[tag + "prior"][:U].any()
    r, grads = RB.record_losses(g, tag, L)
    np.testing.assert_allclose(r["v"].detach().numpy(), g[tag + "v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["pred"].detach().numpy(), g[tag + "pred"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["rf_loss"].item(), g[tag + "rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["cl_loss"].item(), g[tag + "cl_loss"], rtol=1e-5)
    for n, v in grads.items():
        want = g[tag + "g_" + R.key(n)]
        np.testing.assert_allclose(v.numpy(), want, rtol=1e-4, atol=R.grad_bar(g, tag) * np.abs(want).max(), err_msg=n)
    # the prior term is in the record: without it v is another table
    X1, X0, t, cond, users, pos, ni, nu, prior = RB.record_inputs(g, tag)
    P = R.params_from(g, tag, L)
    bare = R.train_losses(P, X1, X0, t, cond, users, pos, ni, nu, U, L)
    assert np.abs(bare["v"].numpy() - g[tag + "v"]).max() > 1e-2
    # one torch.optim.AdamW step on the recorded gradients gives the recorded parameters.  The update is
    # p0 (1 - lr wd) - lr g / (|g| + eps): two roundings (half an ulp each) at the magnitude of its operands, and
    # which way they fall depends on how the host's vector units contract the expression; two such results are
    # each within an ulp of the exact one, so they differ by at most two: 4 x 2^-24 max(|p0|, lr)
    lr = float(g["lr"])
    ps = [torch.nn.Parameter(torch.tensor(g[tag + "p0_" + R.key(n)])) for n in R.param_names(L)]
    for p, n in zip(ps, R.param_names(L)):
        p.grad = torch.tensor(g[tag + "g_" + R.key(n)])
    torch.optim.AdamW(ps, lr=lr).step()
    for p, n in zip(ps, R.param_names(L)):
        p0 = np.abs(g[tag + "p0_" + R.key(n)].astype(np.float64))
        diff = np.abs(p.detach().numpy().astype(np.float64) - g[tag + "p1_" + R.key(n)])
        assert (diff <= 4 * 2.0 ** -24 * np.maximum(p0, lr)).all(), n


def test_inputs_pinned(g, b):
    """X1, cond and prior of the reference against the fp64 restatement on bm3_tiny's parameters."""
    P = {k: b["p_" + k] for k in B.PARAMS}
    x1 = RB.encoder_mean(P, U, I, b["train_rows"], b["train_cols"], B.CASES["A"]["n_layers"])
    np.testing.assert_allclose(g["A_X1"], x1.numpy(), rtol=1e-5, atol=1e-6)
    pr = RB.projected(P)
    cond, prior = RB.rf_inputs_ref(pr["text"], pr["image"], U)
    np.testing.assert_allclose(g["A_cond"], cond.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["A_prior"], prior.numpy(), rtol=1e-5, atol=2e-6)
    assert np.abs(g["A_prior"]).max() > 1.0
    np.testing.assert_allclose(g["A_cond"][U:, :64], pr["image"].numpy(), rtol=1e-5, atol=2e-6)  # image first
    cond_b, prior_b = RB.rf_inputs_ref(pr["text"], None, U)
    np.testing.assert_allclose(g["B_cond"], cond_b.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_prior"], prior_b.numpy(), rtol=1e-5, atol=2e-6)
    assert np.abs(g["A_prior"][U:].astype(np.float64).mean(0)).max() < 1e-6  # centred over the items


def test_bm3_part_pinned(g, b):
    """BM3's loss, terms, reg and ten gradients under the masks this run drew (the RF step draws first, so they are
    not bm3_tiny's), at the bars of test_bm3_restatement_cpu.py."""
    c = B.CASES["A"]
    keep = B.golden_keep(g, "A")
    assert any(not np.array_equal(keep[k], b["A_keep_" + k]) for k in "uitv")
    r = B.bm3_step_ref({k: b["p_" + k] for k in B.PARAMS}, U, I, b["train_rows"], b["train_cols"], g["A_users"],
                       g["A_pos"], keep, c["n_layers"], c["dropout"], dtype=torch.float64)
    np.testing.assert_allclose(r["loss"], g["A_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["terms"], g["A_loss_terms"], rtol=1e-5)
    np.testing.assert_allclose(r["reg"], g["A_reg"], rtol=1e-5)
    B.check_grads(r["grads"], [g["A_g_" + k] for k in B.PARAMS], show="A fp64")
    assert np.array_equal(g["A_users"], b["users"]) and np.array_equal(g["A_pos"], b["items"])


def test_evaluation_mixes_the_user_rows_only(g, b):
    # before warm-up: BM3's scores
    assert np.array_equal(g["A_scores_pre"], b["A_scores"])
    # from warm-up on: the item table is BM3's, the user rows moved by ratio * gen
    assert np.array_equal(g["A_eval_i"], b["A_ib"])
    np.testing.assert_allclose(g["A_eval_u"], b["A_ua"] + 0.2 * g["A_gen"][:U], rtol=0, atol=1e-6)
    assert np.abs(g["A_eval_u"] - b["A_ua"]).max() > 0.05
    # a user's generated row depends on z0 alone: the sampler on the U user rows against zero conditions
    P1 = R.params_from(g, "A_", 2, prefix="p1_")
    z = R.generate(P1, torch.zeros(U, 128), torch.tensor(g["A_z0"][:U]), int(g["steps"]), 2)
    np.testing.assert_allclose(z.numpy(), g["A_gen"][:U], rtol=0, atol=4 * float(g["A_err_sample"]))
    # the scores: the predictor over both halves
    W, bias = b["p_predictor_weight"].astype(np.float64), b["p_predictor_bias"].astype(np.float64)
    pu, pi = g["A_eval_u"] @ W.T + bias, g["A_eval_i"] @ W.T + bias
    np.testing.assert_allclose(pu @ pi.T, g["A_scores_mix"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("tag,L,C", RECORDS)
def test_generate_pinned(g, tag, L, C):
    P = R.params_from(g, tag, L, prefix="p1_")
    z = R.generate(P, torch.tensor(g[tag + "cond"]), torch.tensor(g[tag + "z0"]), int(g["steps"]), L)
    np.testing.assert_allclose(z.numpy(), g[tag + "gen"], rtol=0, atol=4 * float(g[tag + "err_sample"]))


def test_head_zero_prior_is_the_plain_head(g):
    """head_ref with a zero prior gives rf_fixture's guidance bit for bit (the kernel test relies on it)."""
    X1, X0, t, cond, users, pos, ni, nu, prior = RB.record_inputs(g, "A_")
    Xt = t * X1 + (1 - t) * X0
    V = torch.tensor(g["A_v"])
    a, _, _ = RB.head_ref(V, Xt, X1, X0, t, torch.zeros_like(prior))
    assert torch.equal(a, V + (1 - t) ** 2 * 0.1 * R.cos_grad(Xt, X1))


def test_registry_and_yaml():
    from gmr.configurator import Config
    from gmr.rfbm3 import RFBM3
    from gmr.utils import get_model
    assert get_model("RFBM3") is RFBM3
    cfg = Config("RFBM3", "baby", {"synthetic": "tiny"})
    assert cfg["use_rf"] is True and cfg["use_denoise"] is False and cfg["use_2rf"] is False
    assert (cfg["rf_hidden_dim"], cfg["rf_loss_weight"], cfg["rf_infonce_negatives"]) == (128, 0.2, 1024)
    assert (cfg["n_layers"], cfg["dropout"], cfg["reg_weight"], cfg["cl_weight"]) == (1, 0.3, 0.1, 2.0)
