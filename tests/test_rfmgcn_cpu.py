"""The plain torch restatement of RFMGCN (tests/rfmgcn_fixture.py: X1 = all, cond = [a | b], the two-segment centred
prior; the generator's losses with the prior term from tests/rfbm3_fixture.py; MGCN's step from tests/mgcn_fixture.py)
pinned to the reference's golden values (tests/golden/make_golden_rfmgcn.py, on the data, seed and case A of
mgcn_tiny.npz): with it pinned, the GPU tests may use its fp64 run where the reference recorded nothing.  Also what the
reference's evaluation does to the table (every row is mixed), the YAML, the unsupported keys and the registry."""
import numpy as np
import pytest
import torch

import mgcn_fixture as M
import rf_fixture as R
import rfbm3_fixture as RB
import rfmgcn_fixture as RM

U, I, L = 37, 41, 2


@pytest.fixture(autouse=True)
def _feature():
    from gmr.utils import get_model
    get_model("RFMGCN")  # the feature under test: raises ValueError without it


@pytest.fixture(scope="module")
def g(golden):
    return RM.load_golden(golden)


@pytest.fixture(scope="module")
def f(golden):
    return golden("mgcn_tiny")


def test_inputs_pinned(g, f):
    """X1, cond and prior of the reference: from MGCN's golden tables exactly, from the fp64 restatement of the MGCN
    forward at MGCN's table bars (test_mgcn_gpu.py's), and the prior from the golden views at rtol 1e-5."""
    assert g["A_cond"].shape == (U + I, 128) and g["A_prior"].shape == (U + I, 64)
    assert np.array_equal(g["A_X1"], f["A_c"] + f["A_side"])                  # X1 = all
    assert np.array_equal(g["A_cond"], np.concatenate([f["A_a"], f["A_b"]], axis=1))   # the image view first
    assert np.abs(g["A_cond"][:U]).max() > 1e-3 and np.abs(g["A_prior"][:U]).max() > 1e-3   # dense user rows
    # the prior from the recorded views in fp64.  Next to rtol 1e-5, the three fp32 roundings of the reference
    # (a + b, the mean's division, the subtraction; the sum of at most 41 rows adds less than one more) at the
    # magnitude of Z: an entry of a difference of nearly equal numbers has no relative accuracy of its own
    a, b = torch.tensor(f["A_a"], dtype=torch.float64), torch.tensor(f["A_b"], dtype=torch.float64)
    want = RM.prior_ref(a, b, U).numpy()
    zmax = float(((a + b) / 2).abs().max())
    err = np.abs(g["A_prior"] - want)
    print(f"prior: max abs error {err.max():.3e}, max |Z| {zmax:.3e}, atol {4 * 2.0 ** -24 * zmax:.3e}")
    assert (err <= 1e-5 * np.abs(want) + 4 * 2.0 ** -24 * zmax).all()
    for seg in (slice(0, U), slice(U, U + I)):
        assert np.abs(g["A_prior"][seg].astype(np.float64).mean(0)).max() < 1e-8   # each segment centred on its own
    # one mean over all N rows would be another table
    z = ((a + b) / 2).numpy()
    assert np.abs(g["A_prior"] - (z - z.mean(0))).max() > 1e-3
    # the whole chain from the parameters
    r = M.mgcn_step_ref(M.case_params(f, "A"), U, I, f["train_rows"], f["train_cols"], f["users"], f["pos"], f["neg"],
                        1, 0.001, feats=(f["v_feat"], f["t_feat"]))
    X1, cond, prior = RM.rf_inputs_ref(r, U)
    np.testing.assert_allclose(g["A_X1"], X1.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["A_cond"], cond.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["A_prior"], prior.numpy(), rtol=1e-5, atol=2e-6)


def test_prior_ref_segments():
    """prior_ref itself: a single row per segment is its own mean; a segment's mean sees no row of the other."""
    one = torch.tensor([[3.0] * 64, [-5.0] * 64], dtype=torch.float64)
    assert not RM.prior_ref(one, 2 * one, 1).any()
    rng = np.random.default_rng(0)
    a = torch.tensor(np.concatenate([100 + rng.standard_normal((5, 64)), -100 + rng.standard_normal((3, 64))]))
    p = RM.prior_ref(a, a, 5)
    assert float(p.abs().max()) < 10 and float(p[:5].mean(0).abs().max()) < 1e-12


def test_train_step_pinned(g):
    """The generator's step on the recorded inputs and draws: v and pred at test_rfbm3_cpu.py's bars, the losses at
    1e-5 relative, the velocity gradients within 4 x the stored err_grad of the parameter's largest entry."""
    r, grads = RB.record_losses(g, "A_", L)
    np.testing.assert_allclose(r["v"].detach().numpy(), g["A_v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["pred"].detach().numpy(), g["A_pred"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["rf_loss"].item(), g["A_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["cl_loss"].item(), g["A_cl_loss"], rtol=1e-5)
    bar = R.grad_bar(g, "A_")
    assert sum(v.numel() for v in grads.values()) == 125760  # C = 128, two layers
    for n, v in grads.items():
        err = R.rel_to_max(v.numpy(), g["A_g_" + R.key(n)])
        assert err <= bar, (n, err, bar)
    # the fp64 run, which the GPU tests lean on, likewise
    r64, g64 = RB.record_losses(g, "A_", L, dtype=torch.float64)
    np.testing.assert_allclose(r64["rf_loss"].item(), g["A_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r64["cl_loss"].item(), g["A_cl_loss"], rtol=1e-5)
    for n, v in g64.items():
        assert R.rel_to_max(g["A_g_" + R.key(n)], v.numpy()) <= bar, n
    # the prior term is in the record: without it v is another table, on the user rows too
    X1, X0, t, cond, users, pos, ni, nu, prior = RB.record_inputs(g, "A_")
    bare = R.train_losses(R.params_from(g, "A_", L), X1, X0, t, cond, users, pos, ni, nu, U, L)
    assert np.abs(bare["v"].numpy() - g["A_v"])[:U].max() > 1e-3
    # one torch.optim.AdamW step on the recorded gradients gives the recorded parameters, within two ulps at the
    # magnitude of the update's operands (the reasoning is test_rfbm3_cpu.py's)
    lr = float(g["lr"])
    ps = [torch.nn.Parameter(torch.tensor(g["A_p0_" + R.key(n)])) for n in R.param_names(L)]
    for p, n in zip(ps, R.param_names(L)):
        p.grad = torch.tensor(g["A_g_" + R.key(n)])
    torch.optim.AdamW(ps, lr=lr).step()
    for p, n in zip(ps, R.param_names(L)):
        p0 = np.abs(g["A_p0_" + R.key(n)].astype(np.float64))
        diff = np.abs(p.detach().numpy().astype(np.float64) - g["A_p1_" + R.key(n)])
        assert (diff <= 4 * 2.0 ** -24 * np.maximum(p0, lr)).all(), n


def test_generate_pinned(g):
    P = R.params_from(g, "A_", L, prefix="p1_")
    z = R.generate(P, torch.tensor(g["A_cond"]), torch.tensor(g["A_z0"]), int(g["steps"]), L)
    np.testing.assert_allclose(z.numpy(), g["A_gen"], rtol=0, atol=4 * float(g["A_err_sample"]))


def test_evaluation_mixes_every_row(g, f):
    # before warm-up: MGCN's scores
    assert np.array_equal(g["A_scores_pre"], f["A_scores"])
    # from warm-up on: every row moved by ratio * gen, users and items
    al, ratio = f["A_c"] + f["A_side"], float(g["ratio"])
    np.testing.assert_allclose(g["A_eval"], al + ratio * g["A_gen"], rtol=0, atol=1e-6)
    assert np.abs(g["A_eval"] - al)[:U].max() > 0.05 and np.abs(g["A_eval"] - al)[U:].max() > 0.05
    ev = g["A_eval"].astype(np.float64)
    np.testing.assert_allclose(ev[:U] @ ev[U:].T, g["A_scores_mix"], rtol=1e-5, atol=1e-5)
    assert np.abs(g["A_scores_mix"] - g["A_scores_pre"]).max() > np.abs(g["A_scores_pre"]).max()


def test_registry_and_yaml():
    from gmr.configurator import Config
    from gmr.mgcn import MGCN
    from gmr.rfmgcn import RFMGCN
    from gmr.utils import get_model
    assert get_model("RFMGCN") is RFMGCN and issubclass(RFMGCN, MGCN)
    cfg = Config("RFMGCN", "baby", {"synthetic": "tiny"})
    base = Config("MGCN", "baby", {"synthetic": "tiny"})
    for k in ("embedding_size", "n_ui_layers", "n_layers", "knn_k", "reg_weight", "cl_loss", "learning_rate",
              "learning_rate_scheduler", "lambda_coeff"):
        assert cfg[k] == base[k], k
    assert cfg["use_rf"] is True and cfg["use_denoise"] is False and cfg["use_2rf"] is False
    assert (cfg["rf_hidden_dim"], cfg["rf_n_layers"], cfg["rf_loss_weight"], cfg["rf_infonce_negatives"]) == \
        (128, 2, 0.2, 1024)
    assert (cfg["rf_sampling_steps"], cfg["rf_warmup_epochs"], cfg["rf_inference_mix_ratio"]) == (10, 20, 0.05)
    assert cfg["use_wandb"] is None and cfg["wandb_project"] is None


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(over, key):
    from gmr.rf import check_config
    check_config(RM.rfmgcn_config())
    with pytest.raises(NotImplementedError, match=key):
        check_config(RM.rfmgcn_config(**over))
