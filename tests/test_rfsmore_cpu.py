"""The plain torch restatement of RFSMORE (tests/rfsmore_fixture.py: X1 = all, cond = [a | b | gf f], the two-segment
centred prior of their mean; the generator's losses with the prior term from tests/rfbm3_fixture.py at C = 192; SMORE's
step from tests/smore_fixture.py) pinned to the reference's golden values (tests/golden/make_golden_rfsmore.py, on the
data, seed, case B and first keep masks of smore_tiny{,_B}.npz): with it pinned, the GPU tests may use its fp64 run
where the reference recorded nothing.  Also that the third condition block is the gated fusion view and not the plain
one, what the reference's evaluation does to the table, the YAML, the unsupported keys and the registry."""
import numpy as np
import pytest
import torch

import rf_fixture as R
import rfbm3_fixture as RB
import rfsmore_fixture as RS
import smore_fixture as F

U, I, L, P_DROP = 37, 41, 2, 0.1
N = U + I


@pytest.fixture(autouse=True)
def _feature():
    from gmr.utils import get_model
    get_model("RFSMORE")  # the feature under test: raises ValueError without it


@pytest.fixture(scope="module")
def g(golden):
    return RS.load_golden(golden)


@pytest.fixture(scope="module")
def f(golden):
    return RS.smore_golden(golden)


@pytest.fixture(scope="module")
def step64(f):
    """The fp64 restatement of SMORE's case B step with the recorded masks, once."""
    c = F.CASES["B"]
    return F.smore_step_ref(F.case_params(f, "B"), U, I, f["train_rows"], f["train_cols"], f["users"], f["pos"],
                            f["neg"], c["n_layers"], c["cl_loss"], (f["v_feat"], f["t_feat"]),
                            keep=F.golden_keep(f, 0), p=P_DROP)


def test_third_block_is_the_gated_fusion_view(g, f):
    """rfsmore.py:143 reassigns fusion_embeds = fusion_prefer * fusion_embeds before :176 collects the conditions: the
    third block is gf * f with the step's keep mask and 1 / (1 - p), not f."""
    cond, fv, gf = g["B_cond"], g["B_f"], g["B_gf"]
    assert cond.shape == (N, 192) and fv.shape == gf.shape == (N, 64)
    assert np.array_equal(cond[:, 128:], gf * fv)
    assert not np.array_equal(cond[:, 128:], fv) and np.abs(cond[:, 128:] - fv).max() > 1e-2
    keep = F.golden_keep(f, 0)[:, 128:]
    assert 0 < (keep == 0).sum() < keep.size // 5
    assert not gf[keep == 0].any() and (gf[keep == 1] > 0).all()      # the mask
    assert gf.max() > 1.0 and gf.max() <= np.float32(1.0) / np.float32(0.9)   # the scale: a sigmoid over 0.9
    # the evaluation's conditions carry the bare gate: the same first two blocks, another third
    ce = g["B_cond_eval"]
    assert np.array_equal(ce[:, :128], cond[:, :128]) and not np.array_equal(ce[:, 128:], cond[:, 128:])
    gate = ce[:, 128:][np.abs(fv) > 1e-3] / fv[np.abs(fv) > 1e-3]
    assert gate.min() > 0 and gate.max() < 1


def test_inputs_pinned(g, f, step64):
    """cond and prior from the recorded views and gate in fp64; the whole chain from the parameters at SMORE's table
    bars (rtol 1e-5, atol 2e-6)."""
    assert g["B_prior"].shape == (N, 64)
    np.testing.assert_allclose(g["B_X1"], f["B_c"] + f["B_side"], rtol=1e-5, atol=2e-6)    # X1 = all
    assert np.abs(g["B_cond"][:U]).max() > 1e-3 and np.abs(g["B_prior"][:U]).max() > 1e-3   # dense user rows
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    a, b = t64(g["B_cond"][:, :64]), t64(g["B_cond"][:, 64:128])
    cond, want = RS.inputs_ref(a, b, t64(g["B_f"]), t64(g["B_gf"]), U)
    # the third block is one fp32 rounding of the fp64 product
    np.testing.assert_allclose(g["B_cond"], cond.numpy(), rtol=2.0 ** -23, atol=0)
    # next to rtol 1e-5, the fp32 roundings of the reference (the product, two sums, the division by 3, the mean's
    # division and the subtraction: six; the sum of at most 41 rows adds less than one more) at the magnitude of Z
    zmax = float(((a + b + t64(g["B_gf"]) * t64(g["B_f"])) / 3).abs().max())
    err = np.abs(g["B_prior"] - want.numpy())
    print(f"prior: max abs error {err.max():.3e}, max |Z| {zmax:.3e}, atol {7 * 2.0 ** -24 * zmax:.3e}")
    assert (err <= 1e-5 * np.abs(want.numpy()) + 7 * 2.0 ** -24 * zmax).all()
    for seg in (slice(0, U), slice(U, N)):
        assert np.abs(g["B_prior"][seg].astype(np.float64).mean(0)).max() < 1e-7   # each segment centred on its own
    z = ((a + b + t64(g["B_gf"]) * t64(g["B_f"])) / 3).numpy()
    assert np.abs(g["B_prior"] - (z - z.mean(0))).max() > 1e-3    # one mean over all N rows would be another table
    assert np.abs(g["B_prior"] - RS.inputs_ref(a, b, t64(g["B_f"]), torch.ones(N, 64, dtype=torch.float64),
                                               U)[1].numpy()).max() > 1e-3   # and so would the plain fusion view
    # the whole chain from the parameters
    X1, cond, prior = RS.rf_inputs_ref(step64, F.case_params(f, "B"), U, F.golden_keep(f, 0), P_DROP)
    np.testing.assert_allclose(g["B_X1"], X1.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_cond"], cond.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_prior"], prior.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_f"], step64["f"], rtol=1e-5, atol=2e-6)
    # and the evaluation's: no mask
    Xe, ce, _ = RS.rf_inputs_ref(step64, F.case_params(f, "B"), U)
    np.testing.assert_allclose(g["B_cond_eval"], ce.numpy(), rtol=1e-5, atol=2e-6)


def test_inputs_ref_segments():
    """inputs_ref itself: a single row per segment is its own mean; a segment's mean sees no row of the other; a zero
    gate takes the fusion view out of both tables."""
    one = torch.tensor([[3.0] * 64, [-5.0] * 64], dtype=torch.float64)
    assert not RS.inputs_ref(one, 2 * one, one, one, 1)[1].any()
    rng = np.random.default_rng(0)
    a = torch.tensor(np.concatenate([100 + rng.standard_normal((5, 64)), -100 + rng.standard_normal((3, 64))]))
    cond, p = RS.inputs_ref(a, a, a, torch.ones_like(a), 5)
    assert float(p.abs().max()) < 10 and float(p[:5].mean(0).abs().max()) < 1e-12
    assert torch.equal(cond, torch.cat([a, a, a], dim=1))
    cond, p0 = RS.inputs_ref(a, a, a, torch.zeros_like(a), 5)
    assert not cond[:, 128:].any() and torch.allclose(p0, p * 2 / 3, rtol=1e-12, atol=1e-12)


def test_train_step_pinned(g):
    """The generator's step on the recorded inputs and draws at C = 192: v and pred at test_rfmgcn_cpu.py's bars, the
    losses at 1e-5 relative, the velocity gradients within 4 x the stored err_grad of the parameter's largest entry."""
    r, grads = RB.record_losses(g, "B_", L)
    np.testing.assert_allclose(r["v"].detach().numpy(), g["B_v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["pred"].detach().numpy(), g["B_pred"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["rf_loss"].item(), g["B_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["cl_loss"].item(), g["B_cl_loss"], rtol=1e-5)
    bar = R.grad_bar(g, "B_")
    assert sum(v.numel() for v in grads.values()) == RS.N_PARAMS
    assert g["B_p0_condition_encoder_0_weight"].shape == (128, 192)
    for n, v in grads.items():
        err = R.rel_to_max(v.numpy(), g["B_g_" + R.key(n)])
        assert err <= bar, (n, err, bar)
    # the fp64 run, which the GPU tests lean on, likewise
    r64, g64 = RB.record_losses(g, "B_", L, dtype=torch.float64)
    np.testing.assert_allclose(r64["rf_loss"].item(), g["B_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r64["cl_loss"].item(), g["B_cl_loss"], rtol=1e-5)
    for n, v in g64.items():
        assert R.rel_to_max(g["B_g_" + R.key(n)], v.numpy()) <= bar, n
    # the prior term is in the record: without it v is another table, on the user rows too
    X1, X0, t, cond, users, pos, ni, nu, prior = RB.record_inputs(g, "B_")
    bare = R.train_losses(R.params_from(g, "B_", L), X1, X0, t, cond, users, pos, ni, nu, U, L)
    assert np.abs(bare["v"].numpy() - g["B_v"])[:U].max() > 1e-3
    # the third condition block reaches the gradient: every one of its 64 weight columns has one
    assert (np.abs(g["B_g_condition_encoder_0_weight"][:, 128:]).max(0) > 0).all()
    # one torch.optim.AdamW step on the recorded gradients gives the recorded parameters (test_rfmgcn_cpu.py's bound)
    lr = float(g["lr"])
    ps = [torch.nn.Parameter(torch.tensor(g["B_p0_" + R.key(n)])) for n in R.param_names(L)]
    for p, n in zip(ps, R.param_names(L)):
        p.grad = torch.tensor(g["B_g_" + R.key(n)])
    torch.optim.AdamW(ps, lr=lr).step()
    for p, n in zip(ps, R.param_names(L)):
        p0 = np.abs(g["B_p0_" + R.key(n)].astype(np.float64))
        diff = np.abs(p.detach().numpy().astype(np.float64) - g["B_p1_" + R.key(n)])
        assert (diff <= 4 * 2.0 ** -24 * np.maximum(p0, lr)).all(), n


def test_generate_pinned(g):
    P = R.params_from(g, "B_", L, prefix="p1_")
    z0, steps = torch.tensor(g["B_z0"]), int(g["steps"])
    z = R.generate(P, torch.tensor(g["B_cond"]), z0, steps, L)
    np.testing.assert_allclose(z.numpy(), g["B_gen"], rtol=0, atol=4 * float(g["B_err_sample"]))
    ze = R.generate(P, torch.tensor(g["B_cond_eval"]), z0, steps, L)
    np.testing.assert_allclose(ze.numpy(), g["B_gen_eval"], rtol=0, atol=4 * float(g["B_err_sample"]))
    assert np.abs(g["B_gen_eval"] - g["B_gen"]).max() > 1e-3    # the mask moves the sampler's rows


def test_evaluation_mixes_every_row(g, f):
    assert np.array_equal(g["B_scores_pre"], f["B_scores32"])   # before warm-up: SMORE's scores
    al, ratio = g["B_all_eval"], float(g["ratio"])
    ev = al.astype(np.float64)
    np.testing.assert_allclose(ev[:U] @ ev[U:].T, g["B_scores_pre"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(g["B_eval"], al + ratio * g["B_gen_eval"], rtol=0, atol=1e-6)
    assert np.abs(g["B_eval"] - al)[:U].max() > 0.05 and np.abs(g["B_eval"] - al)[U:].max() > 0.05
    ev = g["B_eval"].astype(np.float64)
    np.testing.assert_allclose(ev[:U] @ ev[U:].T, g["B_scores_mix"], rtol=1e-5, atol=1e-4)
    assert float(g["B_score_shift"]) > 1.0


def test_registry_and_yaml():
    from gmr.configurator import Config
    from gmr.rf import RFBackbone
    from gmr.rfsmore import RFSMORE
    from gmr.smore import SMORE
    from gmr.utils import get_model
    assert get_model("RFSMORE") is RFSMORE and issubclass(RFSMORE, SMORE) and issubclass(RFSMORE, RFBackbone)
    assert RFSMORE.rf_condition_dim(None) == 192
    cfg = Config("RFSMORE", "baby", {"synthetic": "tiny"})
    base = Config("SMORE", "baby", {"synthetic": "tiny"})
    for k in ("embedding_size", "n_ui_layers", "n_layers", "image_knn_k", "text_knn_k", "reg_weight", "cl_loss",
              "dropout_rate", "learning_rate", "learning_rate_scheduler", "lambda_coeff", "temperature"):
        assert cfg[k] == base[k], k
    assert cfg["use_rf"] is True and cfg["use_denoise"] is False and cfg["use_2rf"] is False
    assert (cfg["rf_hidden_dim"], cfg["rf_n_layers"], cfg["rf_loss_weight"], cfg["rf_infonce_negatives"]) == \
        (128, 2, 0.2, 1024)
    assert (cfg["rf_sampling_steps"], cfg["rf_warmup_epochs"], cfg["rf_inference_mix_ratio"]) == (10, 20, 0.05)
    assert (cfg["rf_learning_rate"], cfg["rf_contrast_temp"], cfg["rf_dropout"]) == (0.0003, 0.1, 0.1)
    assert cfg["use_wandb"] is None and cfg["wandb_project"] is None


def test_condition_dim_default_is_64_per_modality():
    """RFBackbone asks the model; the default is what the three earlier RF models had hard-coded."""
    from gmr.rf import RFBackbone

    class Two:
        mods = (("image", None, 0), ("text", None, 1))

    class One:
        mods = (("text", None, 0),)

    assert RFBackbone.rf_condition_dim(Two()) == 128 and RFBackbone.rf_condition_dim(One()) == 64


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(over, key):
    from gmr.rf import check_config
    check_config(RS.rfsmore_config())
    with pytest.raises(NotImplementedError, match=key):
        check_config(RS.rfsmore_config(**over))
