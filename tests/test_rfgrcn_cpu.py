"""RFGRCN without a GPU: the golden record of tests/golden/make_golden_rfgrcn.py (the reference RFGRCN on case A of
grcn_tiny.npz, generated rows and conditions 192 wide) against the plain torch restatement of tests/rf_fixture.py /
tests/rfbm3_fixture.py, whose formulas take their widths from the tensors; the packed parameter layout at width 192;
the registry, the YAML and the config checks of gmr/rfgrcn.py."""
import os

import numpy as np
import pytest
import torch

import grcn_fixture as F
import rf_fixture as R
import rfbm3_fixture as RB
import rfgrcn_fixture as RG

TAG = RG.TAG


@pytest.fixture(scope="module")
def g(golden):
    return RG.load_golden(golden)


@pytest.fixture(scope="module")
def f(golden):
    return golden("grcn_tiny")


@pytest.fixture(scope="module")
def step64(g):
    """The restatement's fp64 step on the record, computed once."""
    return RB.record_losses(g, TAG, RG.L, torch.float64)


def test_record_shapes_and_inputs(g, f):
    U, I = int(g["U"]), int(g["I"])
    N = U + I
    assert (U, I) == (37, 41) and g["A_X1"].shape == (N, RG.WIDTH) == g["A_prior"].shape == g["A_X0"].shape
    assert g["A_z0"].shape == g["A_z0_eval"].shape == g["A_gen_eval"].shape == (N, RG.WIDTH)
    # X1 is GRCN's table of case A, and the prior its per-segment centred copy
    np.testing.assert_allclose(g["A_X1"], f["A_result"], rtol=1e-5, atol=2e-6)
    want = RG.prior_ref(torch.tensor(g["A_X1"]), U).numpy()
    assert np.array_equal(g["A_prior"], want)
    assert np.abs(g["A_prior"][:U].mean(0)).max() < 1e-6 and np.abs(g["A_prior"][U:].mean(0)).max() < 1e-6
    # the negatives are stored after the collision rule
    assert not (g["A_neg_items"] == g["A_pos"][:, None]).any() and not (g["A_neg_users"] == g["A_users"][:, None]).any()


def test_restatement_reproduces_the_losses_and_gradients(g, step64):
    r, grads = step64
    np.testing.assert_allclose(r["rf_loss"].item(), g["A_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["cl_loss"].item(), g["A_cl_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["v"].detach().numpy(), g["A_v"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r["pred"].detach().numpy(), g["A_pred"], rtol=1e-5, atol=1e-5)
    worst = 0.0
    for n in R.param_names(RG.L):
        err = R.rel_to_max(g["A_g_" + R.key(n)], grads[n].numpy())
        worst = max(worst, err)
        assert err <= float(g["A_err_grad"]) * 1.001, (n, err)   # the stored spread; fp64 moves it by its own rounding
    assert worst >= 0.5 * float(g["A_err_grad"]), "the spread is the reference's fp32 error, not a loose bound"


def test_restatement_reproduces_the_stepped_parameters(g, step64):
    """One AdamW step (lr 1e-3, weight decay 0.01) from the restatement's fp64 gradients lands on the stored p1 within
    rfbm3_fixture.p1_bound at the record's own gradient spread."""
    _, grads = step64
    lr, b1, b2, eps, wd = float(g["lr"]), 0.9, 0.999, 1e-8, 0.01
    bar = R.grad_bar(g, TAG)
    for n in R.param_names(RG.L):
        p0, gr = g["A_p0_" + R.key(n)].astype(np.float64), grads[n].numpy()
        m, v = (1 - b1) * gr, (1 - b2) * gr * gr
        p1 = p0 * (1 - lr * wd) - lr * (m / (1 - b1)) / (np.sqrt(v / (1 - b2)) + eps)
        assert (np.abs(p1 - g["A_p1_" + R.key(n)]) <= RB.p1_bound(g, TAG, n, bar, lr)).all(), n
        assert np.abs(g["A_p1_" + R.key(n)] - g["A_p0_" + R.key(n)]).max() > 0


def test_sampler_restatement_and_the_recorded_evaluation(g):
    U = int(g["U"])
    VP1 = {n: g["A_p1_" + R.key(n)] for n in R.param_names(RG.L)}
    z64 = RG.generate_ref(VP1, g["A_X1"], g["A_z0"], int(g["steps"]), RG.L, torch.float64)
    assert np.abs(g["A_gen"] - z64).max() <= float(g["A_err_sample"]) * 1.001
    # the evaluation forward of the record: the same start noise and table, so the same rows, mixed at 0.2
    assert np.array_equal(g["A_z0_eval"], g["A_z0"]) and np.array_equal(g["A_gen_eval"], g["A_gen"])
    np.testing.assert_allclose(g["A_eval"], g["A_X1"] + float(g["ratio"]) * g["A_gen_eval"], rtol=0, atol=1e-6)
    # the scores the reference's evaluation reads are the unmixed training table's
    x = g["A_X1"].astype(np.float64)
    np.testing.assert_allclose(g["A_scores_cached"], x[:U] @ x[U:].T, rtol=1e-5, atol=1e-4)
    e = g["A_eval"].astype(np.float64)
    np.testing.assert_allclose(g["A_scores_mix"], e[:U] @ e[U:].T, rtol=1e-5, atol=1e-4)
    assert np.abs(g["A_scores_mix"] - g["A_scores_cached"]).max() > 1.0


def test_param_specs_at_width_192(g):
    from gmr.rf import param_specs
    specs = param_specs(192, RG.L, D=192)
    assert [n for n, _ in specs] == R.param_names(RG.L)
    for n, sh in specs:
        assert tuple(sh) == g["A_p0_" + R.key(n)].shape, n
    assert sum(int(np.prod(sh)) for _, sh in specs) == RG.N_PARAMS == 166848
    d = dict(specs)
    assert d["input_proj.0.weight"] == (128, 192) and d["output_proj.4.weight"] == (192, 128)
    assert d["output_proj.4.bias"] == (192,) and d["time_embed.1.weight"] == (128, 64)
    assert sum(int(np.prod(sh)) for _, sh in param_specs(128, RG.L, D=128)) == RG.N_PARAMS_128


def test_param_specs_default_width_is_unchanged():
    from gmr.rf import param_specs
    specs = param_specs(128, 2)
    assert sum(int(np.prod(sh)) for _, sh in specs) == 125760
    assert specs == param_specs(128, 2, D=64) and dict(specs)["output_proj.4.weight"] == (64, 128)


def test_registry_and_yaml():
    from gmr.configurator import Config
    from gmr.rfgrcn import RFGRCN, check_config
    from gmr.utils import get_model
    assert get_model("RFGRCN") is RFGRCN
    cfg = Config("RFGRCN", "baby", {})
    want = {"use_rf": True, "rf_hidden_dim": 128, "rf_n_layers": 2, "rf_dropout": 0.1, "rf_learning_rate": 0.0001,
            "rf_sampling_steps": 10, "rf_warmup_epochs": 5, "rf_mix_ratio": 0.1, "rf_inference_mix_ratio": 0.2,
            "rf_contrast_temp": 0.2, "rf_loss_weight": 1.0, "use_2rf": False, "use_denoise": False,
            "rf_eval": "cached", "n_layers": 3, "embedding_size": 64, "latent_embedding": 64, "routing": "reference"}
    for k, v in want.items():
        assert cfg[k] == v, (k, cfg[k])
    assert check_config(cfg) == "cached"
    import gmr
    path = os.path.join(os.path.dirname(gmr.__file__), "configs", "model")
    grcn_keys = {ln.split(":")[0] for ln in open(os.path.join(path, "GRCN.yaml")) if ln[:1].isalpha()}
    rf_keys = {ln.split(":")[0] for ln in open(os.path.join(path, "RFGRCN.yaml")) if ln[:1].isalpha()}
    assert grcn_keys <= rf_keys


@pytest.mark.parametrize("over,key,exc", [({"rf_eval": "other"}, "rf_eval", ValueError),
                                          ({"use_2rf": True}, "use_2rf", NotImplementedError),
                                          ({"use_denoise": True}, "use_denoise", NotImplementedError),
                                          ({"rf_hidden_dim": 64}, "rf_hidden_dim", NotImplementedError)])
def test_check_config_names_the_key(over, key, exc):
    from gmr.rfgrcn import check_config
    with pytest.raises(exc, match=key):
        check_config(RG.rfgrcn_config(**over))
    assert check_config(RG.rfgrcn_config(rf_eval="mixed")) == "mixed"


def test_case_config_is_grcn_case_a():
    c = RG.case_config()
    assert c["n_layers"] == F.CASES["A"]["n_layers"] and c["rf_sampling_steps"] == 3 and c["rf_infonce_negatives"] == 7
