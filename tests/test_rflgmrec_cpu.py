"""The plain torch restatement of RFLGMRec (tests/rflgmrec_fixture.py: X1 = cge, cond = [mge_v | mge_t], the
two-segment centred prior of their *sum*; the evaluation with the generated rows mixed into cge before the hypergraph
block; the generator's losses with the prior term from tests/rfbm3_fixture.py at C = 128; LGMRec's forward from
tests/lgmrec_fixture.py) pinned to the reference's golden values (tests/golden/make_golden_rflgmrec.py, on the data,
seed, case B and recorded draws of lgmrec_tiny{,_B}.npz): with it pinned, the GPU tests may use its fp64 run where the
reference recorded nothing.  Also that a restatement which mixes into all instead (the rule of the other RF models)
misses the golden table, the YAML, the unsupported keys and the registry."""
import numpy as np
import pytest
import torch

import lgmrec_fixture as F
import rf_fixture as R
import rfbm3_fixture as RB
import rflgmrec_fixture as RL

U, I, L = 37, 41, 2
N = U + I


@pytest.fixture(autouse=True)
def _feature():
    from gmr.utils import get_model
    get_model("RFLGMRec")  # the feature under test: raises ValueError without it


@pytest.fixture(scope="module")
def g(golden):
    return RL.load_golden(golden)


@pytest.fixture(scope="module")
def f(golden):
    return RL.lgmrec_golden(golden)


def _fw(f, g_key, keep, dtype):
    gd = f[g_key][0] if g_key == "B_g" else f[g_key]
    return RL.forward_ref(F.case_params(f, "B"), (f["v_feat"], f["t_feat"]), U, I, f["train_rows"], f["train_cols"],
                          dict(F.CASES["B"]), gd, keep, dtype)


@pytest.fixture(scope="module")
def train64(f):
    """The fp64 restatement of LGMRec's case B training forward with the recorded draws and masks, once."""
    return _fw(f, "B_g", f["B_keep"][0], torch.float64)


@pytest.fixture(scope="module")
def evals(f):
    """The evaluation forward (recorded Gumbel draws, no dropout) in both precisions, once."""
    return {dt: _fw(f, "B_g_eval", None, dt) for dt in (torch.float64, torch.float32)}


def test_inputs_pinned(g, train64):
    """X1 is cge, the conditions are the propagated modal views (not normalised), the prior is the centred sum."""
    X1, cond, prior = RL.rf_inputs_ref(train64, U)
    assert g["B_X1"].shape == g["B_prior"].shape == (N, 64) and g["B_cond"].shape == (N, 128)
    np.testing.assert_allclose(g["B_X1"], X1.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_cond"], cond.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_prior"], prior.numpy(), rtol=1e-5, atol=2e-6)
    assert np.abs(np.linalg.norm(g["B_cond"][:, :64], axis=1) - 1).min() > 1e-3   # not the normalised views
    assert np.abs(g["B_cond"][:U]).max() > 1e-3 and np.abs(g["B_prior"][:U]).max() > 1e-3   # dense user rows
    # from the recorded views alone: the fp32 roundings of the reference (one sum, the mean's division and the
    # subtraction: three; the sum of at most 41 rows adds less than one more) at the magnitude of Z
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    a, b = t64(g["B_cond"][:, :64]), t64(g["B_cond"][:, 64:])
    want = RL.prior_ref(a, b, U).numpy()
    zmax = float((a + b).abs().max())
    err = np.abs(g["B_prior"] - want)
    print(f"prior: max abs error {err.max():.3e}, max |Z| {zmax:.3e}, atol {4 * 2.0 ** -24 * zmax:.3e}")
    assert (err <= 1e-5 * np.abs(want) + 4 * 2.0 ** -24 * zmax).all()
    for seg in (slice(0, U), slice(U, N)):
        assert np.abs(g["B_prior"][seg].astype(np.float64).mean(0)).max() < 1e-6   # each segment centred on its own
    z = (a + b).numpy()
    assert np.abs(g["B_prior"] - (z - z.mean(0))).max() > 1e-3    # one mean over all N rows would be another table
    assert np.abs(g["B_prior"] - 0.5 * want).max() > 1e-3         # and so would RFMGCN's mean of the views


def test_prior_ref_segments():
    one = torch.tensor([[3.0] * 64, [-5.0] * 64], dtype=torch.float64)
    assert not RL.prior_ref(one, 2 * one, 1).any()
    rng = np.random.default_rng(0)
    a = torch.tensor(np.concatenate([100 + rng.standard_normal((5, 64)), -100 + rng.standard_normal((3, 64))]))
    p = RL.prior_ref(a, a, 5)
    assert float(p.abs().max()) < 10 and float(p[:5].mean(0).abs().max()) < 1e-12
    import rfmgcn_fixture as RM
    assert torch.allclose(p, 2 * RM.prior_ref(a, a, 5), rtol=1e-12, atol=1e-12)   # the sum: twice RFMGCN's mean


def test_train_step_pinned(g):
    """The generator's step on the recorded inputs and draws at C = 128: v and pred at test_rfsmore_cpu.py's bars, the
    losses at 1e-5 relative, the velocity gradients within 4 x the stored err_grad of the parameter's largest entry."""
    r, grads = RB.record_losses(g, "B_", L)
    np.testing.assert_allclose(r["v"].detach().numpy(), g["B_v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["pred"].detach().numpy(), g["B_pred"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["rf_loss"].item(), g["B_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["cl_loss"].item(), g["B_cl_loss"], rtol=1e-5)
    bar = R.grad_bar(g, "B_")
    assert sum(v.numel() for v in grads.values()) == RL.N_PARAMS
    assert g["B_p0_condition_encoder_0_weight"].shape == (128, 128)
    for n, v in grads.items():
        err = R.rel_to_max(v.numpy(), g["B_g_" + R.key(n)])
        assert err <= bar, (n, err, bar)
    r64, g64 = RB.record_losses(g, "B_", L, dtype=torch.float64)
    np.testing.assert_allclose(r64["rf_loss"].item(), g["B_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r64["cl_loss"].item(), g["B_cl_loss"], rtol=1e-5)
    for n, v in g64.items():
        assert R.rel_to_max(g["B_g_" + R.key(n)], v.numpy()) <= bar, n
    # the prior term is in the record: without it v is another table, on the user rows too
    X1, X0, t, cond, users, pos, ni, nu, prior = RB.record_inputs(g, "B_")
    bare = R.train_losses(R.params_from(g, "B_", L), X1, X0, t, cond, users, pos, ni, nu, U, L)
    assert np.abs(bare["v"].numpy() - g["B_v"])[:U].max() > 1e-3
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
    z = R.generate(P, torch.tensor(g["B_cond_eval"]), z0, steps, L)
    np.testing.assert_allclose(z.numpy(), g["B_gen_eval"], rtol=0, atol=4 * float(g["B_err_sample"]))
    assert np.array_equal(g["B_cond_eval"], g["B_cond"])   # no dropout reaches mge: the same conditions


def test_evaluation_mixes_before_the_hypergraph_block(g, f, evals):
    """Before warm-up the table is LGMRec's.  After it, the golden all is the forward from the hypergraph block on
    cge' = cge + ratio gen: the fp64 restatement meets it at rtol 1e-5 next to twice the fp32 restatement's own error
    on the same chain; the restatement that mixes into all instead (the RFMGCN rule) misses it by far more."""
    ratio, steps = float(g["ratio"]), int(g["steps"])
    VP1 = {n: g["B_p1_" + R.key(n)] for n in R.param_names(L)}
    c = dict(F.CASES["B"])
    fw64, fw32 = evals[torch.float64], evals[torch.float32]
    np.testing.assert_allclose(g["B_all_pre"], fw64["all"].numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(g["B_cge_eval"], fw64["cge"].numpy(), rtol=1e-5, atol=2e-6)
    pre = g["B_all_pre"].astype(np.float64)
    np.testing.assert_allclose(pre[:U] @ pre[U:].T, g["B_scores_pre"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(g["B_scores_pre"], f["B_scores"], rtol=1e-5, atol=1e-4)   # LGMRec's own golden scores
    e64 = RL.eval_ref(fw64, VP1, g["B_z0"], U, c, steps, L, ratio)
    e32 = RL.eval_ref(fw32, VP1, g["B_z0"], U, c, steps, L, ratio)
    for k, gk in (("gen", "B_gen_eval"), ("cgemix", "B_cgemix_eval"), ("all", "B_eval")):
        want = e64[k].numpy()
        own = float(np.abs(e32[k].numpy().astype(np.float64) - want).max())
        err = float(np.abs(g[gk] - want).max())
        print(f"{k}: golden against fp64 {err:.3e} (fp32 restatement {own:.3e})")
        np.testing.assert_allclose(g[gk], want, rtol=1e-5, atol=2 * own, err_msg=k)
    np.testing.assert_allclose(g["B_cgemix_eval"], g["B_cge_eval"] + ratio * g["B_gen_eval"], rtol=0, atol=1e-6)
    ev = g["B_eval"].astype(np.float64)
    np.testing.assert_allclose(ev[:U] @ ev[U:].T, g["B_scores_mix"], rtol=1e-5, atol=1e-4)
    # the wrong model: all + ratio gen
    late = RL.eval_ref(fw64, VP1, g["B_z0"], U, c, steps, L, ratio, rule="all")["all"].numpy()
    own = float(np.abs(e32["all"].numpy().astype(np.float64) - e64["all"].numpy()).max())
    miss = np.abs(g["B_eval"] - late)
    print(f"mixing into all instead misses the golden table by {miss.max():.3e} (bar {2 * own:.3e} + 1e-5 |x|)")
    assert (miss > 1e-5 * np.abs(late) + 2 * own).mean() > 0.9 and miss.max() > 1e-2
    assert float(g["B_late_mix_gap"]) > 1e-2 and float(g["B_score_shift"]) > 1.0
    # the user rows move too, through cge' itself and through lat from cge'[U:]
    moved = np.abs(g["B_eval"] - g["B_all_pre"])
    assert moved[:U].max() > 0.05 and moved[U:].max() > 0.05


def test_registry_and_yaml():
    from gmr.configurator import Config
    from gmr.lgmrec import LGMRec
    from gmr.rf import RFBackbone
    from gmr.rflgmrec import RFLGMRec
    from gmr.utils import get_model
    assert get_model("RFLGMRec") is RFLGMRec and issubclass(RFLGMRec, LGMRec) and issubclass(RFLGMRec, RFBackbone)
    assert RFLGMRec.rf_condition_dim(None) == 128
    cfg = Config("RFLGMRec", "baby", {"synthetic": "tiny"})
    base = Config("LGMRec", "baby", {"synthetic": "tiny"})
    for k in ("embedding_size", "feat_embed_dim", "cf_model", "n_ui_layers", "n_mm_layers", "n_hyper_layer",
              "hyper_num", "keep_rate", "alpha", "cl_weight", "reg_weight", "learning_rate", "learning_rate_scheduler"):
        assert cfg[k] == base[k], k
    assert cfg["use_rf"] is True and cfg["use_denoise"] is False and cfg["use_2rf"] is False
    assert (cfg["rf_hidden_dim"], cfg["rf_n_layers"], cfg["rf_loss_weight"], cfg["rf_infonce_negatives"]) == \
        (128, 2, 0.2, 1024)
    assert (cfg["rf_sampling_steps"], cfg["rf_warmup_epochs"], cfg["rf_inference_mix_ratio"]) == (5, 20, 0.05)
    assert (cfg["rf_learning_rate"], cfg["rf_contrast_temp"], cfg["rf_dropout"]) == (0.0003, 0.1, 0.1)
    assert cfg["use_wandb"] is None and cfg["wandb_project"] is None


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(over, key):
    from gmr.rf import check_config
    check_config(RL.rflgmrec_config())
    with pytest.raises(NotImplementedError, match=key):
        check_config(RL.rflgmrec_config(**over))


def test_signatures_name_the_new_entries():
    from gmr import _lib
    for name in ("gmr_rf_sample_mix", "gmr_rf_view_sum_prior", "gmr_rf_view_sum_prior_ws_floats"):
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gmr_rf_view_sum_prior"] == _lib.SIGNATURES["gmr_rf_view_prior"]
