"""The plain torch restatement of LGMRec (tests/lgmrec_fixture.py) at fp64 against the values the reference gave when
rerun in double (tests/golden/lgmrec_tiny.npz, lgmrec_tiny_B.npz), so that the GPU tests may use it where the reference
recorded nothing; its hand-written backward equations against autograd; and the registry, the config file and
check_config, which need no GPU."""
import numpy as np
import pytest
import torch

import lgmrec_fixture as F


@pytest.fixture(scope="module")
def g(golden):
    return dict(golden("lgmrec_tiny"), **golden("lgmrec_tiny_B"))


def _args(g, case):
    return (F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["pos"],
            g["neg"], dict(F.CASES[case]), (g["v_feat"], g["t_feat"]), g[case + "_g"][0])


def _keep(g, case, step=0):
    return g["B_keep"][step] if case == "B" else None


@pytest.fixture(scope="module")
def refs(g):
    return {case: F.lgmrec_step_ref(*_args(g, case), keep=_keep(g, case), g_eval=g[case + "_g_eval"])
            for case in F.CASES}


def test_golden_data_has_the_edge_cases(g):
    U, I = int(g["U"]), int(g["I"])
    assert len(set(g["train_rows"].tolist())) < U          # a user without interactions
    assert len(set(g["train_cols"].tolist())) < I          # an item nobody touched
    assert len(set(g["users"].tolist())) < g["users"].size and len(set(g["pos"].tolist())) < g["pos"].size
    assert g["A_g"].shape == (1, 2, U + I, 4) and g["B_g"].shape == (F.ADAM_STEPS, 2, U + I, 5)
    keep = g["B_keep"]
    assert keep.shape == (F.ADAM_STEPS, 2, U + I, 5) and set(np.unique(keep)) == {0, 1}
    assert not np.array_equal(keep[0], keep[1]) and not np.array_equal(keep[0, 0], keep[0, 1])
    assert float(g["B_softmax_min"]) < 1e-30               # the underflow path is covered
    assert (keep[0].reshape(2 * (U + I), 5).sum(1) == 0).any()   # an all-dropped row: ghe's norm may be clamped


def test_graphs(g, refs):
    U, I = int(g["U"]), int(g["I"])
    r = refs["A"]
    want = F.dense_of(g["norm_adj_idx"], g["norm_adj_val"], (U + I, U + I))
    assert np.array_equal(want != 0, r["norm_adj"] != 0)
    assert np.array_equal(r["norm_adj"].astype(np.float32), want.astype(np.float32))
    assert np.array_equal(r["adj"], F.dense_of(g["adj_idx"], g["adj_val"], (U, I)))
    assert np.array_equal(r["inv_deg"].astype(np.float32), g["inv_deg"])
    assert g["inv_deg"].max() == np.float32(1e7)            # the empty user: 1 / (0 + 1e-7)


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_reproduces_the_reference(g, refs, case):
    r, tag = refs[case], case + "_"
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-9)
    np.testing.assert_allclose(r["terms"], g[tag + "loss_terms"], rtol=1e-9)
    np.testing.assert_allclose(r["all"], g[tag + "all"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["x"], g[tag + "x"], rtol=1e-9, atol=1e-12)
    for got, k in zip(r["grads"], F.PARAMS):
        want = g[tag + "g_" + k]
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=k)
    np.testing.assert_allclose(r["scores"], g[tag + "scores"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("case", ["A", "B"])
def test_hand_backward_against_autograd(g, refs, case):
    hand = F.lgmrec_step_hand(*_args(g, case), keep=_keep(g, case))
    for got, want, k in zip(hand, refs[case]["grads"], F.PARAMS):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("over", [dict(cf_model="mf"), dict(n_mm_layers=0, n_ui_layers=0), dict(n_hyper_layer=3)])
def test_hand_backward_on_other_settings(g, over):
    args = list(_args(g, "B"))
    args[8] = dict(args[8], **over)
    auto = F.lgmrec_step_ref(*args, keep=_keep(g, "B"))["grads"]
    for got, want, k in zip(F.lgmrec_step_hand(*args, keep=_keep(g, "B")), auto, F.PARAMS):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max(), err_msg=k)


def test_fp32_distance_is_the_stored_one(g):
    """The stored distance of fp32 torch from the double rerun, per gradient, is of the size the fp32 restatement
    shows: the bar of the GPU tests is made of it."""
    for case in F.CASES:
        r32 = F.lgmrec_step_ref(*_args(g, case), keep=_keep(g, case), dtype=torch.float32)
        for got, k in zip(r32["grads"], F.PARAMS):
            own = float(g[f"{case}_own_{k}"])
            mine = float(np.abs(got.astype(np.float64) - g[f"{case}_g_{k}"]).max())
            print(f"{case} {k}: stored {own:.3e}, the fp32 restatement {mine:.3e}")
            # twice fp32 torch's own error stays far below the gradient's largest entry: the bar can tell a wrong
            # gradient from a right one
            assert 0 < 2 * own < 1e-4 * np.abs(g[f"{case}_g_{k}"]).max()
            assert mine < 1e-4 * np.abs(g[f"{case}_g_{k}"]).max()


def test_trajectory_reproduces_the_reference(g):
    args = _args(g, "B")
    traj, _ = F.trajectory(*args[:10], g["B_g"], g["B_keep"])
    for k in F.PARAMS:
        want = g[f"traj{F.ADAM_STEPS}_{k}"]
        np.testing.assert_allclose(traj[-1][k], want, rtol=0, atol=1.5 * F.LR, err_msg=k)


def test_registry_and_config():
    from gmr.configurator import Config
    from gmr.trainer import Trainer
    from gmr.utils import get_model, get_trainer
    assert get_model("LGMRec").__name__ == "LGMRec"
    assert get_trainer("LGMRec") is Trainer
    cfg = Config("LGMRec", "baby")
    want = {"embedding_size": 64, "feat_embed_dim": 64, "cf_model": "lightgcn", "n_ui_layers": 2, "n_mm_layers": 2,
            "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 0.5, "alpha": 0.3, "cl_weight": 1e-4, "reg_weight": 1e-6}
    assert {k: cfg[k] for k in want} == want
    assert set(cfg["hyper_parameters"]) >= {"n_ui_layers", "n_mm_layers", "n_hyper_layer", "hyper_num", "keep_rate",
                                            "alpha", "cl_weight", "reg_weight"}


@pytest.mark.parametrize("key,value,kw", [("embedding_size", 32, {}), ("feat_embed_dim", 32, {}), ("cf_model", "ngcf", {}),
                                          ("n_ui_layers", 8, {}), ("n_hyper_layer", 0, {}), ("hyper_num", 65, {}),
                                          ("hyper_num", 0, {}), ("keep_rate", 0.0, {}),
                                          ("image", None, {"has": (False, True)}),
                                          ("text", None, {"has": (True, False)})])
def test_check_config_names_the_key(key, value, kw):
    from gmr.lgmrec import check_config
    assert check_config(F.lgmrec_config()) == ("lightgcn", 2, 2, 1, 4, 1.0)
    cfg = F.lgmrec_config(**({key: value} if value is not None else {}))
    with pytest.raises(NotImplementedError, match=key):
        check_config(cfg, **kw)


def test_world_size_two_raises(monkeypatch):
    from gmr import dist
    from gmr.lgmrec import check_config
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        check_config(F.lgmrec_config())
