"""The plain torch restatement of GRCN (tests/grcn_fixture.py) at fp64 against the values the reference gave when rerun
in double (tests/golden/grcn_tiny.npz, grcn_tiny_B.npz), so that the GPU tests may use it where the reference recorded
nothing; its hand-written backward equations against autograd and the golden values; the init draw, the registry, the
config file and check_config, which need no GPU."""
import numpy as np
import pytest
import torch

import grcn_fixture as F


@pytest.fixture(scope="module")
def g(golden):
    return dict(golden("grcn_tiny"), **golden("grcn_tiny_B"))


def _args(g, case):
    cs = F.CASES[case]
    feats = (g["v_feat"], g["t_feat"] if "t" in cs["mods"] else None)
    return (F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["pos"],
            g["neg"], dict(cs), feats)


@pytest.fixture(scope="module")
def refs(g):
    return {case: F.grcn_step_ref(*_args(g, case)) for case in F.CASES}


@pytest.fixture(scope="module")
def hands(g):
    return {case: F.grcn_step_hand(*_args(g, case)) for case in F.CASES}


def test_golden_data_has_the_edge_cases(g):
    U, I = int(g["U"]), int(g["I"])
    assert len(set(g["train_rows"].tolist())) < U          # a user without items
    assert len(set(g["train_cols"].tolist())) < I          # an item without users
    assert len(set(g["users"].tolist())) < g["users"].size and len(set(g["pos"].tolist())) < g["pos"].size
    E = g["train_rows"].size
    assert g["A_alpha"].shape == (2 * E, 2) and g["C_alpha"].shape == (2 * E, 1)
    assert g["A_result"].shape == (U + I, 192) and g["C_result"].shape == (U + I, 128)
    assert g["A_result0"].shape == (U + I, 64)
    for case in F.CASES:                                   # the margins the maker asserted
        assert (g[case + "_margin"] >= 1e-3).all(), (case, g[case + "_margin"])


@pytest.mark.parametrize("case", list(F.CASES))
def test_margins_and_branches(g, case):
    """On the double restatement every directed edge keeps 1e-3 between the two modalities' values and between the
    winner and 0, and both branches of both selections are taken."""
    P, U, I, rows, cols, *_, cs, feats = _args(g, case)
    T, fe, (rows, cols, *_) = F._inputs(P, U, I, rows, cols, g["users"], g["pos"], g["neg"], feats,
                                        F.params_of(case), torch.float64, False)
    K = {}
    F.grcn_forward(T, fe, rows, cols, cs["n_layers"], K)
    val, arg = K["val"].numpy(), K["arg"].numpy()
    win = val.max(1)
    assert np.abs(win).min() >= 1e-3
    assert 0.1 < (win <= 0).mean() < 0.9
    if val.shape[1] == 2:
        assert np.abs(val[:, 0] - val[:, 1]).min() >= 1e-3
        assert 0.2 < (arg == 0).mean() < 0.8


@pytest.mark.parametrize("case", list(F.CASES))
@pytest.mark.parametrize("which", ["autograd", "hand"])
def test_restatement_reproduces_the_reference(g, refs, hands, case, which):
    r, tag = (refs if which == "autograd" else hands)[case], case + "_"
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-9)
    np.testing.assert_allclose(r["result"], g[tag + "result"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["alpha"], g[tag + "alpha"], rtol=1e-9, atol=1e-12)
    for got, k in zip(r["grads"], F.params_of(case)):
        want = g[tag + "g_" + k]
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("case", list(F.CASES))
def test_hand_backward_against_autograd(refs, hands, case):
    for got, want, k in zip(hands[case]["grads"], refs[case]["grads"], F.params_of(case)):
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=k)


@pytest.mark.parametrize("n_layers,routing", [(0, "reference"), (2, "reference"), (0, "items"), (1, "items"),
                                              (3, "items")])
def test_hand_backward_on_other_settings(g, n_layers, routing):
    args = list(_args(g, "A"))
    args[8] = dict(args[8], n_layers=n_layers, routing=routing)
    auto = F.grcn_step_ref(*args)["grads"]
    for got, want, k in zip(F.grcn_step_hand(*args)["grads"], auto, F.PARAMS):
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=k)


def test_fp32_distance_is_the_stored_one(g):
    """The stored distance of fp32 torch from the double rerun, per gradient, is of the size the fp32 restatement
    shows: the bar of the GPU tests is made of it."""
    for case in F.CASES:
        r32 = F.grcn_step_ref(*_args(g, case), dtype=torch.float32)
        for got, k in zip(r32["grads"], F.params_of(case)):
            own = float(g[f"{case}_own_{k}"])
            mine = float(np.abs(got.astype(np.float64) - g[f"{case}_g_{k}"]).max())
            print(f"{case} {k}: stored {own:.3e}, the fp32 restatement {mine:.3e}")
            assert 0 < 2 * own < 1e-4 * np.abs(g[f"{case}_g_{k}"]).max()
            assert mine < 1e-4 * np.abs(g[f"{case}_g_{k}"]).max()


def test_trajectory_reproduces_the_reference(g):
    traj, _ = F.trajectory(*_args(g, "B"))
    for k in F.PARAMS:
        want = g[f"traj{F.ADAM_STEPS}_{k}"]
        np.testing.assert_allclose(traj[-1][k], want, rtol=0, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("case", ["A", "C"])
def test_init_draw(g, case):
    """The constructor's draws under torch.manual_seed(3) are the reference's, bit for bit, under its names in its
    order, the table full_sort_predict reads before any step included."""
    from gmr.grcn import draw_init
    dims = [g["v_feat"].shape[1]] + ([g["t_feat"].shape[1]] if case == "A" else [])
    torch.manual_seed(3)
    init, result0 = draw_init(int(g["U"]), int(g["I"]), dims)
    assert list(init) == F.STATE_KEYS[:len(F.params_of(case))]
    for k, name in zip(F.params_of(case), init):
        assert np.array_equal(init[name].numpy(), g[f"{case}_init_{k}"]), name
    assert np.array_equal(result0.numpy(), g[case + "_result0"])


def test_registry_and_config():
    from gmr.configurator import Config
    from gmr.trainer import Trainer
    from gmr.utils import get_model, get_trainer
    assert get_model("GRCN").__name__ == "GRCN"
    assert get_trainer("GRCN") is Trainer
    cfg = Config("GRCN", "baby")
    want = {"embedding_size": 64, "latent_embedding": 64, "n_layers": 3, "learning_rate": 0.001}
    assert {k: cfg[k] for k in want} == want
    assert isinstance(cfg["reg_weight"], float)
    assert "reg_weight" in cfg["hyper_parameters"]


@pytest.mark.parametrize("key,value,kw", [("embedding_size", 32, {}), ("latent_embedding", 128, {}),
                                          ("n_layers", -1, {}), ("n_layers", 8, {}),
                                          ("text features alone", None, {"has": (False, True)})])
def test_check_config_names_the_key(key, value, kw):
    from gmr.grcn import check_config
    assert check_config(F.grcn_config()) == 3
    cfg = F.grcn_config(**({key: value} if value is not None else {}))
    with pytest.raises(ValueError, match=key):
        check_config(cfg, **kw)


def test_world_size_two_raises(monkeypatch):
    from gmr import dist
    from gmr.grcn import check_config
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        check_config(F.grcn_config())
