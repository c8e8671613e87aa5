"""The plain-torch restatement of LD4MRec (tests/ld4m_fixture.py) against the values the reference recorded
(tests/golden/ld4mrec_tiny.npz), in fp32 on the CPU; the registry, the yaml and the unsupported settings."""
import numpy as np
import pytest
import torch

import ld4m_fixture as F

L = 2


@pytest.fixture(scope="module")
def g():
    return F.load_golden()


def _P(g):
    return {F.key(n): g["p_" + F.key(n)] for n in F.param_names(L)}


def _step(g, tag, dtype):
    masks = g["d1_masks"] if tag == "d1_" else None
    return F.ld4_step_ref(_P(g), L, int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["t"],
                          g["noise"], g["alpha_bar"], g["user_svd_emb"], g["user_mm_emb"], masks=masks,
                          p_keep=0.9 if masks is not None else 1.0, hist=np.ones(int(g["T"]), np.float32),
                          dtype=dtype)


def test_fixture_layout(g):
    assert list(g["param_names"]) == F.param_names(L)
    assert np.unique(g["users"], return_counts=True)[1].max() >= 3
    assert np.unique(g["t"], return_counts=True)[1].max() >= 3
    assert g["d1_masks"].shape == (L, 16, 64)
    assert np.all(g["d0_g_t_in"] == 0) and np.all(g["p_t_in"] == 0)


def test_schedule_and_tables(g):
    np.testing.assert_array_equal(F.schedule_ref(int(g["T"]), 0.001).numpy(), g["alpha_bar"])
    feats = np.concatenate([g["v_feat"], g["t_feat"]], 1)
    mm = F.user_mm_ref(int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], feats).numpy()
    np.testing.assert_allclose(mm, g["user_mm_emb"], rtol=1e-5, atol=1e-5 * np.abs(mm).max())
    from gmr.ld4mrec import ld4_schedule
    np.testing.assert_array_equal(ld4_schedule(int(g["T"]), 0.001).numpy(), g["alpha_bar"])


@pytest.mark.parametrize("tag", ["d0_", "d1_"])
def test_step_fp32(g, tag):
    r = _step(g, tag, torch.float32)
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(r["rows"], g[tag + "row_loss"], rtol=1e-5)
    names = F.param_names(L)
    F.check_grads(r["grads"], [g[tag + "g_" + F.key(n)] for n in names], names)
    np.testing.assert_allclose(r["hist"], g[tag + "loss_history"], rtol=1e-6)


def test_history_order_matters(g):
    """The rows that share a t compound in batch order: reversing them changes the entry."""
    t, rows = g["t"], g["d0_row_loss"].astype(np.float64) * np.linspace(1, 10, 16)
    a = F.history_ref(np.ones(100, np.float32), t, rows)
    b = F.history_ref(np.ones(100, np.float32), t[::-1], rows[::-1])
    assert np.abs(a - b).max() > 1e-4


@pytest.mark.parametrize("name,t_in", [("scores_t0", None), ("scores_tneg", -0.37)])
def test_predict_fp32(g, name, t_in):
    U = int(g["U"])
    s = F.ld4_predict_ref(_P(g), L, U, int(g["I"]), g["train_rows"], g["train_cols"], np.arange(U),
                          g["user_svd_emb"], g["user_mm_emb"], t_in=t_in, dtype=torch.float32)
    np.testing.assert_allclose(s, g[name], rtol=1e-4, atol=1e-5)


def test_registry_and_yaml():
    from gmr.utils import get_model, get_trainer
    from gmr import trainer
    assert get_model("LD4MRec").__name__ == "LD4MRec"
    assert get_trainer("LD4MRec") is trainer.Trainer
    from gmr.configurator import Config
    c = Config("LD4MRec", "baby", {})
    assert (c["cnet_hidden_size"], c["cnet_n_layers"], c["svd_k"], c["steps"]) == (256, 3, 64, 100)
    assert (c["dropout"], c["smoothing_gamma"], c["min_noise_level"], c["learning_rate"]) == (0.1, 0.1, 0.001, 0.001)


@pytest.mark.parametrize("over,word", [({"cnet_hidden_size": 100}, "cnet_hidden_size"),
                                       ({"cnet_hidden_size": 2048}, "cnet_hidden_size"),
                                       ({"cnet_n_layers": 0}, "cnet_n_layers"), ({"cnet_n_layers": 9}, "cnet_n_layers"),
                                       ({"steps": 2000}, "steps"), ({"svd_k": 37}, "svd_k"),
                                       ({"embedding_size": 32}, "embedding_size")])
def test_unsupported_settings_name_the_key(over, word):
    from gmr.ld4mrec import check_config
    with pytest.raises(NotImplementedError, match=word):
        check_config(F.ld4_config(**over), 37, 41)
    check_config(F.ld4_config(), 37, 41)
