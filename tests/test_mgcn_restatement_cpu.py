"""The plain torch restatement of MGCN (tests/mgcn_fixture.py) at fp64 against the values the reference recorded
(tests/golden/mgcn_tiny.npz), so that the GPU tests may use it where the reference recorded nothing; and the registry,
the config file and check_config, which need no GPU."""
import numpy as np
import pytest

import mgcn_fixture as F


@pytest.fixture(scope="module")
def g(golden):
    return golden("mgcn_tiny")


@pytest.fixture(scope="module")
def refs(g):
    out = {}
    for case, c in F.CASES.items():
        out[case] = F.mgcn_step_ref(F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"],
                                    g["users"], g["pos"], g["neg"], c["n_layers"], c["cl_loss"],
                                    feats=(g["v_feat"], g["t_feat"]))
    return out


def test_golden_data_has_the_edge_cases(g):
    assert int(g["n_isolated"]) >= 1                      # items without an edge: empty rows of adj
    assert len(set(g["users"].tolist())) < g["users"].size and len(set(g["pos"].tolist())) < g["pos"].size
    assert np.array_equal(g["init_image_embedding_weight"], g["v_feat"])


def test_graphs(g, refs):
    U, I = int(g["U"]), int(g["I"])
    r = refs["A"]
    for k, shape in (("adj", (U + I, U + I)), ("image_adj", (I, I)), ("text_adj", (I, I))):
        want = F.dense_of(g[k + "_idx"], g[k + "_val"], shape)
        assert np.array_equal(want != 0, r[k] != 0), k
        np.testing.assert_allclose(r[k], want, rtol=2e-6, atol=0, err_msg=k)
    np.testing.assert_allclose(r["adj"][:U, U:], F.dense_of(g["R_idx"], g["R_val"], (U, I)), rtol=2e-6, atol=0)
    assert not np.allclose(r["image_adj"], r["image_adj"].T)  # row sums on both ends: not symmetric


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_reproduces_the_reference(g, refs, case):
    r, tag = refs[case], case + "_"
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-6)
    np.testing.assert_allclose(r["terms"], g[tag + "loss_terms"], rtol=1e-6)
    for k in ("a", "b", "c", "side"):
        np.testing.assert_allclose(r[k], g[tag + k], rtol=1e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(r["all"], g[tag + "c"] + g[tag + "side"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(r["scores"], g[tag + "scores"], rtol=1e-5, atol=2e-6)
    F.check_grads(r["grads"], [g[tag + "g_" + k] for k in F.PARAMS], show=case)


def test_case_b_gradients_are_large_enough_to_test(g):
    for k in F.PARAMS:
        assert np.abs(g["B_g_" + k]).max() > 1e-4, k


def test_registry_and_config():
    from gmr.configurator import Config
    from gmr.trainer import Trainer
    from gmr.utils import get_model, get_trainer
    assert get_model("MGCN").__name__ == "MGCN"
    assert get_trainer("MGCN") is Trainer
    cfg = Config("MGCN", "baby")
    want = {"embedding_size": 64, "n_ui_layers": 2, "n_layers": 1, "knn_k": 10, "reg_weight": 1e-4, "cl_loss": 0.001,
            "learning_rate": 0.001, "learning_rate_scheduler": [0.96, 50], "lambda_coeff": 0.9}
    assert {k: cfg[k] for k in want} == want


@pytest.mark.parametrize("key,value,kw", [("embedding_size", 32, {}), ("n_ui_layers", 8, {}), ("knn_k", 42, {}),
                                          ("image", None, {"has": (False, True)}),
                                          ("text", None, {"has": (True, False)})])
def test_check_config_names_the_key(key, value, kw):
    from gmr.mgcn import check_config
    cfg = F.mgcn_config(**({key: value} if value is not None else {}))
    assert check_config(F.mgcn_config(), n_items=41) == (2, 1, 5)
    with pytest.raises(NotImplementedError, match=key):
        check_config(cfg, n_items=41, **kw)
