"""The plain torch restatement of the BM3 step (tests/bm3_fixture.py::bm3_step_ref) pinned to the reference's golden
values (bm3_tiny.npz, cases A and B) at the bars of test_freedom_restatement_cpu.py: with it pinned, the GPU tests
may use its fp64 autograd where the reference recorded nothing (one modality, the mid shape).  Also the registry and
check_config, which need no device."""
import numpy as np
import pytest
import torch

from bm3_fixture import CASES, PARAMS, TERMS, bm3_step_ref, check_grads, golden_keep, params_of


@pytest.fixture(autouse=True)
def _feature():
    from gmr.utils import get_model
    get_model("BM3")  # the feature under test: raises ValueError without it


def _ref(g, case, **kw):
    c = CASES[case]
    return bm3_step_ref({k: g["p_" + k] for k in PARAMS}, int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"],
                        g["users"], g["items"], golden_keep(g, case), c["n_layers"], c["dropout"], **kw)


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_pinned(golden, case):
    g = golden("bm3_tiny")
    tag = case + "_"
    r = _ref(g, case, dtype=torch.float64)
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(r["terms"], g[tag + "loss_terms"], rtol=1e-5)
    np.testing.assert_allclose(r["reg"], g[tag + "reg"], rtol=1e-5)
    np.testing.assert_allclose(r["ua"], g[tag + "ua"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["ib"], g[tag + "ib"], rtol=1e-5, atol=1e-6)
    check_grads(r["grads"], [g[tag + "g_" + k] for k in PARAMS], show=f"{case} fp64")


def test_fixture_batch_repeats(golden):
    g = golden("bm3_tiny")
    assert np.bincount(g["users"]).max() >= 3 and np.bincount(g["items"]).max() >= 2
    assert np.array_equal(np.lexsort((g["train_cols"], g["train_rows"])), np.arange(g["train_rows"].size))
    for case, c in CASES.items():
        for k in "uitv":
            rate = g[f"{case}_keep_{k}"].mean()
            assert abs(rate - (1 - c["dropout"])) < 0.05, (case, k, rate)


@pytest.mark.parametrize("mod,gone", [("text", ("v", "vt")), ("image", ("t", "tv"))])
def test_one_modality_is_the_other_dropped_by_hand(golden, mod, gone):
    """A model without a modality computes what the two-modality one does with that modality's two terms left out."""
    g = golden("bm3_tiny")
    one = _ref(g, "A", mods=(mod,))
    both = _ref(g, "A", drop_terms=gone)
    np.testing.assert_allclose(one["loss"], both["loss"], rtol=1e-12)
    for k, a, b in zip(TERMS, one["terms"], both["terms"]):
        if k in gone:
            assert a == 0.0 and b != 0.0
        else:
            np.testing.assert_allclose(a, b, rtol=1e-12, err_msg=k)
    names = params_of((mod,))
    want = dict(zip(PARAMS, both["grads"]))
    for k, v in zip(names, one["grads"]):
        np.testing.assert_allclose(v, want[k], rtol=1e-10, atol=1e-14, err_msg=k)
    for k in set(PARAMS) - set(names):
        assert not np.any(want[k]), k  # the dropped modality's parameters get no gradient


def test_registry_resolves():
    from gmr.bm3 import BM3
    from gmr.utils import get_model
    assert get_model("BM3") is BM3


def test_check_config_names_the_key():
    from bm3_fixture import bm3_config
    from gmr.bm3 import check_config
    assert check_config(bm3_config()) == (1, 0.3)
    with pytest.raises(NotImplementedError, match="embedding_size"):
        check_config(bm3_config(embedding_size=32))
    with pytest.raises(NotImplementedError, match="n_layers"):
        check_config(bm3_config(n_layers=8))
    with pytest.raises(NotImplementedError, match="dropout"):
        check_config(bm3_config(dropout=1.0))
