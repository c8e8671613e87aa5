"""The torch restatement of DDRM in tests/ddrm_fixture.py against the values the reference recorded
(tests/golden/ddrm_tiny.npz): it pins the restatement, so the GPU tests can use its fp64 mode at shapes the fixture
does not have.  Also the host-side pieces of gmr/ddrm.py: the seeded construction and the fp64 schedule."""
import numpy as np
import pytest
import torch

import ddrm_fixture as F


@pytest.fixture(scope="module")
def g():
    return F.load_golden()


def _sched(g):
    return {k: g["sch_" + k] for k in F.TABLES}


def test_model_is_registered():
    from gmr.utils import get_model
    assert get_model("DDRM").__name__ == "DDRM"


def test_construction_bit_exact(g):
    from gmr.utils import get_model  # noqa: F401  (DDRM is registered)
    from gmr.ddrm import init_parameters
    assert list(g["param_names"]) == F.param_names()
    torch.manual_seed(3)
    got = init_parameters(int(g["U"]), int(g["I"]), int(g["H"]))
    assert len(got) == len(F.param_names())
    for n, v in zip(F.param_names(), got):
        np.testing.assert_array_equal(v.numpy(), g["p_" + F.key(n)], err_msg=n)


def test_schedule_tables(g):
    from gmr.ddrm import ddrm_schedule
    for tabs in (F.schedule_ref(100, 1e-4, 5e-4, 5e-3), ddrm_schedule(100, 1e-4, 5e-4, 5e-3)):
        for k in F.TABLES:
            assert tabs[k].dtype == np.float64
            np.testing.assert_allclose(tabs[k], g["sch_" + k], rtol=1e-12, atol=0, err_msg=k)
    s = _sched(g)
    assert s["betas"][0] == 1e-5 and abs(s["betas"][1] - 4.5455e-9) < 1e-12
    assert s["posterior_log_variance_clipped"][0] == s["posterior_log_variance_clipped"][1]


def _step(g, dtype):
    P = {k[2:]: v for k, v in g.items() if k.startswith("p_")}
    return F.step_ref(P, int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["pos"], g["neg"],
                      g["t"], g["noise_u"], g["noise_i"], g["keep_u"], g["keep_i"], _sched(g), dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_step_matches_reference(g, dtype):
    from gmr.utils import get_model
    get_model("DDRM")
    t = g["t"]
    assert t.min() == 0 and t.max() == 99 and len(np.unique(t)) < len(t)
    r = _step(g, dtype)
    np.testing.assert_allclose(r["loss"], g["loss"], rtol=1e-5)
    np.testing.assert_allclose(r["w"], g["row_w"], rtol=1e-5)
    np.testing.assert_allclose(r["sp"], g["row_sp"], rtol=1e-5)
    np.testing.assert_allclose(r["rec"], g["row_rec"], rtol=1e-5)
    names = F.param_names()
    F.check_grads(r["grads"], [g["g_" + F.key(n)] for n in names], names, show=str(dtype))


@pytest.mark.parametrize("name,S,noisy", [("s0", 0, False), ("s3", 3, False), ("s3n", 3, True)])
def test_scores_match_reference(g, name, S, noisy):
    from gmr.utils import get_model
    get_model("DDRM")
    P = {k[2:]: v for k, v in g.items() if k.startswith("p_")}
    sc, _, _ = F.predict_ref(P, int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["noise_" + name], S,
                             _sched(g), step_noise=g["step_noise_s3n"] if noisy else None, dtype=torch.float64)
    want = g["scores_" + name]
    np.testing.assert_allclose(sc, want, rtol=0, atol=1e-5 * np.abs(want).max())
