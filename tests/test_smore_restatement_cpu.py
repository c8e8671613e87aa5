"""The plain torch restatement of SMORE (tests/smore_fixture.py: real cosine / sine matrices, no torch.fft) at fp64
against the values the reference gave when rerun in double (tests/golden/smore_tiny.npz, smore_tiny_B.npz), so that
the GPU tests may use it where the reference recorded nothing; its spectrum step against torch.fft's autograd; and the
registry, the config file and check_config, which need no GPU."""
import numpy as np
import pytest
import torch

import smore_fixture as F


@pytest.fixture(scope="module")
def g(golden):
    return dict(golden("smore_tiny"), **golden("smore_tiny_B"))


@pytest.fixture(scope="module")
def refs(g):
    out = {}
    for case, c in F.CASES.items():
        keep = F.golden_keep(g) if case == "B" else None
        out[case] = F.smore_step_ref(F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"],
                                     g["train_cols"], g["users"], g["pos"], g["neg"], c["n_layers"], c["cl_loss"],
                                     (g["v_feat"], g["t_feat"]), keep=keep, p=c["dropout_rate"])
    return out


def test_golden_data_has_the_edge_cases(g):
    assert int(g["n_isolated"]) >= 1                      # items without an edge: empty rows of adj
    assert len(set(g["users"].tolist())) < g["users"].size and len(set(g["pos"].tolist())) < g["pos"].size
    assert np.array_equal(g["init_image_embedding_weight"], g["v_feat"])
    assert len(F.PARAMS) == 29 and [g["init_" + k].shape for k in F.FILTERS] == [(1, 33, 2)] * 3
    keep = g["B_keep"]
    assert keep.shape == (F.ADAM_STEPS, int(g["U"]) + int(g["I"]), 192) and set(np.unique(keep)) == {0, 1}
    assert not np.array_equal(keep[0], keep[1]) and not np.array_equal(keep[0, :, :64], keep[0, :, 64:128])


def test_graphs(g, refs):
    U, I = int(g["U"]), int(g["I"])
    r = refs["A"]
    for k, shape in (("adj", (U + I, U + I)), ("image_adj", (I, I)), ("text_adj", (I, I)), ("fusion_adj", (I, I))):
        want = F.dense_of(g[k + "_idx"], g[k + "_val"], shape)
        assert np.array_equal(want != 0, r[k] != 0), k
        np.testing.assert_allclose(r[k], want, rtol=2e-6, atol=0, err_msg=k)
    # the fusion graph: the union of the patterns, the larger value where both graphs hold an entry
    av, at, af = (F.dense_of(g[k + "_idx"], g[k + "_val"], (I, I)) for k in ("image_adj", "text_adj", "fusion_adj"))
    both, off = (av != 0) & (at != 0), ~np.eye(I, dtype=bool)
    assert np.array_equal(af != 0, (av != 0) | (at != 0))
    assert np.array_equal(af[both], np.maximum(av, at)[both]) and np.array_equal(af[~both], (av + at)[~both])
    assert (both & off).any(1).sum() >= 3 and ((av != 0) ^ (at != 0)).any(1).sum() >= 3
    assert (av != 0).sum(1).max() == F.IMAGE_K and (at != 0).sum(1).max() == F.TEXT_K


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_reproduces_the_reference(g, refs, case):
    r, tag = refs[case], case + "_"
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-9)
    np.testing.assert_allclose(r["terms"], g[tag + "loss_terms"], rtol=1e-9)
    for k in ("c", "side"):
        np.testing.assert_allclose(r[k], g[tag + k], rtol=1e-9, atol=1e-12, err_msg=k)
    np.testing.assert_allclose(r["scores"], g[tag + "scores"], rtol=1e-9, atol=1e-12)
    for got, k in zip(r["grads"], F.PARAMS):
        want = g[tag + "g_" + k]
        print(f"{case} {k}: max error {np.abs(got - want).max():.3e}, largest gradient {np.abs(want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=k)
    # the reference's fp32 run is fp32-close to its double rerun
    np.testing.assert_allclose(g[tag + "loss32"], g[tag + "loss"], rtol=1e-6)
    np.testing.assert_allclose(g[tag + "scores32"], g[tag + "scores"], rtol=1e-4, atol=1e-5)


def test_filter_gradients_of_the_real_bins(g):
    """Im W_0 and Im W_32 of the three filters have no effect: their gradients are exactly 0 in the reference."""
    for case in "AB":
        for k in F.FILTERS:
            gr = g[f"{case}_g_{k}"].reshape(33, 2)
            assert gr[0, 1] == 0.0 and gr[32, 1] == 0.0 and np.abs(gr[1:32]).min() > 0


def test_case_b_gradients_are_large_enough_to_test(g):
    for k in F.PARAMS:
        assert np.abs(g["B_g_" + k]).max() > 5e-5, k


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 5e-6)])
def test_spectrum_step_against_torch_fft(dtype, tol):
    """The matrix form against torch.fft with autograd on random rows: the three outputs and the five gradients.  In
    fp64 the two agree to rounding; in fp32 the matrix form is as close to fp64 as torch.fft is."""
    rng = np.random.default_rng(5)
    data = [rng.standard_normal(s) for s in ((37, 64), (37, 64), (1, 33, 2), (1, 33, 2), (1, 33, 2))]
    cot = [torch.tensor(rng.standard_normal((37, 64)), dtype=dtype) for _ in range(3)]

    def run(fn, dt):
        x = [torch.tensor(d, dtype=dt, requires_grad=True) for d in data]
        out = fn(*x)[:3]
        sum((o * c.to(dt)).sum() for o, c in zip(out, cot)).backward()
        return [o.detach().double().numpy() for o in out] + [t.grad.double().numpy() for t in x]

    got, want = run(F.spectrum_ref, dtype), run(F.spectrum_fft, torch.float64)
    own = run(F.spectrum_fft, dtype)
    for a, b, o, k in zip(got, want, own, ("image_conv", "text_conv", "fusion_conv", "dV", "dT", "dWi", "dWt", "dWf")):
        scale = np.abs(b).max()
        print(f"{dtype} {k}: matrix form {np.abs(a - b).max() / scale:.2e}, torch.fft "
              f"{np.abs(o - b).max() / scale:.2e}")
        np.testing.assert_allclose(a, b, rtol=0, atol=tol * scale, err_msg=k)
    for k in (5, 6, 7):      # Im W_0, Im W_32: exactly 0 in both
        for r in (got[k], want[k]):
            assert r[0, 0, 1] == 0.0 and r[0, 32, 1] == 0.0


def test_spectrum_exact_cases():
    C, S, ck = F.trig()
    assert not S[0].any() and not S[32].any() and C[0].eq(0.125).all() and C[32].abs().eq(0.125).all()
    e0 = torch.zeros(1, 64, dtype=torch.float64)
    e0[0, 0] = 1
    re, im = F.rfft_ref(e0)
    assert re.eq(0.125).all() and not im.any()                    # an impulse: a flat spectrum of 1/8
    x = torch.tensor(np.random.default_rng(1).standard_normal((5, 64)))
    one = torch.tensor([[1.0, 0.0]] * 33, dtype=torch.float64)
    ic, tc, fc, _ = F.spectrum_ref(x, torch.zeros_like(x), one, one, one)
    np.testing.assert_allclose(ic.numpy(), x.numpy(), rtol=0, atol=1e-14)   # W = 1: the identity
    assert not tc.any() and not fc.any()                          # a zero T: no text and no fusion signal


def test_trajectory_of_the_restatement_is_fp32_close_to_the_reference(g):
    c = F.CASES["B"]
    traj, _ = F.trajectory(F.case_params(g, "B"), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"],
                           g["users"], g["pos"], g["neg"], c["n_layers"], c["cl_loss"], (g["v_feat"], g["t_feat"]),
                           g["B_keep"], c["dropout_rate"])
    for k in F.PARAMS:
        want = g[f"traj{F.ADAM_STEPS}_{k}"]
        # three Adam steps move an entry by at most 3 lr (1.1 lr each early on): the distance stays a fraction of it
        np.testing.assert_allclose(traj[-1][k], want, rtol=0, atol=1.5 * F.LR, err_msg=k)


def test_registry_and_config():
    from gmr.configurator import Config
    from gmr.trainer import Trainer
    from gmr.utils import get_model, get_trainer
    assert get_model("SMORE").__name__ == "SMORE"
    assert get_trainer("SMORE") is Trainer
    cfg = Config("SMORE", "baby")
    want = {"embedding_size": 64, "n_ui_layers": 4, "n_layers": 1, "image_knn_k": 40, "text_knn_k": 15,
            "reg_weight": 1e-4, "cl_loss": 0.01, "dropout_rate": 0.1, "learning_rate": 0.001,
            "learning_rate_scheduler": [0.96, 50], "temperature": 0.2, "lambda_coeff": 0.9}
    assert {k: cfg[k] for k in want} == want


@pytest.mark.parametrize("key,value,kw", [("embedding_size", 32, {}), ("n_ui_layers", 8, {}), ("image_knn_k", 42, {}),
                                          ("text_knn_k", 0, {}), ("dropout_rate", 1.0, {}), ("sparse", False, {}),
                                          ("image", None, {"has": (False, True)}),
                                          ("text", None, {"has": (True, False)})])
def test_check_config_names_the_key(key, value, kw):
    from gmr.smore import check_config
    cfg = F.smore_config(**({key: value} if value is not None else {}))
    assert check_config(F.smore_config(), n_items=41) == (2, 1, 5, 3, 0.0)
    with pytest.raises(NotImplementedError, match=key):
        check_config(cfg, n_items=41, **kw)


def test_world_size_two_raises(monkeypatch):
    from gmr import dist
    from gmr.smore import check_config
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        check_config(F.smore_config(), n_items=41)
