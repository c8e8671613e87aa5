"""RFFREEDOM (gmr/rffreedom.py) against the reference's golden values (tests/golden/make_golden_rffreedom.py, on the
data and the pruned graph of freedom_tiny.npz case A) and against FREEDOM itself."""
import numpy as np
import pytest
import torch

import rf_fixture as R
from freedom_fixture import DEV, PARAMS, build_freedom

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def f(golden):
    return golden("freedom_tiny")


@pytest.fixture(scope="module")
def g(golden):
    return R.load_golden(golden)


def _batch(f):
    return [torch.as_tensor(f[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _model(f, g=None, prefix="p0_", **over):
    m, cfg, ds, tl = R.build_rffreedom(f, **over)
    m.prune_edges(keep_idx=torch.as_tensor(f["degree_idx"]))
    if g is not None:
        m.rf_generator.load_reference_state({n: g["A_" + prefix + R.key(n)] for n in R.param_names(2)})
    return m


def test_registry():
    from gmr.rffreedom import RFFREEDOM
    from gmr.utils import get_model
    assert get_model("RFFREEDOM") is RFFREEDOM


def test_use_rf_false_is_freedom(f):
    a = _model(f, use_rf=False)
    b, *_ = build_freedom(f, "A")
    b.prune_edges(keep_idx=torch.as_tensor(f["degree_idx"]))
    assert a.rf_generator is None
    la, lb = a.rec_step(*_batch(f)), b.rec_step(*_batch(f))
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, b.slab.grad)
    users = torch.arange(a.n_users, device=DEV)
    assert torch.equal(a.full_sort_predict([users]), b.full_sort_predict([users]))
    assert a.extra_state() == b.extra_state()


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(f, over, key):
    with pytest.raises(NotImplementedError, match=key):
        R.build_rffreedom(f, **over)


def test_step_parity(f, g):
    m = _model(f, g)
    assert m._training_epoch == -1
    m.pre_epoch_processing()  # draws a graph of its own; the reference's is installed again below
    m.prune_edges(keep_idx=torch.as_tensor(f["degree_idx"]))
    assert m._training_epoch == 0 and m.rf_generator.epoch == 0
    b, *_ = build_freedom(f, "A")
    b.prune_edges(keep_idx=torch.as_tensor(f["degree_idx"]))
    want_loss = b.rec_step(*_batch(f))
    loss = m.rec_step(*_batch(f), rf_draws=R.draws(g, "A_"))
    # FREEDOM's loss and its eight gradients: FREEDOM's, bit for bit, and the reference's
    assert torch.equal(loss, want_loss) and torch.equal(m.slab.grad, b.slab.grad)
    np.testing.assert_allclose(loss.item(), f["A_loss"], rtol=1e-5)
    for v, k in zip(m.grad_views(), PARAMS):
        if not k.endswith("_bias"):
            want = f["A_g_" + k]
            np.testing.assert_allclose(v.cpu().numpy(), want, rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=k)
    # the RF step saw the reference's target and conditions
    np.testing.assert_allclose(m._x1.cpu().numpy(), g["A_X1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m.rf_conditions().cpu().numpy(), g["A_cond"], rtol=1e-5, atol=1e-6)
    terms = m.rf_loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], g["A_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1], g["A_cl_loss"], rtol=1e-5)
    bar = R.grad_bar(g, "A_")
    for (name, _), got in zip(m.rf_generator.specs, m.rf_generator.grad_views()):
        want = g["A_g_" + R.key(name)]
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=bar * np.abs(want).max(), err_msg=name)
    assert m.extra_state() == {"epoch_ctr": m._epoch, "rf_epoch": 0, "rf_step": 1}


def test_predict(f, g):
    m = _model(f, g, prefix="p1_", rf_warmup_epochs=1)
    users = torch.arange(m.n_users, device=DEV)
    b, *_ = build_freedom(f, "A")
    m._training_epoch = 0
    m.rf_generator.set_epoch(0)  # before warm-up: FREEDOM's scores
    pre = m.full_sort_predict([users])
    assert torch.equal(pre, b.full_sort_predict([users]))
    np.testing.assert_allclose(pre.cpu().numpy(), g["A_scores_pre"], rtol=1e-5, atol=1e-5)
    m.rf_generator.set_epoch(1)  # warmed up: + 0.2 generate(cond) with the recorded start noise
    z0 = torch.as_tensor(g["A_z0"]).to(DEV)
    mix = m.full_sort_predict([users], z0=z0)
    np.testing.assert_allclose(m._gen.cpu().numpy(), g["A_gen"], rtol=0, atol=4 * float(g["A_err_sample"]))
    np.testing.assert_allclose(mix.cpu().numpy(), g["A_scores_mix"], rtol=1e-5, atol=1e-5)
    # Philox start noise: deterministic at a given step counter, finite, and another table than FREEDOM's
    s1, s2 = m.full_sort_predict([users]).clone(), m.full_sort_predict([users])
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all()) and not torch.equal(s1, pre)


def test_quick_start(tmp_path, monkeypatch):
    """quick_start("RFFREEDOM", "baby", ...) on the tiny synthetic shape with configs/model/RFFREEDOM.yaml (dropout
    0.1, 1,024 Philox negatives per anchor): two epochs, the metric keys, and a checkpoint that holds the velocity
    parameters, the AdamW moments and the RF counters as plain ints."""
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False,
                "rf_warmup_epochs": 1}
    results = quick_start("RFFREEDOM", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("RFFREEDOM", "baby", dict(cfg_dict))
    assert cfg["use_rf"] is True and cfg["use_denoise"] is False and cfg["rf_hidden_dim"] == 128
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "RFFREEDOM-baby.pth"), map_location="cpu", weights_only=True)
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(ck["state_dict"])
    gg = ck["generated_graphs"]
    assert gg["rf_epoch"] == ck["epoch"] and gg["rf_step"] > 0 and type(gg["rf_step"]) is int


def _fit_setup(f, **over):
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.trainer import Trainer
    U, I = int(f["U"]), int(f["I"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(U), 6)
    cols = np.concatenate([rng.choice(I, 6, replace=False) for _ in range(U)])
    labels = np.zeros(rows.size)
    labels[4::6] = 1
    labels[5::6] = 2
    m, cfg, ds, _ = R.build_rffreedom(f, rows, cols, labels, rf_dropout=0.1, rf_warmup_epochs=1, **over)
    tr, va, te = ds.split()
    return cfg, tr, va, TrainDataLoader, EvalDataLoader, Trainer


def test_fit_and_evaluate(f):
    """Two epochs through the generic Trainer (the path of main.py --model RFFREEDOM): construction, train steps with
    Philox draws, and evaluation before and after warm-up."""
    from gmr.rffreedom import RFFREEDOM
    cfg, tr, va, TrainDataLoader, EvalDataLoader, Trainer = _fit_setup(f)
    tl = TrainDataLoader(cfg, tr, batch_size=16)
    m = RFFREEDOM(cfg, tl)
    cfg["epochs"] = 2
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=16)
    p0 = m.rf_generator.slab.data.clone()
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    assert np.isfinite(trainer.train_loss_dict[0]) and np.isfinite(trainer.train_loss_dict[1])
    assert "recall@10" in valid
    gen = m.rf_generator
    assert m._training_epoch == 1 and gen.warmed_up() and gen.step_ctr > 0
    assert bool(torch.isfinite(m.rf_loss_terms()).all()) and not torch.equal(gen.slab.data, p0)
    res = trainer.evaluate(vl)
    assert all(np.isfinite(v) for v in res.values())
    sd = m.state_dict()
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(sd)
