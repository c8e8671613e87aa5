"""RFBM3 (gmr/rfbm3.py) against the reference's golden values (tests/golden/make_golden_rfbm3.py, on the data and
seed of bm3_tiny.npz) with its dropout masks and RF draws injected, against the BM3 class itself, and, where the
reference recorded nothing (one modality, the mid shape), against the fp64 restatement of tests/rfbm3_fixture.py,
which tests/test_rfbm3_cpu.py pins to the same golden values."""
import numpy as np
import pytest
import torch

import bm3_fixture as B
import rf_fixture as R
import rfbm3_fixture as RB

pytestmark = pytest.mark.gpu
DEV = B.DEV


@pytest.fixture(scope="module")
def b(golden):
    return golden("bm3_tiny")


@pytest.fixture(scope="module")
def g(golden):
    return RB.load_golden(golden)


def _batch(b):
    return [torch.as_tensor(b[k].astype(np.int32)).to(DEV) for k in ("users", "items")]


def _keep(g, b, mods=("image", "text")):
    ks = B.batch_keep(B.golden_keep(g, "A"), b["users"], b["items"], mods)
    return [None if k is None else torch.as_tensor(k).to(DEV) for k in ks]


def _model(b, g=None, prefix="p0_", **over):
    m, cfg, ds, tl = RB.build_rfbm3(b, **over)
    if g is not None:
        m.rf_generator.load_reference_state({n: g["A_" + prefix + R.key(n)] for n in R.param_names(2)})
    return m


def _grads(m):
    return [v.cpu().numpy().copy() for v in m.grad_views()]


def test_registry():
    from gmr.rfbm3 import RFBM3
    from gmr.utils import get_model
    assert get_model("RFBM3") is RFBM3


def test_init_parity(b):
    m = _model(b)
    ref, *_ = B.build_bm3(b, "A")
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == B.PARAMS
    for p, q, k in zip(m._params(), ref._params(), B.PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), b["p_" + k]), k
        assert torch.equal(p, q), k
    assert m.rf_generator.C == 128 and m.rf_generator.N == m.N


def test_use_rf_false_is_bm3(b):
    a = _model(b, use_rf=False)
    ref, *_ = B.build_bm3(b, "A")
    assert a.rf_generator is None
    users, items = _batch(b)
    la, lb = a.rec_step(users, items, None), ref.rec_step(users, items, None)  # the same Philox masks
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, ref.slab.grad)
    au = torch.arange(a.n_users, device=DEV)
    assert torch.equal(a.full_sort_predict([au]), ref.full_sort_predict([au]))
    assert a.extra_state() == ref.extra_state()


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(b, over, key):
    with pytest.raises(NotImplementedError, match=key):
        RB.build_rfbm3(b, **over)


def test_step_parity(b, g):
    m = _model(b, g)
    assert m._training_epoch == -1
    m.pre_epoch_processing()
    assert m._training_epoch == 0 and m.rf_generator.epoch == 0
    ref, *_ = B.build_bm3(b, "A")
    users, items = _batch(b)
    keep = _keep(g, b)
    p0, v0 = m.slab.data.clone(), m.rf_generator.slab.data.clone()
    want_loss = ref.rec_step(users, items, None, keep=keep)
    loss = m.rec_step(users, items, None, keep=keep, rf_draws=RB.draws(g, "A_"))
    # BM3's loss and its ten gradients: the BM3 class's bit for bit, and the reference's; parameters untouched
    assert torch.equal(loss, want_loss) and torch.equal(m.slab.grad, ref.slab.grad) and torch.equal(m.slab.data, p0)
    np.testing.assert_allclose(loss.item(), g["A_loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[1:7], g["A_loss_terms"], rtol=1e-5)
    np.testing.assert_allclose(terms[7], g["A_reg"], rtol=1e-5)
    B.check_grads(_grads(m), [g["A_g_" + k] for k in B.PARAMS], show="A")
    # the RF step saw the reference's target, conditions and prior; their user rows are exactly zero
    U = m.n_users
    np.testing.assert_allclose(m._x1.cpu().numpy(), g["A_X1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m._cond.cpu().numpy(), g["A_cond"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m._prior.cpu().numpy(), g["A_prior"], rtol=1e-5, atol=2e-6)
    assert not m._cond[:U].any() and not m._prior[:U].any()
    gen = m.rf_generator
    terms = m.rf_loss_terms().cpu().numpy()
    print(f"rf_loss {terms[0]:.7f} ({g['A_rf_loss']:.7f}), cl_loss {terms[1]:.7f} ({g['A_cl_loss']:.7f})")
    np.testing.assert_allclose(terms[0], g["A_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1], g["A_cl_loss"], rtol=1e-5)
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), g["A_v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gen._w["pred"].cpu().numpy(), g["A_pred"], rtol=1e-5, atol=1e-6)
    bar = R.grad_bar(g, "A_")
    worst = 0.0
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        want = g["A_g_" + R.key(name)]
        worst = max(worst, R.rel_to_max(got.cpu().numpy(), want))
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=bar * np.abs(want).max(), err_msg=name)
    print(f"velocity gradients: worst error relative to the parameter's max {worst:.3e} (bar {bar:.3e})")
    assert not torch.equal(gen.slab.data, v0)
    for (name, _), p in zip(gen.specs, gen.param_views()):
        got, want = p.cpu().numpy(), g["A_p1_" + R.key(name)]
        assert (np.abs(got - want) <= RB.p1_bound(g, "A_", name, bar, float(g["lr"]))).all(), name
    assert m.extra_state() == {"counters": {"step": 1}, "rf_epoch": 0, "rf_step": 1}


def test_predict(b, g):
    m = _model(b, g, prefix="p1_", rf_warmup_epochs=1)
    U = m.n_users
    users = torch.arange(U, device=DEV)
    ref, *_ = B.build_bm3(b, "A")
    want_pre = ref.full_sort_predict([users])
    ref_items = ref._pred[U:].clone()
    m._training_epoch = 0
    m.rf_generator.set_epoch(0)  # before warm-up: the BM3 class's scores, bit for bit
    pre = m.full_sort_predict([users])
    assert torch.equal(pre, want_pre)
    np.testing.assert_allclose(pre.cpu().numpy(), g["A_scores_pre"], rtol=1e-5, atol=1e-5)
    m.rf_generator.set_epoch(1)  # warmed up: the user rows + 0.2 generate(0) from the recorded start noise
    z0 = torch.as_tensor(g["A_z0"]).to(DEV)
    mix = m.full_sort_predict([users], z0=z0)
    err = np.abs(m._gen[:U].cpu().numpy().astype(np.float64) - g["A_gen"][:U]).max()
    print(f"sampler on the user rows: max abs error {err:.3e} (bar {4 * float(g['A_err_sample']):.3e})")
    np.testing.assert_allclose(m._gen[:U].cpu().numpy(), g["A_gen"][:U], rtol=0, atol=4 * float(g["A_err_sample"]))
    np.testing.assert_allclose(m._eval[:U].cpu().numpy(), g["A_eval_u"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mix.cpu().numpy(), g["A_scores_mix"], rtol=1e-5, atol=1e-5)
    # the item rows are not mixed: the table and P(ib) are BM3's bit for bit
    assert torch.equal(m._eval[U:], ref._eval[U:]) and torch.equal(m._pred[U:], ref_items)
    assert not torch.equal(m._pred[:U], ref._pred[:U])
    # the first U rows of an N-row draw and a U-row draw are the same start noise
    assert torch.equal(m.full_sort_predict([users], z0=z0[:U]), mix)
    # Philox start noise: deterministic at a given step counter, finite, and another table than BM3's
    s1, s2 = m.full_sort_predict([users]).clone(), m.full_sort_predict([users])
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all()) and not torch.equal(s1, pre)


def _restatement_check(m, d_rows, d_cols, users_np, items_np, tk, mods, what, n_layers, dropout):
    """One rec_step with injected masks and draws against the fp64 restatement: BM3's part at test_bm3_gpu.py's
    bars, the RF losses at 1e-5, v at rtol 1e-5 next to twice the fp32 restatement's own error, the velocity gradients
    at 4x that restatement's own error (floored at 1e-6 of the parameter's largest gradient, the rule of
    test_rf_kernels_shapes_gpu.py); measured errors and bars are printed."""
    U, I, N = m.n_users, m.n_items, m.N
    gen = m.rf_generator
    names = B.params_of(mods)
    P = {k: p.detach().cpu().numpy() for k, p in zip(names, m._params())}
    VP = {n: v.cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    rng = np.random.default_rng(11)
    dr = RB.random_draws(rng, N, U, I, users_np, items_np)
    users, items = torch.as_tensor(users_np.astype(np.int32)).to(DEV), torch.as_tensor(items_np.astype(np.int32)).to(DEV)
    keep = [None if k is None else torch.as_tensor(k).to(DEV) for k in B.batch_keep(tk, users_np, items_np, mods)]
    loss = m.rec_step(users, items, None, keep=keep, rf_draws={k: torch.as_tensor(v).to(DEV) for k, v in dr.items()})
    r = B.bm3_step_ref(P, U, I, d_rows, d_cols, users_np, items_np, tk, n_layers, dropout, mods=mods)
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy()[1:7], r["terms"], rtol=1e-5)
    B.check_grads(_grads(m), r["grads"], names=names, show=what)
    res = {}
    for dt in (torch.float64, torch.float32):
        pr = RB.projected(P, mods, dt)
        cond, prior = RB.rf_inputs_ref(pr.get("text"), pr.get("image"), U)
        X1 = RB.encoder_mean(P, U, I, d_rows, d_cols, n_layers, dt)
        VPt = {n: torch.tensor(v, dtype=dt, requires_grad=True) for n, v in VP.items()}
        c = lambda a: torch.tensor(a, dtype=dt)  # noqa: E731
        li = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
        out = RB.train_losses(VPt, X1, c(dr["X0"]), c(dr["t"]), cond, prior, li(users_np), li(items_np),
                              li(dr["neg_items"]), li(dr["neg_users"]), U, gen.L)
        res[dt] = (out, R.grads_of(VPt, out["total"]), X1, cond, prior)
    o64, g64, X1, cond, prior = res[torch.float64]
    o32, g32, *_ = res[torch.float32]
    np.testing.assert_allclose(m._x1.cpu().numpy(), X1.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m._cond.cpu().numpy(), cond.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m._prior.cpu().numpy(), prior.numpy(), rtol=1e-5, atol=2e-6)
    terms = m.rf_loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], o64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(terms[1], o64["cl_loss"].item(), rtol=1e-5)
    v64 = o64["v"].detach().numpy()
    own = float(np.abs(o32["v"].detach().numpy().astype(np.float64) - v64).max())
    err = float(np.abs(gen._w["V"].cpu().numpy().astype(np.float64) - v64).max())
    print(f"{what}: v max abs error {err:.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), v64, rtol=1e-5, atol=2 * own)
    worst = (0.0, 0.0)
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        want = g64[name].numpy()
        own = R.rel_to_max(g32[name].numpy(), want)
        bar = max(4 * own, 1e-6)
        err = R.rel_to_max(got.cpu().numpy(), want)
        worst = max(worst, (err, bar))
        assert err <= bar, (name, err, bar)
    print(f"{what}: velocity gradients, worst error relative to the parameter's max {worst[0]:.3e} (bar {worst[1]:.3e})")


@pytest.mark.parametrize("mod", ["text", "image"])
def test_one_modality(b, mod):
    m, *_ = RB.build_rfbm3(b, mods=(mod,), rf_n_layers=1)
    assert m.rf_generator.C == 64 and m._cond.shape == (m.N, 64)
    c = B.CASES["A"]
    _restatement_check(m, b["train_rows"], b["train_cols"], b["users"], b["items"], B.golden_keep(b, "A"), (mod,),
                       mod, c["n_layers"], c["dropout"])


def test_mid_shape_step():
    """U = 300, I = 1,100 (9 blocks of the inputs kernel, 350 of the head), widths 37 / 50, B = 700 (2B > 256)."""
    m, d = RB.build_rfbm3_mid("B")
    rng = np.random.default_rng(6)
    p = B.CASES["B"]["dropout"]
    tk = {k: (rng.random((n, 64)) >= p).astype(np.uint8) for k, n in (("u", d["U"]), ("i", d["I"]), ("t", d["I"]),
                                                                       ("v", d["I"]))}
    _restatement_check(m, d["rows"], d["cols"], d["users"], d["items"], tk, ("image", "text"), "mid",
                       B.CASES["B"]["n_layers"], p)


def test_philox_step_is_finite_and_reproducible(b):
    users, items = _batch(b)
    outs = []
    for _ in range(2):
        m = _model(b, rf_dropout=0.1, rf_infonce_negatives=1024)
        m.pre_epoch_processing()
        losses = [m.rec_step(users, items, None).item() for _ in range(2)]
        outs.append((losses, m.rf_loss_terms().clone(), m.slab.grad.clone(), m.rf_generator.slab.data.clone(),
                     m.rf_generator.slab.grad.clone()))
    (la, ta, ga, pa, va), (lb, tb, gb, pb, vb) = outs
    assert np.isfinite(la).all() and bool(torch.isfinite(ta).all()) and bool(torch.isfinite(va).all())
    assert la == lb and torch.equal(ta, tb) and torch.equal(ga, gb) and torch.equal(pa, pb) and torch.equal(va, vb)
    assert m.extra_state() == {"counters": {"step": 2}, "rf_epoch": 0, "rf_step": 2}


def test_fit_and_evaluate():
    """Two epochs through the generic Trainer on gmr/synthetic.py data (the path of main.py --model RFBM3) with
    rf_warmup_epochs 1: finite losses and metrics, and an evaluation that changes the user table only."""
    from gmr.bm3 import BM3
    from gmr.configurator import Config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.rfbm3 import RFBM3
    from gmr.synthetic import make_dataset
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    cfg = Config("RFBM3", "baby", {"synthetic": "tiny", "epochs": 2, "save_recommended_topk": False,
                                   "rf_warmup_epochs": 1, "rf_infonce_negatives": 64, "rf_sampling_steps": 2})
    init_seed(999)
    ds = make_dataset(cfg, "tiny", seed=0)
    tr, va, te = ds.split()
    tl = TrainDataLoader(cfg, tr, batch_size=cfg["train_batch_size"], shuffle=True)
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
    m = RFBM3(cfg, tl)
    p0 = m.rf_generator.slab.data.clone()
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    assert np.isfinite(trainer.train_loss_dict[0]) and np.isfinite(trainer.train_loss_dict[1])
    assert "recall@10" in valid and all(np.isfinite(v) for v in trainer.evaluate(vl).values())
    gen = m.rf_generator
    assert m._training_epoch == 1 and gen.warmed_up() and gen.step_ctr == 2 * len(tl)
    assert bool(torch.isfinite(m.rf_loss_terms()).all()) and not torch.equal(gen.slab.data, p0)
    # evaluation after warm-up against BM3's own tables on the same parameters
    U = m.n_users
    usr, itm = (x.clone() for x in m.forward_embeddings())
    bu, bi = BM3.forward_embeddings(m)
    assert torch.equal(itm, bi) and not torch.equal(usr, bu) and bool(torch.isfinite(usr).all())
    sd = m.state_dict()
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(sd)
