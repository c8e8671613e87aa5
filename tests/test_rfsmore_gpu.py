"""RFSMORE (gmr/rfsmore.py) against the reference's golden values (tests/golden/make_golden_rfsmore.py, on the data,
seed, case B and first keep masks of smore_tiny{,_B}.npz) with its RF draws and SMORE's masks injected, against the
SMORE class itself, and, where the reference recorded nothing (the mid shape), against the fp64 restatement of
tests/rfsmore_fixture.py, which tests/test_rfsmore_cpu.py pins to the same golden values."""
import numpy as np
import pytest
import torch

import rf_fixture as R
import rfbm3_fixture as RB
import rfsmore_fixture as RS
import smore_fixture as F

pytestmark = pytest.mark.gpu
DEV = F.DEV
NAN = float("nan")


@pytest.fixture(scope="module")
def f(golden):
    return RS.smore_golden(golden)


@pytest.fixture(scope="module")
def g(golden):
    return RS.load_golden(golden)


def _batch(f):
    return [torch.as_tensor(f[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _keep(f, step=0):
    return torch.as_tensor(F.golden_keep(f, step)).to(DEV)


def _model(f, g=None, prefix="p0_", **over):
    m, cfg, ds, tl = RS.build_rfsmore(f, **over)
    if g is not None:
        m.rf_generator.load_reference_state({n: g["B_" + prefix + R.key(n)] for n in R.param_names(2)})
    return m


def _rf_state(m):
    gen = m.rf_generator
    return (m.rf_loss_terms().clone(), gen.slab.grad.clone(), gen.slab.data.clone(), gen.exp_avg.clone(),
            gen.exp_avg_sq.clone())


def test_registry():
    from gmr.rfsmore import RFSMORE
    from gmr.utils import get_model
    assert get_model("RFSMORE") is RFSMORE


def test_init_parity(f):
    m, *_ = RS.build_rfsmore(f, "A")
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == F.PARAMS
    for p, k in zip(m._params(), F.PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), f["init_" + k]), k
    gen = m.rf_generator
    assert gen.C == 192 and gen.N == m.N and gen.L == 2 and gen.slab.numel == RS.N_PARAMS
    assert m._cond.shape == (m.N, 192) and m._prior.shape == m._gen.shape == m._mix.shape == (m.N, 64)


def test_use_rf_false_is_smore(f):
    a = _model(f, use_rf=False)
    ref, *_ = F.build_smore(f, "B")
    assert a.rf_generator is None and not any(hasattr(a, k) for k in ("_gen", "_prior", "_cond", "_mix", "_pws"))
    assert list(a.state_dict()) == F.STATE_KEYS
    users, pos, neg = _batch(f)
    la, lb = a.rec_step(users, pos, neg, keep=_keep(f)), ref.rec_step(users, pos, neg, keep=_keep(f))
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, ref.slab.grad)
    la, lb = a.rec_step(users, pos, neg), ref.rec_step(users, pos, neg)   # the Philox masks of step 1
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, ref.slab.grad)
    au = torch.arange(a.n_users, device=DEV)
    assert torch.equal(a.full_sort_predict([au]), ref.full_sort_predict([au]))
    a.pre_epoch_processing()
    assert a.extra_state() == {"counters": {"step": 2}}


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(f, over, key):
    with pytest.raises(NotImplementedError, match=key):
        RS.build_rfsmore(f, **over)


def test_step_parity(f, g):
    m = _model(f, g)
    assert m._training_epoch == -1
    m.pre_epoch_processing()
    assert m._training_epoch == 0 and m.rf_generator.epoch == 0
    ref, *_ = F.build_smore(f, "B")
    users, pos, neg = _batch(f)
    gen = m.rf_generator
    p0, v0 = m.slab.data.clone(), gen.slab.data.clone()
    seen = {}
    step = gen.train_step

    def spy(X1, cond, *a, **kw):
        seen.update(X1=X1.data_ptr(), cond=cond.data_ptr(), ldc=cond.stride(0), prior=kw["prior"].data_ptr())
        return step(X1, cond, *a, **kw)

    gen.train_step = spy
    want_loss = ref.rec_step(users, pos, neg, keep=_keep(f))
    loss = m.rec_step(users, pos, neg, rf_draws=RS.draws(g), keep=_keep(f))
    del gen.train_step
    # SMORE's loss and its 29 gradients: the SMORE class's bit for bit; parameters untouched
    assert torch.equal(loss, want_loss) and torch.equal(m.slab.data, p0)
    assert torch.equal(m.loss_terms(), ref.loss_terms())
    assert len(m.grad_views()) == 29
    for a, b, k in zip(m.grad_views(), ref.grad_views(), F.PARAMS):
        assert torch.equal(a, b), k
    assert torch.equal(m.slab.grad, ref.slab.grad)
    np.testing.assert_allclose(loss.item(), f["B_loss"], rtol=1e-5)
    # the RF step saw the model's own tables
    assert seen == {"X1": m.all.data_ptr(), "cond": m._cond.data_ptr(), "ldc": 192, "prior": m._prior.data_ptr()}
    for k in ("abf", "saved", "all"):      # intact after the backward
        assert torch.equal(getattr(m, k), getattr(ref, k)), k
    np.testing.assert_allclose(m.all.cpu().numpy(), g["B_X1"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m._cond.cpu().numpy(), g["B_cond"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m._prior.cpu().numpy(), g["B_prior"], rtol=1e-5, atol=2e-6)
    # the third block is gf * f of this step: the mask's zeros are in it, and it is not the plain fusion view
    third, fus, gf = m._cond[:, 128:], m.abf[:, 128:], m.saved[:, 384:]
    assert torch.equal(third, gf * fus) and not torch.equal(third, fus)
    assert torch.equal(third == 0, (_keep(f)[:, 128:] == 0) | (fus == 0))
    assert torch.equal(m._cond[:, :128], m.abf[:, :128])
    assert bool(m._prior[:m.n_users].any()) and bool(m._cond[:m.n_users].any())  # dense user rows
    terms = m.rf_loss_terms().cpu().numpy()
    print(f"rf_loss {terms[0]:.7f} ({g['B_rf_loss']:.7f}), cl_loss {terms[1]:.7f} ({g['B_cl_loss']:.7f})")
    np.testing.assert_allclose(terms[0], g["B_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1], g["B_cl_loss"], rtol=1e-5)
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), g["B_v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gen._w["pred"].cpu().numpy(), g["B_pred"], rtol=1e-5, atol=1e-6)
    bar = R.grad_bar(g, "B_")
    worst = 0.0
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        err = R.rel_to_max(got.cpu().numpy(), g["B_g_" + R.key(name)])
        worst = max(worst, err)
        assert err <= bar, (name, err, bar)
    print(f"velocity gradients: worst error relative to the parameter's max {worst:.3e} (bar {bar:.3e})")
    assert not torch.equal(gen.slab.data, v0)
    for (name, _), p in zip(gen.specs, gen.param_views()):
        got, want = p.cpu().numpy(), g["B_p1_" + R.key(name)]
        assert (np.abs(got - want) <= RB.p1_bound(g, "B_", name, bar, float(g["lr"]))).all(), name
    assert m.extra_state() == {"counters": {"step": 1}, "rf_epoch": 0, "rf_step": 1}


def test_step_repeats_on_nan_filled_buffers(f, g):
    """Nothing of a step reads what an earlier step left: SMORE's work buffers, the conditions, the prior, its
    workspace and the generator's work buffers filled with NaN, the velocity state put back, and the step repeats bit
    for bit."""
    m = _model(f, g)
    m.pre_epoch_processing()
    users, pos, neg = _batch(f)
    gen = m.rf_generator
    v0 = gen.slab.data.clone()
    loss = m.rec_step(users, pos, neg, rf_draws=RS.draws(g), keep=_keep(f)).clone()
    first, first_grad = _rf_state(m), m.slab.grad.clone()
    bufs = [m.vt, m.spec, m.conv, m.gates_i, m.pur, m.abf, m.c, m.side, m.all, m.saved, m.dall, m.gtab, m.dabf, m.dc,
            m.zf, m.dpur, m.zp, m.dvt, m._ws, m._loss, *m._h, *m._layers, *m._t, m._cond, m._prior, m._pws, m._gen,
            m._mix, *[v for v in m._w.values() if torch.is_tensor(v) and v.is_floating_point()]]
    w = gen._w
    bufs += [v for v in w.values() if torch.is_tensor(v) and v.is_floating_point()]
    bufs += [v for k in ("Y", "A") for v in w[k].values()]
    for t in bufs:
        t.fill_(NAN)
    m.slab.grad.fill_(NAN)
    gen.slab.grad.fill_(NAN)
    gen.slab.data.copy_(v0)
    gen.exp_avg.zero_()
    gen.exp_avg_sq.zero_()
    gen.step_ctr = 0
    again = m.rec_step(users, pos, neg, rf_draws=RS.draws(g), keep=_keep(f))
    assert torch.equal(again, loss) and torch.equal(m.slab.grad, first_grad)
    for a, b, what in zip(_rf_state(m), first, ("losses", "gradients", "parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), what


def test_predict(f, g):
    m = _model(f, g, prefix="p1_", rf_warmup_epochs=1)
    U = m.n_users
    users = torch.arange(U, device=DEV)
    ref, *_ = F.build_smore(f, "B")
    want_pre = ref.full_sort_predict([users])
    gen = m.rf_generator
    m._training_epoch = 0
    gen.set_epoch(0)  # before warm-up: the SMORE class's scores bit for bit, and the sampler is not launched
    m._gen.fill_(NAN)
    m._cond.fill_(NAN)
    pre = m.full_sort_predict([users])
    assert torch.equal(pre, want_pre) and bool(torch.isnan(m._gen).all()) and bool(torch.isnan(m._cond).all())
    np.testing.assert_allclose(pre.cpu().numpy(), g["B_scores_pre"], rtol=1e-5, atol=1e-4)
    gen.set_epoch(1)  # warmed up: every row + 0.2 generate(cond) from the recorded start noise, no dropout
    z0 = torch.as_tensor(g["B_z0"]).to(DEV)
    mix = m.full_sort_predict([users], z0=z0)
    np.testing.assert_allclose(m._cond.cpu().numpy(), g["B_cond_eval"], rtol=1e-5, atol=2e-6)
    gate = m.saved[:, 384:]
    assert bool((gate > 0).all()) and bool((gate < 1).all())   # the bare sigmoid gate
    spread = 4 * float(g["B_err_sample"])
    err = np.abs(m._gen.cpu().numpy().astype(np.float64) - g["B_gen_eval"]).max()
    print(f"sampler on all N rows: max abs error {err:.3e} (bar {spread:.3e})")
    np.testing.assert_allclose(m._gen.cpu().numpy(), g["B_gen_eval"], rtol=0, atol=spread)
    # SMORE's table bar next to the sampler's spread times the mix ratio
    np.testing.assert_allclose(m._mix.cpu().numpy(), g["B_eval"], rtol=1e-5, atol=2e-6 + spread * float(g["ratio"]))
    want = g["B_scores_mix"]
    serr = np.abs(mix.cpu().numpy().astype(np.float64) - want).max()
    # a score is a 64-term product of two rows within the table bar: its error is at most the sum over the terms of
    # |u| d_i + |i| d_u with d = 1e-5 |x| + 2e-6 + spread ratio
    ev = np.abs(g["B_eval"].astype(np.float64))
    d = 1e-5 * ev + 2e-6 + spread * float(g["ratio"])
    sbar = (ev[:U] @ d[U:].T + d[:U] @ ev[U:].T).max() + 1e-5 * np.abs(want).max()
    print(f"mixed scores: max abs error {serr:.3e} (bar {sbar:.3e}, largest score {np.abs(want).max():.3f})")
    assert serr <= sbar
    # the user rows differ from SMORE's, and so do the item rows; SMORE's own table is not touched
    assert float((m._mix[:U] - ref.all[:U]).abs().max()) > 0.05 and float((m._mix[U:] - ref.all[U:]).abs().max()) > 0.05
    assert torch.equal(m.all, ref.all) and torch.equal(m.abf, ref.abf)
    assert float((mix - pre).abs().max()) > 1.0
    # Philox start noise: deterministic at a given step counter, finite, and another table than SMORE's
    s1, s2 = m.full_sort_predict([users]).clone(), m.full_sort_predict([users])
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all()) and not torch.equal(s1, pre)


def test_no_mixed_table_leaks_into_training(f, g):
    """A training step after a warmed-up evaluation is the same step without it, bit for bit."""
    users, pos, neg = _batch(f)
    au = torch.arange(int(f["U"]), device=DEV)
    outs = []
    for evaluate in (False, True):
        m = _model(f, g)  # rf_warmup_epochs 0: warmed up from the first epoch
        m.pre_epoch_processing()
        if evaluate:
            assert m.rf_generator.warmed_up()
            ref, *_ = F.build_smore(f, "B")
            assert not torch.equal(m.full_sort_predict([au]), ref.full_sort_predict([au]))
        loss = m.rec_step(users, pos, neg, rf_draws=RS.draws(g), keep=_keep(f)).clone()
        outs.append((loss, m.slab.grad.clone(), m.all.clone(), m._cond.clone(), m._prior.clone(), *_rf_state(m)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_mid_shape_step():
    """U = 300, I = 1,100 (3 + 9 blocks of the inputs kernel with both last blocks short; N = 1,400 = 43 sampler tiles
    and 24 rows; widths 37 / 50; B = 700 with repeated users), n_layers 2, dropout 0.1 with the model's own Philox
    masks read back from the device (saved's gate blocks are zero where dropped).  X0 and t are the model's Philox
    draws read back likewise; the InfoNCE negatives are injected.  All of it goes to the fp64 restatement: SMORE's loss
    at 1e-5 and its tables at the table bars, the RF tables at the table bars, the RF losses at 1e-5, v at rtol 1e-5
    next to twice the fp32 restatement's own error, the velocity gradients at 4x that restatement's own error (floored
    at 1e-6 of the parameter's largest gradient: the rule of test_rfmgcn_gpu.py)."""
    m, d = RS.build_rfsmore_mid()
    m.pre_epoch_processing()
    U, I, N = m.n_users, m.n_items, m.N
    assert -(-U // 128) == 3 and -(-I // 128) == 9 and N % 32 == 24 and m.dropout_rate == 0.1
    gen = m.rf_generator
    P = {k: v.detach().cpu().numpy() for k, v in zip(F.PARAMS, m._params())}
    VP = {n: v.cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    users, pos, neg = (torch.as_tensor(d[k]).to(DEV) for k in ("users", "pos", "neg"))
    rng = np.random.default_rng(11)
    ni = R.collide(rng.integers(0, I, (len(d["pos"]), 7)), d["pos"], I).astype(np.int32)
    nu = R.collide(rng.integers(0, U, (len(d["users"]), 7)), d["users"], U).astype(np.int32)
    loss = m.rec_step(users, pos, neg, rf_draws={"neg_items": torch.as_tensor(ni).to(DEV),
                                                 "neg_users": torch.as_tensor(nu).to(DEV)})
    keep = (m.saved[:, 256:] != 0).cpu().numpy().astype(np.uint8)   # a sigmoid is never 0: the zeros are the mask
    assert keep.shape == (N, 192) and abs(keep.mean() - 0.9) < 0.01
    dr = {"X0": gen._w["X0"].cpu().numpy(), "t": gen._w["t"].cpu().numpy().reshape(N, 1), "neg_items": ni,
          "neg_users": nu}
    assert np.isfinite(dr["X0"]).all() and abs(dr["X0"].mean()) < 0.02 and abs(dr["X0"].std() - 1) < 0.02
    c = F.CASES["B"]
    res = {}
    for dt in (torch.float64, torch.float32):
        gr = F.graphs_ref(U, I, d["rows"], d["cols"], (d["v_feat"], d["t_feat"]), dt, *RS.MID_K)
        r = F.smore_step_ref(P, U, I, d["rows"], d["cols"], d["users"], d["pos"], d["neg"], c["n_layers"],
                             c["cl_loss"], (d["v_feat"], d["t_feat"]), keep=keep, p=c["dropout_rate"], dtype=dt,
                             graphs=gr)
        X1, cond, prior = RS.rf_inputs_ref(r, P, U, keep, c["dropout_rate"], dt)
        out, grads = RS.rf_step_ref(VP, X1, cond, prior, dr, d["users"], d["pos"], U, gen.L, dt)
        res[dt] = (r, X1, cond, prior, out, grads)
    r, X1, cond, prior, o64, g64 = res[torch.float64]
    r32, _, _, _, o32, g32 = res[torch.float32]
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy()[1:], r["terms"], rtol=1e-5)
    for k in ("c", "side", "all"):
        F.bar(getattr(m, k), r[k], r32[k], f"mid {k}")
    np.testing.assert_allclose(m.all.cpu().numpy(), X1.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m._cond.cpu().numpy(), cond.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m._prior.cpu().numpy(), prior.numpy(), rtol=1e-5, atol=2e-6)
    assert (m._cond[:, 128:] == 0).float().mean().item() > 0.05   # the mask is in the condition
    terms = m.rf_loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], o64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(terms[1], o64["cl_loss"].item(), rtol=1e-5)
    v64 = o64["v"].detach().numpy()
    own = float(np.abs(o32["v"].detach().numpy().astype(np.float64) - v64).max())
    err = float(np.abs(gen._w["V"].cpu().numpy().astype(np.float64) - v64).max())
    print(f"mid: v max abs error {err:.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), v64, rtol=1e-5, atol=2 * own)
    worst = (0.0, 0.0)
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        want = g64[name].numpy()
        bar = max(4 * R.rel_to_max(g32[name].numpy(), want), 1e-6)
        err = R.rel_to_max(got.cpu().numpy(), want)
        worst = max(worst, (err, bar))
        assert err <= bar, (name, err, bar)
    print(f"mid: velocity gradients, worst error relative to the parameter's max {worst[0]:.3e} (bar {worst[1]:.3e})")
    # the evaluation at this shape: the sampler over 44 tiles from an injected z0 against the fp64 restatement
    gen.set_epoch(gen.warmup_epochs)
    z0 = rng.standard_normal((N, 64)).astype(np.float32)
    m.forward_embeddings(z0=torch.as_tensor(z0).to(DEV))
    VP1 = {n: v.cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    ce = m._cond.cpu().numpy()
    want = {}
    for dt in (torch.float32, torch.float64):
        Pv = {n: torch.tensor(v, dtype=dt) for n, v in VP1.items()}
        with torch.no_grad():
            want[dt] = R.generate(Pv, torch.tensor(ce, dtype=dt), torch.tensor(z0, dtype=dt), gen.sampling_steps,
                                  gen.L).numpy().astype(np.float64)
    w = want[torch.float64]
    sbar = max(4 * np.abs(want[torch.float32] - w).max(), 1e-6 * np.abs(w).max())
    serr = np.abs(m._gen.cpu().numpy() - w).max()
    print(f"mid: sampler max abs error {serr:.3e} (bar {sbar:.3e})")
    assert serr <= sbar
    # all + ratio * gen: one product and one sum, contracted or not
    mix = m.all.double() + gen.inference_mix_ratio * m._gen.double()
    assert float((m._mix.double() - mix).abs().max()) <= 2.0 ** -22 * float(mix.abs().max())


def test_philox_step_is_finite_and_reproducible(f):
    users, pos, neg = _batch(f)
    outs = []
    for _ in range(2):
        m = _model(f, rf_dropout=0.1, rf_infonce_negatives=1024)
        m.pre_epoch_processing()
        losses = [m.rec_step(users, pos, neg).item() for _ in range(2)]
        outs.append((losses, m.slab.grad.clone(), m._cond.clone(), *_rf_state(m)))
    a, b = outs
    assert np.isfinite(a[0]).all() and all(bool(torch.isfinite(t).all()) for t in a[1:])
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert m.extra_state() == {"counters": {"step": 2}, "rf_epoch": 0, "rf_step": 2}


def test_fit_and_evaluate():
    """Two epochs through the generic Trainer on gmr/synthetic.py data (the path of main.py --model RFSMORE) with
    rf_warmup_epochs 1: finite losses and metrics, and an evaluation that changes both halves of the table."""
    from gmr.configurator import Config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.rfsmore import RFSMORE
    from gmr.smore import SMORE
    from gmr.synthetic import make_dataset
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    cfg = Config("RFSMORE", "baby", {"synthetic": "tiny", "epochs": 2, "save_recommended_topk": False,
                                     "rf_warmup_epochs": 1, "rf_infonce_negatives": 64, "rf_sampling_steps": 2})
    init_seed(999)
    ds = make_dataset(cfg, "tiny", seed=0)
    tr, va, te = ds.split()
    tl = TrainDataLoader(cfg, tr, batch_size=cfg["train_batch_size"], shuffle=True)
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
    m = RFSMORE(cfg, tl)
    p0 = m.rf_generator.slab.data.clone()
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    assert np.isfinite(trainer.train_loss_dict[0]) and np.isfinite(trainer.train_loss_dict[1])
    assert "recall@10" in valid and all(np.isfinite(v) for v in trainer.evaluate(vl).values())
    gen = m.rf_generator
    assert m._training_epoch == 1 and gen.warmed_up() and gen.step_ctr == 2 * len(tl) == m._step
    assert bool(torch.isfinite(m.rf_loss_terms()).all()) and not torch.equal(gen.slab.data, p0)
    usr, itm = (x.clone() for x in m.forward_embeddings())
    bu, bi = SMORE.forward_embeddings(m)
    assert not torch.equal(itm, bi) and not torch.equal(usr, bu)
    assert bool(torch.isfinite(usr).all()) and bool(torch.isfinite(itm).all())
    sd = m.state_dict()
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(sd)


def test_quick_start(tmp_path, monkeypatch):
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False,
                "rf_warmup_epochs": 1, "rf_infonce_negatives": 64, "rf_sampling_steps": 2}
    results = quick_start("RFSMORE", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("RFSMORE", "baby", dict(cfg_dict))
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and want <= set(best_test)
    assert all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "RFSMORE-baby.pth"), map_location="cpu", weights_only=True)
    assert {"config", "epoch", "state_dict", "optimizer", "best_valid_score"} <= set(ck)
    assert list(ck["state_dict"])[:len(F.STATE_KEYS)] == F.STATE_KEYS
    assert {"counters", "rf_epoch", "rf_step"} == set(ck["generated_graphs"])


def test_world_size_two_raises(f, monkeypatch):
    from gmr import dist
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        RS.build_rfsmore(f)
