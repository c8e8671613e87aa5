"""RFLGMRec (gmr/rflgmrec.py) against the reference's golden values (tests/golden/make_golden_rflgmrec.py, on the data,
seed, case B and recorded draws of lgmrec_tiny{,_B}.npz) with its RF draws and LGMRec's Gumbel draws and masks
injected, against the LGMRec class itself, and, where the reference recorded nothing (the mid shape), against the fp64
restatement of tests/rflgmrec_fixture.py, which tests/test_rflgmrec_cpu.py pins to the same golden values.

Tables go at the project's bar (lgmrec_fixture.bar: rtol 1e-5 against the fp64 restatement, atol twice the fp32
restatement's own error); a golden fp32 table is met within that bar next to the golden table's own distance from the
fp64 restatement."""
import numpy as np
import pytest
import torch

import lgmrec_fixture as F
import rf_fixture as R
import rfbm3_fixture as RB
import rflgmrec_fixture as RL

pytestmark = pytest.mark.gpu
DEV = F.DEV
NAN = float("nan")
L = 2


@pytest.fixture(scope="module")
def f(golden):
    return RL.lgmrec_golden(golden)


@pytest.fixture(scope="module")
def g(golden):
    return RL.load_golden(golden)


def _batch(f):
    return [torch.as_tensor(f[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _draws(f, step=0):
    return {"g": torch.as_tensor(f["B_g"][step]).to(DEV), "keep": torch.as_tensor(f["B_keep"][step]).to(DEV)}


def _model(f, g=None, prefix="p0_", **over):
    m, cfg, ds, tl = RL.build_rflgmrec(f, **over)
    if g is not None:
        m.rf_generator.load_reference_state({n: g["B_" + prefix + R.key(n)] for n in R.param_names(L)})
    return m


def _rf_state(m):
    gen = m.rf_generator
    return (m.rf_loss_terms().clone(), gen.slab.grad.clone(), gen.slab.data.clone(), gen.exp_avg.clone(),
            gen.exp_avg_sq.clone())


def _against_golden(got, gold, r64, r32, what):
    """The bar against the fp64 restatement, and the golden fp32 table within that bar plus its own distance."""
    F.bar(got, r64, r32, what)
    own = float(np.abs(np.asarray(r32, np.float64) - r64).max())
    gown = float(np.abs(gold.astype(np.float64) - r64).max())
    np.testing.assert_allclose(got.cpu().numpy(), gold, rtol=1e-5, atol=2 * own + gown, err_msg=what)


def test_registry_and_init(f):
    from gmr.rflgmrec import RFLGMRec
    from gmr.utils import get_model
    assert get_model("RFLGMRec") is RFLGMRec
    m, *_ = RL.build_rflgmrec(f, "A")
    assert [n.replace(".", "_") for n, p in m.named_parameters() if p.requires_grad] == F.PARAMS
    for p, k in zip(m._params(), F.PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), f["A_init_" + k]), k
    gen = m.rf_generator
    assert gen.C == 128 and gen.N == m.N and gen.L == 2 and gen.slab.numel == RL.N_PARAMS
    assert m._prior.shape == m._mixc.shape == (m.N, 64)


def test_use_rf_false_is_lgmrec(f):
    a = _model(f, use_rf=False)
    ref, *_ = F.build_lgmrec(f, "B")
    assert a.rf_generator is None and not any(hasattr(a, k) for k in ("_gen", "_prior", "_mixc", "_pws"))
    assert list(a.state_dict()) == list(ref.state_dict())
    users, pos, neg = _batch(f)
    la, lb = a.rec_step(users, pos, neg, **_draws(f)), ref.rec_step(users, pos, neg, **_draws(f))
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, ref.slab.grad)
    la, lb = a.rec_step(users, pos, neg), ref.rec_step(users, pos, neg)   # the Philox draws of step 1
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, ref.slab.grad)
    au = torch.arange(a.n_users, device=DEV)
    assert torch.equal(a.full_sort_predict([au]), ref.full_sort_predict([au]))
    a.pre_epoch_processing()
    assert a.extra_state() == {"counters": {"step": 2, "eval_pass": 1}} == ref.extra_state()


@pytest.mark.parametrize("over,key", [({"use_denoise": True}, "use_denoise"), ({"use_2rf": True}, "use_2rf"),
                                      ({"rf_hidden_dim": 256}, "rf_hidden_dim")])
def test_unsupported_settings_raise(f, over, key):
    with pytest.raises(NotImplementedError, match=key):
        RL.build_rflgmrec(f, **over)


def test_world_size_two_raises(f, monkeypatch):
    from gmr import dist
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        RL.build_rflgmrec(f)


def test_step_parity(f, g):
    m = _model(f, g)
    assert m._training_epoch == -1
    m.pre_epoch_processing()
    assert m._training_epoch == 0 and m.rf_generator.epoch == 0
    ref, *_ = F.build_lgmrec(f, "B")
    users, pos, neg = _batch(f)
    gen = m.rf_generator
    p0, v0 = m.slab.data.clone(), gen.slab.data.clone()
    seen = {}
    step = gen.train_step

    def spy(X1, cond, *a, **kw):
        seen.update(X1=X1.data_ptr(), cond=cond.data_ptr(), ldc=cond.stride(0), prior=kw["prior"].data_ptr())
        seen["tables"] = tuple(x.clone() for x in (X1, cond, kw["prior"]))
        return step(X1, cond, *a, **kw)

    gen.train_step = spy
    want_loss = ref.rec_step(users, pos, neg, **_draws(f))
    loss = m.rec_step(users, pos, neg, rf_draws=RL.draws(g), **_draws(f))
    del gen.train_step
    # LGMRec's loss terms and its six gradients: the LGMRec class's bit for bit; parameters untouched
    assert torch.equal(loss, want_loss) and torch.equal(m.slab.data, p0)
    assert torch.equal(m.loss_terms(), ref.loss_terms())
    assert len(m.grad_views()) == 6
    for a, b, k in zip(m.grad_views(), ref.grad_views(), F.PARAMS):
        assert torch.equal(a, b), k
    assert torch.equal(m.slab.grad, ref.slab.grad)
    assert torch.equal(m.all, ref.all) and torch.equal(m.cge, ref.cge) and torch.equal(m.S, ref.S)
    np.testing.assert_allclose(loss.item(), f["B_loss"], rtol=1e-5)
    # the RF step saw the model's own tables, no copy: cge, and the hop buffer that held mge at that moment
    assert seen["X1"] == m.cge.data_ptr() and seen["cond"] == m._mm[0].data_ptr() and seen["ldc"] == 128
    assert seen["prior"] == m._prior.data_ptr()
    X1, cond, prior = (x.cpu().numpy() for x in seen["tables"])
    np.testing.assert_allclose(X1, g["B_X1"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(cond, g["B_cond"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(prior, g["B_prior"], rtol=1e-5, atol=2e-6)
    assert not torch.equal(m._mm[0], seen["tables"][1])   # the backward has reused the buffer since
    assert np.abs(prior[:m.n_users]).max() > 1e-3 and np.abs(cond[:m.n_users]).max() > 1e-3   # dense user rows
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
    assert m.extra_state() == {"counters": {"step": 1, "eval_pass": 0}, "rf_epoch": 0, "rf_step": 1}


def test_conditions_are_the_forwards_mge(f, g):
    """The RF step trains on cge and mge as the step's forward wrote them: a second model's _forward with the same
    draws, its cge and mge snapshotted before any backward, and train_step on the snapshots gives the step's RF
    losses and velocity gradients bit for bit.  An RF step after the backward would read gradient rows in mge."""
    users, pos, neg = _batch(f)
    m = _model(f, g)
    m.pre_epoch_processing()
    m.rec_step(users, pos, neg, rf_draws=RL.draws(g), **_draws(f))
    other = _model(f, g)
    other.pre_epoch_processing()
    cge = other._forward(train=True, step=0, **_draws(f))
    snap_cge, snap_mge = cge.clone(), other.mge.clone()
    _, _, prior = other.rf_step_inputs(cge)
    terms = other.rf_generator.train_step(snap_cge, snap_mge, users, pos, prior=prior.clone(), **RL.draws(g))
    assert torch.equal(terms, m.rf_loss_terms())
    assert torch.equal(other.rf_generator.slab.grad, m.rf_generator.slab.grad)
    assert torch.equal(other.rf_generator.slab.data, m.rf_generator.slab.data)
    # and the buffer does not survive the step: what m.mge names now is not the forward's table
    assert not torch.equal(m.mge, snap_mge)
    late = _model(f, g).rf_generator.train_step(snap_cge, m.mge, users, pos, prior=prior, **RL.draws(g))
    assert not torch.equal(late, m.rf_loss_terms())


def test_predict(f, g):
    m = _model(f, g, prefix="p1_", rf_warmup_epochs=1)
    U = m.n_users
    users = torch.arange(U, device=DEV)
    ref, *_ = F.build_lgmrec(f, "B")
    noise = torch.as_tensor(f["B_g_eval"]).to(DEV)
    want_pre = ref.full_sort_predict([users], noise)
    gen = m.rf_generator
    m._training_epoch = 0
    gen.set_epoch(0)  # before warm-up: the LGMRec class's tables bit for bit, and the sampler is not launched
    m._mixc.fill_(NAN)
    pre = m.full_sort_predict([users], noise)
    assert torch.equal(pre, want_pre) and torch.equal(m.all, ref.all) and bool(torch.isnan(m._mixc).all())
    np.testing.assert_allclose(pre.cpu().numpy(), g["B_scores_pre"], rtol=1e-5, atol=1e-4)
    cge0, E0 = m.cge.clone(), m.slab.view("E").clone()
    gen.set_epoch(1)  # warmed up: cge' = cge + 0.2 generate(mge) from the recorded start noise, then the hypergraph block
    z0 = torch.as_tensor(g["B_z0"]).to(DEV)
    mix = m.full_sort_predict([users], noise, z0=z0)
    assert torch.equal(m.cge, cge0) and torch.equal(m.cge, ref.cge) and torch.equal(m.slab.view("E"), E0)
    # the fp64 and fp32 restatements of the same chain
    c = dict(F.CASES["B"])
    VP1 = {n: g["B_p1_" + R.key(n)] for n in R.param_names(L)}
    ev = {}
    for dt in (torch.float64, torch.float32):
        fw = RL.forward_ref(F.case_params(f, "B"), (f["v_feat"], f["t_feat"]), U, m.n_items, f["train_rows"],
                            f["train_cols"], c, f["B_g_eval"], None, dt)
        ev[dt] = {k: v.numpy().astype(np.float64) for k, v in
                  RL.eval_ref(fw, VP1, g["B_z0"], U, c, int(g["steps"]), L, float(g["ratio"])).items()}
        ev[dt]["cond"] = torch.cat(fw["mge"], dim=1).numpy().astype(np.float64)
    e64, e32 = ev[torch.float64], ev[torch.float32]
    _against_golden(m.mge, g["B_cond_eval"], e64["cond"], e32["cond"], "eval conditions")
    _against_golden(m._mixc, g["B_cgemix_eval"], e64["cgemix"], e32["cgemix"], "cge'")
    _against_golden(m.all, g["B_eval"], e64["all"], e32["all"], "all from cge'")
    want = g["B_scores_mix"]
    serr = np.abs(mix.cpu().numpy().astype(np.float64) - want).max()
    # a score is a 64-term product of two rows within the table bar: its error is at most the sum over the terms of
    # |u| d_i + |i| d_u with d the table bar
    a = np.abs(g["B_eval"].astype(np.float64))
    d = 1e-5 * a + 2 * np.abs(e32["all"] - e64["all"]).max() + np.abs(g["B_eval"] - e64["all"]).max()
    sbar = (a[:U] @ d[U:].T + d[:U] @ a[U:].T).max() + 1e-5 * np.abs(want).max()
    print(f"mixed scores: max abs error {serr:.3e} (bar {sbar:.3e}, largest score {np.abs(want).max():.3f})")
    assert serr <= sbar
    # it is not the other RF models' rule: all + ratio gen is far from the table
    late = ref.all.double() + float(g["ratio"]) * torch.as_tensor(g["B_gen_eval"]).to(DEV).double()
    assert float((m.all.double() - late).abs().max()) > 1e-2
    moved = (m.all - ref.all).abs()
    assert float(moved[:U].max()) > 0.05 and float(moved[U:].max()) > 0.05
    assert float((mix - pre).abs().max()) > 1.0
    # Philox draws: deterministic at given counters, finite, and another table than LGMRec's
    n0 = m._eval_pass
    s1 = m.full_sort_predict([users]).clone()
    assert m._eval_pass == n0 + 1
    m._eval_pass = n0
    s2 = m.full_sort_predict([users])
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all()) and not torch.equal(s1, pre)


def test_no_mixed_table_leaks_into_training(f, g):
    """A training step after a warmed-up evaluation is the same step without it, bit for bit."""
    users, pos, neg = _batch(f)
    au = torch.arange(int(f["U"]), device=DEV)
    noise = torch.as_tensor(f["B_g_eval"]).to(DEV)
    outs = []
    for evaluate in (False, True):
        m = _model(f, g)  # rf_warmup_epochs 0: warmed up from the first epoch
        m.pre_epoch_processing()
        if evaluate:
            assert m.rf_generator.warmed_up()
            ref, *_ = F.build_lgmrec(f, "B")
            assert not torch.equal(m.full_sort_predict([au], noise), ref.full_sort_predict([au], noise))
        loss = m.rec_step(users, pos, neg, rf_draws=RL.draws(g), **_draws(f)).clone()
        outs.append((loss, m.slab.grad.clone(), m.all.clone(), m._prior.clone(), *_rf_state(m)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cf_model", ["lightgcn", "mf"])
def test_mid_shape(cf_model):
    """U = 300, I = 1,100 (3 + 9 blocks of the prior kernel with both last blocks short; N = 1,400 = 43 sampler tiles
    and 24 rows; widths 37 / 50; B = 700 with repeated users), case B's settings (n_hyper_layer 2, hyper_num 5,
    keep_rate 0.5), at cf_model lightgcn and mf, with injected Gumbel draws, keep masks and InfoNCE negatives; X0 and t
    are the model's Philox draws read back.  One step and one warm evaluation against the fp64 restatement: LGMRec's
    loss at 1e-5, the RF tables and the evaluation tables at the bar, the RF losses at 1e-5, v at rtol 1e-5 next to
    twice the fp32 restatement's own error, the velocity gradients at 4x that restatement's own error (floored at 1e-6
    of the parameter's largest gradient: the rule of test_rfsmore_gpu.py)."""
    m, d = RL.build_rflgmrec_mid(cf_model=cf_model)
    m.pre_epoch_processing()
    U, I, N, H = m.n_users, m.n_items, m.N, m.hyper_num
    assert -(-U // 128) == 3 and -(-I // 128) == 9 and N % 32 == 24 and m.n_hyper_layer == 2 and m.keep_rate == 0.5
    gen = m.rf_generator
    P = {k: v.detach().cpu().numpy().copy() for k, v in zip(F.PARAMS, m._params())}
    VP = {n: v.cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    users, pos, neg = (torch.as_tensor(d[k]).to(DEV) for k in ("users", "pos", "neg"))
    rng = np.random.default_rng(11)
    gd = rng.gumbel(size=(2, N, H)).astype(np.float32)
    keep = (rng.random((2, N, H)) < 0.5).astype(np.uint8)
    ni = R.collide(rng.integers(0, I, (len(d["pos"]), 7)), d["pos"], I).astype(np.int32)
    nu = R.collide(rng.integers(0, U, (len(d["users"]), 7)), d["users"], U).astype(np.int32)
    E0 = m.slab.view("E").clone()
    seen = {}
    step = gen.train_step

    def spy(X1, cond, *a, **kw):
        seen["tables"] = tuple(x.clone() for x in (X1, cond, kw["prior"]))
        seen["X1"] = X1.data_ptr()
        return step(X1, cond, *a, **kw)

    gen.train_step = spy
    loss = m.rec_step(users, pos, neg, g=torch.as_tensor(gd).to(DEV), keep=torch.as_tensor(keep).to(DEV),
                      rf_draws={"neg_items": torch.as_tensor(ni).to(DEV), "neg_users": torch.as_tensor(nu).to(DEV)})
    del gen.train_step
    assert seen["X1"] == (m.slab.view("E") if cf_model == "mf" else m.cge).data_ptr()
    dr = {"X0": gen._w["X0"].cpu().numpy(), "t": gen._w["t"].cpu().numpy().reshape(N, 1), "neg_items": ni,
          "neg_users": nu}
    assert np.isfinite(dr["X0"]).all() and abs(dr["X0"].mean()) < 0.02 and abs(dr["X0"].std() - 1) < 0.02
    c = dict(F.CASES["B"], cf_model=cf_model)
    feats = (d["v_feat"], d["t_feat"])
    res = {}
    for dt in (torch.float64, torch.float32):
        fw = RL.forward_ref(P, feats, U, I, d["rows"], d["cols"], c, gd, keep, dt)
        X1, cond, prior = RL.rf_inputs_ref(fw, U)
        out, grads = RL.rf_step_ref(VP, X1.numpy(), cond.numpy(), prior.numpy(), dr, d["users"], d["pos"], U, gen.L, dt)
        res[dt] = (X1.numpy(), cond.numpy(), prior.numpy(), out, grads)
    r = F.lgmrec_step_ref(P, U, I, d["rows"], d["cols"], d["users"], d["pos"], d["neg"], c, feats, gd, keep)
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy()[1:], r["terms"], rtol=1e-5)
    a64, a32 = res[torch.float64], res[torch.float32]
    for i, what in enumerate(("X1 = cge", "cond = mge", "prior")):
        F.bar(seen["tables"][i], a64[i].astype(np.float64), a32[i], f"mid {cf_model} {what}")
    o64, g64, o32, g32 = a64[3], a64[4], a32[3], a32[4]
    terms = m.rf_loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], o64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(terms[1], o64["cl_loss"].item(), rtol=1e-5)
    v64 = o64["v"].detach().numpy()
    own = float(np.abs(o32["v"].detach().numpy().astype(np.float64) - v64).max())
    err = float(np.abs(gen._w["V"].cpu().numpy().astype(np.float64) - v64).max())
    print(f"mid {cf_model}: v max abs error {err:.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), v64, rtol=1e-5, atol=2 * own)
    worst = (0.0, 0.0)
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        want = g64[name].numpy()
        bar = max(4 * R.rel_to_max(g32[name].numpy(), want), 1e-6)
        err = R.rel_to_max(got.cpu().numpy(), want)
        worst = max(worst, (err, bar))
        assert err <= bar, (name, err, bar)
    print(f"mid {cf_model}: velocity gradients, worst error relative to the parameter's max {worst[0]:.3e} "
          f"(bar {worst[1]:.3e})")
    # the warm evaluation at this shape: the sampler over 44 tiles with the mix as its epilogue, then the hypergraph
    # block on cge', from injected noise and z0
    gen.set_epoch(gen.warmup_epochs)
    ge = rng.gumbel(size=(2, N, H)).astype(np.float32)
    z0 = rng.standard_normal((N, 64)).astype(np.float32)
    m.forward_embeddings(noise=torch.as_tensor(ge).to(DEV), z0=torch.as_tensor(z0).to(DEV))
    assert torch.equal(m.slab.view("E"), E0)   # the parameter table is not written (at mf it is cge itself)
    VP1 = {n: v.cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    ev = {}
    for dt in (torch.float64, torch.float32):
        fw = RL.forward_ref(P, feats, U, I, d["rows"], d["cols"], c, ge, None, dt)
        ev[dt] = {k: v.numpy().astype(np.float64) for k, v in
                  RL.eval_ref(fw, VP1, z0, U, c, gen.sampling_steps, gen.L, gen.inference_mix_ratio).items()}
    F.bar(m._mixc, ev[torch.float64]["cgemix"], ev[torch.float32]["cgemix"], f"mid {cf_model} cge'")
    F.bar(m.all, ev[torch.float64]["all"], ev[torch.float32]["all"], f"mid {cf_model} all from cge'")


def test_philox_step_is_finite_and_reproducible(f):
    users, pos, neg = _batch(f)
    outs = []
    for _ in range(2):
        m = _model(f, rf_dropout=0.1, rf_infonce_negatives=1024)
        m.pre_epoch_processing()
        losses = [m.rec_step(users, pos, neg).item() for _ in range(2)]
        tab = torch.cat([x.clone() for x in m.forward_embeddings()])
        outs.append((losses, m.slab.grad.clone(), m._prior.clone(), tab, *_rf_state(m)))
    a, b = outs
    assert np.isfinite(a[0]).all() and all(bool(torch.isfinite(t).all()) for t in a[1:])
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert m.extra_state() == {"counters": {"step": 2, "eval_pass": 1}, "rf_epoch": 0, "rf_step": 2}


def test_fit_and_evaluate():
    """Two epochs through the generic Trainer on gmr/synthetic.py data (the path of main.py --model RFLGMRec) with
    rf_warmup_epochs 1: finite losses and metrics, and an evaluation that changes both halves of the table."""
    from gmr.configurator import Config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.lgmrec import LGMRec
    from gmr.rflgmrec import RFLGMRec
    from gmr.synthetic import make_dataset
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    cfg = Config("RFLGMRec", "baby", {"synthetic": "tiny", "epochs": 2, "save_recommended_topk": False,
                                      "rf_warmup_epochs": 1, "rf_infonce_negatives": 64, "rf_sampling_steps": 2})
    init_seed(999)
    ds = make_dataset(cfg, "tiny", seed=0)
    tr, va, te = ds.split()
    tl = TrainDataLoader(cfg, tr, batch_size=cfg["train_batch_size"], shuffle=True)
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
    m = RFLGMRec(cfg, tl)
    p0 = m.rf_generator.slab.data.clone()
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    assert np.isfinite(trainer.train_loss_dict[0]) and np.isfinite(trainer.train_loss_dict[1])
    assert "recall@10" in valid and all(np.isfinite(v) for v in trainer.evaluate(vl).values())
    gen = m.rf_generator
    assert m._training_epoch == 1 and gen.warmed_up() and gen.step_ctr == 2 * len(tl) == m._step
    assert bool(torch.isfinite(m.rf_loss_terms()).all()) and not torch.equal(gen.slab.data, p0)
    noise = torch.as_tensor(np.random.default_rng(0).gumbel(size=(2, m.N, m.hyper_num)).astype(np.float32)).to(DEV)
    usr, itm = (x.clone() for x in m.forward_embeddings(noise))
    bu, bi = LGMRec.forward_embeddings(m, noise)
    assert not torch.equal(itm, bi) and not torch.equal(usr, bu)
    assert bool(torch.isfinite(usr).all()) and bool(torch.isfinite(itm).all())
    sd = m.state_dict()
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(sd)


def test_quick_start(tmp_path, monkeypatch):
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False,
                "rf_warmup_epochs": 1, "rf_infonce_negatives": 64, "rf_sampling_steps": 2}
    results = quick_start("RFLGMRec", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    assert "recall@10" in best_valid and all(0.0 <= v <= 1.0 for v in best_valid.values())
    ck = torch.load(str(saved / "RFLGMRec-baby.pth"), map_location="cpu", weights_only=True)
    assert {"config", "epoch", "state_dict", "optimizer", "best_valid_score"} <= set(ck)
    assert list(ck["state_dict"])[:len(F.STATE_KEYS)] == F.STATE_KEYS
    assert {"counters", "rf_epoch", "rf_step"} == set(ck["generated_graphs"])
    assert set(ck["generated_graphs"]["counters"]) == {"step", "eval_pass"}
