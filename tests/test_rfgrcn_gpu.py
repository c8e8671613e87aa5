"""RFGRCN (gmr/rfgrcn.py) against the reference's golden values (tests/golden/make_golden_rfgrcn.py: case A of
grcn_tiny.npz with the RF draws recorded) with those draws injected, against the GRCN class itself, and, where the
reference recorded nothing (image features alone, D = C = 128), against the fp64 restatement on the model's own tables.

Bars (tests/rfgrcn_fixture.py): tables at rtol 1e-5 / atol 2e-6, losses at rtol 1e-5, velocity gradients at 4x the
record's fp32-vs-fp64 spread relative to the parameter's largest gradient (rf_fixture.grad_bar), the sampler's rows at
4x the record's fp32-vs-fp64 spread (floored at 1e-6 of the largest value) next to what the table bar on the
conditions moves the fp64 sampler by (measured on the restatement: the conditions of the record are the CPU table, the
model's its own).

Seen on the MI355X: X1 and prior 9.5e-07 from the record on entries up to 9 (table bar 1e-5 |x| + 2e-6); rf_loss
1.2456543 and cl_loss 8.7382126, the record's to eight digits; velocity gradients 8.8e-07 of the parameter's largest
(bar 2.9e-06); cached scores 1.5e-05 on scores up to 96 (bar 4.2e-03); sampler rows 5.9e-07 from the fp64 run on the
model's table and 7.7e-07 from the record (bar 4.6e-06; the conditions move the fp64 rows by 1.1e-07); mixed table
9.5e-07 (bar 4.4e-05 at that entry), mixed scores 6.1e-05 (bar 4.5e-03); image only: worst gradient 4.4e-07 (bar
1.5e-06).
"""
import numpy as np
import pytest
import torch

import grcn_fixture as F
import rf_fixture as R
import rfbm3_fixture as RB
import rfgrcn_fixture as RG

pytestmark = pytest.mark.gpu
DEV = F.DEV
NAN = float("nan")
L = RG.L


@pytest.fixture(scope="module")
def f(golden):
    return golden("grcn_tiny")


@pytest.fixture(scope="module")
def g(golden):
    return RG.load_golden(golden)


def _batch(f):
    return [torch.as_tensor(f[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _model(f, g=None, prefix="p0_", case="A", **over):
    m, cfg, ds, tl = RG.build_rfgrcn(f, case, **over)
    if g is not None:
        m.rf_generator.load_reference_state({n: g["A_" + prefix + R.key(n)] for n in R.param_names(L)})
    return m


def _spy(gen, seen):
    step = gen.train_step

    def spy(X1, cond, *a, **kw):
        seen.update(X1=X1.data_ptr(), cond=cond.data_ptr(), ld=X1.stride(0), prior=kw["prior"].data_ptr())
        seen["tables"] = (X1.clone(), kw["prior"].clone())
        return step(X1, cond, *a, **kw)

    gen.train_step = spy


def test_registry_and_init(f):
    from gmr.rfgrcn import RFGRCN
    from gmr.utils import get_model
    assert get_model("RFGRCN") is RFGRCN
    m, *_ = RG.build_rfgrcn(f, as_drawn=True)
    assert [n.replace(".", "_") for n, p in m.named_parameters() if p.requires_grad] == F.PARAMS
    for p, k in zip(m._params(), F.PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), f["A_init_" + k]), k
    gen = m.rf_generator
    assert gen.D == gen.C == m.width == 192 and gen.N == m.N and gen.L == 2 and gen.slab.numel == RG.N_PARAMS
    assert m._prior.shape == (m.N, 192) and m._mix is None and m.rf_eval == "cached"
    assert _model(f, rf_eval="mixed")._mix.shape == (m.N, 192)


def test_use_rf_false_is_grcn(f):
    a = _model(f, use_rf=False)
    ref, *_ = F.build_grcn(f, "A")
    assert a.rf_generator is None and not any(hasattr(a, k) for k in ("_prior", "_mix", "_pws"))
    assert list(a.state_dict()) == list(ref.state_dict())
    users, pos, neg = _batch(f)
    la, lb = a.rec_step(users, pos, neg), ref.rec_step(users, pos, neg)
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, ref.slab.grad)
    au = torch.arange(a.n_users, device=DEV)
    assert torch.equal(a.full_sort_predict([au]), ref.full_sort_predict([au]))
    assert a.extra_state() == {} and not hasattr(ref, "extra_state")


@pytest.mark.parametrize("over,key,exc", [({"use_denoise": True}, "use_denoise", NotImplementedError),
                                          ({"use_2rf": True}, "use_2rf", NotImplementedError),
                                          ({"rf_hidden_dim": 64}, "rf_hidden_dim", NotImplementedError),
                                          ({"rf_eval": "other"}, "rf_eval", ValueError)])
def test_unsupported_settings_raise(f, over, key, exc):
    with pytest.raises(exc, match=key):
        RG.build_rfgrcn(f, **over)


def test_world_size_two_raises(f, monkeypatch):
    from gmr import dist
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        RG.build_rfgrcn(f)


def test_step_parity(f, g):
    m = _model(f, g)
    assert m._training_epoch == -1
    m.pre_epoch_processing()
    assert m._training_epoch == 0 and m.rf_generator.epoch == 0
    ref, *_ = F.build_grcn(f, "A")
    users, pos, neg = _batch(f)
    gen = m.rf_generator
    p0, v0 = m.slab.data.clone(), gen.slab.data.clone()
    seen = {}
    _spy(gen, seen)
    want_loss = ref.rec_step(users, pos, neg)
    loss = m.rec_step(users, pos, neg, rf_draws=RG.draws(g))
    del gen.train_step
    # GRCN's loss and its eight gradients: the GRCN class's bit for bit; parameters untouched
    assert torch.equal(loss, want_loss) and torch.equal(m.slab.data, p0)
    assert torch.equal(m.loss_terms(), ref.loss_terms())
    assert len(m.grad_views()) == 8
    for a, b, k in zip(m.grad_views(), ref.grad_views(), F.PARAMS):
        assert torch.equal(a, b), k
    assert torch.equal(m.slab.grad, ref.slab.grad)
    np.testing.assert_allclose(loss.item(), f["A_loss"], rtol=1e-5)
    # the RF step saw the model's own table, no copy, as X1 and as cond; GRCN's backward has not written it
    assert seen["X1"] == seen["cond"] == m.result.data_ptr() and seen["ld"] == 192
    assert seen["prior"] == m._prior.data_ptr()
    assert torch.equal(m.result, seen["tables"][0]) and torch.equal(m.result, ref.result)
    fw = m.result.clone()
    m._forward()
    assert torch.equal(m.result, fw), "self.result after rec_step is what _forward wrote"
    X1, prior = (x.cpu().numpy() for x in seen["tables"])
    print(f"X1 max abs error {np.abs(X1 - g['A_X1']).max():.3e}, prior {np.abs(prior - g['A_prior']).max():.3e} "
          f"(table bar: 1e-5 |x| + 2e-6)")
    np.testing.assert_allclose(X1, g["A_X1"], **RG.TABLE)
    np.testing.assert_allclose(prior, g["A_prior"], **RG.TABLE)
    terms = m.rf_loss_terms().cpu().numpy()
    print(f"rf_loss {terms[0]:.7f} ({g['A_rf_loss']:.7f}), cl_loss {terms[1]:.7f} ({g['A_cl_loss']:.7f})")
    np.testing.assert_allclose(terms[0], g["A_rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1], g["A_cl_loss"], rtol=1e-5)
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), g["A_v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gen._w["pred"].cpu().numpy(), g["A_pred"], rtol=1e-5, atol=1e-6)
    bar = R.grad_bar(g, "A_")
    worst = 0.0
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        err = R.rel_to_max(got.cpu().numpy(), g["A_g_" + R.key(name)])
        worst = max(worst, err)
        assert err <= bar, (name, err, bar)
    print(f"velocity gradients: worst error relative to the parameter's max {worst:.3e} (bar {bar:.3e})")
    assert not torch.equal(gen.slab.data, v0)
    for (name, _), p in zip(gen.specs, gen.param_views()):
        got, want = p.cpu().numpy(), g["A_p1_" + R.key(name)]
        assert (np.abs(got - want) <= RB.p1_bound(g, "A_", name, bar, float(g["lr"]))).all(), name
    assert m.extra_state() == {"rf_epoch": 0, "rf_step": 1}


@pytest.mark.parametrize("warm", [False, True])
def test_cached_evaluation_is_grcn(f, g, warm):
    """rf_eval: cached (the reference as written): the scores are GRCN's bit for bit, before any step (the init table)
    and after one, whatever the warm-up state; the sampler is never launched."""
    m = _model(f, g, rf_warmup_epochs=0 if warm else 5)
    ref, *_ = F.build_grcn(f, "A")
    m.pre_epoch_processing()
    assert m.rf_warm() == warm
    au = torch.arange(m.n_users, device=DEV)
    gen = m.rf_generator
    gen.generate = None  # a call would raise
    s0 = m.full_sort_predict([au])
    t0 = torch.as_tensor(f["A_result0"]).to(DEV)
    assert torch.equal(s0, ref.full_sort_predict([au]))
    want0 = torch.empty_like(s0)
    from gmr import kernels as K
    K.gemm(t0[:m.n_users].contiguous(), t0[m.n_users:].contiguous(), want0, trans_b=True)
    assert torch.equal(s0, want0), "before any step: the init table's scores"
    users, pos, neg = _batch(f)
    m.rec_step(users, pos, neg, rf_draws=RG.draws(g))
    ref.rec_step(users, pos, neg)
    s1 = m.full_sort_predict([au])
    assert torch.equal(s1, ref.full_sort_predict([au])) and not torch.equal(s1, s0)
    serr = np.abs(s1.cpu().numpy().astype(np.float64) - g["A_scores_cached"]).max()
    a = np.abs(g["A_X1"].astype(np.float64))
    d = 1e-5 * a + 2e-6
    U = m.n_users
    sbar = (a[:U] @ d[U:].T + d[:U] @ a[U:].T).max() + 1e-5 * np.abs(g["A_scores_cached"]).max()
    print(f"cached scores: max abs error {serr:.3e} (bar {sbar:.3e})")
    assert serr <= sbar


def test_mixed_evaluation(f, g):
    m = _model(f, g, prefix="p1_", rf_eval="mixed", rf_warmup_epochs=1)
    ref, *_ = F.build_grcn(f, "A")
    U = m.n_users
    au = torch.arange(U, device=DEV)
    gen = m.rf_generator
    m.pre_epoch_processing()           # epoch 0: before warm-up the recomputed GRCN table bit for bit, no sampler
    assert not m.rf_warm()
    m._mix.fill_(NAN)
    usr, itm = m.forward_embeddings()
    assert torch.equal(torch.cat([usr, itm]), ref.forward()) and bool(torch.isnan(m._mix).all())
    assert usr.data_ptr() == m.result.data_ptr()
    m.pre_epoch_processing()           # epoch 1: warmed up
    assert m.rf_warm()
    z0 = torch.as_tensor(g["A_z0_eval"]).to(DEV)
    scores = m.full_sort_predict([au], z0=z0)
    res = m.result.clone()
    assert torch.equal(res, ref.result), "the mix is written to a table of its own"
    np.testing.assert_allclose(res.cpu().numpy(), g["A_X1"], **RG.TABLE)
    # the sampler's rows from the recorded z0 on the model's own table
    rows = gen.generate(m.result, z0=z0).cpu().numpy().astype(np.float64)
    VP1 = {n: g["A_p1_" + R.key(n)] for n in R.param_names(L)}
    own = RG.generate_ref(VP1, res.cpu().numpy(), g["A_z0_eval"], int(g["steps"]), L, torch.float64)
    rec = RG.generate_ref(VP1, g["A_X1"], g["A_z0_eval"], int(g["steps"]), L, torch.float64)
    moved = float(np.abs(own - rec).max())   # what the table bar on the conditions does to the fp64 sampler
    sb = max(4 * float(g["A_err_sample"]), 1e-6 * float(np.abs(g["A_gen_eval"]).max()))
    err_own = float(np.abs(rows - own).max())
    err_rec = float(np.abs(rows - g["A_gen_eval"]).max())
    print(f"sampler rows: {err_own:.3e} from the fp64 run on the model's table, {err_rec:.3e} from the record "
          f"(sampler bar {sb:.3e}, the conditions move the fp64 rows by {moved:.3e})")
    assert err_own <= sb and err_rec <= sb + moved
    # the mixed table: one fused multiply-add per element on those rows
    ratio = float(g["ratio"])
    mix = m._mix.cpu().numpy().astype(np.float64)
    tb = 1e-5 * np.abs(g["A_eval"]) + 2e-6 + ratio * (sb + moved) + 2.0 ** -23 * np.abs(g["A_eval"])
    terr = np.abs(mix - g["A_eval"])
    print(f"mixed table: max abs error {terr.max():.3e} (bar at that entry {tb.flat[terr.argmax()]:.3e})")
    assert (terr <= tb).all()
    want = g["A_scores_mix"]
    a = np.abs(g["A_eval"].astype(np.float64))
    sbar = (a[:U] @ tb[U:].T + tb[:U] @ a[U:].T).max() + 1e-5 * np.abs(want).max()
    serr = np.abs(scores.cpu().numpy().astype(np.float64) - want).max()
    print(f"mixed scores: max abs error {serr:.3e} (bar {sbar:.3e}, largest score {np.abs(want).max():.3f})")
    assert serr <= sbar
    assert float((scores - ref.full_sort_predict([au])).abs().max()) > 1.0
    # Philox start noise: deterministic at the generator's counters, finite, another table
    s1, s2 = m.full_sort_predict([au]).clone(), m.full_sort_predict([au])
    assert torch.equal(s1, s2) and bool(torch.isfinite(s1).all()) and not torch.equal(s1, scores)


def test_image_only_runs_at_128(f):
    """Case C (image features alone): D = C = 128.  One step with injected draws against the fp64 restatement on the
    model's own table; the velocity gradients at 4x the fp32 restatement's own error (floored at 1e-6)."""
    m = _model(f, case="C")
    ref, *_ = F.build_grcn(f, "C")
    m.pre_epoch_processing()
    gen = m.rf_generator
    U, I, N = m.n_users, m.n_items, m.N
    assert m.width == gen.D == gen.C == 128 and gen.slab.numel == RG.N_PARAMS_128
    VP = {n: v.cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    users, pos, neg = _batch(f)
    rng = np.random.default_rng(5)
    dr = {"X0": rng.standard_normal((N, 128)).astype(np.float32), "t": rng.random((N, 1)).astype(np.float32),
          "neg_items": R.collide(rng.integers(0, I, (16, 7)), f["pos"], I).astype(np.int32),
          "neg_users": R.collide(rng.integers(0, U, (16, 7)), f["users"], U).astype(np.int32)}
    seen = {}
    _spy(gen, seen)
    loss = m.rec_step(users, pos, neg, rf_draws={k: torch.as_tensor(v).to(DEV) for k, v in dr.items()})
    del gen.train_step
    assert torch.equal(loss, ref.rec_step(users, pos, neg)) and torch.equal(m.slab.grad, ref.slab.grad)
    X1, prior = (x.cpu().numpy() for x in seen["tables"])
    assert X1.shape == (N, 128) and seen["ld"] == 128
    np.testing.assert_allclose(X1, f["C_result"], **RG.TABLE)
    np.testing.assert_allclose(prior, RG.prior_ref(torch.tensor(X1, dtype=torch.float64), U).numpy(), **RG.TABLE)
    res = {dt: RG.rf_step_ref(VP, X1, X1, prior, dr, f["users"], f["pos"], U, L, dt)
           for dt in (torch.float64, torch.float32)}
    (o64, g64), (_, g32) = res[torch.float64], res[torch.float32]
    terms = m.rf_loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], o64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(terms[1], o64["cl_loss"].item(), rtol=1e-5)
    worst = (0.0, 0.0, 0.0)
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        want = g64[name].numpy()
        bar = RG.grad_bar(g32[name].numpy(), want)
        err = R.rel_to_max(got.cpu().numpy(), want)
        worst = max(worst, (err / bar, err, bar))
        assert err <= bar, (name, err, bar)
    print(f"image only: rf {terms[0]:.7f} cl {terms[1]:.7f}; worst gradient error {worst[1]:.3e} (bar {worst[2]:.3e})")
    m2 = _model(f, case="C", rf_eval="mixed")
    m2.pre_epoch_processing()
    usr, itm = m2.forward_embeddings()
    assert usr.shape[1] == 128 and bool(torch.isfinite(usr).all()) and bool(torch.isfinite(itm).all())
    assert not torch.equal(torch.cat([usr, itm]), m2.result)


def test_philox_steps_are_finite_and_reproducible(f):
    users, pos, neg = _batch(f)
    outs = []
    for _ in range(2):
        m = _model(f, rf_dropout=0.1, rf_infonce_negatives=40, rf_eval="mixed")
        m.pre_epoch_processing()
        v0 = m.rf_generator.slab.data.clone()
        losses = [m.rec_step(users, pos, neg).item() for _ in range(2)]
        tab = torch.cat([x.clone() for x in m.forward_embeddings()])
        gen = m.rf_generator
        outs.append((losses, m.slab.grad.clone(), m._prior.clone(), tab, m.rf_loss_terms().clone(), gen.slab.grad.clone(),
                     gen.slab.data.clone()))
        assert not torch.equal(gen.slab.data, v0)
    a, b = outs
    assert np.isfinite(a[0]).all() and all(bool(torch.isfinite(t).all()) for t in a[1:])
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert m.extra_state() == {"rf_epoch": 0, "rf_step": 2}


def test_fit_and_evaluate():
    """Two epochs through the generic Trainer on gmr/synthetic.py data (the path of main.py --model RFGRCN) with
    rf_eval: mixed and rf_warmup_epochs 1: finite losses and metrics, and an evaluation the generator moves."""
    from gmr.configurator import Config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.rfgrcn import RFGRCN
    from gmr.synthetic import make_dataset
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    cfg = Config("RFGRCN", "baby", {"synthetic": "tiny", "epochs": 2, "save_recommended_topk": False,
                                    "rf_warmup_epochs": 1, "rf_infonce_negatives": 64, "rf_sampling_steps": 2,
                                    "rf_eval": "mixed"})
    init_seed(999)
    ds = make_dataset(cfg, "tiny", seed=0)
    tr, va, te = ds.split()
    tl = TrainDataLoader(cfg, tr, batch_size=cfg["train_batch_size"], shuffle=True)
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
    m = RFGRCN(cfg, tl)
    p0 = m.rf_generator.slab.data.clone()
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    assert np.isfinite(trainer.train_loss_dict[0]) and np.isfinite(trainer.train_loss_dict[1])
    assert "recall@10" in valid and all(np.isfinite(v) for v in trainer.evaluate(vl).values())
    gen = m.rf_generator
    assert m._training_epoch == 1 and gen.warmed_up() and gen.step_ctr == 2 * len(tl)
    assert bool(torch.isfinite(m.rf_loss_terms()).all()) and not torch.equal(gen.slab.data, p0)
    usr, itm = (x.clone() for x in m.forward_embeddings())
    assert not torch.equal(torch.cat([usr, itm]), m.result) and bool(torch.isfinite(usr).all())
    sd = m.state_dict()
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(sd)
