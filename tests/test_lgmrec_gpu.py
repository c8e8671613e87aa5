"""LGMRec on the HIP path vs golden vectors from the reference (models/lgmrec.py; tiny shape,
tests/golden/make_golden_lgmrec.py: the reference rerun in double with its recorded Gumbel draws and dropout masks).
Case A: the init as drawn, one hyperedge layer, H 4, no dropout.  Case B: scaled tables and hyperedge weights (softmax
rows saturate, probabilities underflow to 0), two hyperedge layers, H 5, keep_rate 0.5, then three Adam steps.  Every
gradient is held to rtol 1e-5 + twice fp32 torch's own distance from the double rerun, stored per gradient by the
maker."""
import numpy as np
import pytest
import torch

import lgmrec_fixture as F
from lgmrec_fixture import CASES, DEV, PARAMS, build_lgmrec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return dict(golden("lgmrec_tiny"), **golden("lgmrec_tiny_B"))


def _args(g, case):
    return (F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["pos"],
            g["neg"], dict(CASES[case]), (g["v_feat"], g["t_feat"]), g[case + "_g"][0])


@pytest.fixture(scope="module")
def ref32(g):
    """The fp32 restatement of both cases on the CPU: what fp32 torch gives for the tables the reference kept no
    distance for."""
    return {case: F.lgmrec_step_ref(*_args(g, case), keep=_keep_np(g, case), g_eval=g[case + "_g_eval"],
                                    dtype=torch.float32) for case in CASES}


def _keep_np(g, case, step=0):
    return g["B_keep"][step] if case == "B" else None


def _draws(g, case, step=0):
    k = _keep_np(g, case, step)
    return (torch.as_tensor(g[case + "_g"][step]).to(DEV).contiguous(),
            None if k is None else torch.as_tensor(k).to(DEV).contiguous())


def _batch(g):
    return [torch.as_tensor(g[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _grads(m):
    return [v.cpu().numpy().copy() for v in m.grad_views()]


def _dense(csr):
    rp, col, val = (t.cpu().numpy() for t in (csr.rowptr, csr.col, csr.val))
    out = np.zeros((csr.n_rows, csr.n_cols), np.float64)
    for r in range(csr.n_rows):
        out[r, col[rp[r]:rp[r + 1]]] = val[rp[r]:rp[r + 1]]
    return out


def _bar_own(got, want, own, what, rtol=1e-5):
    got = got.astype(np.float64)
    print(f"{what}: max abs error {np.abs(got - want).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=2 * own, err_msg=what)


@pytest.mark.parametrize("case", ["A", "B"])
def test_init_parity(g, case):
    m, *_ = build_lgmrec(g, "A", **CASES[case])      # as constructed: case B's parameters before their scaling
    assert [n.replace(".", "_") for n, p in m.named_parameters() if p.requires_grad] == PARAMS
    assert list(m.state_dict()) == F.STATE_KEYS
    for p, k in zip(m._params(), PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), g[f"{case}_init_{k}"]), k
    assert [tuple(v.shape) for v in m.grad_views()] == [g[f"{case}_init_{k}"].shape for k in PARAMS]
    sd = m.state_dict()
    assert np.array_equal(sd["image_embedding.weight"].cpu().numpy(), g["v_feat"])
    assert np.array_equal(sd["text_embedding.weight"].cpu().numpy(), g["t_feat"])


def test_graphs(g):
    m, *_ = build_lgmrec(g, "A")
    U, I = m.n_users, m.n_items
    got, want = _dense(m.norm_adj), F.dense_of(g["norm_adj_idx"], g["norm_adj_val"], (U + I, U + I))
    assert np.array_equal(got != 0, want != 0)
    assert np.array_equal(got.astype(np.float32), want.astype(np.float32))       # exact
    adj = F.dense_of(g["adj_idx"], g["adj_val"], (U, I))
    assert np.array_equal(_dense(m.adj), adj) and np.array_equal(_dense(m.adj_t), adj.T)
    assert np.array_equal(m.inv_deg.cpu().numpy(), g["inv_deg"])
    assert np.array_equal(_dense(m.adj_mean), adj * g["inv_deg"].astype(np.float64)[:, None])
    assert np.array_equal(_dense(m.adj_mean_t), _dense(m.adj_mean).T)


@pytest.mark.parametrize("case", ["A", "B"])
def test_step_parity(g, ref32, case):
    tag = case + "_"
    m, *_ = build_lgmrec(g, case)
    users, pos, neg = _batch(g)
    gum, keep = _draws(g, case)
    loss = m.rec_step(users, pos, neg, g=gum, keep=keep)
    print(f"{case}: loss {loss.item():.7f} (reference {g[tag + 'loss']:.7f})")
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    print(f"{case}: terms {terms[1:]} (reference {g[tag + 'loss_terms']})")
    np.testing.assert_allclose(terms[0], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1:], g[tag + "loss_terms"], rtol=1e-5)
    r32 = ref32[case]
    F.bar(m.all, g[tag + "all"], r32["all"], f"{case} all")
    H = m.hyper_num
    S64 = F.lgmrec_step_ref(*_args(g, case), keep=_keep_np(g, case))
    for k, got in (("S", m.S), ("h", m.h)):
        got = got.cpu().numpy().reshape(-1, 2, H).transpose(1, 0, 2)
        F.bar(got, S64[k], r32[k], f"{case} {k}")
    if case == "B":
        assert (m.S == 0).any() or float(m.S.min()) < 1e-30    # the underflow path ran
    first = _grads(m)
    for got, k in zip(first, PARAMS):
        assert np.isfinite(got).all(), k
        _bar_own(got, g[tag + "g_" + k], float(g[tag + "own_" + k]), f"{case} gradient {k}")
    # every work buffer filled with NaN: nothing of a step reads what an earlier step left
    bufs = [m.S, m.h, m.dL, m.acc, m.mge_u, m.all, m.CLN, m.nrmCL, m.nrm3, m.dall, m.dK, m.dmge, m._ws, m._loss,
            *m.proj.values(), *[d[:, :64 + H] for d in m.dproj.values()], *m._mm, *m.lats, *m.dlat, *m.ilay,
            *m._layers, *m._t, *([m.cge] if m.cge is not None else []), *([m.di] if m.di is not None else []),
            *[v for v in m._w.values() if torch.is_tensor(v) and v.is_floating_point()]]
    for t in bufs:
        t.fill_(float("nan"))
    m.slab.grad.fill_(float("nan"))
    m.load_extra_state({"counters": {"step": 0, "eval_pass": 0}})
    again = m.rec_step(users, pos, neg, g=gum, keep=keep)
    assert again.item() == loss.item()
    for a, b, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b), k
    assert m.extra_state() == {"counters": {"step": 1, "eval_pass": 0}}


def test_loader_plans_give_the_same_step(g):
    m, cfg, ds, tl = build_lgmrec(g, "B")
    d = tl.epoch()
    b, sizes, u, p, ng, pb, pc = next(iter(tl.batches(d)))
    gum, keep = _draws(g, "B")
    with_plans = m.rec_step(u, p, ng, pb, pc, g=gum, keep=keep).item()
    first = _grads(m)
    assert m.rec_step(u, p, ng, g=gum, keep=keep).item() == with_plans
    for a, b_, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b_), k


def test_calculate_loss_scales_by_upstream(g):
    m, *_ = build_lgmrec(g, "A")
    users, pos, neg = _batch(g)
    base = m.rec_step(users, pos, neg).item()
    want = _grads(m)
    m.load_extra_state({"counters": {"step": 0, "eval_pass": 0}})
    inter = torch.stack([torch.as_tensor(g[k]) for k in ("users", "pos", "neg")]).to(DEV)
    out = m.calculate_loss(inter)
    assert out.item() == base
    (3.0 * out).backward()
    for p, w, k in zip(m._params(), want, PARAMS):
        np.testing.assert_allclose(p.grad.cpu().numpy(), 3.0 * w, rtol=1e-6, atol=0, err_msg=k)


@pytest.mark.parametrize("over", [dict(cf_model="mf"), dict(n_mm_layers=0, n_ui_layers=0), dict(n_hyper_layer=3),
                                  dict(n_mm_layers=3, n_ui_layers=1)])
def test_other_settings_against_the_restatement(g, over):
    """The branches the two golden cases do not take, against the fp64 restatement (pinned to the reference by
    tests/test_lgmrec_restatement_cpu.py), with the atol of fp32 torch's own error on the same step."""
    m, *_ = build_lgmrec(g, "B", **over)
    users, pos, neg = _batch(g)
    gum, keep = _draws(g, "B")
    loss = m.rec_step(users, pos, neg, g=gum, keep=keep)
    args = list(_args(g, "B"))
    args[8] = dict(args[8], **over)
    r64 = F.lgmrec_step_ref(*args, keep=_keep_np(g, "B"))
    r32 = F.lgmrec_step_ref(*args, keep=_keep_np(g, "B"), dtype=torch.float32)
    np.testing.assert_allclose(loss.item(), r64["loss"], rtol=1e-5)
    for got, w64, w32, k in zip(_grads(m), r64["grads"], r32["grads"], PARAMS):
        F.bar(got, w64, w32, f"{over} gradient {k}")


@pytest.mark.parametrize("case", ["A", "B"])
def test_predict(g, ref32, case):
    """full_sort_predict with the recorded evaluation draws against the golden scores, and Trainer.evaluate's top-K,
    fused and unfused, which agree with each other (one set of Philox draws per evaluation pass)."""
    from gmr.dataloader import EvalDataLoader
    from gmr.dataset import RecDataset
    from gmr.trainer import Trainer
    m, cfg, ds, tl = build_lgmrec(g, case)
    m.eval()
    U, I = m.n_users, m.n_items
    scores = m.full_sort_predict([torch.arange(U, device=DEV)], g[case + "_g_eval"])
    F.bar(scores, g[case + "_scores"], ref32[case]["scores"], f"{case} scores")
    again = m.full_sort_predict([torch.arange(U, device=DEV)], noise=g[case + "_g_eval"])
    assert torch.equal(scores, again)                                  # injected noise: reproducible
    assert m.extra_state()["counters"]["eval_pass"] == 0
    rng = np.random.default_rng(4)
    ev = RecDataset.from_arrays(cfg, np.arange(U), rng.integers(0, I, U), np.zeros(U), U, I, g["v_feat"], g["t_feat"])
    vl = EvalDataLoader(cfg, ev, additional_dataset=ds, batch_size=16)
    tr = Trainer(cfg, m)
    tops = []
    for fused in (True, False):
        tr.fused_eval = fused
        m.load_extra_state({"counters": {"step": 0, "eval_pass": 5}})
        tops.append(tr.topk_all(vl, 10).cpu().numpy()[:U])
        assert m.extra_state()["counters"]["eval_pass"] == 6          # one draw per evaluation pass
    assert np.array_equal(tops[0], tops[1])
    res = tr.evaluate(vl)
    assert all(np.isfinite(v) and 0 <= v <= 1 for v in res.values())


def test_philox_evaluations(g):
    m, *_ = build_lgmrec(g, "B")
    m.eval()
    m.load_extra_state({"counters": {"step": 0, "eval_pass": 3}})
    u1, i1 = (t.clone() for t in m.forward_embeddings())
    S1 = m.S.clone()
    assert torch.equal(m.S, m.h)                                       # evaluation drops nothing
    m.load_extra_state({"counters": {"step": 0, "eval_pass": 3}})
    u2, i2 = m.forward_embeddings()
    assert torch.equal(u1, u2) and torch.equal(i1, i2)                 # the same counter: the same bits
    u3, _ = m.forward_embeddings()                                     # the next pass: other draws
    assert not torch.equal(u1, u3) and not torch.equal(S1, m.S)
    assert bool(torch.isfinite(u3).all())
    # a training step without injected draws drops about half of the entries, and the next step other ones
    m.train()
    users, pos, neg = _batch(g)
    m.rec_step(users, pos, neg)
    k0 = m.h != 0
    for v in m.grad_views():
        assert bool(torch.isfinite(v).all())
    m.rec_step(users, pos, neg)
    k1 = m.h != 0
    kept = (m.S != 0)
    n = int(kept.sum().item())
    share = (k1 & kept).float().sum().item() / n
    assert abs(share - 0.5) <= 5 * np.sqrt(0.25 / n) and not torch.equal(k0, k1)


def test_adam_trajectory(g):
    """Case B, three Adam steps with the reference's draws against the reference's own fp32 torch.optim.Adam run, on
    every parameter.  The tolerance is lattice_fixture.adam_reach's rule: twice the distance of the reference's fp32
    run from the same three steps of the fp64 restatement, three roundings of the parameter, and per element the reach
    of gradients within the gradient bar through Adam's division.  rtol 0."""
    from gmr.trainer import Trainer
    m, cfg, *_ = build_lgmrec(g, "B")
    opt = Trainer(cfg, m).optimizer
    users, pos, neg = _batch(g)
    args = _args(g, "B")[:10] + (g["B_g"], g["B_keep"])
    t64, g64 = F.trajectory(*args)
    _, g32 = F.trajectory(*args, dtype=torch.float32)
    # the stored distance of the reference's own fp32 gradients for the first step
    for k in PARAMS:
        g32[0][k] = g64[0][k] + float(g["B_own_" + k])
    reach = F.adam_reach(g64, g32, lr=F.LR)
    for j in range(F.ADAM_STEPS):
        gum, keep = _draws(g, "B", j)
        m.rec_step(users, pos, neg, g=gum, keep=keep)
        opt.step()
    j = F.ADAM_STEPS - 1
    for p, k in zip(m._params(), PARAMS):
        want = g[f"traj{j + 1}_{k}"]
        err32 = float(np.abs(want.astype(np.float64) - t64[j][k]).max())
        atol = 2 * err32 + F.ADAM_STEPS * np.spacing(np.float32(np.abs(want).max())) + reach[j][k]
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want)
        print(f"step {j + 1} {k}: max abs error {err.max():.3e} (fp32 torch {err32:.3e}, reach up to "
              f"{np.max(reach[j][k]):.3e}, median {np.median(reach[j][k]):.3e})")
        assert (err <= atol).all(), (k, float((err - atol).max()))


def _tiny_split(g, cfg):
    from gmr.dataset import RecDataset
    U, I = int(g["U"]), int(g["I"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(U), 6)
    cols = np.concatenate([rng.choice(I, 6, replace=False) for _ in range(U)])
    labels = np.zeros(rows.size)
    labels[4::6] = 1
    labels[5::6] = 2
    return RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"], g["t_feat"]).split()


def test_fit_and_resume(g, tmp_path):
    """Two epochs through the generic Trainer with dropout on: it trains, evaluates and writes a checkpoint; a fresh
    model and trainer resumed from the first epoch's checkpoint draw the second epoch's noise and masks and end with
    the same parameters, bit for bit."""
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.trainer import Trainer
    from gmr.utils import get_model

    def make(epochs, sub):
        cfg = F.lgmrec_config(**dict(CASES["B"], learning_rate=0.01, epochs=epochs,
                                     checkpoint_dir=str(tmp_path / sub), eval_step=1))
        tr_ds, va, te = _tiny_split(g, cfg)
        tl = TrainDataLoader(cfg, tr_ds, batch_size=16)
        torch.manual_seed(3)
        m = get_model("LGMRec")(cfg, tl)
        vl = EvalDataLoader(cfg, va, additional_dataset=tr_ds, batch_size=16)
        return m, Trainer(cfg, m), tl, vl

    m, trainer, tl, vl = make(2, "full")
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=True)
    l0, l1 = trainer.train_loss_dict[0], trainer.train_loss_dict[1]
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0, (l0, l1)
    assert "recall@10" in valid and 0.0 <= valid["recall@10"] <= 1.0
    assert m.extra_state()["counters"]["step"] == 2 * len(tl)
    ck = torch.load(str(tmp_path / "full" / "LGMRec-baby.pth"), map_location="cpu", weights_only=True)
    assert list(ck["state_dict"]) == F.STATE_KEYS
    m1, t1, tl1, vl1 = make(1, "part")
    t1.fit(tl1, valid_data=vl1, test_data=vl1, saved=False)
    t1._save_checkpoint(0)
    m2, t2, tl2, vl2 = make(2, "part")
    t2.resume_checkpoint(str(tmp_path / "part" / "LGMRec-baby.pth"), train_data=tl2)
    assert t2.start_epoch == 1 and m2.extra_state()["counters"]["step"] == len(tl)
    t2.fit(tl2, valid_data=vl2, test_data=vl2, saved=False)
    assert torch.equal(m2.slab.data, m.slab.data)
    # without the step counter the second epoch draws the first one's noise: other parameters
    m3, t3, tl3, vl3 = make(2, "part")
    t3.resume_checkpoint(str(tmp_path / "part" / "LGMRec-baby.pth"), train_data=tl3)
    m3.load_extra_state({"counters": {"step": 0, "eval_pass": 0}})
    t3.fit(tl3, valid_data=vl3, test_data=vl3, saved=False)
    assert not torch.equal(m3.slab.data, m.slab.data)


def test_quick_start(tmp_path, monkeypatch):
    """quick_start("LGMRec", "baby", ...) on the tiny synthetic shape with LGMRec.yaml's values."""
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False}
    results = quick_start("LGMRec", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("LGMRec", "baby", dict(cfg_dict))
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and want <= set(best_test)
    assert all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "LGMRec-baby.pth"), map_location="cpu", weights_only=True)
    assert list(ck["state_dict"]) == F.STATE_KEYS


def test_unsupported_settings_raise(g):
    with pytest.raises(NotImplementedError, match="hyper_num"):
        build_lgmrec(g, "A", hyper_num=65)
    with pytest.raises(NotImplementedError, match="text features"):
        build_lgmrec(g, "A", t_feat=None)
    with pytest.raises(NotImplementedError, match="image features"):
        build_lgmrec(g, "A", v_feat=None)
    with pytest.raises(NotImplementedError, match="embedding_size"):
        build_lgmrec(g, "A", embedding_size=32)
    # the entry points themselves report H out of range through the error string
    from gmr import _lib
    from gmr.kernels import ptr, stream
    x = torch.zeros(8, 256, device=DEV)
    with pytest.raises(RuntimeError, match="hyper_num: 1..64"):
        _lib.call("gmr_lgm_apply", 8, ptr(x), 256, 65, ptr(x), ptr(x), 256, 0, 0, stream())
    with pytest.raises(RuntimeError, match="hyper_num: 1..64"):
        _lib.call("gmr_lgm_lat", 8, ptr(x), 256, 0, ptr(x), ptr(x), 256, ptr(x), x.numel(), 0, ptr(x), stream())


def test_injected_draws_are_validated(g):
    """Injected draws reach the row kernel as packed float32 / uint8 (2, N, H) tensors or not at all: a bool mask and a
    non-contiguous one give the step of the packed bytes, another dtype or shape raises."""
    m, *_ = build_lgmrec(g, "B")
    users, pos, neg = _batch(g)
    gum, keep = _draws(g, "B")
    base = m.rec_step(users, pos, neg, g=gum, keep=keep).item()
    first = _grads(m)
    wide = torch.zeros((2, m.N, 2 * m.hyper_num), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = keep
    for kp, gg in ((keep.bool(), gum), (wide[:, :, ::2], gum), (keep.cpu().numpy(), gum.cpu().numpy())):
        assert m.rec_step(users, pos, neg, g=gg, keep=kp).item() == base
        for a, b, k in zip(_grads(m), first, PARAMS):
            assert np.array_equal(a, b), k
    with pytest.raises(TypeError, match="keep"):
        m.rec_step(users, pos, neg, g=gum, keep=keep.long())
    with pytest.raises(TypeError, match="g must be"):
        m.rec_step(users, pos, neg, g=gum.double(), keep=keep)
    with pytest.raises(ValueError, match="keep"):
        m.rec_step(users, pos, neg, g=gum, keep=keep[:, :-1])
    with pytest.raises(ValueError, match="noise"):
        m.forward_embeddings(noise=gum[:, :, :-1])
