"""MGCN on the HIP path vs golden vectors from the reference (models/mgcn.py; tiny shape,
tests/golden/make_golden_mgcn.py).  Case A: the init as drawn, one item-graph layer, cl_loss 0.001; case B: scaled
parameters, two layers, cl_loss 0.1 (every gradient large enough to test).  The mid shape goes against the fp64
restatement of tests/mgcn_fixture.py, which tests/test_mgcn_restatement_cpu.py pins to the same golden values."""
import numpy as np
import pytest
import torch

import mgcn_fixture as F
from mgcn_fixture import CASES, DEV, PARAMS, build_mgcn, build_mgcn_mid, check_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("mgcn_tiny")


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


def test_init_parity(g):
    m, *_ = build_mgcn(g, "A")
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == PARAMS
    assert list(m.state_dict()) == F.STATE_KEYS
    for p, k in zip(m._params(), PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), g["init_" + k]), k
    assert [tuple(v.shape) for v in m.grad_views()] == [g["init_" + k].shape for k in PARAMS]


def test_graphs(g):
    m, *_ = build_mgcn(g, "A")
    U, I = m.n_users, m.n_items
    for csr, k, shape in ((m.norm_adj, "adj", (U + I, U + I)), (m.R, "R", (U, I)), (m.mm_adj["image"], "image_adj", (I, I)),
                          (m.mm_adj["text"], "text_adj", (I, I))):
        got, want = _dense(csr), F.dense_of(g[k + "_idx"], g[k + "_val"], shape)
        assert np.array_equal(got != 0, want != 0), k
        assert np.isfinite(got).all(), k
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0, err_msg=k)
    assert np.array_equal(_dense(m.R_t), _dense(m.R).T)
    assert np.array_equal(_dense(m.mm_adj_t["text"]), _dense(m.mm_adj["text"]).T)
    empty = np.flatnonzero(np.diff(m.norm_adj.rowptr.cpu().numpy()) == 0)
    assert empty.size == int(g["n_isolated"]) and empty.min() >= U   # the isolated items: empty rows, no inf


@pytest.mark.parametrize("case", ["A", "B"])
def test_forward_tables(g, case):
    m, *_ = build_mgcn(g, case)
    ua, ia = m.forward()
    tag, U = case + "_", m.n_users
    got = {"a": m.ab[:, :64], "b": m.ab[:, 64:], "c": m.c, "side": m.side}
    for k, v in got.items():
        np.testing.assert_allclose(v.cpu().numpy(), g[tag + k], rtol=1e-5, atol=2e-6, err_msg=k)
    al = g[tag + "c"] + g[tag + "side"]
    np.testing.assert_allclose(ua.cpu().numpy(), al[:U], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(ia.cpu().numpy(), al[U:], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("case", ["A", "B"])
def test_step_parity(g, case):
    tag = case + "_"
    m, *_ = build_mgcn(g, case)
    users, pos, neg = _batch(g)
    loss = m.rec_step(users, pos, neg)
    print(f"{case}: loss {loss.item():.7f} (reference {g[tag + 'loss']:.7f})")
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    print(f"{case}: terms {terms[1:]} (reference {g[tag + 'loss_terms']})")
    np.testing.assert_allclose(terms[0], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1:], g[tag + "loss_terms"], rtol=1e-5)
    want = [g[tag + "g_" + k] for k in PARAMS]
    first = _grads(m)
    check_grads(first, want, show=case)
    # every work buffer filled with NaN: nothing of a step reads what an earlier step left
    bufs = [m.vt, m.pur, m.gates_i, m.ab, m.c, m.side, m.all, m.saved, m.wab, m.dall, m.gtab, m.dab, m.dc, m.zf, m.r,
            m.dpur, m.zp, m.dvt, m._loss, *m._h, *m._layers, *m._t,
            *[v for v in m._w.values() if torch.is_tensor(v) and v.is_floating_point()]]
    for t in bufs:
        t.fill_(float("nan"))
    m.slab.grad.fill_(float("nan"))
    again = m.rec_step(users, pos, neg)
    assert again.item() == loss.item()
    for a, b, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b), k


def test_loader_plans_give_the_same_step(g):
    """The plans of the loader's epoch draw and the model's own plans scatter the same sums."""
    m, cfg, ds, tl = build_mgcn(g, "B")
    d = tl.epoch()
    b, sizes, u, p, ng, pb, pc = next(iter(tl.batches(d)))
    with_plans = m.rec_step(u, p, ng, pb, pc).item()
    first = _grads(m)
    assert m.rec_step(u, p, ng).item() == with_plans
    for a, b_, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b_), k


def test_fused_infonce_route_agrees(g, monkeypatch):
    """GMR_MGCN_NCE_FUSED=1 (gmr_contrast_fused_f32, no B x B block) against the default GEMM route: the loss at the
    parity tests' 1e-5, the gradients at 1e-5 of their largest entry (its split-bf16 passes measured 2.9e-6)."""
    import gmr.mgcn as M
    m, *_ = build_mgcn(g, "B")
    users, pos, neg = _batch(g)
    base = m.rec_step(users, pos, neg).item()
    want, terms = _grads(m), m.loss_terms().cpu().numpy().copy()
    monkeypatch.setattr(M, "NCE_FUSED", True)
    fused = m.rec_step(users, pos, neg).item()
    np.testing.assert_allclose(fused, base, rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy(), terms, rtol=1e-5)
    for a, b, k in zip(_grads(m), want, PARAMS):
        print(f"fused route {k}: {np.abs(a - b).max() / np.abs(b).max():.2e} of the largest entry")
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5 * np.abs(b).max(), err_msg=k)


def test_calculate_loss_scales_by_upstream(g):
    m, *_ = build_mgcn(g, "B")
    users, pos, neg = _batch(g)
    base = m.rec_step(users, pos, neg).item()
    want = _grads(m)
    inter = torch.stack([torch.as_tensor(g[k]) for k in ("users", "pos", "neg")]).to(DEV)
    out = m.calculate_loss(inter)
    assert out.item() == base
    (3.0 * out).backward()
    for p, w, k in zip(m._params(), want, PARAMS):
        np.testing.assert_allclose(p.grad.cpu().numpy(), 3.0 * w, rtol=1e-6, atol=0, err_msg=k)


@pytest.mark.parametrize("case", ["A", "B"])
def test_predict(g, case):
    """full_sort_predict against the golden scores, and Trainer.evaluate's top-K (the fused score -> mask -> top-K)
    against the top-K of the golden scores outside near-ties: the golden scores of the picked items equal the k
    largest golden scores within the scores' own tolerance."""
    from gmr.dataloader import EvalDataLoader
    from gmr.dataset import RecDataset
    from gmr.trainer import Trainer
    m, cfg, ds, tl = build_mgcn(g, case)
    U, I = m.n_users, m.n_items
    users = torch.arange(U, device=DEV)
    scores = m.full_sort_predict([users])
    want = g[case + "_scores"]
    np.testing.assert_allclose(scores.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    rng = np.random.default_rng(4)
    ev = RecDataset.from_arrays(cfg, np.arange(U), rng.integers(0, I, U), np.zeros(U), U, I, g["v_feat"], g["t_feat"])
    vl = EvalDataLoader(cfg, ev, additional_dataset=ds, batch_size=16)
    tr = Trainer(cfg, m)
    k = 10
    top = tr.topk_all(vl, k).cpu().numpy()[:U]
    res = tr.evaluate(vl)
    assert all(np.isfinite(v) and 0 <= v <= 1 for v in res.values())
    ref = want.astype(np.float64).copy()
    ref[g["train_rows"], g["train_cols"]] = -1e10
    eu = vl.eval_u_np
    got_val = np.take_along_axis(ref[eu], top.astype(np.int64), axis=1)
    want_val = -np.sort(-ref[eu], axis=1)[:, :k]
    np.testing.assert_allclose(got_val, want_val, rtol=1e-5, atol=1e-5)


def test_mid_shape_step():
    """700 rows over 300 users and 1100 items: several tiles and blocks, repeated users and items, isolated items,
    feature widths that are no multiple of 4, two item-graph layers."""
    m, d = build_mgcn_mid("B")
    assert np.setdiff1d(np.arange(d["I"]), d["cols"]).size > 0
    users, pos, neg = (torch.as_tensor(d[k]).to(DEV) for k in ("users", "pos", "neg"))
    P = {k: v.detach().cpu().numpy() for k, v in zip(PARAMS, m._params())}
    loss = m.rec_step(users, pos, neg)
    c = CASES["B"]
    r = F.mgcn_step_ref(P, d["U"], d["I"], d["rows"], d["cols"], d["users"], d["pos"], d["neg"], c["n_layers"],
                        c["cl_loss"], feats=(d["v_feat"], d["t_feat"]), knn_k=10)
    print(f"mid: loss {loss.item():.7f} (fp64 {r['loss']:.7f}), terms {m.loss_terms().cpu().numpy()[1:]} / {r['terms']}")
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy()[1:], r["terms"], rtol=1e-5)
    np.testing.assert_allclose(m.all.cpu().numpy(), r["all"], rtol=1e-5, atol=2e-6)
    check_grads(_grads(m), r["grads"], show="mid")


def test_short_batch_keeps_the_configured_divisor(g):
    """A last batch shorter than train_batch_size: means over its rows, the L2 term over the configured size."""
    m, *_ = build_mgcn(g, "B")
    users, pos, neg = (t[:11].contiguous() for t in _batch(g))
    loss = m.rec_step(users, pos, neg)
    r = F.mgcn_step_ref(F.case_params(g, "B"), m.n_users, m.n_items, g["train_rows"], g["train_cols"], g["users"][:11],
                        g["pos"][:11], g["neg"][:11], 2, 0.1, feats=(g["v_feat"], g["t_feat"]), batch_size=16)
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy()[1:], r["terms"], rtol=1e-5)
    check_grads(_grads(m), r["grads"], show="short")


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


def test_checkpoint_reproduces_the_next_step(g, tmp_path):
    """A checkpoint written after one optimiser step, loaded into a fresh model and trainer: the next step's loss,
    gradients and updated parameters equal the uninterrupted run's bit for bit."""
    from gmr.trainer import Trainer
    users, pos, neg = _batch(g)

    def make():
        m, cfg, _, _ = build_mgcn(g, "B")
        cfg["checkpoint_dir"] = str(tmp_path)
        return m, Trainer(cfg, m)

    m, tr = make()
    m.rec_step(users, pos, neg)
    tr.optimizer.step()
    tr._save_checkpoint(0)
    nxt = m.rec_step(users, pos, neg).item()
    grads = m.slab.grad.clone()
    tr.optimizer.step()
    m2, tr2 = make()
    tr2.resume_checkpoint(str(tmp_path / "MGCN-baby.pth"))
    assert m2.rec_step(users, pos, neg).item() == nxt
    assert torch.equal(m2.slab.grad, grads)
    tr2.optimizer.step()
    assert torch.equal(m2.slab.data, m.slab.data)


def test_fit(g):
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.mgcn import MGCN
    from gmr.trainer import Trainer
    cfg = F.mgcn_config(**CASES["B"], learning_rate=0.01)
    tr, va, te = _tiny_split(g, cfg)
    tl = TrainDataLoader(cfg, tr, batch_size=16)
    m = MGCN(cfg, tl)
    cfg["epochs"] = 3
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=16)
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    l0, l2 = trainer.train_loss_dict[0], trainer.train_loss_dict[2]
    assert np.isfinite(l0) and np.isfinite(l2) and l2 < l0, (l0, l2)
    assert "recall@10" in valid and 0.0 <= valid["recall@10"] <= 1.0


def test_quick_start(tmp_path, monkeypatch):
    """quick_start("MGCN", "baby", ...) on the tiny synthetic shape with MGCN.yaml's values: the metric keys of
    Trainer.fit and the reference's checkpoint and state_dict keys."""
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False}
    results = quick_start("MGCN", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("MGCN", "baby", dict(cfg_dict))
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and want <= set(best_test)
    assert all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "MGCN-baby.pth"), map_location="cpu", weights_only=True)
    assert {"config", "epoch", "state_dict", "optimizer", "best_valid_score"} <= set(ck)
    assert list(ck["state_dict"]) == F.STATE_KEYS


def test_world_size_two_raises(g, monkeypatch):
    from gmr import dist
    from gmr.mgcn import check_config
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        check_config(F.mgcn_config(), n_items=41)
    with pytest.raises(NotImplementedError, match="world size"):
        build_mgcn(g, "A")
