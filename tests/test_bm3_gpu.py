"""BM3 on the HIP path vs golden vectors from the reference (models/bm3.py; tiny shape,
tests/golden/make_golden_bm3.py) with the reference's dropout masks injected.  Case A: one layer, dropout 0.3;
case B: two layers, dropout 0.5.  One-modality models and the mid shape go against the fp64 restatement of
tests/bm3_fixture.py, which tests/test_bm3_restatement_cpu.py pins to the same golden values."""
import numpy as np
import pytest
import torch

from bm3_fixture import (CASES, DEV, PARAMS, batch_keep, bm3_step_ref, build_bm3, build_bm3_mid, check_grads,
                         golden_keep, params_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("bm3_tiny")


def _batch(g):
    return [torch.as_tensor(g[k].astype(np.int32)).to(DEV) for k in ("users", "items")]


def _keep(g, case, mods=("image", "text")):
    ks = batch_keep(golden_keep(g, case), g["users"], g["items"], mods)
    return [None if k is None else torch.as_tensor(k).to(DEV) for k in ks]


def _grads(m):
    return [v.cpu().numpy().copy() for v in m.grad_views()]


def test_init_parity(g):
    m, *_ = build_bm3(g, "A")
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == PARAMS
    for p, k in zip(m._params(), PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), g["p_" + k]), k
    assert [tuple(v.shape) for v in m.grad_views()] == [g["p_" + k].shape for k in PARAMS]


@pytest.mark.parametrize("case", ["A", "B"])
def test_encoder(g, case):
    m, *_ = build_bm3(g, case)
    ua, ib = m.forward()
    np.testing.assert_allclose(ua.cpu().numpy(), g[case + "_ua"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ib.cpu().numpy(), g[case + "_ib"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", ["A", "B"])
def test_step_parity(g, case):
    tag = case + "_"
    m, *_ = build_bm3(g, case)
    users, items = _batch(g)
    keep = _keep(g, case)
    loss = m.rec_step(users, items, None, keep=keep)
    print(f"{case}: loss {loss.item():.7f} (reference {g[tag + 'loss']:.7f})")
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1:7], g[tag + "loss_terms"], rtol=1e-5)
    np.testing.assert_allclose(terms[7], g[tag + "reg"], rtol=1e-5)
    want = [g[tag + "g_" + k] for k in PARAMS]
    first = _grads(m)
    check_grads(first, want, show=case)
    assert m.extra_state() == {"counters": {"step": 1}}
    # every work buffer filled with NaN: nothing of a step reads what an earlier step left
    for t in [m.g, m.tv, m.gtab, m._eval, m._pred, m._sq, m._loss, *m._layers, *m._t,
              *[v for v in m._w.values() if torch.is_tensor(v) and v.is_floating_point()]]:
        t.fill_(float("nan"))
    m.slab.grad.fill_(float("nan"))
    again = m.rec_step(users, items, None, keep=keep)
    assert again.item() == loss.item()
    for a, b, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b), k


def test_calculate_loss_scales_by_upstream(g):
    m, *_ = build_bm3(g, "A")
    users, items = _batch(g)
    m.load_extra_state({"counters": {"step": 7}})
    base = m.rec_step(users, items, None).item()
    want = _grads(m)
    m.load_extra_state({"counters": {"step": 7}})  # the same drawn masks
    inter = torch.stack([torch.as_tensor(g[k]) for k in ("users", "items")]).to(DEV)
    out = m.calculate_loss(inter)
    assert out.item() == base
    (3.0 * out).backward()
    for p, w, k in zip(m._params(), want, PARAMS):
        np.testing.assert_allclose(p.grad.cpu().numpy(), 3.0 * w, rtol=1e-6, atol=0, err_msg=k)


@pytest.mark.parametrize("case", ["A", "B"])
def test_predict(g, case):
    m, *_ = build_bm3(g, case)
    U = m.n_users
    users = torch.arange(U, device=DEV)
    scores = m.full_sort_predict([users])
    np.testing.assert_allclose(scores.cpu().numpy(), g[case + "_scores"], rtol=1e-5, atol=1e-5)
    usr, itm = m.forward_embeddings()
    k = 10
    out = torch.zeros((U, k), dtype=torch.int32, device=DEV)
    buf = torch.empty((U, (m.n_items + 3) // 4 * 4), device=DEV)
    rows = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    cols = torch.tensor([3, 7], dtype=torch.int32, device=DEV)
    m.topk_from_embeddings(usr, itm, users.to(torch.int32), rows, cols, k, out, buf)
    ref = scores.clone()
    ref[rows.long(), cols.long()] = -1e10
    want_val = torch.topk(ref, k, dim=-1)[0]
    got_val = torch.gather(ref, 1, out.long())
    np.testing.assert_allclose(got_val.cpu().numpy(), want_val.cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mod", ["text", "image"])
def test_one_modality(g, mod):
    m, *_ = build_bm3(g, "A", mods=(mod,))
    names = params_of((mod,))
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == names
    P = {k: p.detach().cpu().numpy() for k, p in zip(names, m._params())}
    users, items = _batch(g)
    loss = m.rec_step(users, items, None, keep=_keep(g, "A", (mod,)))
    c = CASES["A"]
    r = bm3_step_ref(P, int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["items"],
                     golden_keep(g, "A"), c["n_layers"], c["dropout"], mods=(mod,))
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[1:7], r["terms"], rtol=1e-5)
    gone = (3, 5) if mod == "text" else (2, 4)   # v, vt / t, tv of [ui, iu, t, v, tv, vt]
    assert all(r["terms"][i] == 0 and terms[1 + i] == 0 for i in gone)
    check_grads(_grads(m), r["grads"], names=names, show=mod)


def test_mid_shape_step():
    """700 rows over 300 users and 1100 items: 44 tiles, repeated users and items, a short last tile."""
    m, d = build_bm3_mid("B")
    rng = np.random.default_rng(6)
    p = CASES["B"]["dropout"]
    tk = {k: (rng.random((n, 64)) >= p).astype(np.uint8) for k, n in (("u", d["U"]), ("i", d["I"]), ("t", d["I"]),
                                                                       ("v", d["I"]))}
    users, items = (torch.as_tensor(d[k]).to(DEV) for k in ("users", "items"))
    keep = [torch.as_tensor(k).to(DEV) for k in batch_keep(tk, d["users"], d["items"])]
    P = {k: v.detach().cpu().numpy() for k, v in zip(PARAMS, m._params())}
    loss = m.rec_step(users, items, None, keep=keep)
    r = bm3_step_ref(P, d["U"], d["I"], d["rows"], d["cols"], d["users"], d["items"], tk, CASES["B"]["n_layers"], p)
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.loss_terms().cpu().numpy()[1:7], r["terms"], rtol=1e-5)
    check_grads(_grads(m), r["grads"], show="mid")


def test_resume_reproduces_the_next_step(g):
    """extra_state carries the Philox step counter: a model resumed mid-run draws the masks of the next step."""
    from gmr.slab import FlatAdam
    users, items = _batch(g)
    m, *_ = build_bm3(g, "A")
    opt = FlatAdam(m.optim_slabs(), lr=1e-2)
    losses = []
    for _ in range(2):
        losses.append(m.rec_step(users, items, None).item())
        opt.step()
    assert losses[0] != losses[1]
    st, data = m.extra_state(), m.slab.data.clone()
    nxt = m.rec_step(users, items, None).item()
    m2, *_ = build_bm3(g, "A")
    m2.slab.data.copy_(data)
    fresh = m2.rec_step(users, items, None).item()   # step counter 0: other masks
    m2.load_extra_state(st)
    assert m2.rec_step(users, items, None).item() == nxt and fresh != nxt


def test_fit(g):
    from bm3_fixture import bm3_config
    from gmr.bm3 import BM3
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.trainer import Trainer
    U, I = int(g["U"]), int(g["I"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(U), 6)
    cols = np.concatenate([rng.choice(I, 6, replace=False) for _ in range(U)])
    labels = np.zeros(rows.size)
    labels[4::6] = 1
    labels[5::6] = 2
    cfg = bm3_config(**CASES["A"])
    ds = RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"], g["t_feat"])
    tr, va, te = ds.split()
    tl = TrainDataLoader(cfg, tr, batch_size=16)
    m = BM3(cfg, tl)
    cfg["epochs"] = 2
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=16)
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    l0, l1 = trainer.train_loss_dict[0], trainer.train_loss_dict[1]
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0, (l0, l1)
    assert "recall@10" in valid and 0.0 <= valid["recall@10"] <= 1.0
    assert m.extra_state()["counters"]["step"] == 2 * len(tl)


def test_quick_start(tmp_path, monkeypatch):
    """quick_start("BM3", "baby", ...) on the tiny synthetic shape with BM3.yaml's values: the metric keys of
    Trainer.fit, the reference's checkpoint keys and the step counter in the checkpoint."""
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False}
    results = quick_start("BM3", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("BM3", "baby", dict(cfg_dict))
    assert (cfg["n_layers"], cfg["dropout"], cfg["reg_weight"], cfg["cl_weight"]) == (1, 0.3, 0.1, 2.0)
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and want <= set(best_test)
    assert all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "BM3-baby.pth"), map_location="cpu", weights_only=True)
    assert {"config", "epoch", "state_dict", "optimizer", "best_valid_score"} <= set(ck)
    assert set(ck["state_dict"]) == {n.replace("_weight", ".weight").replace("_bias", ".bias") for n in PARAMS}
    assert ck["generated_graphs"]["counters"]["step"] > 0
