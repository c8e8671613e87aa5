"""FREEDOM on the HIP path vs golden vectors from the reference (models/freedom.py; tiny shape,
tests/golden/make_golden_freedom.py).  Case A: one mm layer, two UI layers, the reference's own pruned
graph installed; case B: two mm layers, three UI layers, no pruning."""
import numpy as np
import pytest
import torch

from freedom_fixture import DEV, PARAMS, build_freedom, coo_keys, csr_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("freedom_tiny")


@pytest.fixture(scope="module")
def model_a(g):
    """Case A with the reference's draw installed as the pruned graph."""
    m, *_ = build_freedom(g, "A")
    m.prune_edges(keep_idx=torch.as_tensor(g["degree_idx"]))
    return m


def _params(m):
    return [p.detach().cpu().numpy() for p in m._params()]


def _batch(g):
    return [torch.as_tensor(g[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _check_grads(got, g, tag):
    for v, k in zip(got, PARAMS):
        want = g[tag + "g_" + k]
        if k.endswith("_bias"):
            # analytically zero (the pos and neg terms cancel); bounded against the layer's weight gradient
            gw = g[tag + "g_" + k.replace("_bias", "_weight")]
            np.testing.assert_allclose(v, want, rtol=0, atol=1e-4 * np.abs(gw).max(), err_msg=k)
        else:
            np.testing.assert_allclose(v, want, rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=k)


def test_registry():
    from gmr.freedom import FREEDOM
    from gmr.utils import get_model
    assert get_model("FREEDOM") is FREEDOM


def test_init_parity(g):
    m, *_ = build_freedom(g, "A")
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == PARAMS
    for v, k in zip(_params(m), PARAMS):
        assert np.array_equal(v, g["p_" + k]), k


def test_graphs(g):
    import scipy.sparse as sp
    m, *_ = build_freedom(g, "A")
    N, I = m.N, m.n_items
    key, val = csr_keys(m.norm_adj)
    wkey, wval = coo_keys(g["norm_adj_idx"], g["norm_adj_val"], N)
    assert np.array_equal(key, wkey)
    np.testing.assert_allclose(val, wval, rtol=1e-6)
    np.testing.assert_allclose(m.edge_values.cpu().numpy(), g["edge_values"], rtol=1e-6)
    for name, want in (("image", g["knn_ind_image"]), ("text", g["knn_ind_text"])):
        got = m.knn_ind[name].cpu().numpy()
        assert np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1)), name
    key, val = csr_keys(m.mm_adj)
    wkey, wval = coo_keys(g["mm_adj_idx"], g["mm_adj_val"], I)
    assert np.array_equal(key, wkey)
    np.testing.assert_allclose(val, wval, rtol=1e-6)
    a = m.mm_adj
    t = sp.csr_matrix((a.val.cpu().numpy(), a.col.cpu().numpy(), a.rowptr.cpu().numpy()), shape=(I, I)).T.tocsr()
    t.sort_indices()
    at = m.mm_adj_t
    assert np.array_equal(at.rowptr.cpu().numpy(), t.indptr) and np.array_equal(at.col.cpu().numpy(), t.indices)
    assert np.array_equal(at.val.cpu().numpy(), t.data)


def test_pruning_with_reference_draw(g, model_a):
    m = model_a
    key, val = csr_keys(m.masked_adj)
    wkey, wval = coo_keys(g["masked_adj_idx"], g["masked_adj_val"], m.N)
    assert np.array_equal(key, wkey)
    np.testing.assert_allclose(val, wval, rtol=1e-6)
    ua, ia = m.forward(m.masked_adj)
    np.testing.assert_allclose(ua.cpu().numpy(), g["A_ua"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ia.cpu().numpy(), g["A_ia"], rtol=1e-5, atol=1e-6)


def test_pruning_draw_keeps_m_edges(g):
    m, *_ = build_freedom(g, "A")
    E = len(g["train_rows"])
    keep = m.prune_edges()
    assert int(keep.sum()) == int(E * (1. - 0.8)) and m.masked_adj.nnz == 2 * int(E * (1. - 0.8))
    u = torch.full((E,), 0.5, device=DEV)
    u[:3] = 0.999999  # near-certain picks: -log u ~ 1e-6
    keep = m.prune_edges(u=u).cpu().numpy()
    assert keep[:3].all()


@pytest.mark.parametrize("case", ["A", "B"])
def test_step_parity(g, case, model_a):
    tag = case + "_"
    if case == "A":
        m = model_a
    else:
        m, *_ = build_freedom(g, "B")
        m.pre_epoch_processing()
        assert m.masked_adj is m.norm_adj
    loss = m.rec_step(*_batch(g))
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[0], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1:], g[tag + "loss_terms"], rtol=1e-5)
    _check_grads([v.cpu().numpy() for v in m.grad_views()], g, tag)
    # the autograd wrapper fills the same .grads
    inter = torch.stack([torch.as_tensor(g[k]) for k in ("users", "pos", "neg")]).to(DEV)
    out = m.calculate_loss(inter)
    out.backward()
    np.testing.assert_allclose(out.item(), g[tag + "loss"], rtol=1e-5)
    _check_grads([p.grad.cpu().numpy() for p in m._params()], g, tag)


@pytest.mark.parametrize("case", ["A", "B"])
def test_predict(g, case, model_a):
    m = model_a if case == "A" else build_freedom(g, "B")[0]
    if case == "A":
        assert m.masked_adj is not m.norm_adj  # the pruned graph is installed; predict must not use it
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


def test_fit(g):
    from freedom_fixture import CASES, freedom_config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.freedom import FREEDOM
    from gmr.trainer import Trainer
    U, I = int(g["U"]), int(g["I"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(U), 6)
    cols = np.concatenate([rng.choice(I, 6, replace=False) for _ in range(U)])
    labels = np.zeros(rows.size)
    labels[4::6] = 1
    labels[5::6] = 2
    cfg = freedom_config(**CASES["A"])
    ds = RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"], g["t_feat"])
    tr, va, te = ds.split()
    tl = TrainDataLoader(cfg, tr, batch_size=16)
    m = FREEDOM(cfg, tl)
    cfg["epochs"] = 2
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=16)
    graphs, states = [], []
    pre = m.pre_epoch_processing

    def recording_pre():
        states.append(m.extra_state())
        pre()
        graphs.append(csr_keys(m.masked_adj)[0])

    m.pre_epoch_processing = recording_pre
    trainer = Trainer(cfg, m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
    assert np.isfinite(trainer.train_loss_dict[0]) and np.isfinite(trainer.train_loss_dict[1])
    assert "recall@10" in valid
    assert len(graphs) == 2 and graphs[0].size == graphs[1].size and not np.array_equal(graphs[0], graphs[1])
    assert states[0] != states[1]
    m.load_extra_state(states[0])
    pre()
    assert np.array_equal(csr_keys(m.masked_adj)[0], graphs[0])


def test_quick_start(tmp_path, monkeypatch):
    """quick_start("FREEDOM", "baby", ...) on the tiny synthetic shape, as tests/test_quick_start_gpu.py drives the
    other models: two epochs (two prunings), the metric keys of Trainer.fit, the reference's checkpoint keys and
    the pruning counter in the checkpoint."""
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False}
    results = quick_start("FREEDOM", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("FREEDOM", "baby", dict(cfg_dict))
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and want <= set(best_test)
    assert all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "FREEDOM-baby.pth"), map_location="cpu", weights_only=True)
    assert {"config", "epoch", "state_dict", "optimizer", "best_valid_score"} <= set(ck)
    assert set(ck["state_dict"]) == {n.replace("_weight", ".weight").replace("_bias", ".bias") for n in PARAMS}
    assert ck["generated_graphs"] == {"epoch_ctr": ck["epoch"] + 1}
