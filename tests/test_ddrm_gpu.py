"""DDRM on the GPU: construction, one training step and the prediction against the values the reference recorded
(tests/golden/ddrm_tiny.npz), a mid shape against the fp64 restatement of tests/ddrm_fixture.py, the unsupported
settings, and an end-to-end run with checkpoint / resume on synthetic data."""
import numpy as np
import pytest
import torch

import ddrm_fixture as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def i32(a):
    return dev(np.asarray(a).astype(np.int32))


@pytest.fixture(scope="module")
def g():
    from gmr.utils import get_model
    assert get_model("DDRM").__name__ == "DDRM"
    return F.load_golden()


def _sched(g):
    return {k: g["sch_" + k] for k in F.TABLES}


# ----------------------------------------------------------------------------- construction
def test_construction(g):
    m = F.build_ddrm(g)
    names = F.param_names()
    assert [n for n, _ in m.named_parameters()] == names == list(g["param_names"])
    sd = m.state_dict()
    assert list(sd) == names
    for n in names:
        assert tuple(sd[n].shape) == g["p_" + F.key(n)].shape, n
        np.testing.assert_array_equal(sd[n].cpu().numpy(), g["p_" + F.key(n)], err_msg=n)   # bit for bit
    for k in F.TABLES:
        np.testing.assert_allclose(m.schedule[k], g["sch_" + k], rtol=1e-12, atol=0, err_msg=k)
    assert m.optim_slabs() == [m.slab] and len(m.grad_views()) == len(names)
    for gv, n in zip(m.grad_views(), names):
        assert tuple(gv.shape) == tuple(sd[n].shape), n


@pytest.mark.parametrize("over,word", [
    ({"dropout": True}, "dropout"), ({"A_split": True}, "A_split"), ({"act": "relu"}, "act"), ({"norm": True}, "norm"),
    ({"dims": [300, 100]}, "dims"), ({"dims": [302]}, "dims"), ({"dims": [1028]}, "dims"),
    ({"embedding_size": 32}, "embedding_size"), ({"noise_scale": 0}, "noise_scale"),
    ({"lightGCN_n_layers": 8}, "lightGCN_n_layers")])
def test_unsupported(g, over, word):
    with pytest.raises(NotImplementedError, match=word):
        F.build_ddrm(g, **over)


def test_unsupported_world_size(g, monkeypatch):
    from gmr import dist
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        F.build_ddrm(g)


# ----------------------------------------------------------------------------- the recorded step
def _recorded_step(m, g):
    return m.rec_step(i32(g["users"]), i32(g["pos"]), i32(g["neg"]), t=i32(g["t"]), noise_u=dev(g["noise_u"]),
                      noise_i=dev(g["noise_i"]), keep_u=dev(g["keep_u"]), keep_i=dev(g["keep_i"]))


def test_step_matches_reference(g):
    m = F.build_ddrm(g)
    loss = _recorded_step(m, g)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    for i, k in enumerate(("row_w", "row_sp", "row_rec")):
        np.testing.assert_allclose(terms[i], g[k], rtol=1e-5, err_msg=k)
    names = F.param_names()
    F.check_grads(F.model_grads(m), [g["g_" + F.key(n)] for n in names], names, show="tiny")
    assert m.extra_state()["counters"] == {"step": 1, "eval_pass": 0}
    # the same step again: the same bits (no atomics, fixed-order sums)
    g1 = m.slab.grad.clone()
    loss2 = _recorded_step(m, g)
    assert loss2.item() == loss.item() and torch.equal(m.slab.grad, g1)


def test_calculate_loss_autograd(g):
    m = F.build_ddrm(g)
    loss = m.calculate_loss([dev(g["users"]), dev(g["pos"]), dev(g["neg"])])
    (3.0 * loss).backward()
    sd = dict(m.named_parameters())
    w = sd["item_reverse_model.out_layers.0.weight"]
    assert torch.isfinite(loss) and w.grad is not None
    np.testing.assert_allclose(w.grad.cpu().numpy(), 3.0 * m.slab.gview("iW2").cpu().numpy(), rtol=1e-6)


# ----------------------------------------------------------------------------- mid shape, fp64 restatement
def test_mid_shape_against_fp64():
    U, I, B = 301, 203, 257
    rows, cols = F.mid_data(U, I)
    m = F.build_model(rows, cols, U, I, batch=B)
    rng = np.random.default_rng(6)
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    users[5] = users[6] = users[4] = U - 1          # the user with no train edge, three times
    pos[9] = pos[8]
    neg[11] = neg[10] = pos[8]
    nu, ni = (rng.standard_normal((B, 64)).astype(np.float32) for _ in range(2))
    loss = m.rec_step(i32(users), i32(pos), i32(neg), noise_u=dev(nu), noise_i=dev(ni)).item()  # t, masks drawn
    t = m._w["t"][:B].cpu().numpy()
    ku, ki = m._w["ukeep"][:B].cpu().numpy(), m._w["ikeep"][:B].cpu().numpy()
    assert t.min() >= 0 and t.max() < 100 and len(np.unique(t)) > 50
    assert 0.45 < ku.mean() < 0.55 and 0.45 < ki.mean() < 0.55 and not np.array_equal(ku, ki)
    r = F.step_ref(F.model_params(m), U, I, rows, cols, users, pos, neg, t, nu, ni, ku, ki, m.schedule,
                   dtype=torch.float64)
    print(f"mid: loss {loss:.8f} ref {r['loss']:.8f}")
    np.testing.assert_allclose(loss, r["loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    for i, k in enumerate(("w", "sp", "rec")):
        np.testing.assert_allclose(terms[i], r[k], rtol=1e-5, err_msg=k)
    F.check_grads(F.model_grads(m), r["grads"], F.param_names(), show="mid")
    # prediction at the same shape: the history-mean SpMM (one user without history), 3 chain steps, Philox noise off
    m.sampling_steps = 3
    n0 = rng.standard_normal((U, 64)).astype(np.float32)
    sc = m.eval().full_sort_predict([torch.arange(U, device=DEV)], noise=n0).cpu().numpy()
    want, gen, _ = F.predict_ref(F.model_params(m), U, I, rows, cols, n0, 3, m.schedule)
    np.testing.assert_allclose(sc, want, rtol=0, atol=1e-5 * np.abs(want).max())


# ----------------------------------------------------------------------------- prediction
@pytest.mark.parametrize("name,S,noisy", [("s0", 0, False), ("s3", 3, False), ("s3n", 3, True)])
def test_scores_match_reference(g, name, S, noisy):
    m = F.build_ddrm(g, sampling_steps=S, sampling_noise=noisy).eval()
    U = int(g["U"])
    sc = m.full_sort_predict([torch.arange(U, device=DEV)], noise=g["noise_" + name],
                             step_noise=g["step_noise_s3n"] if noisy else None).cpu().numpy()
    want = g["scores_" + name]
    assert sc.shape == want.shape
    np.testing.assert_allclose(sc, want, rtol=0, atol=1e-5 * np.abs(want).max())
    assert m.extra_state()["counters"]["eval_pass"] == 0  # nothing drawn


def _loaders(cfg, rows, cols, U, I, rng):
    from gmr.dataloader import EvalDataLoader
    from gmr.dataset import RecDataset
    tr = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I)
    eu = np.arange(U)
    ei = rng.integers(0, I, U)
    ev = RecDataset.from_arrays(cfg, eu, ei, np.ones(U), U, I)
    return EvalDataLoader(cfg, ev, additional_dataset=tr, batch_size=cfg["eval_batch_size"])


@pytest.mark.parametrize("S,noisy", [(0, False), (3, True)])
def test_topk_paths_and_batch_split(g, S, noisy):
    """The fused score -> mask -> top-K path and the unfused one give the same top-K by position from the same
    tables, and with Philox noise a user's top-K does not depend on the eval batch size."""
    from gmr.trainer import Trainer
    U, I = int(g["U"]), int(g["I"])
    tops = []
    for eb, fused in ((16, True), (16, False), (5, False), (37, True)):
        m = F.build_ddrm(g, sampling_steps=S, sampling_noise=noisy, eval_batch_size=eb)
        tr = Trainer(m.config, m)
        tr.fused_eval = fused
        ev = _loaders(m.config, g["train_rows"], g["train_cols"], U, I, np.random.default_rng(1))
        m.eval()
        val = torch.empty((U, 10), device=DEV)
        top = tr.topk_all(ev, 10, out_val=val).cpu().numpy().copy()
        assert m.extra_state()["counters"]["eval_pass"] == 1
        tops.append((top, val.cpu().numpy().copy()))
    (t0, v0) = tops[0]
    for t1, v1 in tops[1:]:
        np.testing.assert_allclose(v1, v0, rtol=1e-5, atol=1e-5 * np.abs(v0).max())
        # positions agree, or the two scores tie inside 1e-5
        bad = (t1 != t0) & (np.abs(v1 - v0) > 1e-5 * np.abs(v0))
        assert not bad.any()
    assert np.array_equal(tops[1][0], tops[2][0])  # the same unfused kernels at two batch sizes: the same bits
    # a second pass draws other noise
    m.forward_embeddings()
    assert m.extra_state()["counters"]["eval_pass"] == 2


# ----------------------------------------------------------------------------- end to end
def _e2e(tmp_path, epochs):
    from gmr.configurator import Config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.quick_start import build_data
    from gmr.utils import get_model, get_trainer, init_seed
    cfg = Config("DDRM", "baby", {"synthetic": "tiny", "epochs": epochs, "train_batch_size": 512,
                                  "eval_batch_size": 256, "topk": [5, 10], "valid_metric": "Recall@10", "seed": 999,
                                  "sampling_steps": 2, "sampling_noise": True, "checkpoint_dir": str(tmp_path),
                                  "save_recommended_topk": False})
    tr_ds, va_ds, te_ds = build_data(cfg).split()
    init_seed(999)
    tl = TrainDataLoader(cfg, tr_ds, batch_size=512, shuffle=True)
    va = EvalDataLoader(cfg, va_ds, additional_dataset=tr_ds, batch_size=256)
    tl.pretrain_setup()
    m = get_model("DDRM")(cfg, tl)
    return cfg, tl, va, m, get_trainer("DDRM")(cfg, m)


def test_end_to_end_and_resume(tmp_path):
    cfg, tl, va, m, tr = _e2e(tmp_path, 3)
    tr._train_data = tl
    losses = []
    for e in range(3):
        m.pre_epoch_processing()
        losses.append(tr._train_epoch(tl, e)[0])
        if e == 1:
            res = tr.evaluate(va)   # advances the eval-pass counter before the save
            assert len(res) > 0 and all(np.isfinite(x) and 0 <= x <= 1 for x in res.values()), res
            tr._save_checkpoint(1)
    assert all(np.isfinite(losses)), losses
    want_p = m.slab.data.cpu().numpy().copy()
    want_top = tr.topk_all(va, 10).cpu().numpy().copy()
    st = m.extra_state()["counters"]
    assert st["step"] > 0 and st["eval_pass"] == 2

    cfg2, tl2, va2, m2, tr2 = _e2e(tmp_path, 3)
    tr2.resume_checkpoint(str(tmp_path / "DDRM-baby.pth"), train_data=tl2)
    assert tr2.start_epoch == 2 and m2.extra_state()["counters"]["eval_pass"] == 1
    m2.pre_epoch_processing()
    loss2 = tr2._train_epoch(tl2, 2)[0]
    assert loss2 == losses[2]
    np.testing.assert_array_equal(m2.slab.data.cpu().numpy(), want_p)
    np.testing.assert_array_equal(tr2.topk_all(va2, 10).cpu().numpy(), want_top)
    assert m2.extra_state()["counters"] == st


def test_quick_start_runs(tmp_path, monkeypatch):
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    res = quick_start("DDRM", "baby", {"synthetic": "tiny", "epochs": 2, "train_batch_size": 512,
                                       "eval_batch_size": 256, "topk": [5, 10], "valid_metric": "Recall@10",
                                       "save_recommended_topk": False}, save_model=False)
    assert len(res) == 1 and all(np.isfinite(x) for x in res[0][2].values())
