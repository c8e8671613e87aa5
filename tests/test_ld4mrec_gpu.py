"""LD4MRec on the GPU: construction, one training step and the prediction against the values the reference recorded
(tests/golden/ld4mrec_tiny.npz), a mid shape against the fp64 restatement of tests/ld4m_fixture.py, and an
end-to-end run with checkpoint / resume on synthetic data."""
import numpy as np
import pytest
import torch

import ld4m_fixture as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
L = 2


def dev(a):
    return torch.as_tensor(a).to(DEV)


@pytest.fixture(scope="module")
def g():
    return F.load_golden()


# ----------------------------------------------------------------------------- construction
def test_construction(g):
    m = F.build_ld4(g, svd=False)
    names = F.param_names(L)
    assert [n for n, _ in m.named_parameters()] == names
    sd = m.state_dict()
    assert set(sd) == set(names) | {"loss_history"}
    for n in names:
        assert tuple(sd[n].shape) == g["p_" + F.key(n)].shape, n
        np.testing.assert_array_equal(sd[n].cpu().numpy(), g["p_" + F.key(n)], err_msg=n)   # bit for bit
    np.testing.assert_array_equal(sd["loss_history"].cpu().numpy(), np.ones(100, np.float32))
    np.testing.assert_allclose(m.alpha_bar.cpu().numpy(), g["alpha_bar"], rtol=1e-6)
    np.testing.assert_allclose(m.user_mm_emb.cpu().numpy(), g["user_mm_emb"], rtol=1e-5)
    E, want = m.user_svd_emb.cpu().numpy().astype(np.float64), g["user_svd_emb"].astype(np.float64)
    assert E.shape == want.shape
    np.testing.assert_allclose(E @ E.T, want @ want.T, rtol=0, atol=1e-4 * np.abs(want @ want.T).max())


def test_unsupported(g):
    with pytest.raises(NotImplementedError, match="cnet_hidden_size"):
        F.build_ld4(g, cnet_hidden_size=96)
    with pytest.raises(NotImplementedError, match="svd_k"):
        F.build_ld4(g, svd=False, svd_k=37)


# ----------------------------------------------------------------------------- the recorded step
@pytest.mark.parametrize("tag,dropout", [("d0_", 0.0), ("d1_", 0.1)])
def test_step_matches_reference(g, tag, dropout):
    m = F.build_ld4(g, dropout=dropout)
    users = dev(g["users"].astype(np.int32))
    masks = [dev(x) for x in g["d1_masks"]] if dropout else None
    loss = m.rec_step(users, t=dev(g["t"].astype(np.int32)), noise=dev(g["noise"]), masks=masks)
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(m.row_loss.cpu().numpy(), g[tag + "row_loss"], rtol=1e-5)
    names = F.param_names(L)
    F.check_grads(F.model_grads(m, L), [g[tag + "g_" + F.key(n)] for n in names], names, show=tag)
    np.testing.assert_allclose(m.loss_history.cpu().numpy(), g[tag + "loss_history"], rtol=1e-6)
    assert m.extra_state()["counters"]["step"] == 1


def test_unaligned_svd_k_against_fp64(g):
    """svd_k = 6: the modal block of the condition and of cond_proj starts 6 floats into a row, off the 16-byte
    grid of the aligned GEMM loads.  Own SVD table, the fixture's batch, t, noise and masks, fp64 restatement."""
    m = F.build_ld4(g, svd=False, svd_k=6, dropout=0.1)
    svd = m.user_svd_emb.cpu().numpy()
    assert svd.shape == (37, 6)
    masks = [dev(x) for x in g["d1_masks"]]
    loss = m.rec_step(dev(g["users"].astype(np.int32)), t=dev(g["t"].astype(np.int32)), noise=dev(g["noise"]),
                      masks=masks).item()
    U, I = int(g["U"]), int(g["I"])
    P = F.model_params(m, L)
    r = F.ld4_step_ref(P, L, U, I, g["train_rows"], g["train_cols"], g["users"], g["t"], g["noise"], g["alpha_bar"],
                       svd, g["user_mm_emb"], masks=g["d1_masks"], p_keep=float(np.float32(0.9)), dtype=torch.float64)
    np.testing.assert_allclose(loss, r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.row_loss.cpu().numpy(), r["rows"], rtol=1e-5)
    F.check_grads(F.model_grads(m, L), r["grads"], F.param_names(L))
    s = m.eval().full_sort_predict([torch.arange(U, device=DEV)]).cpu().numpy()
    want = F.ld4_predict_ref(P, L, U, I, g["train_rows"], g["train_cols"], np.arange(U), svd, g["user_mm_emb"])
    np.testing.assert_allclose(s, want, rtol=1e-4, atol=1e-5)


def test_injected_uniforms_draw_t(g):
    """rec_step(u=...) draws t from the injected uniforms: under the all-ones history t = floor(100 u)."""
    m = F.build_ld4(g)
    u = (np.arange(16, dtype=np.float32) * 6 + 2.5) / 100          # mid-bin points of bins 2, 8, 14, ...
    m.rec_step(dev(g["users"].astype(np.int32)), u=dev(u), noise=dev(g["noise"]))
    np.testing.assert_array_equal(m._w["t"][:16].cpu().numpy(), np.arange(16) * 6 + 2)


def test_calculate_loss_autograd(g):
    m = F.build_ld4(g)
    loss = m.calculate_loss([dev(g["users"])])
    (3.0 * loss).backward()
    sd = dict(m.named_parameters())
    w = sd["cnet.output_proj.weight"]
    assert torch.isfinite(loss) and w.grad is not None
    np.testing.assert_allclose(w.grad.cpu().numpy(), 3.0 * m.slab.gview("Wo").cpu().numpy(), rtol=1e-6)
    assert float(sd["t_in"].grad.abs().max()) == 0.0


def _check_top10(got, ref):
    for u in range(ref.shape[0]):
        gi, ri = np.argsort(-got[u], kind="stable")[:10], np.argsort(-ref[u], kind="stable")[:10]
        for a, b in zip(gi, ri):
            # positions agree, or the two items tie inside 1e-5 |s| in the reference
            assert a == b or abs(ref[u, a] - ref[u, b]) <= 1e-5 * abs(ref[u, b]), (u, a, b)


@pytest.mark.parametrize("name,t_in", [("scores_t0", 0.0), ("scores_tneg", -0.37)])
def test_scores_match_reference(g, name, t_in):
    m = F.build_ld4(g, dropout=0.1).eval()
    with torch.no_grad():
        m.t_in.fill_(t_in)
    U = int(g["U"])
    s = m.full_sort_predict([torch.arange(U, device=DEV)]).cpu().numpy()
    assert s.shape == g[name].shape
    np.testing.assert_allclose(s, g[name], rtol=1e-4, atol=1e-5)
    _check_top10(s, g[name])


# ----------------------------------------------------------------------------- mid shape, fp64 restatement
@pytest.mark.parametrize("layers", [1, 3])
def test_mid_shape_against_fp64(layers):
    U, I, B = 300, 1103, 700
    m, rows, cols, v, tf = F.build_ld4_mid(layers, U=U, I=I, batch=B)
    rng = np.random.default_rng(4)
    users = rng.integers(0, U, B)
    noise = rng.standard_normal((B, I)).astype(np.float32)
    P = F.model_params(m, layers)
    mm = F.user_mm_ref(U, I, rows, cols, np.concatenate([v, tf], 1))
    np.testing.assert_allclose(m.user_mm_emb.cpu().numpy(), mm.numpy(), rtol=1e-5, atol=1e-6 * float(mm.abs().max()))
    svd = m.user_svd_emb.cpu().numpy()
    loss = m.rec_step(dev(users.astype(np.int32)), noise=dev(noise)).item()   # t and the masks from the device
    t = m._w["t"][:B].cpu().numpy()
    assert t.min() >= 0 and t.max() < 100 and len(np.unique(t)) > 50
    masks = [m._w["mask"][l, :B].cpu().numpy() for l in range(layers)]
    assert all(0.85 < k.mean() < 0.95 for k in masks)
    r = F.ld4_step_ref(P, layers, U, I, rows, cols, users, t, noise, m.alpha_bar.cpu().numpy(), svd, mm, masks=masks,
                       p_keep=float(np.float32(0.9)), hist=np.ones(100, np.float32), dtype=torch.float64)
    print(f"mid L={layers}: loss {loss:.8f} ref {r['loss']:.8f}")
    np.testing.assert_allclose(loss, r["loss"], rtol=1e-5)
    np.testing.assert_allclose(m.row_loss.cpu().numpy(), r["rows"], rtol=1e-5)
    names = F.param_names(layers)
    F.check_grads(F.model_grads(m, layers), r["grads"], names, show=f"mid L={layers}")
    np.testing.assert_allclose(m.loss_history.cpu().numpy(), r["hist"], rtol=1e-6)
    # prediction at the same shape (one block of users past a 256-row tile)
    eu = np.arange(U)
    s = m.eval().full_sort_predict([dev(eu)]).cpu().numpy()
    want = F.ld4_predict_ref(P, layers, U, I, rows, cols, eu, svd, mm)
    np.testing.assert_allclose(s, want, rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------- end to end
def _e2e(tmp_path, epochs):
    from gmr.configurator import Config
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.quick_start import build_data
    from gmr.utils import get_model, get_trainer, init_seed
    cfg = Config("LD4MRec", "baby", {"synthetic": "tiny", "epochs": epochs, "train_batch_size": 512,
                                     "eval_batch_size": 256, "svd_k": 8, "cnet_hidden_size": 64, "cnet_n_layers": 2,
                                     "topk": [5, 10], "valid_metric": "Recall@10", "seed": 999,
                                     "checkpoint_dir": str(tmp_path), "save_recommended_topk": False})
    tr_ds, va_ds, te_ds = build_data(cfg).split()
    init_seed(999)
    tl = TrainDataLoader(cfg, tr_ds, batch_size=512, shuffle=True)
    va = EvalDataLoader(cfg, va_ds, additional_dataset=tr_ds, batch_size=256)
    te = EvalDataLoader(cfg, te_ds, additional_dataset=tr_ds, batch_size=256)
    tl.pretrain_setup()
    m = get_model("LD4MRec")(cfg, tl)
    return cfg, tl, va, te, m, get_trainer("LD4MRec")(cfg, m)


def _scores(m, n=64):
    return m.eval().full_sort_predict([torch.arange(n, device=DEV)]).cpu().numpy().copy()


def test_end_to_end_and_resume(tmp_path):
    cfg, tl, va, te, m, tr = _e2e(tmp_path, 3)
    tr._train_data = tl
    losses = []
    for e in range(3):
        m.pre_epoch_processing()
        losses.append(tr._train_epoch(tl, e)[0])
        if e == 1:
            tr._save_checkpoint(1)
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses
    hist = m.loss_history.cpu().numpy()
    assert np.isfinite(hist).all() and (hist != 1).sum() > 50
    res = tr.evaluate(va)
    assert len(res) > 0 and all(np.isfinite(x) and 0 <= x <= 1 for x in res.values()), res
    want = _scores(m)
    assert float(m.t_in.detach().abs().max()) == 0.0

    cfg2, tl2, _, _, m2, tr2 = _e2e(tmp_path, 3)
    m2.set_user_svd_emb(-m2.user_svd_emb)   # a construction whose SVD came out with other signs
    tr2.resume_checkpoint(str(tmp_path / "LD4MRec-baby.pth"), train_data=tl2)
    assert tr2.start_epoch == 2 and m2.extra_state()["counters"]["step"] > 0
    m2.pre_epoch_processing()
    loss2 = tr2._train_epoch(tl2, 2)[0]
    assert loss2 == losses[2]
    np.testing.assert_array_equal(_scores(m2), want)
    ck = torch.load(str(tmp_path / "LD4MRec-baby.pth"), map_location="cpu", weights_only=True)
    assert tuple(ck["generated_graphs"]["user_svd_emb"].shape) == (m.n_users, 8)
    assert "loss_history" in ck["state_dict"] and "user_svd_emb" not in ck["state_dict"]


def test_quick_start_runs(tmp_path, monkeypatch):
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    res = quick_start("LD4MRec", "baby", {"synthetic": "tiny", "epochs": 1, "train_batch_size": 512,
                                          "eval_batch_size": 256, "svd_k": 8, "cnet_hidden_size": 64,
                                          "cnet_n_layers": 1, "topk": [5, 10], "valid_metric": "Recall@10",
                                          "save_recommended_topk": False}, save_model=False)
    assert len(res) == 1 and all(np.isfinite(x) for x in res[0][2].values())
