"""SMORE on the HIP path vs golden vectors from the reference (models/smore.py; tiny shape,
tests/golden/make_golden_smore.py: the reference rerun in double).  Case A: the init as drawn, one item-graph layer, no
dropout; case B: scaled parameters, two layers, dropout 0.1 with the reference's three masks injected.

Bars (test_mgcn_kernels_gpu.py's rule): rtol 1e-5 against fp64, and next to it an entry may be off by twice the largest
error of the same computation done by fp32 torch on the CPU (the restatement of tests/smore_fixture.py, which
tests/test_smore_restatement_cpu.py pins to the golden values) against fp64, measured here and printed."""
import hashlib

import numpy as np
import pytest
import torch

import smore_fixture as F
from smore_fixture import CASES, DEV, PARAMS, build_smore

pytestmark = pytest.mark.gpu

# sha256 over the loss bits and every gradient of MGCN's step on mgcn_tiny.npz, taken at the commit before SMORE
MGCN_DIGESTS = {"A": "70cdd1b6eecaaae573734a99b09aad7cb3000f8484a836e6074d9d61b7f7b6c9",
                "B": "0e7daaa9115d8ce3c38e9f7c487df0c2effe097bfa3b5d199ad1513e303ee6d4"}


@pytest.fixture(scope="module")
def g(golden):
    return dict(golden("smore_tiny"), **golden("smore_tiny_B"))


@pytest.fixture(scope="module")
def ref32(g):
    """The fp32 restatement of both cases on the CPU: what fp32 torch gives for the same step."""
    out = {}
    for case, c in CASES.items():
        out[case] = F.smore_step_ref(F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"],
                                     g["train_cols"], g["users"], g["pos"], g["neg"], c["n_layers"], c["cl_loss"],
                                     (g["v_feat"], g["t_feat"]), keep=_keep_np(g, case), p=c["dropout_rate"],
                                     dtype=torch.float32)
    return out


def _keep_np(g, case, step=0):
    return F.golden_keep(g, step) if case == "B" else None


def _keep(g, case, step=0):
    k = _keep_np(g, case, step)
    return None if k is None else torch.as_tensor(k).to(DEV)


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
    m, *_ = build_smore(g, "A")
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == PARAMS
    assert list(m.state_dict()) == F.STATE_KEYS
    for p, k in zip(m._params(), PARAMS):
        assert np.array_equal(p.detach().cpu().numpy(), g["init_" + k]), k
    assert [tuple(v.shape) for v in m.grad_views()] == [g["init_" + k].shape for k in PARAMS]


def test_graphs(g):
    m, *_ = build_smore(g, "A")
    U, I = m.n_users, m.n_items
    for csr, k, shape in ((m.norm_adj, "adj", (U + I, U + I)), (m.R, "R", (U, I)),
                          (m.mm_adj["image"], "image_adj", (I, I)), (m.mm_adj["text"], "text_adj", (I, I)),
                          (m.mm_adj["fusion"], "fusion_adj", (I, I))):
        got, want = _dense(csr), F.dense_of(g[k + "_idx"], g[k + "_val"], shape)
        assert np.array_equal(got != 0, want != 0), k
        assert np.isfinite(got).all(), k
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0, err_msg=k)
    # the fusion graph is the restatement's union of the model's own two graphs, exactly: pattern and values
    av, at = (torch.tensor(_dense(m.mm_adj[k]), dtype=torch.float32) for k in ("image", "text"))
    assert np.array_equal(_dense(m.mm_adj["fusion"]), F.fusion_ref(av, at).numpy().astype(np.float64))
    col, rp = m.mm_adj["fusion"].col.cpu().numpy(), m.mm_adj["fusion"].rowptr.cpu().numpy()
    assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(I))       # columns ascending, no duplicates
    for k in ("image", "text", "fusion"):
        assert np.array_equal(_dense(m.mm_adj_t[k]), _dense(m.mm_adj[k]).T), k
    assert np.array_equal(_dense(m.R_t), _dense(m.R).T)


@pytest.mark.parametrize("case", ["A", "B"])
def test_step_parity(g, ref32, case):
    tag = case + "_"
    m, *_ = build_smore(g, case)
    users, pos, neg = _batch(g)
    keep = _keep(g, case)
    loss = m.rec_step(users, pos, neg, keep=keep)
    print(f"{case}: loss {loss.item():.7f} (reference {g[tag + 'loss']:.7f})")
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    print(f"{case}: terms {terms[1:]} (reference {g[tag + 'loss_terms']})")
    np.testing.assert_allclose(terms[0], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1:], g[tag + "loss_terms"], rtol=1e-5)
    r32 = ref32[case]
    for k, got in (("c", m.c), ("side", m.side)):
        F.bar(got, g[tag + k], r32[k], f"{case} {k}")
    F.bar(m.all, g[tag + "c"] + g[tag + "side"], r32["all"], f"{case} all")
    first = _grads(m)
    for got, w32, k in zip(first, r32["grads"], PARAMS):
        F.bar(got, g[tag + "g_" + k], w32, f"{case} gradient {k}")
    for k, got in zip(PARAMS[:3], first[:3]):      # Im W_0, Im W_32: exactly 0
        assert got[0, 0, 1] == 0.0 and got[0, 32, 1] == 0.0, k
    # every work buffer filled with NaN: nothing of a step reads what an earlier step left
    bufs = [m.vt, m.spec, m.conv, m.gates_i, m.pur, m.abf, m.c, m.side, m.all, m.saved, m.dall, m.gtab, m.dabf, m.dc,
            m.zf, m.dpur, m.zp, m.dvt, m._ws, m._loss, *m._h, *m._layers, *m._t,
            *[v for v in m._w.values() if torch.is_tensor(v) and v.is_floating_point()]]
    for t in bufs:
        t.fill_(float("nan"))
    m.slab.grad.fill_(float("nan"))
    m.load_extra_state({"counters": {"step": 0}})
    again = m.rec_step(users, pos, neg, keep=keep)
    assert again.item() == loss.item()
    for a, b, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b), k
    assert torch.equal(m.all, m.c + m.side)         # all, side and c stay alive after a step
    assert m.extra_state() == {"counters": {"step": 1}}


def test_loader_plans_give_the_same_step(g):
    m, cfg, ds, tl = build_smore(g, "B")
    d = tl.epoch()
    b, sizes, u, p, ng, pb, pc = next(iter(tl.batches(d)))
    keep = _keep(g, "B")
    with_plans = m.rec_step(u, p, ng, pb, pc, keep=keep).item()
    first = _grads(m)
    assert m.rec_step(u, p, ng, keep=keep).item() == with_plans
    for a, b_, k in zip(_grads(m), first, PARAMS):
        assert np.array_equal(a, b_), k


def test_calculate_loss_scales_by_upstream(g):
    m, *_ = build_smore(g, "A")
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
def test_predict(g, ref32, case):
    """full_sort_predict against the golden scores (evaluation: no dropout), and Trainer.evaluate's top-K, fused and
    unfused, against the top-K of the golden scores outside near-ties."""
    from gmr.dataloader import EvalDataLoader
    from gmr.dataset import RecDataset
    from gmr.trainer import Trainer
    m, cfg, ds, tl = build_smore(g, case)
    U, I = m.n_users, m.n_items
    scores = m.full_sort_predict([torch.arange(U, device=DEV)])
    want, s32 = g[case + "_scores"], ref32[case]["scores"]
    own = float(np.abs(s32.astype(np.float64) - want).max())
    F.bar(scores, want, s32, f"{case} scores")
    rng = np.random.default_rng(4)
    ev = RecDataset.from_arrays(cfg, np.arange(U), rng.integers(0, I, U), np.zeros(U), U, I, g["v_feat"], g["t_feat"])
    vl = EvalDataLoader(cfg, ev, additional_dataset=ds, batch_size=16)
    tr = Trainer(cfg, m)
    tops = []
    for fused in (True, False):
        tr.fused_eval = fused
        tops.append(tr.topk_all(vl, 10).cpu().numpy()[:U])
    res = tr.evaluate(vl)
    assert all(np.isfinite(v) and 0 <= v <= 1 for v in res.values())
    ref = want.copy()
    ref[g["train_rows"], g["train_cols"]] = -1e10
    eu = vl.eval_u_np
    want_val = -np.sort(-ref[eu], axis=1)[:, :10]
    for top in tops:
        np.testing.assert_allclose(np.take_along_axis(ref[eu], top.astype(np.int64), axis=1), want_val, rtol=1e-5,
                                   atol=2 * own)
    assert np.array_equal(tops[0], tops[1])


def test_evaluation_draws_nothing(g):
    m, *_ = build_smore(g, "B")
    assert m.dropout_rate == 0.1
    u1, i1 = (t.clone() for t in m.forward_embeddings())
    saved = m.saved.clone()
    u2, i2 = m.forward_embeddings()
    assert torch.equal(u1, u2) and torch.equal(i1, i2)
    assert m.extra_state() == {"counters": {"step": 0}}
    # the gate rows of an evaluation are plain sigmoids: none is 0, none is above 1
    gates = saved[:, 256:]
    assert bool((gates > 0).all()) and bool((gates <= 1).all())
    # a training step without injected masks drops about a tenth of them, and the next step other ones
    users, pos, neg = _batch(g)
    m.rec_step(users, pos, neg)
    k0 = m.saved[:, 256:] != 0
    m.rec_step(users, pos, neg)
    k1 = m.saved[:, 256:] != 0
    n = k0.numel()
    assert abs(k0.float().mean().item() - 0.9) <= 5 * np.sqrt(0.09 / n) and not torch.equal(k0, k1)


def test_adam_trajectory(g):
    """Case B, three Adam steps with the reference's masks against the reference's own fp32 torch.optim.Adam run, on
    every parameter.  The tolerance is measured (lattice_fixture.adam_reach's rule): twice the distance of the
    reference's fp32 run from the same three steps of the fp64 restatement, three roundings of the parameter, and per
    element the reach of gradients within the gradient bar through Adam's division.  rtol 0."""
    from gmr.trainer import Trainer
    c = CASES["B"]
    m, cfg, *_ = build_smore(g, "B")
    opt = Trainer(cfg, m).optimizer
    users, pos, neg = _batch(g)
    args = (F.case_params(g, "B"), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["pos"],
            g["neg"], c["n_layers"], c["cl_loss"], (g["v_feat"], g["t_feat"]), g["B_keep"], c["dropout_rate"])
    t64, g64 = F.trajectory(*args)
    _, g32 = F.trajectory(*args, dtype=torch.float32)
    reach = F.adam_reach(g64, g32, lr=F.LR)
    im0 = [p.detach().cpu().numpy()[0, [0, 32], 1].copy() for p in m._params()[:3]]
    for j in range(F.ADAM_STEPS):
        m.rec_step(users, pos, neg, keep=_keep(g, "B", j))
        opt.step()
    j = F.ADAM_STEPS - 1
    worst = 0.0
    for p, k in zip(m._params(), PARAMS):
        want = g[f"traj{j + 1}_{k}"]
        err32 = float(np.abs(want.astype(np.float64) - t64[j][k]).max())
        atol = 2 * err32 + F.ADAM_STEPS * np.spacing(np.float32(np.abs(want).max())) + reach[j][k]
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want)
        worst = max(worst, float(np.max(atol)))
        print(f"step {j + 1} {k}: max abs error {err.max():.3e} (fp32 torch {err32:.3e}, reach up to "
              f"{np.max(reach[j][k]):.3e}, median {np.median(reach[j][k]):.3e})")
        assert (err <= atol).all(), (k, float((err - atol).max()))
    print(f"largest tolerance of the trajectory: {worst:.3e} ({worst / F.LR:.2f} lr)")
    # Im W_0 and Im W_32 of the three filters have a zero gradient: Adam leaves them as they were
    for p, before, k in zip(m._params()[:3], im0, PARAMS):
        assert np.array_equal(p.detach().cpu().numpy()[0, [0, 32], 1], before), k


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
    model and trainer resumed from the first epoch's checkpoint draw the second epoch's masks and end with the same
    parameters, bit for bit."""
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.trainer import Trainer
    from gmr.utils import get_model

    def make(epochs, sub):
        cfg = F.smore_config(**dict(CASES["B"], learning_rate=0.01, epochs=epochs,
                                    checkpoint_dir=str(tmp_path / sub), eval_step=1))
        tr_ds, va, te = _tiny_split(g, cfg)
        tl = TrainDataLoader(cfg, tr_ds, batch_size=16)
        torch.manual_seed(3)
        m = get_model("SMORE")(cfg, tl)
        vl = EvalDataLoader(cfg, va, additional_dataset=tr_ds, batch_size=16)
        return m, Trainer(cfg, m), tl, vl

    m, trainer, tl, vl = make(2, "full")
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=True)
    l0, l1 = trainer.train_loss_dict[0], trainer.train_loss_dict[1]
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0, (l0, l1)
    assert "recall@10" in valid and 0.0 <= valid["recall@10"] <= 1.0
    assert m.extra_state()["counters"]["step"] == 2 * len(tl)
    ck = torch.load(str(tmp_path / "full" / "SMORE-baby.pth"), map_location="cpu", weights_only=True)
    assert list(ck["state_dict"]) == F.STATE_KEYS
    m1, t1, tl1, vl1 = make(1, "part")
    t1.fit(tl1, valid_data=vl1, test_data=vl1, saved=False)
    t1._save_checkpoint(0)
    m2, t2, tl2, vl2 = make(2, "part")
    t2.resume_checkpoint(str(tmp_path / "part" / "SMORE-baby.pth"), train_data=tl2)
    assert t2.start_epoch == 1 and m2.extra_state()["counters"]["step"] == len(tl)
    t2.fit(tl2, valid_data=vl2, test_data=vl2, saved=False)
    assert torch.equal(m2.slab.data, m.slab.data)
    # without the step counter the second epoch draws the first one's masks: other parameters
    m3, t3, tl3, vl3 = make(2, "part")
    t3.resume_checkpoint(str(tmp_path / "part" / "SMORE-baby.pth"), train_data=tl3)
    m3.load_extra_state({"counters": {"step": 0}})
    t3.fit(tl3, valid_data=vl3, test_data=vl3, saved=False)
    assert not torch.equal(m3.slab.data, m.slab.data)


def test_quick_start(tmp_path, monkeypatch):
    """quick_start("SMORE", "baby", ...) on the tiny synthetic shape with SMORE.yaml's values."""
    from gmr.configurator import Config
    from gmr.quick_start import quick_start
    monkeypatch.chdir(tmp_path)
    saved = tmp_path / "saved"
    cfg_dict = {"synthetic": "tiny", "epochs": 2, "checkpoint_dir": str(saved), "save_recommended_topk": False}
    results = quick_start("SMORE", "baby", cfg_dict, save_model=True)
    assert len(results) == 1
    _, best_valid, best_test = results[0]
    cfg = Config("SMORE", "baby", dict(cfg_dict))
    want = {f"{mt.lower()}@{k}" for mt in cfg["metrics"] for k in cfg["topk"]}
    assert set(best_valid) == want and want <= set(best_test)
    assert all(0.0 <= best_valid[k] <= 1.0 for k in want)
    ck = torch.load(str(saved / "SMORE-baby.pth"), map_location="cpu", weights_only=True)
    assert list(ck["state_dict"]) == F.STATE_KEYS


def test_unsupported_settings_raise(g, monkeypatch):
    from gmr import dist
    with pytest.raises(NotImplementedError, match="embedding_size"):
        build_smore(g, "A", embedding_size=32)
    with pytest.raises(NotImplementedError, match="sparse"):
        build_smore(g, "A", sparse=False)
    m, *_ = build_smore(g, "A")
    monkeypatch.setattr(dist, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="one device"):
        m.rec_step(*_batch(g))
    monkeypatch.setattr(dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        build_smore(g, "A")


def mgcn_digest(m, users, pos, neg):
    loss = m.rec_step(users, pos, neg)
    h = hashlib.sha256(loss.cpu().numpy().tobytes())
    for v in m.grad_views():
        h.update(np.ascontiguousarray(v.cpu().numpy()).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("case", ["A", "B"])
def test_mgcn_is_unchanged(golden, case):
    """MGCN shares its loss, its scatters and its behaviour backward with SMORE now: the loss and every gradient of
    its step on mgcn_tiny.npz have the bits they had before."""
    from mgcn_fixture import build_mgcn
    gm = golden("mgcn_tiny")
    m, *_ = build_mgcn(gm, case)
    users, pos, neg = (torch.as_tensor(gm[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg"))
    assert mgcn_digest(m, users, pos, neg) == MGCN_DIGESTS[case]
