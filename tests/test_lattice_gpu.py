"""LATTICE on the HIP path vs golden vectors from the reference (models/lattice.py rerun in double on the tiny shape,
tests/golden/make_golden_lattice.py).  Case A: both modalities, lightgcn, one item-graph layer, lambda 0.9; case B: two
layers, lambda 0.5, embedding tables times 8; case C: text only, mf.  The bar is test_mgcn_kernels_gpu's: rtol 1e-5
against fp64 with an atol of twice fp32 torch's own error, which the fp32 restatement of tests/lattice_fixture.py
measures here (tests/test_lattice_restatement_cpu.py pins that restatement to the same golden values)."""
import functools

import numpy as np
import pytest
import torch

import lattice_fixture as F
from lattice_fixture import CASES, DEV, bar, build_lattice, params_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    main = golden("lattice_tiny")
    return {c: (main if c == "A" else dict(main, **golden(F.FILES[c]))) for c in CASES}


_G = {}


@functools.lru_cache(maxsize=None)
def ref32(case):
    """The build step, the frozen step and the scores of the fp32 restatement: fp32 torch's own error."""
    r = F.Restatement(_G[case], case, dtype=torch.float32)
    build = r.step(True)
    adj = r.item_adj()
    return {"build": build, "item_adj": adj, "frozen": r.step(False), "scores": r.scores()}


def _ref32(g, case):
    _G[case] = g[case]
    return ref32(case)


def _batch(d):
    return [torch.as_tensor(d[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _grads(m):
    return [v.cpu().numpy().copy() for v in m.grad_views()]


def _dense(G):
    col, val = G.col.cpu().numpy().astype(np.int64), G.val.cpu().numpy().astype(np.float64)
    out = np.zeros((col.shape[0], col.shape[0]))
    np.add.at(out, (np.arange(col.shape[0])[:, None].repeat(col.shape[1], 1), col), val)
    return out


def test_registered(g):
    from gmr.utils import get_model
    from gmr.lattice import LATTICE
    assert get_model("LATTICE") is LATTICE


@pytest.mark.parametrize("case", list(CASES))
def test_init_parity(g, case):
    d = g[case]
    m, *_ = build_lattice(d, case)
    names = params_of(case)
    assert [n.replace(".", "_") for n, _ in m.named_parameters()] == names == [str(n) for n in d[case + "_params"]]
    P = F.case_params(d, case)
    for p, k in zip(m._params(), names):
        assert np.array_equal(p.detach().cpu().numpy(), P[k]), k
    assert [tuple(v.shape) for v in m.grad_views()] == [P[k].shape for k in names]
    assert len(m.optim_slabs()) == 2 and not hasattr(m, "tape_safe")


@pytest.mark.parametrize("case", list(CASES))
def test_graph(g, case):
    """The original and the learned lists (as sets per row) and item_adj, densified."""
    d, tag = g[case], case + "_"
    m, *_ = build_lattice(d, case)
    users, pos, neg = _batch(d)
    m.rec_step(users, pos, neg)
    k, G = m.knn_k, m.graph
    col = G.col.cpu().numpy()
    for j, name in enumerate(CASES[case]["mods"]):
        Mk = m.M * k
        for kind, got in (("learn", col[:, j * k:(j + 1) * k]), ("orig", col[:, Mk + j * k:Mk + (j + 1) * k])):
            assert np.array_equal(np.sort(got, 1), d[tag + kind + "_" + name + "_idx"]), (kind, name)
    bar(_dense(G), d[tag + "item_adj"], _ref32(g, case)["item_adj"], case + " item_adj")
    # the transpose the backward multiplies by
    t = G.csr_t
    rp, tc, tv = (x.cpu().numpy() for x in (t.rowptr, t.col, t.val))
    dt = np.zeros_like(d[tag + "item_adj"])
    for r in range(t.n_rows):
        np.add.at(dt[r], tc[rp[r]:rp[r + 1]], tv[rp[r]:rp[r + 1]].astype(np.float64))
    np.testing.assert_allclose(dt, _dense(G).T, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", list(CASES))
def test_steps(g, case):
    """The build step and the frozen step after it: loss and every gradient; the graph slab is marked on the frozen
    step; a second run from NaN-filled work buffers gives the same bits."""
    d, tag = g[case], case + "_"
    m, *_ = build_lattice(d, case)
    users, pos, neg = _batch(d)
    names, r32 = params_of(case), _ref32(g, case)
    got = {}
    for step in ("build", "frozen"):
        loss = m.rec_step(users, pos, neg).item()
        print(f"{case} {step}: loss {loss:.7f} (reference {d[tag + step + '_loss']:.7f})")
        np.testing.assert_allclose(loss, d[tag + step + "_loss"], rtol=1e-5)
        terms = m.loss_terms().cpu().numpy()
        np.testing.assert_allclose(terms[1] + terms[2], d[tag + step + "_loss"], rtol=1e-5)
        assert m.gslab.has_grad == (step == "build")
        grads = _grads(m)
        for k, gv, h, g32 in zip(names, grads, d[tag + step + "_has_grad"], r32[step]["grads"]):
            if h:
                bar(gv, d[tag + step + "_g_" + k], g32, f"{case} {step} {k}")
            elif step == "frozen" or k != "modal_weight":
                assert not gv.any(), k  # the reference leaves .grad = None
        got[step] = (loss, grads)
    # every work buffer filled with NaN: nothing of a step reads what an earlier step left
    m2, *_ = build_lattice(d, case)
    bufs = [m2.feats, m2.nfeat, m2.fnrm, m2.hn, m2.hnrm, m2.tab, m2.gtab, m2.dA, m2.dr, m2.dv, m2.parts, m2.dn, m2.dfeat,
            m2._loss, m2.graph.val, m2.graph.v, m2.graph.r, m2.graph.s, *m2._h, *m2._g, *m2._layers, *m2._t]
    for t in bufs:
        t.fill_(float("nan"))
    m2.slab.grad.fill_(float("nan"))
    m2.gslab.grad.fill_(float("nan"))
    for step in ("build", "frozen"):
        assert m2.rec_step(users, pos, neg).item() == got[step][0]
        for a, b, k in zip(_grads(m2), got[step][1], names):
            assert np.array_equal(a, b), (step, k)


@pytest.mark.parametrize("case", list(CASES))
def test_predict(g, case):
    """full_sort_predict against the golden scores; an evaluation between two steps leaves the training graph alone;
    the fused and the unfused evaluation paths give the same top-k."""
    from gmr.dataloader import EvalDataLoader
    from gmr.dataset import RecDataset
    from gmr.trainer import Trainer
    d = g[case]
    m, cfg, ds, tl = build_lattice(d, case)
    U, I = m.n_users, m.n_items
    users, pos, neg = _batch(d)
    m.rec_step(users, pos, neg)
    before = (m.graph.col.clone(), m.graph.val.clone())
    scores = m.full_sort_predict([torch.arange(U, device=DEV)])
    want, s32 = d[case + "_scores"], _ref32(g, case)["scores"]
    own = float(np.abs(s32.astype(np.float64) - want).max())
    print(f"{case} scores: max abs error {np.abs(scores.cpu().numpy() - want).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(scores.cpu().numpy(), want, rtol=1e-5, atol=2 * own)
    assert torch.equal(m.graph.col, before[0]) and torch.equal(m.graph.val, before[1])
    assert not m.build_item_graph
    rng = np.random.default_rng(4)
    v = d["v_feat"] if "image" in CASES[case]["mods"] else None
    ev = RecDataset.from_arrays(cfg, np.arange(U), rng.integers(0, I, U), np.zeros(U), U, I, v, d["t_feat"])
    vl = EvalDataLoader(cfg, ev, additional_dataset=ds, batch_size=16)
    tr = Trainer(cfg, m)
    tops = []
    for fused in (True, False):
        tr.fused_eval = fused
        tops.append(tr.topk_all(vl, 10).cpu().numpy()[:U])
    ref = want.copy()
    ref[d["train_rows"], d["train_cols"]] = -1e10
    eu = vl.eval_u_np
    want_val = -np.sort(-ref[eu], axis=1)[:, :10]
    for top in tops:  # the golden scores of the picked items are the 10 largest golden scores, outside near-ties
        np.testing.assert_allclose(np.take_along_axis(ref[eu], top.astype(np.int64), axis=1), want_val, rtol=1e-5,
                                   atol=2 * own)
    assert np.array_equal(tops[0], tops[1])


def test_adam_trajectory(g):
    """Case A, four Adam steps across an epoch boundary (build, frozen, frozen, pre_epoch_processing, build) against
    the reference's own torch.optim.Adam run.  The tolerance is measured, as in the other trajectory tests here
    (rfbm3_fixture.p1_bound): twice the distance of the same four steps taken by fp32 torch on the CPU from the
    restatement, four roundings of the parameter (one per step), and per element the reach of gradients within the
    gradient bar through Adam's division (lattice_fixture.adam_reach: an entry whose gradient is near eps moves by a
    large share of lr for a small change of the gradient, and the CPU restatement shares the reference's summation
    order, so its own distance does not show this).  rtol 0.  The graph-side moments after step 2 equal those after
    step 1 bit for bit."""
    from gmr.trainer import Trainer
    d = g["A"]
    m, cfg, *_ = build_lattice(d, "A")
    tr = Trainer(cfg, m)
    opt = tr.optimizer
    users, pos, neg = _batch(d)
    names = params_of("A")
    r32, r64 = F.Restatement(d, "A", dtype=torch.float32), F.Restatement(d, "A")
    own = r32.trajectory()
    r64.trajectory()
    reach = F.adam_reach(r64.grad_log, r32.grad_log)
    m.pre_epoch_processing()
    moments = None
    for j, kind in enumerate(F.TRAJ_STEPS):
        if j == 3:
            m.pre_epoch_processing()
        m.rec_step(users, pos, neg)
        assert m.gslab.has_grad == (kind == "build")
        opt.step()
        for p, k in zip(m._params(), names):
            want = d[f"traj{j + 1}_{k}"]
            err32 = float(np.abs(own[j][k] - want).max())
            atol = 2 * err32 + 4 * np.spacing(np.float32(np.abs(want).max())) + reach[j][k]
            got = p.detach().cpu().numpy()
            err = np.abs(got.astype(np.float64) - want)
            print(f"step {j + 1} {k}: max abs error {err.max():.3e} (fp32 torch {err32:.3e}, reach up to "
                  f"{np.max(reach[j][k]):.3e}, median {np.median(reach[j][k]):.3e})")
            assert (err <= atol).all(), (f"step {j + 1} {k}", float((err - atol).max()))
        st = opt.state[1]
        if j == 0:
            moments = (st["exp_avg"].clone(), st["exp_avg_sq"].clone())
        if j in (1, 2):
            assert torch.equal(st["exp_avg"], moments[0]) and torch.equal(st["exp_avg_sq"], moments[1])
            assert st["step"] == 1 and opt.state[0]["step"] == j + 1
    assert opt.state[1]["step"] == 2 and opt.state[0]["step"] == 4


def test_calculate_loss_scales_by_upstream(g):
    d = g["B"]
    m, *_ = build_lattice(d, "B")
    users, pos, neg = _batch(d)
    base = m.rec_step(users, pos, neg).item()
    want = _grads(m)
    m.pre_epoch_processing()
    inter = torch.stack([torch.as_tensor(d[k]) for k in ("users", "pos", "neg")]).to(DEV)
    out = m.calculate_loss(inter)
    assert out.item() == base
    (3.0 * out).backward()
    for p, w, k in zip(m._params(), want, params_of("B")):
        np.testing.assert_allclose(p.grad.cpu().numpy(), 3.0 * w, rtol=1e-6, atol=0, err_msg=k)


def test_short_batch_keeps_the_configured_divisor(g):
    """A last batch shorter than train_batch_size: the mean over its rows, the L2 term over the configured size."""
    d = g["B"]
    m, *_ = build_lattice(d, "B")
    users, pos, neg = (t[:11].contiguous() for t in _batch(d))
    loss = m.rec_step(users, pos, neg).item()
    r = F.Restatement(d, "B")
    lt = lambda a: torch.as_tensor(np.asarray(a[:11]).astype(np.int64))  # noqa: E731
    want = r.step(True, batch=(lt(d["users"]), lt(d["pos"]), lt(d["neg"])))
    np.testing.assert_allclose(loss, want["loss"], rtol=1e-5)
    full = m.rec_step(*_batch(d)).item()  # then a full batch again: the frozen step's loss
    np.testing.assert_allclose(full, d["B_frozen_loss"], rtol=1e-5)


def test_unsupported_settings_raise(g, monkeypatch):
    from gmr import dist
    with pytest.raises(NotImplementedError, match="ngcf"):
        build_lattice(g["A"], "A", cf_model="ngcf")
    with pytest.raises(NotImplementedError, match="knn_k"):
        build_lattice(g["A"], "A", knn_k=65)
    with pytest.raises(NotImplementedError, match="embedding_size"):
        build_lattice(g["A"], "A", embedding_size=32)
    m, *_ = build_lattice(g["A"], "A")
    monkeypatch.setattr(dist, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="one device"):
        m.rec_step(*_batch(g["A"]))


def _tiny_split(d, cfg):
    from gmr.dataset import RecDataset
    U, I = int(d["U"]), int(d["I"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(U), 6)
    cols = np.concatenate([rng.choice(I, 6, replace=False) for _ in range(U)])
    labels = np.zeros(rows.size)
    labels[4::6] = 1
    labels[5::6] = 2
    return RecDataset.from_arrays(cfg, rows, cols, labels, U, I, d["v_feat"], d["t_feat"]).split()


def test_fit_and_resume(g, tmp_path):
    """Two epochs through the generic Trainer: it trains, evaluates and writes a checkpoint; a fresh model and trainer
    resumed from the first epoch's checkpoint rebuild the graph at the epoch the uninterrupted run rebuilds it and end
    with the same parameters, bit for bit."""
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.lattice import LATTICE
    from gmr.trainer import Trainer
    d = g["A"]

    def make(epochs, sub):
        cfg = F.lattice_config(learning_rate=0.01, epochs=epochs, checkpoint_dir=str(tmp_path / sub), eval_step=1)
        tr_ds, va, te = _tiny_split(d, cfg)
        tl = TrainDataLoader(cfg, tr_ds, batch_size=16)
        torch.manual_seed(3)
        m = LATTICE(cfg, tl)
        vl = EvalDataLoader(cfg, va, additional_dataset=tr_ds, batch_size=16)
        return m, Trainer(cfg, m), tl, vl

    builds = []

    def count(m):
        orig = m._build

        def wrapped(G):
            if G is m.graph:
                builds.append(1)
            return orig(G)
        m._build = wrapped

    m, trainer, tl, vl = make(2, "full")
    count(m)
    best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=True)
    assert len(builds) == 2  # one graph per epoch; the evaluations build their own
    l0, l1 = trainer.train_loss_dict[0], trainer.train_loss_dict[1]
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0, (l0, l1)
    assert "recall@10" in valid and 0.0 <= valid["recall@10"] <= 1.0
    # one epoch, checkpoint, then a fresh pair resumed for the second epoch
    m1, t1, tl1, vl1 = make(1, "part")
    t1.fit(tl1, valid_data=vl1, test_data=vl1, saved=False)
    t1._save_checkpoint(0)
    m2, t2, tl2, vl2 = make(2, "part")
    t2.resume_checkpoint(str(tmp_path / "part" / "LATTICE-baby.pth"), train_data=tl2)
    assert t2.start_epoch == 1 and m2.build_item_graph
    del builds[:]
    count(m2)
    t2.fit(tl2, valid_data=vl2, test_data=vl2, saved=False)
    assert len(builds) == 1
    assert torch.equal(m2.slab.data, m.slab.data) and torch.equal(m2.gslab.data, m.gslab.data)
