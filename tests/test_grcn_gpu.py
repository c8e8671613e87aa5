"""GRCN on the HIP path vs golden vectors from the reference (models/grcn.py; tiny shape,
tests/golden/make_golden_grcn.py: the reference rerun in double).  Case A: both modalities, n_layers 3.  Case B:
n_layers 1, reg_weight 0.1, then three Adam steps.  Case C: image features only.  Loss, result, alpha and every gradient
are held to rtol 1e-5 + twice fp32 torch's own distance from the double rerun (stored per gradient by the maker; for
the tables, the fp32 restatement's)."""
import numpy as np
import pytest
import torch

import grcn_fixture as F
from grcn_fixture import CASES, DEV, build_grcn, params_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return dict(golden("grcn_tiny"), **golden("grcn_tiny_B"))


def _args(g, case, **over):
    cs = dict(CASES[case], **over)
    feats = (g["v_feat"], g["t_feat"] if "t" in cs["mods"] else None)
    return (F.case_params(g, case), int(g["U"]), int(g["I"]), g["train_rows"], g["train_cols"], g["users"], g["pos"],
            g["neg"], cs, feats)


@pytest.fixture(scope="module")
def ref32(g):
    """The fp32 restatement of the cases on the CPU: what fp32 torch gives for the tables the maker kept no distance
    for."""
    return {case: F.grcn_step_ref(*_args(g, case), dtype=torch.float32) for case in CASES}


def _batch(g):
    return [torch.as_tensor(g[k].astype(np.int32)).to(DEV) for k in ("users", "pos", "neg")]


def _grads(m):
    return [v.cpu().numpy().copy() for v in m.grad_views()]


def _bar_own(got, want, own, what, rtol=1e-5):
    got = got.astype(np.float64)
    print(f"{what}: max abs error {np.abs(got - want).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=2 * own, err_msg=what)


def _buffers(m):
    return [m.Wv, m.WTv, m.Z, m.F, m.nrmF, m.P, m.nrm0, m.nrmY, m.alpha, m.dalpha, m.ds, m.dw, m.RA, m.RD, m.DY, m.x,
            m.x1, m.nrmE, m.dx1, m.dx, m.dxd, m.dZ, m.result, m.G, m._loss,
            *[v for v in m._w.values() if torch.is_tensor(v)]]


@pytest.mark.parametrize("case", ["A", "C"])
def test_init_parity(g, case):
    m, *_ = build_grcn(g, case, as_drawn=True)
    names = params_of(case)
    assert [n for n, _ in m.named_parameters()] == F.STATE_KEYS[:len(names)]
    assert list(m.state_dict()) == F.STATE_KEYS[:len(names)]
    assert all(p.requires_grad for p in m.parameters())
    for p, k in zip(m._params(), names):
        assert np.array_equal(p.detach().cpu().numpy(), g[f"{case}_init_{k}"]), k
    assert [tuple(v.shape) for v in m.grad_views()] == [g[f"{case}_init_{k}"].shape for k in names]
    assert np.array_equal(m._table.cpu().numpy(), g[case + "_result0"])


def test_graph_lists(g):
    m, *_ = build_grcn(g, "A")
    U, I, E = m.n_users, m.n_items, m.E
    gr = m.graph
    rows, cols = g["train_rows"], g["train_cols"]
    rp, col, trp, tcol, c2r, r2c = (t.cpu().numpy() for t in (gr.rowptr, gr.col, gr.trp, gr.tcol, gr.csc2csr, gr.csr2csc))
    urow = np.repeat(np.arange(U), np.diff(rp))
    assert sorted(zip(urow.tolist(), col.tolist())) == sorted(zip(rows.tolist(), cols.tolist()))
    irow = np.repeat(np.arange(I), np.diff(trp))
    assert np.array_equal(urow[c2r], tcol) and np.array_equal(col[c2r], irow)
    assert np.array_equal(c2r[r2c], np.arange(E)) and (np.diff(trp) == 0).any() and (np.diff(rp) == 0).any()
    assert np.array_equal(gr.rowptr_n.cpu().numpy(), np.concatenate([rp, E + trp[1:]]))
    assert np.array_equal(gr.col_n.cpu().numpy(), np.concatenate([col + U, tcol]))


@pytest.mark.parametrize("case", list(CASES))
def test_step_parity(g, ref32, case):
    tag, names = case + "_", params_of(case)
    m, *_ = build_grcn(g, case)
    users, pos, neg = _batch(g)
    loss = m.rec_step(users, pos, neg)
    print(f"{case}: loss {loss.item():.7f} (reference {g[tag + 'loss']:.7f})")
    np.testing.assert_allclose(loss.item(), g[tag + "loss"], rtol=1e-5)
    terms = m.loss_terms().cpu().numpy()
    np.testing.assert_allclose(terms[1] + terms[2], g[tag + "loss"], rtol=1e-5)
    r32 = ref32[case]
    F.bar(m.result, g[tag + "result"], r32["result"], f"{case} result")
    F.bar(m.alpha_ref_order(), g[tag + "alpha"], r32["alpha"], f"{case} alpha")
    # the refined weights: every edge on the reference's side of the max and of the ReLU
    val = g[tag + "alpha"] * np.concatenate([F.case_params(g, case)["model_specific_conf"][g["train_rows"]],
                                            F.case_params(g, case)["model_specific_conf"][m.n_users + g["train_cols"]]])
    E, pos_e = m.E, m._edge_pos.cpu().numpy()
    arg = m.arg.cpu().numpy()
    arg_ref = np.concatenate([arg[E:2 * E][m.graph.csr2csc.cpu().numpy()][pos_e], arg[:E][pos_e]])
    assert np.array_equal(arg_ref & 1, val.argmax(1)) and np.array_equal(arg_ref < 2, val.max(1) > 0)
    first = _grads(m)
    for got, k in zip(first, names):
        assert np.isfinite(got).all(), k
        _bar_own(got, g[tag + "g_" + k], float(g[tag + "own_" + k]), f"{case} gradient {k}")
    # every work buffer filled with NaN: nothing of a step reads what an earlier step left
    for t in _buffers(m):
        if t.is_floating_point():
            t.fill_(float("nan"))
    m.slab.grad.fill_(float("nan"))
    again = m.rec_step(users, pos, neg)
    assert again.item() == loss.item()
    for a, b, k in zip(_grads(m), first, names):
        assert np.array_equal(a, b), k


@pytest.mark.parametrize("over", [dict(routing="items", n_layers=3), dict(routing="items", n_layers=1),
                                  dict(routing="items", n_layers=3, mods="v"), dict(n_layers=0)])
def test_other_settings_against_the_restatement(g, over):
    """The routing over the user's items (not a reference setting) and n_layers 0, against the fp64 restatement (pinned
    to the reference and to its hand-written backward by tests/test_grcn_restatement_cpu.py), with the atol of fp32
    torch's own error on the same step."""
    case = "C" if over.get("mods") == "v" else "A"
    cfg_over = {k: v for k, v in over.items() if k != "mods"}
    m, *_ = build_grcn(g, case, **cfg_over)
    users, pos, neg = _batch(g)
    loss = m.rec_step(users, pos, neg)
    r64 = F.grcn_step_ref(*_args(g, case, **cfg_over))
    r32 = F.grcn_step_ref(*_args(g, case, **cfg_over), dtype=torch.float32)
    np.testing.assert_allclose(loss.item(), r64["loss"], rtol=1e-5)
    F.bar(m.result, r64["result"], r32["result"], f"{over} result")
    F.bar(m.alpha_ref_order(), r64["alpha"], r32["alpha"], f"{over} alpha")
    for got, w64, w32, k in zip(_grads(m), r64["grads"], r32["grads"], params_of(case)):
        F.bar(got, w64, w32, f"{over} gradient {k}")


def test_loader_plans_give_the_same_step(g):
    m, cfg, ds, tl = build_grcn(g, "A")
    d = tl.epoch()
    b, sizes, u, p, ng, pb, pc = next(iter(tl.batches(d)))
    with_plans = m.rec_step(u, p, ng, pb, pc).item()
    first = _grads(m)
    assert m.rec_step(u, p, ng).item() == with_plans
    for a, b_, k in zip(_grads(m), first, F.PARAMS):
        assert np.array_equal(a, b_), k


def test_calculate_loss_scales_by_upstream(g):
    m, *_ = build_grcn(g, "A")
    users, pos, neg = _batch(g)
    base = m.rec_step(users, pos, neg).item()
    want = _grads(m)
    inter = torch.stack([torch.as_tensor(g[k]) for k in ("users", "pos", "neg")]).to(DEV)
    out = m.calculate_loss(inter)
    assert out.item() == base
    (3.0 * out).backward()
    for p, w, k in zip(m._params(), want, F.PARAMS):
        np.testing.assert_allclose(p.grad.cpu().numpy(), 3.0 * w, rtol=1e-6, atol=0, err_msg=k)


@pytest.mark.parametrize("case", ["A", "C"])
def test_predict_reads_the_stored_table(g, ref32, case):
    """full_sort_predict scores from the table the last forward wrote: the random init table before any step, the
    step's result after one; evaluation recomputes nothing."""
    m, *_ = build_grcn(g, case)
    U = m.n_users
    m.eval()
    allu = [torch.arange(U, device=DEV)]
    t0 = g[case + "_result0"]
    want0 = t0[:U].astype(np.float64) @ t0[U:].astype(np.float64).T
    F.bar(m.full_sort_predict(allu), want0, t0[:U] @ t0[U:].T, f"{case} scores before any step")
    m.train()
    users, pos, neg = _batch(g)
    m.rec_step(users, pos, neg)
    m.eval()
    r32 = ref32[case]["result"]
    scores = m.full_sort_predict(allu)
    F.bar(scores, g[case + "_scores"], r32[:U] @ r32[U:].T, f"{case} scores after a step")
    with torch.no_grad():
        m.model_specific_conf.mul_(0.5)          # the parameters move, the table stays: nothing is recomputed
    assert torch.equal(m.full_sort_predict(allu), scores)


def test_adam_trajectory(g):
    """Case B, three Adam steps against the reference's own fp32 torch.optim.Adam run, on every parameter.  The
    tolerance is lattice_fixture.adam_reach's rule: twice the distance of the reference's fp32 run from the same three
    steps of the fp64 restatement, three roundings of the parameter, and per element the reach of gradients within the
    gradient bar through Adam's division.  rtol 0."""
    from gmr.trainer import Trainer
    m, cfg, *_ = build_grcn(g, "B")
    opt = Trainer(cfg, m).optimizer
    users, pos, neg = _batch(g)
    t64, g64 = F.trajectory(*_args(g, "B"))
    _, g32 = F.trajectory(*_args(g, "B"), dtype=torch.float32)
    for k in F.PARAMS:  # the stored distance of the reference's own fp32 gradients for the first step
        g32[0][k] = g64[0][k] + float(g["B_own_" + k])
    reach = F.adam_reach(g64, g32, lr=F.LR)
    for j in range(F.ADAM_STEPS):
        m.rec_step(users, pos, neg)
        opt.step()
    j = F.ADAM_STEPS - 1
    for p, k in zip(m._params(), F.PARAMS):
        want = g[f"traj{j + 1}_{k}"]
        err32 = float(np.abs(want.astype(np.float64) - t64[j][k]).max())
        atol = 2 * err32 + F.ADAM_STEPS * np.spacing(np.float32(np.abs(want).max())) + reach[j][k]
        err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want)
        print(f"step {j + 1} {k}: max abs error {err.max():.3e} (fp32 torch {err32:.3e}, reach up to "
              f"{np.max(reach[j][k]):.3e}, median {np.median(reach[j][k]):.3e})")
        assert (err <= atol).all(), (k, float((err - atol).max()))


def _tiny_split(g, cfg, t_feat=True):
    from gmr.dataset import RecDataset
    U, I = int(g["U"]), int(g["I"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(U), 6)
    cols = np.concatenate([rng.choice(I, 6, replace=False) for _ in range(U)])
    labels = np.zeros(rows.size)
    labels[4::6] = 1
    labels[5::6] = 2
    return RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"], g["t_feat"] if t_feat else None).split()


@pytest.mark.parametrize("t_feat", [True, False])
def test_trainer_epoch_twice_the_same_bits(g, tmp_path, t_feat):
    """One epoch through the generic Trainer plus evaluation; a second run from the same seed ends with the same
    parameters and the same metrics, bit for bit."""
    from gmr.dataloader import EvalDataLoader, TrainDataLoader
    from gmr.trainer import Trainer
    from gmr.utils import get_model

    def run(sub):
        cfg = F.grcn_config(learning_rate=0.01, epochs=1, checkpoint_dir=str(tmp_path / sub), eval_step=1)
        tr_ds, va, te = _tiny_split(g, cfg, t_feat)
        tl = TrainDataLoader(cfg, tr_ds, batch_size=16)
        torch.manual_seed(3)
        m = get_model("GRCN")(cfg, tl)
        vl = EvalDataLoader(cfg, va, additional_dataset=tr_ds, batch_size=16)
        trainer = Trainer(cfg, m)
        best, valid, test = trainer.fit(tl, valid_data=vl, test_data=vl, saved=False)
        assert np.isfinite(trainer.train_loss_dict[0])
        assert "recall@10" in valid and 0.0 <= valid["recall@10"] <= 1.0
        return m.slab.data.clone(), m.result.clone(), valid

    a, b = run("a"), run("b")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[1].shape[1] == (192 if t_feat else 128)


def test_unsupported_settings_raise(g):
    with pytest.raises(ValueError, match="text features alone"):
        build_grcn(g, "A", v_feat=None)
    with pytest.raises(ValueError, match="embedding_size"):
        build_grcn(g, "A", embedding_size=32)
    with pytest.raises(ValueError, match="latent_embedding"):
        build_grcn(g, "A", latent_embedding=32)
    with pytest.raises(ValueError, match="routing"):
        build_grcn(g, "A", routing="both")
