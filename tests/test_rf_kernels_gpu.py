"""The rectified-flow kernels (csrc/rf.hip) and gmr.rf.RFGenerator against the reference's golden values
(tests/golden/make_golden_rffreedom.py) and the pinned restatement (tests/rf_fixture.py, tests/test_rf_cpu.py).

Bars: losses rtol 1e-5, values 1e-5 (the project's FREEDOM bars).  The sampler output and the velocity gradients
pass through several LayerNorms; their bars are 4x the reference's own fp32-vs-fp64 error on the same record
(err_sample: absolute; err_grad: relative to the parameter's largest gradient), both sides being fp32 with
different summation orders."""
import numpy as np
import pytest
import torch

import rf_fixture as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORDS = [("A_", 2), ("B_", 1)]
U, I, N = 37, 41, 78


@pytest.fixture(scope="module")
def g(golden):
    return R.load_golden(golden)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _batch(g, tag):
    return _dev(g[tag + "users"], torch.int32), _dev(g[tag + "pos"], torch.int32)


def _check_grads(gen, want, bar, show=None):
    worst = 0.0
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        w = want[name]
        worst = max(worst, R.rel_to_max(got.cpu().numpy(), w))
    if show:
        print(f"{show}: worst gradient error relative to the parameter's max {worst:.3e} (bar {bar:.3e})")
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        w = want[name]
        np.testing.assert_allclose(got.cpu().numpy(), w, rtol=1e-4, atol=bar * np.abs(w).max(), err_msg=name)


# ------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("tag,L", RECORDS)
def test_sample_golden(g, tag, L):
    gen = R.build_generator(g, tag, L, prefix="p1_")
    out = gen.generate(_dev(g[tag + "cond"]), z0=_dev(g[tag + "z0"]), n_steps=int(g["steps"]))
    bar = 4 * float(g[tag + "err_sample"])
    err = np.abs(out.cpu().numpy().astype(np.float64) - g[tag + "gen"]).max()
    print(f"sampler {tag}: max abs error {err:.3e} (bar {bar:.3e})")
    np.testing.assert_allclose(out.cpu().numpy(), g[tag + "gen"], rtol=0, atol=bar)


@pytest.fixture(scope="module")
def sample_case(g):
    """One run over 2 tiles + 5 rows with record A's stepped parameters, and the restatement on the same rows."""
    from gmr import _lib
    tr = int(_lib.load().gmr_rf_tile_rows())
    n = 2 * tr + 5
    rng = np.random.default_rng(5)
    cond = rng.standard_normal((n, 128)).astype(np.float32)
    cond[::3] = 0.0  # user-like rows
    z0 = rng.standard_normal((n, 64)).astype(np.float32)
    gen = R.build_generator(g, "A_", 2, prefix="p1_")
    P = R.params_from(g, "A_", 2, prefix="p1_")
    return tr, n, cond, z0, gen, P


@pytest.mark.parametrize("rows,steps", [(1, 3), ("tile+1", 3), ("tile+1", 1), ("all", 2)])
def test_sample_restatement(g, sample_case, rows, steps):
    tr, n, cond, z0, gen, P = sample_case
    k = {"tile+1": tr + 1, "all": n}.get(rows, rows)
    out = gen.generate(_dev(cond[:k]), z0=_dev(z0[:k]), n_steps=steps)
    assert out.shape == (k, 64)
    want = R.generate(P, torch.tensor(cond[:k]), torch.tensor(z0[:k]), steps, 2).numpy()
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=4 * float(g["A_err_sample"]))


def test_sample_rows_do_not_depend_on_the_tiling(sample_case):
    tr, n, cond, z0, gen, _ = sample_case
    full = gen.generate(_dev(cond), z0=_dev(z0), n_steps=3).cpu().numpy()
    for k in (1, tr - 1, tr + 1):
        part = gen.generate(_dev(cond[:k]), z0=_dev(z0[:k]), n_steps=3).cpu().numpy()
        assert np.array_equal(part, full[:k]), k
    # strided operands and output (the backbone's work-table views)
    cw, ow = torch.zeros((n, 192), device=DEV), torch.full((n, 80), 7.0, device=DEV)
    cw[:, 64:192] = _dev(cond)
    gen.generate(cw[:, 64:192], z0=_dev(z0), n_steps=3, out=ow[:, 8:72])
    assert np.array_equal(ow[:, 8:72].cpu().numpy(), full) and bool((ow[:, :8] == 7).all() and (ow[:, 72:] == 7).all())


def test_sample_rejects_unsupported_shapes(sample_case):
    from gmr import _lib
    from gmr.kernels import ptr, stream
    _, n, cond, z0, gen, _ = sample_case
    c, z, o = _dev(cond), _dev(z0), torch.empty((n, 64), device=DEV)
    for hidden, C, L in ((256, 128, 2), (128, 96, 2), (128, 128, 0), (128, 128, 5)):
        with pytest.raises(RuntimeError, match="-1000"):
            _lib.call("gmr_rf_sample", n, hidden, C, L, 3, ptr(z), 64, ptr(c), 128, ptr(gen.slab.data), ptr(o), 64,
                      stream())


def test_composed_sampler_agrees(g):
    gen = R.build_generator(g, "A_", 2, prefix="p1_")
    cond, z0 = _dev(g["A_cond"]), _dev(g["A_z0"])
    a = gen.generate(cond, z0=z0, n_steps=3, fused=True).cpu().numpy()
    b = gen.generate(cond, z0=z0, n_steps=3, fused=False).cpu().numpy()
    np.testing.assert_allclose(b, g["A_gen"], rtol=0, atol=4 * float(g["A_err_sample"]))
    np.testing.assert_allclose(a, b, rtol=0, atol=4 * float(g["A_err_sample"]))


# ------------------------------------------------------------------------------------------------ training step
def _p1_bound(g, tag, name, bar, lr):
    """Bound on a stepped parameter given gradients within `bar`: the first AdamW step moves p by
    lr g / (|g| + eps), whose slope in g is at most 1 / (|g| + eps) and whose range is 2 lr; so an element's
    error is at most lr min(2, dg / (|g| + eps)) with dg the gradient bound, next to the 1e-5 value bar."""
    gw = g[tag + "g_" + R.key(name)].astype(np.float64)
    dg = 1e-4 * np.abs(gw) + bar * np.abs(gw).max()
    return 1e-5 * np.abs(g[tag + "p1_" + R.key(name)]) + lr * np.minimum(2.0, dg / (np.abs(gw) + 1e-8))


@pytest.mark.parametrize("tag,L", RECORDS)
def test_train_step_golden(g, tag, L):
    gen = R.build_generator(g, tag, L)
    users, pos = _batch(g, tag)
    X1, cond = _dev(g[tag + "X1"]), _dev(g[tag + "cond"])
    loss = gen.train_step(X1, cond, users, pos, **R.draws(g, tag)).cpu().numpy()
    w = gen._w
    np.testing.assert_allclose(w["V"].cpu().numpy(), g[tag + "v"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss[0], g[tag + "rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(loss[1], g[tag + "cl_loss"], rtol=1e-5)
    np.testing.assert_allclose(loss[2], g[tag + "rf_loss"] + g[tag + "cl_loss"], rtol=1e-5)
    bar = R.grad_bar(g, tag)
    _check_grads(gen, {n: g[tag + "g_" + R.key(n)] for n in R.param_names(L)}, bar, show="train step " + tag)
    assert gen.step_ctr == 1
    for (name, _), p in zip(gen.specs, gen.param_views()):
        got, want = p.cpu().numpy(), g[tag + "p1_" + R.key(name)]
        assert (np.abs(got - want) <= _p1_bound(g, tag, name, bar, float(g["lr"]))).all(), name
    # a second generator, the same step: bit-identical
    gen2 = R.build_generator(g, tag, L)
    loss2 = gen2.train_step(X1, cond, users, pos, **R.draws(g, tag)).cpu().numpy()
    assert np.array_equal(loss, loss2) and torch.equal(gen.slab.grad, gen2.slab.grad)
    assert torch.equal(gen.slab.data, gen2.slab.data) and torch.equal(gen.exp_avg_sq, gen2.exp_avg_sq)


def test_train_step_strided_target(g):
    """X1 and the conditions as views of a wider table (FREEDOM's work table) give the same step."""
    tag = "B_"
    users, pos = _batch(g, tag)
    a, b = R.build_generator(g, tag, 1), R.build_generator(g, tag, 1)
    wide = torch.zeros((N, 192), device=DEV)
    wide[:, :64], wide[:, 64:128] = _dev(g[tag + "X1"]), _dev(g[tag + "cond"])
    la = a.train_step(_dev(g[tag + "X1"]), _dev(g[tag + "cond"]), users, pos, **R.draws(g, tag))
    lb = b.train_step(wide[:, :64], wide[:, 64:128], users, pos, **R.draws(g, tag))
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, b.slab.grad)


def test_train_step_dropout_masks(g):
    """Dropout 0.1 with injected keep masks against the restatement's autograd."""
    tag, L, p = "A_", 2, 0.1
    rng = np.random.default_rng(9)
    masks = {s: rng.random((N, 128)) < 1 - p for s in R.drop_sites(L)}
    gen = R.build_generator(g, tag, L, dropout=p)
    users, pos = _batch(g, tag)
    loss = gen.train_step(_dev(g[tag + "X1"]), _dev(g[tag + "cond"]), users, pos, apply=False,
                          masks={s: torch.as_tensor(m) for s, m in masks.items()}, **R.draws(g, tag)).cpu().numpy()
    P = {n: torch.tensor(g[tag + "p0_" + R.key(n)], requires_grad=True) for n in R.param_names(L)}
    r = R.train_losses(P, *R.record_inputs(g, tag), 37, L, masks={s: torch.as_tensor(m) for s, m in masks.items()},
                       p=p)
    assert abs(r["rf_loss"].item() - float(g[tag + "rf_loss"])) > 1e-3  # the masks matter
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), r["v"].detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss[0], r["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(loss[1], r["cl_loss"].item(), rtol=1e-5)
    want = {n: v.numpy() for n, v in R.grads_of(P, r["total"]).items()}
    _check_grads(gen, want, R.grad_bar(g, tag), show="dropout masks")


def test_repeated_anchors_accumulate(g):
    """d(weight * cl_loss) / d pred through the sorted scatter: the batch repeats a user and an item."""
    tag, L = "A_", 2
    gen = R.build_generator(g, tag, L)
    users, pos = _batch(g, tag)
    gen.train_step(_dev(g[tag + "X1"]), _dev(g[tag + "cond"]), users, pos, apply=False, **R.draws(g, tag))
    X1, _, _, _, u, p_, ni, nu = R.record_inputs(g, tag)
    pred = gen._w["pred"].cpu().clone().requires_grad_(True)
    cl = R.infonce(pred[U:], X1[U:], p_, ni, 0.2) + R.infonce(pred[:U], X1[:U], u, nu, 0.2)
    want = torch.autograd.grad(cl, pred)[0].numpy()
    got = gen._w["dpred"].cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * np.abs(want).max())
    rep = [int(x) for x in set(g[tag + "users"].tolist()) if (g[tag + "users"] == x).sum() > 1]
    assert rep and np.abs(got[rep]).max() > 0
    untouched = np.setdiff1d(np.arange(N), np.concatenate([g[tag + "users"], g[tag + "pos"] + U]))
    assert not got[untouched].any()


# ------------------------------------------------------------------------------------------------ sampled InfoNCE
def _infonce_alone(gen, pred, target, idx, neg, n, row_off=0):
    B = len(idx)
    parts = torch.zeros(B, dtype=torch.float64, device=DEV)
    contrib = torch.zeros((B, 64), device=DEV)
    gen.infonce(_dev(pred), _dev(target), row_off, n, _dev(idx, torch.int32), parts, contrib,
                neg=_dev(neg, torch.int32), coef=1.0 / B)
    return parts.cpu().numpy(), contrib.cpu().numpy()


def test_infonce_collision_rule_in_kernel(g):
    """Raw draws: one equal to the positive, one equal to n - 1 with the positive n - 1 (wraps to 0)."""
    gen = R.build_generator(g, "A_", 2)
    rng = np.random.default_rng(2)
    n, B, S = 41, 6, 7
    pred = rng.standard_normal((n, 64)).astype(np.float32)
    target = rng.standard_normal((n, 64)).astype(np.float32)
    idx = np.array([3, n - 1, 0, 3, 17, n - 1])
    raw = rng.integers(0, n, (B, S))
    raw[0, 2], raw[1, 4], raw[1, 5], raw[2, 0], raw[4, 1] = 3, n - 1, n - 1, 0, raw[4, 0]
    parts, contrib = _infonce_alone(gen, pred, target, idx, raw, n)
    fixed = R.collide(raw, idx, n)
    assert fixed[1, 4] == 0 and fixed[0, 2] == 4 and not (fixed == idx[:, None]).any()
    p = torch.tensor(pred, requires_grad=True)
    a = torch.nn.functional.normalize(p[idx], dim=1)
    t = torch.tensor(target)
    pos = torch.exp((a * torch.nn.functional.normalize(t[idx], dim=1)).sum(-1) / 0.2)
    tn = torch.nn.functional.normalize(t[torch.as_tensor(fixed)], dim=1)
    rows = -torch.log(pos / (pos + torch.exp(torch.bmm(a.unsqueeze(1), tn.transpose(1, 2)).squeeze(1) / 0.2).sum(1)))
    np.testing.assert_allclose(parts, rows.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(parts.mean(), R.infonce(p, t, torch.as_tensor(idx), torch.as_tensor(fixed), 0.2).item(),
                               rtol=1e-5)
    # per-anchor gradient rows: anchors 0 and 3 share a positive and hold different negatives
    for b in range(B):
        want = torch.autograd.grad(rows[b] / B, p, retain_graph=True)[0][idx[b]].numpy()
        np.testing.assert_allclose(contrib[b], want, rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=str(b))
    # the already-fixed indices give the same result bit for bit (the rule is idempotent)
    parts2, contrib2 = _infonce_alone(gen, pred, target, idx, fixed, n)
    assert np.array_equal(parts, parts2) and np.array_equal(contrib, contrib2)


# ------------------------------------------------------------------------------------------------ AdamW
def _adamw(p, grads, lr, wd, kernel="gmr_adamw_f32"):
    from gmr import _lib
    from gmr.kernels import ptr, stream
    p = _dev(p.copy())
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k, gr in enumerate(grads, 1):
        bc1, bc2 = 1 - 0.9 ** k, 1 - 0.999 ** k
        third = 1.0 - lr * wd if kernel == "gmr_adamw_f32" else wd
        _lib.call(kernel, p.numel(), ptr(p), ptr(_dev(gr)), ptr(m), ptr(v), 0.9, 0.999, 1e-8, third, lr / bc1,
                  bc2 ** 0.5, stream())
    return p.cpu().numpy()


@pytest.mark.parametrize("steps", [1, 3])
def test_adamw_matches_torch(steps):
    rng = np.random.default_rng(steps)
    n, lr = 1000 + 3, 1e-3  # not a multiple of 4
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) * 0.1 for _ in range(steps)]
    for wd in (0.01, 0.1):
        p = torch.nn.Parameter(torch.tensor(p0))
        opt = torch.optim.AdamW([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        for gr in grads:
            p.grad = torch.tensor(gr)
            opt.step()
        want = p.detach().numpy()
        np.testing.assert_allclose(_adamw(p0, grads, lr, wd), want, rtol=1e-6, atol=1e-7)
        if wd == 0.1:  # the L2 form (gmr_adam_f32 folds the decay into the gradient) is another update
            l2 = _adamw(p0, grads, lr, wd, kernel="gmr_adam_f32")
            assert np.abs(l2 - want).max() > 100 * (1e-6 * np.abs(want).max() + 1e-7)


# ------------------------------------------------------------------------------------------------ Philox paths
def test_philox_draws(g):
    tag, L = "A_", 2
    users, pos = _batch(g, tag)
    X1, cond = _dev(g[tag + "X1"]), _dev(g[tag + "cond"])

    def run(step):
        gen = R.build_generator(g, tag, L, dropout=0.1, seed=11)
        gen.step_ctr = step
        loss = gen.train_step(X1, cond, users, pos, apply=False).clone()
        return gen, loss

    a, la = run(4)
    b, lb = run(4)
    c, lc = run(5)
    assert torch.equal(la, lb) and torch.equal(a.slab.grad, b.slab.grad) and torch.equal(a._w["X0"], b._w["X0"])
    assert not torch.equal(la, lc) and not torch.equal(a._w["X0"], c._w["X0"]) and not torch.equal(a._w["t"], c._w["t"])
    assert bool(torch.isfinite(la).all() and torch.isfinite(a.slab.grad).all())
    x0, t = a._w["X0"].cpu().numpy(), a._w["t"].cpu().numpy()
    assert 0.0 <= t.min() and t.max() < 1.0 and abs(t.mean() - 0.5) < 4 * (1 / 12 / N) ** 0.5
    assert abs(x0.mean()) < 4 / (N * 64) ** 0.5 and abs(x0.std() - 1) < 4 / (2 * N * 64) ** 0.5
    m1, m2 = a._w["M"]["input"].cpu().numpy(), a._w["M"]["out"].cpu().numpy()
    assert set(np.unique(m1)) <= {0, 1} and not np.array_equal(m1, m2)  # sites draw their own masks
    n = m1.size
    assert abs(m1.mean() - 0.9) < 4 * (0.9 * 0.1 / n) ** 0.5
    # eval noise: keyed on the step counter too
    z1 = a.generate(cond).clone()
    assert torch.equal(z1, b.generate(cond)) and bool(torch.isfinite(z1).all())
    assert not torch.equal(z1, c.generate(cond))


def test_philox_negatives(g):
    """Negatives drawn in the kernel (1,024 per anchor): the same at the same (seed, step), others at the next
    step, finite losses and gradient rows, every loss positive."""
    gen = R.build_generator(g, "A_", 2, seed=3)
    rng = np.random.default_rng(1)
    pred, target = rng.standard_normal((N, 64)).astype(np.float32), rng.standard_normal((N, 64)).astype(np.float32)
    idx = _dev(np.arange(16) % I, torch.int32)

    def run(step, n_neg):
        gen.step_ctr, gen.n_neg = step, n_neg
        parts = torch.zeros(16, dtype=torch.float64, device=DEV)
        contrib = torch.zeros((16, 64), device=DEV)
        gen.infonce(_dev(pred), _dev(target), U, I, idx, parts, contrib, site=2)
        return parts.cpu().numpy(), contrib.cpu().numpy()

    a, b, c = run(0, 1024), run(0, 1024), run(1, 1024)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and (a[0] > 0).all()
