"""The rectified-flow kernels (csrc/rf.hip) past the tiny golden shape, called through _lib.call against torch fp64
autograd of the same formula, and gmr.rf.RFGenerator at a mid shape against tests/rf_fixture.py in fp64.

  gmr_rf_act_fwd / _bwd   N = 1 .. 2247 rows: 1 .. 36 blocks of the backward, a partly filled last block, the 16-stride
                          loop of rf_parts_reduce_kernel (13 blocks and more) and its remainder loop
  head / interp / time    N = 1, 5, 1027 with X1 a view of a 192-wide table, zero targets, t = 0 and t just under 1
  gmr_rf_losses           more than 256 row parts and contrastive parts per thread stride
  sampled InfoNCE         0 .. 1024 negatives per anchor (0, 1, 2, 3 and 64 iterations of the slot loop), and the
                          in-kernel Philox draw against tests/philox_ref.py bit for bit
  gmr_rf_rand             the replica, bit for bit, with the n % 4 tail
  RFGenerator             U = 700, I = 900 (25 blocks), B = 300 (2B > 256), 40 negatives, C = 64 / 128

Bars.  Element-wise kernels: a few fp32 roundings, stated at each check.  LayerNorm rows (out, dy, dres): 3e-5 of the
row's largest expected value: every element is at most three terms, each a product with |xhat| <= sqrt(128), built
from 128-term butterfly sums (7 levels) and about six further fp32 operations, 13 x 2^-24 x 3 x 11.3 = 2.6e-5.
d_ln_w, d_ln_b, the velocity gradients and the sampler: 4 x the error of the same torch formula in fp32 on the CPU
against fp64 (both sides are fp32 with different summation orders), relative to the parameter's largest gradient
(absolute for the sampler), floored at 1e-6 x max.  Every such bar is measured on the restatement alone and printed
next to the observed error.

Seen on the MI355X: d_ln_w / d_ln_b errors 6.5e-8 .. 2.4e-7 of the largest gradient over all N and option sets (bars
1.0e-6 .. 1.3e-6, mostly the floor), and equal bit for bit to the stated order of the column reduction; train step,
worst gradient error relative to the parameter's max 7.0e-7 (bar 2.9e-6) at C = 64 and 9.6e-7 (bar 3.3e-6) at
C = 128; sampler, max abs error 6.7e-7 (bar 4.8e-6) at C = 64 and 7.0e-7 (bar 4.6e-6) at C = 128.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import philox_ref
import rf_fixture as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D = 128, 64


def dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _call(name, *args):
    from gmr import _lib
    from gmr.kernels import stream
    return _lib.call(name, *args, stream())


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _row_rel(got, want):
    """Largest error of a row relative to the row's largest expected value."""
    want = np.asarray(want, np.float64)
    scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-30)
    return float((np.abs(np.asarray(got, np.float64) - want) / scale).max())


# ------------------------------------------------------------------------------------------------ act fwd / bwd
def _act_inputs(N, seed):
    rng = np.random.default_rng(seed)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    y = f(N, H)
    if N >= 3:
        y[N // 2] = 0.5  # a constant row: variance 0
    if N >= 2:
        y[N - 1] *= 1e3
    return {"y": y, "g": (1 + 0.1 * f(H)).astype(np.float32), "b": 0.1 * f(H), "res": f(N, H), "add1": f(N, H),
            "add2": f(N, H), "dout": f(N, H), "mask": (rng.random((N, H)) < 0.9).astype(np.uint8)}


def _act_ref(x, ln, res, mask, scale, adds, dtype):
    """out and the gradients of sum(out * dout): dy, dres (the pre-activation's), d_ln_w, d_ln_b."""
    t = lambda a: torch.tensor(a, dtype=dtype)  # noqa: E731
    y = t(x["y"]).requires_grad_(True)
    g, b = t(x["g"]).requires_grad_(True), t(x["b"]).requires_grad_(True)
    r = (t(x["res"]) if res else torch.zeros_like(y)).requires_grad_(True)
    pre = (F.layer_norm(y, (H,), g, b, 1e-5) if ln else y) + r
    a = F.silu(pre)
    if mask:
        a = a * (t(x["mask"]) * torch.tensor(scale, dtype=torch.float32).to(dtype))
    for k in adds:
        a = a + t(x[k])
    gr = torch.autograd.grad((a * t(x["dout"])).sum(), [y, r] + ([g, b] if ln else []))
    return [a.detach().numpy()] + [v.numpy() for v in gr]


def _parts_reduce_fixed_order(P):
    """rf_parts_reduce_kernel's stated order in fp32 (adds only, so IEEE arithmetic reproduces it bit for bit): part q
    of four takes the blocks q, q + 4, ... of P (nblk x 256), sixteen-strided into four interleaved accumulators
    a0..a3, then one at a time into a0; (a0 + a1) + (a2 + a3); the four parts added in order."""
    nblk = P.shape[0]
    red = []
    for q in range(4):
        a = [np.zeros(256, np.float32) for _ in range(4)]
        i = q
        while i + 12 < nblk:
            for u in range(4):
                a[u] = a[u] + P[i + 4 * u]
            i += 16
        while i < nblk:
            a[0] = a[0] + P[i]
            i += 4
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    return ((red[0] + red[1]) + red[2]) + red[3]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 769, 1024, 1091, 2247])
def test_act_fwd_bwd(N):
    from gmr import _lib
    x = _act_inputs(N, N)
    d = {k: dev(v) for k, v in x.items()}
    scale = 1.0 / (1.0 - 0.1)
    nparts = int(_lib.load().gmr_rf_act_parts_floats(N))
    assert nparts == -(-N // 64) * 256
    combo = 0
    for ln in (True, False):
        for res in (True, False):
            for mask in (True, False):
                combo += 1
                adds = [["add1", "add2"], [], ["add1"], ["add2"]][combo % 4]
                want_dres = combo % 2 == 1
                o = lambda k, on: _ptr(d[k]) if on else None  # noqa: E731
                out = torch.full((N, H), float("nan"), device=DEV)
                _call("gmr_rf_act_fwd", N, _ptr(d["y"]), o("g", ln), o("b", ln), o("res", res), o("mask", mask), scale,
                      o("add1", "add1" in adds), o("add2", "add2" in adds), _ptr(out))
                dy = torch.full((N, H), float("nan"), device=DEV)
                dres = torch.full((N, H), float("nan"), device=DEV) if want_dres else None
                parts = torch.full((nparts,), float("nan"), device=DEV) if ln else None
                dg = torch.full((H,), float("nan"), device=DEV) if ln else None
                db = torch.full((H,), float("nan"), device=DEV) if ln else None
                # LN off: parts and d_ln_* are NULL, and that is accepted
                _call("gmr_rf_act_bwd", N, _ptr(d["y"]), o("g", ln), o("b", ln), o("res", res), o("mask", mask), scale,
                      _ptr(d["dout"]), _ptr(dy), _ptr(dres), _ptr(parts), _ptr(dg), _ptr(db))
                w64 = _act_ref(x, ln, res, mask, scale, adds, torch.float64)
                tag = f"N={N} ln={ln} res={res} mask={mask} adds={adds}"
                assert _row_rel(out.cpu().numpy(), w64[0]) <= 3e-5, tag
                assert _row_rel(dy.cpu().numpy(), w64[1]) <= 3e-5, tag
                if want_dres:
                    assert _row_rel(dres.cpu().numpy(), w64[2]) <= 3e-5, tag
                if ln:
                    # the column reduction alone, exactly: the documented fixed order over the block partials
                    order = _parts_reduce_fixed_order(parts.cpu().numpy().reshape(-1, 256))
                    assert np.array_equal(dg.cpu().numpy(), order[:H]), tag
                    assert np.array_equal(db.cpu().numpy(), order[H:]), tag
                    w32 = _act_ref(x, ln, res, mask, scale, adds, torch.float32)
                    for name, got, i in (("d_ln_w", dg, 3), ("d_ln_b", db, 4)):
                        bar = max(4 * R.rel_to_max(w32[i], w64[i]), 1e-6)
                        err = R.rel_to_max(got.cpu().numpy(), w64[i])
                        print(f"act bwd {tag} {name}: error relative to max {err:.3e} (bar {bar:.3e})")
                        assert err <= bar, (tag, name, err, bar)


def test_act_bwd_needs_ln_outputs():
    x = {k: dev(v) for k, v in _act_inputs(5, 0).items()}
    dy = torch.empty((5, H), device=DEV)
    with pytest.raises(RuntimeError, match="gmr_rf_act_bwd"):
        _call("gmr_rf_act_bwd", 5, _ptr(x["y"]), _ptr(x["g"]), _ptr(x["b"]), None, None, 1.0, _ptr(x["dout"]), _ptr(dy),
              None, None, None, None)


# ------------------------------------------------------------------------------------------------ head, interp, time
@pytest.fixture(scope="module", params=[1, 5, 1027])
def head_case(request):
    N = request.param
    rng = np.random.default_rng(40 + N)
    wide = np.zeros((N, 192), np.float32)
    wide[:, 64:128] = rng.standard_normal((N, D))
    wide[:, :64], wide[:, 128:] = 7.0, -7.0  # neighbours the kernels must not read as X1
    t = rng.random(N).astype(np.float32)
    if N >= 5:
        wide[1, 64:128] = 0.0   # X1 == 0
        wide[3, 64:128] = 0.0
        t[2], t[3], t[4] = 0.0, np.float32(1.0 - 2.0 ** -24), np.float32(1.0 - 2.0 ** -24)
    X0 = rng.standard_normal((N, D)).astype(np.float32)
    V = rng.standard_normal((N, D)).astype(np.float32)
    dpred = rng.standard_normal((N, D)).astype(np.float32)
    return N, wide, t, X0, V, dpred


def test_interp_and_time_embed(head_case):
    N, wide, t, X0, _, _ = head_case
    dw, dt, dx0 = dev(wide), dev(t), dev(X0)
    X1 = dw[:, 64:128]
    Xt = torch.full((N, D), float("nan"), device=DEV)
    _call("gmr_rf_interp", N, _ptr(X1), 192, _ptr(dx0), _ptr(dt), _ptr(Xt))
    t64, x1, x0 = t.astype(np.float64)[:, None], wide[:, 64:128].astype(np.float64), X0.astype(np.float64)
    want = t64 * x1 + (1 - t64) * x0
    # two products and a sum (possibly contracted), 1 - t rounded once: 4 roundings of the terms' magnitudes
    bound = 4 * 2.0 ** -24 * (np.abs(t64 * x1) + np.abs((1 - t64) * x0)) + 1e-30
    assert (np.abs(Xt.cpu().numpy() - want) <= bound).all()
    S = torch.full((N, 64), float("nan"), device=DEV)
    _call("gmr_rf_time_embed", N, _ptr(dt), _ptr(S))
    ws = R.sinusoidal(torch.tensor(t64)).numpy()
    # the fp32 frequency exp(-k ln(1e4) / 31) carries <= 1e-6 relative error (exponent up to 9.21 rounded to 2^-24,
    # the exponential's own last places); the argument is below 1 and sin / cos have slope <= 1
    np.testing.assert_allclose(S.cpu().numpy(), ws, rtol=0, atol=2e-6)


def test_head_fwd_bwd(head_case):
    N, wide, t, X0, V, dpred = head_case
    dw, dt, dx0 = dev(wide), dev(t), dev(X0)
    X1 = dw[:, 64:128]
    t64 = torch.tensor(t, dtype=torch.float64)[:, None]
    x1, x0 = torch.tensor(wide[:, 64:128], dtype=torch.float64), torch.tensor(X0, dtype=torch.float64)
    xt32 = (t[:, None] * wide[:, 64:128] + (1 - t[:, None]) * X0).astype(np.float32)  # the kernel's fp32 input
    xt = torch.tensor(xt32, dtype=torch.float64)
    v_in = torch.tensor(V, dtype=torch.float64, requires_grad=True)
    v = v_in + (1 - t64) ** 2 * 0.1 * R.cos_grad(xt, x1)      # the formulas of R.train_losses
    pred = xt + (1 - t64) * v
    rows = ((v - (x1 - x0)) ** 2).sum(1)
    if N >= 5:
        assert not R.cos_grad(xt, x1)[1].any() and bool(torch.isfinite(v).all())  # zero target: no guidance
    dV_ = dev(V.copy())
    predk = torch.full((N, D), float("nan"), device=DEV)
    parts = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    _call("gmr_rf_head_fwd", N, _ptr(dV_), _ptr(dev(xt32)), _ptr(X1), 192, _ptr(dx0), _ptr(dt), 0.1, _ptr(predk),
          _ptr(parts))
    np.testing.assert_allclose(dV_.cpu().numpy(), v.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(predk.cpu().numpy(), pred.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(parts.cpu().numpy(), rows.detach().numpy(), rtol=1e-5)
    # backward of mse(v, X1 - X0) + sum(pred * dpred) to the guided velocity, from the kernel's own fp32 v
    vk = dV_.cpu().double().requires_grad_(True)
    obj = F.mse_loss(vk, x1 - x0) + ((xt + (1 - t64) * vk) * torch.tensor(dpred, dtype=torch.float64)).sum()
    want = torch.autograd.grad(obj, vk)[0].numpy()
    got = torch.full((N, D), float("nan"), device=DEV)
    _call("gmr_rf_head_bwd", N, _ptr(dV_), _ptr(X1), 192, _ptr(dx0), _ptr(dt), _ptr(dev(dpred)), _ptr(got))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-6 * np.abs(want).max())


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("N,B", [(1, 0), (300, 1), (1027, 513)])
def test_losses(N, B):
    rng = np.random.default_rng(N + B)
    rowparts, clparts = rng.random(N) * 50, rng.random(2 * B) * 5
    weight = 0.7
    out = torch.full((3,), float("nan"), device=DEV)
    dr = dev(rowparts)
    dc = dev(clparts) if B else None
    _call("gmr_rf_losses", N, _ptr(dr), B, _ptr(dc), weight, _ptr(out))
    rf = rowparts.sum() / (N * D)
    cl = clparts.sum() / B if B else 0.0
    got = out.cpu().numpy()
    np.testing.assert_allclose(got, [rf, cl, rf + float(np.float32(weight)) * cl], rtol=1e-6)
    if B == 0:
        assert got[1] == 0.0


# ------------------------------------------------------------------------------------------------ sampled InfoNCE
N_ANCH, N_SIDE, ROW_OFF, TEMP = 9, 41, 37, 0.2
IDX = np.array([3, N_SIDE - 1, 0, 3, 17, N_SIDE - 1, 5, 5, 22])  # duplicate anchors


@pytest.fixture(scope="module")
def nce_tables():
    rng = np.random.default_rng(12)
    n_rows = ROW_OFF + N_SIDE
    return (rng.standard_normal((n_rows, D)).astype(np.float32), rng.standard_normal((n_rows, D)).astype(np.float32))


def _infonce(pred, target, n_neg, neg=None, seed=0, step=0, site=0):
    parts = torch.full((N_ANCH,), float("nan"), dtype=torch.float64, device=DEV)
    contrib = torch.full((N_ANCH, D), float("nan"), device=DEV)
    dp, dt, di = dev(pred), dev(target), dev(IDX, torch.int32)
    dn = dev(np.ascontiguousarray(neg), torch.int32) if neg is not None else None
    _call("gmr_rf_infonce_sampled_fwd_bwd", N_ANCH, N_SIDE, _ptr(dp), D, _ptr(dt), D, ROW_OFF, _ptr(di), n_neg,
          _ptr(dn), seed, step, site, 1.0 / TEMP, 1.0 / N_ANCH, _ptr(parts), _ptr(contrib), D)
    return parts.cpu().numpy(), contrib.cpu().numpy()


@pytest.mark.parametrize("n_neg", [0, 1, 15, 16, 17, 40, 1024])
def test_infonce_injected(nce_tables, n_neg):
    """Per-row losses and gradient rows against R.infonce in fp64.  With one negative far from the anchor the loss is
    about 6e-4: -logf(pos / ttl) gave it to 8.4e-5 relative (the quotient rounds next to 1), log1pf(sum / pos) keeps
    it within the bar."""
    pred, target = nce_tables
    rng = np.random.default_rng(n_neg)
    raw = rng.integers(0, N_SIDE, (N_ANCH, max(n_neg, 1)))
    if n_neg:
        raw[0, 0], raw[1, -1], raw[2, 0] = IDX[0], N_SIDE - 1, 0  # the positive itself; n - 1 wraps to 0
        raw[4, n_neg // 2] = raw[4, 0]
    parts, contrib = _infonce(pred, target, n_neg, raw)
    if n_neg == 0:
        assert not parts.any() and not contrib.any()
        return
    fixed = R.collide(raw, IDX, N_SIDE)
    assert fixed[1, -1] == 0 and fixed[0, 0] == IDX[0] + 1 and not (fixed == IDX[:, None]).any()
    p = torch.tensor(pred[ROW_OFF:], dtype=torch.float64, requires_grad=True)
    t = torch.tensor(target[ROW_OFF:], dtype=torch.float64)
    for b in range(N_ANCH):
        row = R.infonce(p, t, torch.as_tensor(IDX[b:b + 1]), torch.as_tensor(fixed[b:b + 1]), TEMP)
        np.testing.assert_allclose(parts[b], row.item(), rtol=1e-5, err_msg=str(b))
        want = torch.autograd.grad(row / N_ANCH, p)[0][IDX[b]].numpy()
        np.testing.assert_allclose(contrib[b], want, rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=str(b))


@pytest.mark.parametrize("site", [2, 3])
@pytest.mark.parametrize("n_neg", [7, 40])
def test_infonce_philox_draw_is_the_replica(nce_tables, n_neg, site):
    """Slot s of anchor b takes draw k = b n_neg + s: word k & 3 of Philox(seed + site mix, step, k >> 2), mapped to
    (x * n) >> 32.  The run that draws in the kernel equals the run given those raw draws, bit for bit."""
    pred, target = nce_tables
    seed, step = 999, 5
    k = np.arange(N_ANCH * n_neg, dtype=np.uint64)
    words = philox_ref.philox(philox_ref.site_seed(seed, site), step, k >> np.uint64(2))
    x = words[np.arange(k.size), (k & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    raw = ((x * np.uint64(N_SIDE)) >> np.uint64(32)).astype(np.int64).reshape(N_ANCH, n_neg)
    assert raw.min() >= 0 and raw.max() < N_SIDE and len(np.unique(raw)) > N_SIDE // 2
    a = _infonce(pred, target, n_neg, None, seed, step, site)
    b = _infonce(pred, target, n_neg, raw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.isfinite(a[0]).all() and (a[0] > 0).all()


# ------------------------------------------------------------------------------------------------ uniform draws
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_rand_is_the_replica(n):
    """out[4 i + q] = (x_q >> 8) / 2^24 with x = Philox(seed + site mix, step, i), exactly; the tail n % 4 too."""
    for seed, step, site in ((0, 0, 0), (11, 4, 1), (2 ** 64 - 3, 2 ** 33 + 7, 16)):
        out = torch.full((n + 3,), -1.0, device=DEV)
        _call("gmr_rf_rand", n, seed, step, site, _ptr(out))
        words = philox_ref.philox(philox_ref.site_seed(seed, site), step, np.arange((n + 3) // 4))
        want = ((words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(-1)[:n]
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want), (n, seed, step, site)
        assert (got[n:] == -1.0).all()  # nothing past n


@pytest.mark.parametrize("n", [1, 5, 1027])
def test_randn_follows_the_replica(n):
    """out[4 i ..] = Box-Muller of the word pairs (x, y) and (z, w): r (cos, sin)(2 pi u2), r = sqrt(-2 ln u1).  The
    fp32 angle carries up to 2 x 2 pi 2^-24 = 7.5e-7 (the constant and the product, one rounding each), the device
    logarithm and sine a few ulp more: 2e-6 of r, and r <= sqrt(48 ln 2) = 5.8."""
    seed, step, site = 11, 4, 1
    out = torch.full((n + 3,), -9.0, device=DEV)
    _call("gmr_rf_randn", n, seed, step, site, _ptr(out))
    words = philox_ref.philox(philox_ref.site_seed(seed, site), step, np.arange((n + 3) // 4))
    u = philox_ref.u32_to_unit(words).astype(np.float64)
    want = np.empty((words.shape[0], 4))
    for h in (0, 1):
        r, a = np.sqrt(-2.0 * np.log(u[:, 2 * h])), 2.0 * np.pi * u[:, 2 * h + 1]
        want[:, 2 * h], want[:, 2 * h + 1] = r * np.cos(a), r * np.sin(a)
    got = out.cpu().numpy()
    np.testing.assert_allclose(got[:n], want.reshape(-1)[:n], rtol=0, atol=2e-6 * 5.8)
    assert (got[n:] == -9.0).all()


# ------------------------------------------------------------------------------------------------ the generator
@pytest.fixture(scope="module", params=[64, 128])
def mid_generator(request):
    from gmr.rf import RFGenerator
    C, L, U, I, B, S, p = request.param, 2, 700, 900, 300, 40, 0.1
    N = U + I
    torch.manual_seed(5)
    gen = RFGenerator(U, I, C, DEV, n_layers=L, dropout=p, learning_rate=1e-3, sampling_steps=4, warmup_epochs=0,
                      contrast_temp=0.2, contrast_weight=1.0, n_negatives=S)
    rng = np.random.default_rng(C)
    with torch.no_grad():  # LayerNorm weights and biases away from their 1 / 0 initial values
        for (name, sh), v in zip(gen.specs, gen.param_views()):
            if len(sh) == 1:
                v.add_(dev((0.1 * rng.standard_normal(sh)).astype(np.float32)))
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    x = {"X1": 0.5 * f(N, D), "X0": f(N, D), "t": rng.random((N, 1)).astype(np.float32), "cond": f(N, C),
         "users": rng.integers(0, U, B), "pos": rng.integers(0, I, B), "neg_items": rng.integers(0, I, (B, S)),
         "neg_users": rng.integers(0, U, (B, S))}
    x["cond"][:U] = 0.0  # user rows carry no condition
    x["users"][:3], x["pos"][:3] = x["users"][3], x["pos"][3]
    x["neg_items"][0, 0], x["neg_users"][1, 5] = x["pos"][0], x["users"][1]
    masks = {s: rng.random((N, H)) < 1 - p for s in R.drop_sites(L)}
    params = {n: v.detach().cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    assert list(params) == R.param_names(L)
    return gen, x, masks, params, (C, L, U, I, B, S, p)


def _train_ref(x, masks, params, dims, dtype):
    C, L, U, I, B, S, p = dims
    P = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in params.items()}
    f = lambda k: torch.tensor(x[k], dtype=dtype)  # noqa: E731
    i = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    r = R.train_losses(P, f("X1"), f("X0"), f("t"), f("cond"), i(x["users"]), i(x["pos"]),
                       i(R.collide(x["neg_items"], x["pos"], I)), i(R.collide(x["neg_users"], x["users"], U)), U, L,
                       masks={s: torch.as_tensor(m) for s, m in masks.items()}, p=p)
    return r, {n: v.numpy() for n, v in R.grads_of(P, r["total"]).items()}


def test_train_step_mid_shape(mid_generator):
    from test_rf_kernels_gpu import _check_grads
    gen, x, masks, params, dims = mid_generator
    C, L, U, I, B, S, p = dims
    assert -(-(U + I) // 64) == 25 and 2 * B > 256
    loss = gen.train_step(dev(x["X1"]), dev(x["cond"]), dev(x["users"], torch.int32), dev(x["pos"], torch.int32),
                          X0=dev(x["X0"]), t=dev(x["t"]), neg_items=dev(x["neg_items"]),
                          neg_users=dev(x["neg_users"]), masks={s: torch.as_tensor(m) for s, m in masks.items()},
                          apply=False).cpu().numpy()
    r64, g64 = _train_ref(x, masks, params, dims, torch.float64)
    r32, g32 = _train_ref(x, masks, params, dims, torch.float32)
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), r64["v"].detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss[0], r64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(loss[1], r64["cl_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(loss[2], r64["total"].item(), rtol=1e-5)
    bar = max(4 * max(R.rel_to_max(g32[n], g64[n]) for n in g64), 1e-6)
    _check_grads(gen, g64, bar, show=f"mid shape train step C={C}")


def test_generate_mid_shape(mid_generator):
    gen, x, _, params, dims = mid_generator
    C, L, U, I, B, S, p = dims
    steps = 4
    out = gen.generate(dev(x["cond"]), z0=dev(x["X0"]), n_steps=steps).cpu().numpy()
    want = {}
    for dtype in (torch.float32, torch.float64):
        P = {n: torch.tensor(v, dtype=dtype) for n, v in params.items()}
        with torch.no_grad():
            want[dtype] = R.generate(P, torch.tensor(x["cond"], dtype=dtype), torch.tensor(x["X0"], dtype=dtype), steps,
                                     L).numpy().astype(np.float64)
    w = want[torch.float64]
    bar = max(4 * np.abs(want[torch.float32] - w).max(), 1e-6 * np.abs(w).max())
    err = np.abs(out - w).max()
    print(f"mid shape sampler C={C}: max abs error {err:.3e} (bar {bar:.3e})")
    assert err <= bar
