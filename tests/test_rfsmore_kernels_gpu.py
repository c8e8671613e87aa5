"""The kernels RFSMORE adds, called by name past the tiny golden shape, against torch fp64 of the same formula.

  gmr_rf_view3_inputs   (U, I) = (1, 1) both priors exactly zero; (127, 129) and (128, 128) around the 128-row block;
                        (300, 2100) 3 + 17 blocks, so every one of the mean kernel's 16 partial chains of the item
                        segment adds more than once.  Every input a column block of a wider table (192 and 448 wide)
                        between sentinels that would wreck the result if read; cond and prior column blocks of wider
                        NaN-filled tables whose other columns must stay NaN.  Column means of about 0.5 next to unit
                        spread (a prior that is not centred, or centred on the other segment's mean, is far outside the
                        bar; the two segments' means differ by 2).
  gmr_rf_sample         C = 192: N = 1, 31, 32, 33, 97 (one row, a short tile, a full tile, a tile and one row, three
                        tiles and one row), L = 1, 2, 4, n_steps = 1, 3; cond a view at column 64 of a 320-wide table
                        with sentinels on both sides, out a strided view.  The fused launch against
                        rf_fixture.generate in fp64 and against the composed sampler.
  RFGenerator           train_step at C = 192 on U = 700, I = 900, B = 300, 40 negatives with injected draws and
                        dropout masks (the mid shape of tests/test_rf_kernels_shapes_gpu.py): the condition encoder's
                        N x 192 forward GEMM and its 128 x 192 dW = dY^T cond.

Bars.  cond: bit for bit (two copies and one fp32 product).  prior: rtol 1e-5, atol 2e-6, the model tests' table bar.
Sampler and velocity gradients: 4 x the error of the same torch formula in fp32 on the CPU against fp64, absolute for
the sampler (floored at 1e-6 of the largest value) and relative to the parameter's largest gradient (floored at 1e-6)
for the gradients, as tests/test_rf_kernels_shapes_gpu.py does for C = 64 / 128; losses rtol 1e-5.

Seen on the MI355X (each test prints its observed error next to its bar): prior 3.0e-7 .. 3.5e-7 from fp64 on priors up
to 2.4; fused sampler at C = 192, worst over the thirty cases 9.4e-7 (N = 97, L = 4, one step; bar 4.4e-6), the
composed sampler 4.7e-7, fused against composed at most 9.8e-7; train step at C = 192, worst gradient error relative
to the parameter's max 8.9e-7 (bar 3.4e-6).
"""
import numpy as np
import pytest
import torch

import rf_fixture as R
import rfsmore_fixture as RS

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D, C = 128, 64, 192
NAN = float("nan")
SENTINEL = 1e30


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


def test_param_floats_192():
    from gmr import _lib
    lib = _lib.load()
    for L in (1, 2, 3, 4):
        n = int(lib.gmr_rf_param_floats(192, L))
        assert n > 0 and n == int(lib.gmr_rf_param_floats(128, L)) + 128 * 64
    assert int(lib.gmr_rf_param_floats(192, 2)) == RS.N_PARAMS
    assert int(lib.gmr_rf_param_floats(256, 2)) == -1 and int(lib.gmr_rf_param_floats(96, 2)) == -1


# ------------------------------------------------------------------------------------------------ the inputs kernel
def _view3_tables(U, I, seed):
    """a, b, f as column blocks (1, 0, 2) of three 192-wide tables and g as block 6 of a 448-wide one, every other
    column a sentinel."""
    rng = np.random.default_rng(seed)
    N = U + I
    shift = np.where(np.arange(N) < U, 1.5, -0.5)[:, None]   # the two segments' means differ by 2
    x = {}
    for k, width, blk in (("a", 192, 1), ("b", 192, 0), ("f", 192, 2), ("g", 448, 6)):
        wide = np.full((N, width), SENTINEL, np.float32)
        if k == "g":   # a gate after dropout: a sigmoid over 0.9, or 0
            v = (1 / (1 + np.exp(-rng.standard_normal((N, D))))) / 0.9 * (rng.random((N, D)) < 0.9)
        else:
            v = rng.standard_normal((N, D)) + 0.5 + (shift if k == "a" else 0.0)
        wide[:, D * blk:D * blk + D] = v.astype(np.float32)
        x[k] = (wide, blk)
    return x


def _run_view3(U, I, x):
    from gmr import _lib
    N = U + I
    d = {k: dev(w) for k, (w, _) in x.items()}
    v = {k: d[k][:, D * blk:D * blk + D] for k, (_, blk) in x.items()}
    cond = torch.full((N, 320), NAN, device=DEV)
    prior = torch.full((N, 192), NAN, device=DEV)
    n = int(_lib.load().gmr_rf_view3_inputs_ws_floats(U, I))
    assert n == (-(-U // 128) + -(-I // 128) + 2) * 64
    ws = torch.full((n,), NAN, device=DEV)
    _call("gmr_rf_view3_inputs", U, I, _ptr(v["a"]), 192, _ptr(v["b"]), 192, _ptr(v["f"]), 192, _ptr(v["g"]), 448,
          _ptr(cond[:, 64:]), 320, _ptr(prior[:, 64:]), 192, _ptr(ws))
    return cond.cpu().numpy(), prior.cpu().numpy()


@pytest.mark.parametrize("U,I", [(1, 1), (127, 129), (128, 128), (300, 2100)])
def test_view3_inputs(U, I):
    x = _view3_tables(U, I, U + I)
    a, b, f, g = (x[k][0][:, D * x[k][1]:D * x[k][1] + D] for k in "abfg")
    cond, prior = _run_view3(U, I, x)
    # nothing outside the two blocks is written
    assert np.isnan(cond[:, :64]).all() and np.isnan(cond[:, 256:]).all()
    assert np.isnan(prior[:, :64]).all() and np.isnan(prior[:, 128:]).all()
    cond, prior = cond[:, 64:256], prior[:, 64:128]
    assert np.array_equal(cond[:, :64], a) and np.array_equal(cond[:, 64:128], b)
    assert np.array_equal(cond[:, 128:], g * f)   # the fp32 product, one rounding
    assert (g == 0).any() and (cond[:, 128:][g == 0] == 0).all()   # dropped gate entries: zeros in the condition
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    _, want = RS.inputs_ref(t64(a), t64(b), t64(f), t64(g), U)
    want = want.numpy()
    err = np.abs(prior - want)
    print(f"view3 inputs U={U} I={I}: prior max abs error {err.max():.3e} (largest |prior| {np.abs(want).max():.3f})")
    np.testing.assert_allclose(prior, want, rtol=1e-5, atol=2e-6)
    if U == 1 and I == 1:
        assert not prior.any()   # a single row is its own mean
    else:
        z = (a.astype(np.float64) + b + g.astype(np.float64) * f) / 3
        assert np.abs(prior - (z - z.mean(0))).max() > 0.1   # one mean over all N rows is another table
    # two runs are bit-identical: fixed-order sums, no float atomics
    c2, p2 = _run_view3(U, I, x)
    assert np.array_equal(c2[:, 64:256], cond) and np.array_equal(p2[:, 64:128], prior)


def test_view3_inputs_rejects_bad_arguments():
    from gmr import _lib
    U, I = 5, 3
    N = U + I
    tab = torch.ones((N, 448), device=DEV)
    cond = torch.full((N, 320), NAN, device=DEV)
    prior = torch.full((N, 192), NAN, device=DEV)
    ws = torch.full((int(_lib.load().gmr_rf_view3_inputs_ws_floats(U, I)),), NAN, device=DEV)
    p, pc, pp, pw = tab.data_ptr(), cond.data_ptr(), prior.data_ptr(), ws.data_ptr()   # byte addresses
    ok = [U, I, p, 448, p + 256, 448, p + 512, 448, p + 768, 448, pc, 320, pp, 192, pw]
    bad = []
    for i, v in ((0, 0), (1, 0),                      # an empty segment
                 (2, None), (4, None), (6, None), (8, None), (10, None), (12, None), (14, None),   # null pointers
                 (2, p + 4), (8, p + 772), (10, pc + 4), (12, pp + 8), (14, pw + 4),   # misaligned
                 (3, 446), (5, 450), (7, 449), (9, 447), (11, 322), (13, 190),    # strides that are no multiple of 4
                 (3, 60), (9, 32), (11, 188), (13, 60)):                           # too narrow
        args = list(ok)
        args[i] = v
        bad.append(args)
    for args in bad:
        with pytest.raises(RuntimeError, match="gmr_rf_view3_inputs"):
            _call("gmr_rf_view3_inputs", *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(cond).all()) and bool(torch.isnan(prior).all()) and bool(torch.isnan(ws).all())
    assert int(_lib.load().gmr_rf_view3_inputs_ws_floats(0, 3)) == -1
    assert int(_lib.load().gmr_rf_view3_inputs_ws_floats(3, 0)) == -1
    _call("gmr_rf_view3_inputs", *ok)
    assert bool(torch.isfinite(cond[:, :192]).all()) and bool(torch.isfinite(prior[:, :64]).all())


# ------------------------------------------------------------------------------------------------ the sampler
def _generator(N, L, seed):
    """An RFGenerator at C = 192 on N = U + I rows with its LayerNorm weights and biases away from 1 / 0."""
    from gmr.rf import RFGenerator
    torch.manual_seed(seed)
    gen = RFGenerator(N // 2, N - N // 2, C, DEV, n_layers=L, dropout=0.1, sampling_steps=3, n_negatives=7)
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for (name, sh), v in zip(gen.specs, gen.param_views()):
            if len(sh) == 1:
                v.add_(dev((0.1 * rng.standard_normal(sh)).astype(np.float32)))
    params = {n: v.detach().cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    assert list(params) == R.param_names(L) and params["condition_encoder.0.weight"].shape == (H, C)
    return gen, params


@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 97])
def test_sample_192(N, L, n_steps):
    gen, params = _generator(N, L, 100 * L + N)
    rng = np.random.default_rng(7 * N + L)
    cond = rng.standard_normal((N, C)).astype(np.float32)
    cond[:, 128:] *= 1.5   # the second K chunk matters
    z0 = rng.standard_normal((N, D)).astype(np.float32)
    wide = np.full((N, 320), SENTINEL, np.float32)
    wide[:, 64:256] = cond
    dw = dev(wide)
    outw = torch.full((N, 160), NAN, device=DEV)
    got = gen.generate(dw[:, 64:256], z0=dev(z0), n_steps=n_steps, out=outw[:, 32:96])
    assert got.data_ptr() == outw[:, 32:96].data_ptr()
    ow = outw.cpu().numpy()
    assert np.isnan(ow[:, :32]).all() and np.isnan(ow[:, 96:]).all()   # nothing outside the block
    out = ow[:, 32:96]
    want = {}
    for dtype in (torch.float32, torch.float64):
        P = {n: torch.tensor(v, dtype=dtype) for n, v in params.items()}
        with torch.no_grad():
            want[dtype] = R.generate(P, torch.tensor(cond, dtype=dtype), torch.tensor(z0, dtype=dtype), n_steps,
                                     L).numpy().astype(np.float64)
    w = want[torch.float64]
    bar = max(4 * np.abs(want[torch.float32] - w).max(), 1e-6 * np.abs(w).max())
    err = np.abs(out - w).max()
    print(f"sampler C=192 N={N} L={L} steps={n_steps}: max abs error {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    # the second chunk is in the product: without the last 64 condition columns the rows are others
    P = {n: torch.tensor(v, dtype=torch.float64) for n, v in params.items()}
    c0 = torch.tensor(cond, dtype=torch.float64)
    c0[:, 128:] = 0
    with torch.no_grad():
        assert float((R.generate(P, c0, torch.tensor(z0, dtype=torch.float64), n_steps, L) -
                      torch.tensor(w)).abs().max()) > 100 * bar
    # fused and composed agree under the same bar (the composed path runs the training kernels and the GEMM)
    comp = gen.generate(dw[:, 64:256], z0=dev(z0), n_steps=n_steps, fused=False).cpu().numpy()
    cerr = np.abs(comp - w).max()
    print(f"composed: max abs error {cerr:.3e}; fused vs composed {np.abs(comp - out).max():.3e}")
    assert cerr <= bar and np.abs(comp - out).max() <= bar


def test_sample_rows_do_not_depend_on_the_tile():
    """One fixed summation order per row: a row gives the same bits whichever tile and tile row it falls in."""
    gen, _ = _generator(97, 2, 3)
    rng = np.random.default_rng(3)
    cond = dev(rng.standard_normal((97, C)).astype(np.float32))
    z0 = dev(rng.standard_normal((97, D)).astype(np.float32))
    full = gen.generate(cond, z0=z0, n_steps=2)
    part = gen.generate(cond[37:90], z0=z0[37:90].contiguous(), n_steps=2)
    assert torch.equal(full[37:90], part)


def test_sample_rejects_other_widths():
    gen, _ = _generator(8, 1, 0)
    z0, out = torch.zeros((8, D), device=DEV), torch.zeros((8, D), device=DEV)
    cond = torch.zeros((8, 256), device=DEV)
    for c, ldc in ((256, 256), (96, 256), (192, 188)):
        with pytest.raises(RuntimeError, match="gmr_rf_sample"):
            _call("gmr_rf_sample", 8, H, c, 1, 1, _ptr(z0), D, _ptr(cond), ldc, _ptr(gen.slab.data), _ptr(out), D)
    from gmr.rf import RFGenerator
    with pytest.raises(NotImplementedError, match="64, 128 or 192"):
        RFGenerator(4, 4, 256, DEV)


# ------------------------------------------------------------------------------------------------ the training step
def test_train_step_192_mid_shape():
    from gmr.rf import RFGenerator
    from test_rf_kernels_gpu import _check_grads
    L, U, I, B, S, p = 2, 700, 900, 300, 40, 0.1
    N = U + I
    torch.manual_seed(5)
    gen = RFGenerator(U, I, C, DEV, n_layers=L, dropout=p, learning_rate=1e-3, sampling_steps=4, warmup_epochs=0,
                      contrast_temp=0.2, contrast_weight=1.0, n_negatives=S)
    rng = np.random.default_rng(C)
    with torch.no_grad():
        for (name, sh), v in zip(gen.specs, gen.param_views()):
            if len(sh) == 1:
                v.add_(dev((0.1 * rng.standard_normal(sh)).astype(np.float32)))
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    x = {"X1": 0.5 * f(N, D), "X0": f(N, D), "t": rng.random((N, 1)).astype(np.float32), "cond": f(N, C),
         "prior": 0.3 * f(N, D), "users": rng.integers(0, U, B), "pos": rng.integers(0, I, B),
         "neg_items": rng.integers(0, I, (B, S)), "neg_users": rng.integers(0, U, (B, S))}
    x["users"][:3], x["pos"][:3] = x["users"][3], x["pos"][3]
    x["neg_items"][0, 0], x["neg_users"][1, 5] = x["pos"][0], x["users"][1]
    masks = {s: rng.random((N, H)) < 1 - p for s in R.drop_sites(L)}
    params = {n: v.detach().cpu().numpy().copy() for (n, _), v in zip(gen.specs, gen.param_views())}
    assert -(-N // 64) == 25 and 2 * B > 256
    loss = gen.train_step(dev(x["X1"]), dev(x["cond"]), dev(x["users"], torch.int32), dev(x["pos"], torch.int32),
                          X0=dev(x["X0"]), t=dev(x["t"]), neg_items=dev(x["neg_items"]),
                          neg_users=dev(x["neg_users"]), masks={s: torch.as_tensor(m) for s, m in masks.items()},
                          apply=False, prior=dev(x["prior"])).cpu().numpy()
    import rfbm3_fixture as RB
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in params.items()}
        t_ = lambda k: torch.tensor(x[k], dtype=dtype)  # noqa: E731
        i_ = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
        r = RB.train_losses(P, t_("X1"), t_("X0"), t_("t"), t_("cond"), t_("prior"), i_(x["users"]), i_(x["pos"]),
                            i_(R.collide(x["neg_items"], x["pos"], I)), i_(R.collide(x["neg_users"], x["users"], U)),
                            U, L, masks={s: torch.as_tensor(m) for s, m in masks.items()}, p=p)
        res[dtype] = (r, {n: v.numpy() for n, v in R.grads_of(P, r["total"]).items()})
    r64, g64 = res[torch.float64]
    _, g32 = res[torch.float32]
    np.testing.assert_allclose(gen._w["V"].cpu().numpy(), r64["v"].detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss[0], r64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(loss[1], r64["cl_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(loss[2], r64["total"].item(), rtol=1e-5)
    bar = max(4 * max(R.rel_to_max(g32[n], g64[n]) for n in g64), 1e-6)
    for (name, _), got in zip(gen.specs, gen.grad_views()):
        err = R.rel_to_max(got.cpu().numpy(), g64[name])
        assert err <= bar, (name, err, bar)
    _check_grads(gen, g64, bar, show="mid shape train step C=192")
    # the 128 x 192 weight gradient, both K chunks' columns
    gw = gen.slab.gview("condition_encoder.0.weight").cpu().numpy()
    assert gw.shape == (H, C) and (np.abs(gw[:, 128:]).max(0) > 0).all()
