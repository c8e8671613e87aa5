"""The two entry points RFBM3 adds, by name, against the fp64 restatement of tests/rfbm3_fixture.py.

  gmr_rf_head_prior_fwd   N = 1, 3, 4, 5, 130 (one wave per row, four rows per block: a single row, a partly filled
                          block, one full block, one row into the second, 33 blocks), X1 and the prior as views of
                          wider tables, rows with t = 0, t = 0.5 and t = 1 - 2^-24, one all-zero X_t row (the cosine
                          gradient's clamps); with an all-zero prior it is gmr_rf_head_fwd bit for bit
  gmr_rf_item_inputs      I = 1, 5, 41, 1100 (one row, less than a row group, less than a block, 9 blocks with a short
                          last one), U = 0 and 3, both modalities / image only / text only, all tables views of wider
                          ones; user rows and the columns past the tables keep a sentinel; two runs bit for bit

Bars: rtol 1e-5 against fp64, and next to it an entry may be off by twice the largest error in its row (its column
for the prior's mean) of the same formula done by fp32 torch on the CPU against fp64, measured here and printed (the
rule of test_bm3_kernels_gpu.py, taken per row because the zero X_t row's values are 1e6 times the others').

Seen on the MI355X: head at N = 130, median row error of V 1.2e-7 (fp32 torch 1.3e-7), of the row partials 2.0e-6
(6.3e-6), the zero X_t row 0.17 on values of 1e6; prior at I = 1,100 with both modalities 5.7e-7 (fp32 torch 5.7e-7)."""
import numpy as np
import pytest
import torch

import rfbm3_fixture as RB

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64


def dev(a):
    return torch.as_tensor(a).to(DEV)


def _call(name, *args):
    from gmr import _lib
    from gmr.kernels import stream
    return _lib.call(name, *args, stream())


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


# ------------------------------------------------------------------------------------------------ head with prior
def _head_case(N):
    rng = np.random.default_rng(100 + N)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    X1w, Pw, X0, Xt, V = f(N, 192), f(N, 192) * 2.0, f(N, D), f(N, D), f(N, D)
    t = rng.random(N).astype(np.float32)
    for i, s in enumerate((0.0, 0.5, 1.0 - 2.0 ** -24)[:N]):
        t[i] = s
    zr = 3 if N >= 4 else 0  # the all-zero X_t row: at t = 0, or past the three special rows at t = 0.25
    Xt[zr] = 0.0
    if zr == 3:
        t[3] = 0.25
    assert N < 3 or (t[2] < 1.0 and np.float32(1.0) - t[2] == np.float32(2.0 ** -24))
    return X1w, Pw, X0, Xt, V, t, zr


def _head_ref(V, Xt, X1, X0, t, prior, dtype):
    c = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype)  # noqa: E731
    v, pred, rows = RB.head_ref(c(V), c(Xt), c(X1), c(X0), c(t)[:, None], None if prior is None else c(prior))
    return v.numpy(), pred.numpy(), rows.numpy()


def _row_bar(got, ref64, ref32, what):
    """rtol 1e-5 + twice fp32 torch's own error in the same row."""
    got, ref32 = np.asarray(got, np.float64), np.asarray(ref32, np.float64)
    own = np.abs(ref32 - ref64).reshape(len(ref64), -1).max(axis=1)
    err = np.abs(got - ref64).reshape(len(ref64), -1).max(axis=1)
    print(f"{what}: largest row error {err.max():.3e} (fp32 torch {own.max():.3e}); "
          f"median row {np.median(err):.3e} ({np.median(own):.3e})")
    bound = 1e-5 * np.abs(ref64) + 2 * own.reshape((-1,) + (1,) * (ref64.ndim - 1))
    assert (np.abs(got - ref64) <= bound).all(), what


def _run_head(N, X1, ld1, X0, Xt, V, t, prior, ldp):
    # every device tensor is held in a name until the results are read: a temporary's block would go back to the
    # allocator as soon as its pointer is taken, and the next upload would land in it
    dV, dXt, dX0, dt = dev(V.copy()), dev(Xt), dev(X0), dev(t)
    pred = torch.full((N, D), float("nan"), device=DEV)
    parts = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    if prior is None:
        _call("gmr_rf_head_fwd", N, _ptr(dV), _ptr(dXt), _ptr(X1), ld1, _ptr(dX0), _ptr(dt), 0.1, _ptr(pred),
              _ptr(parts))
    else:
        _call("gmr_rf_head_prior_fwd", N, _ptr(dV), _ptr(dXt), _ptr(X1), ld1, _ptr(dX0), _ptr(dt), _ptr(prior), ldp,
              RB.PRIOR_SCALE, RB.COS_SCALE, _ptr(pred), _ptr(parts))
    torch.cuda.synchronize()
    return dV.cpu().numpy(), pred.cpu().numpy(), parts.cpu().numpy()


@pytest.mark.parametrize("N", [1, 3, 4, 5, 130])
@pytest.mark.parametrize("ld1,ldp", [(64, 64), (192, 192), (64, 192)])
def test_head_prior_fwd(N, ld1, ldp):
    X1w, Pw, X0, Xt, V, t, zr = _head_case(N)
    x1, pr = X1w[:, 64:128], Pw[:, 128:192]
    dX1 = dev(X1w)[:, 64:128] if ld1 == 192 else dev(np.ascontiguousarray(x1))
    dP = dev(Pw)[:, 128:192] if ldp == 192 else dev(np.ascontiguousarray(pr))
    assert N == 1 or (dX1.stride(0) == ld1 and dP.stride(0) == ldp)  # a single row's stride is never used
    v, pred, parts = _run_head(N, dX1, ld1, X0, Xt, V, t, dP, ldp)
    w64 = _head_ref(V, Xt, x1, X0, t, pr, torch.float64)
    w32 = _head_ref(V, Xt, x1, X0, t, pr, torch.float32)
    assert np.isfinite(w64[0]).all() and np.abs(w64[0][zr]).max() > 1e3  # the zero X_t row: 1 / 1e-8
    for got, a, b, what in zip((v, pred, parts), w64, w32, ("V", "pred", "row partials")):
        _row_bar(got, a, b, f"head N={N} ld1={ld1} ldp={ldp} {what}")
    # the prior is in it
    bare = _head_ref(V, Xt, x1, X0, t, None, torch.float64)[0]
    assert N < 2 or np.abs(v[1] - bare[1]).max() > 1e-2


@pytest.mark.parametrize("N", [1, 3, 4, 5, 130])
def test_head_zero_prior_is_head_fwd(N):
    X1w, Pw, X0, Xt, V, t, zr = _head_case(N)
    dX1 = dev(X1w)[:, 64:128]
    zero = torch.zeros((N, 192), device=DEV)[:, 64:128]
    a = _run_head(N, dX1, 192, X0, Xt, V, t, None, 0)
    b = _run_head(N, dX1, 192, X0, Xt, V, t, zero, 192)
    for x, y, what in zip(a, b, ("V", "pred", "row partials")):
        assert np.array_equal(x, y), what


def test_head_prior_bad_args():
    N = 4
    z = torch.zeros((N, D), device=DEV)
    p = torch.zeros(N, dtype=torch.float64, device=DEV)
    for prior, ldp in ((None, 64), (z, 32)):
        with pytest.raises(RuntimeError, match="gmr_rf_head_prior_fwd"):
            _call("gmr_rf_head_prior_fwd", N, _ptr(z), _ptr(z), _ptr(z), 64, _ptr(z), _ptr(z[:, 0].contiguous()),
                  _ptr(prior), ldp, 0.2, 0.1, _ptr(z), _ptr(p))


# ------------------------------------------------------------------------------------------------ item inputs
SENT = 7.25


def _inputs_run(I, U, tv, hasT, hasV, fill):
    """The kernel on views of wider tables pre-filled with `fill` (item rows) and SENT (user rows, spare columns)."""
    from gmr import _lib
    C = 64 * (hasT + hasV)
    N = U + I
    cond = torch.full((N, C + 64), SENT, device=DEV)
    prior = torch.full((N, 128), SENT, device=DEV)
    cond[U:, :C] = fill
    prior[U:, :64] = fill
    ws = torch.full((int(_lib.load().gmr_rf_item_inputs_ws_floats(I)),), float("nan"), device=DEV)
    T = tv[:, 0:64] if hasT else None
    V = tv[:, 128:192] if hasV else None
    _call("gmr_rf_item_inputs", I, U, _ptr(T), 192, _ptr(V), 192, _ptr(cond), C + 64, _ptr(prior), 128, _ptr(ws))
    torch.cuda.synchronize()
    return cond.cpu().numpy(), prior.cpu().numpy()


@pytest.mark.parametrize("I", [1, 5, 41, 128, 129, 1100])  # 128 / 129: one full 128-row block, and one row past it
@pytest.mark.parametrize("U", [0, 3])
@pytest.mark.parametrize("mods", ["both", "image", "text"])
def test_item_inputs(I, U, mods):
    hasT, hasV = mods != "image", mods != "text"
    C = 64 * (hasT + hasV)
    rng = np.random.default_rng(I + 10 * U)
    wide = (rng.standard_normal((I, 192)) + 0.5).astype(np.float32)  # a mean next to the spread, as projected rows
    tv = dev(wide)
    cond, prior = _inputs_run(I, U, tv, hasT, hasV, float("nan"))
    # user rows and the columns past the tables: untouched
    assert (cond[:U] == SENT).all() and (prior[:U] == SENT).all()
    assert (cond[:, C:] == SENT).all() and (prior[:, 64:] == SENT).all()
    # conditions: the rows themselves, image first
    T, V = (wide[:, 0:64] if hasT else None), (wide[:, 128:192] if hasV else None)
    want_cond = np.concatenate([x for x in (V, T) if x is not None], axis=1)
    assert np.array_equal(cond[U:, :C], want_cond)
    # prior against fp64; the bar of a column is twice fp32 torch's own error in that column
    ref = {}
    for dt in (torch.float64, torch.float32):
        c = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt)  # noqa: E731
        wc, wp = RB.rf_inputs_ref(c(T), c(V), U)
        ref[dt] = wp.numpy()[U:]
        assert not wp[:U].any() and np.array_equal(wc.numpy()[U:].astype(np.float32), want_cond)
    r64 = ref[torch.float64]
    own = np.abs(ref[torch.float32].astype(np.float64) - r64).max(axis=0)
    err = np.abs(prior[U:, :64].astype(np.float64) - r64)
    print(f"prior I={I} U={U} {mods}: max abs error {err.max():.3e} (fp32 torch {own.max():.3e})")
    assert (err <= 1e-5 * np.abs(r64) + 2 * own[None, :]).all()
    if I == 1:
        assert not prior[U:, :64].any()  # a single item is its own mean
    # a second run over other leftovers: bit-identical
    cond2, prior2 = _inputs_run(I, U, tv, hasT, hasV, -3.0)
    assert np.array_equal(cond, cond2) and np.array_equal(prior, prior2)


def test_item_inputs_bad_args():
    from gmr import _lib
    I, U = 5, 2
    tv = torch.zeros((I, 192), device=DEV)
    cond, prior = torch.zeros((U + I, 128), device=DEV), torch.zeros((U + I, 64), device=DEV)
    ws = torch.zeros(int(_lib.load().gmr_rf_item_inputs_ws_floats(I)), device=DEV)
    ok = [I, U, _ptr(tv), 192, _ptr(tv[:, 64:]), 192, _ptr(cond), 128, _ptr(prior), 64, _ptr(ws)]
    _call("gmr_rf_item_inputs", *ok)
    for pos, val in ((2, None), (3, 190), (7, 64), (9, 32), (0, 0), (10, None)):
        bad = list(ok)
        bad[pos] = val
        if pos == 2:
            bad[4] = None  # neither table
        with pytest.raises(RuntimeError, match="gmr_rf_item_inputs"):
            _call("gmr_rf_item_inputs", *bad)
