"""The denoiser kernels of csrc/gendiff.hip past the B = 24 fixture, called through _lib.call against fp64 references on
the CPU (F.layer_norm, exact GELU and torch autograd).

  gmr_layernorm_fwd / _bwd   one wave per row, four rows per forward block, eight per backward block, 16 part groups
                             in ln_param_reduce_kernel:
                               D 32 (half the wave idle), 64, 128, 256, 512, 1024: every PER instantiation
                               rows 1; 3, 4, 5 (a forward block short, full, one over); 8, 9 (the same for the
                               backward block); 130 (P = 17: the second step of p += 16); 1000 at D = 64 and 512
                             six option sets that between them hold gelu 0 / 1, b absent / a matrix / a broadcast row
                             (ldb == 0), keep bytes present / absent, contiguous / strided a, y, s_out, dy, dx, and
                             both accumulate flags 0 / 1 from non-zero buffers (NaN-filled ones where the flag is 0);
                             from three rows on, one row is constant (variance 0) and the last is scaled by 1e3
  gmr_adaln_fwd / _bwd       (rows, D) = (1, 64), (7, 48), (300, 512); t an array, and t_const with t = NULL;
                             lds > 2 D and every operand strided
  gmr_xattn_table / fwd / bwd  (D, nhead) = (64, 1), (64, 8), (96, 8) (the second 64-column block half empty), (512, 8),
                             (512, 16); rows 1, 127, 128, 129 (the second chunk), 1000, and 4097 at D = 64 (the
                             32-chunk cap, chunk = 129); two layers a layer_stride apart that exceeds the tensors;
                             masks with a row that keeps no head and, with more than one head, a head no row keeps;
                             drawn masks replayed, and drawn in two calls

Bars.  adaLN and s_out are element-wise: a few fp32 roundings, counted at the check.  Everything else stands behind a
sum: 4 x the error of the same torch formula in fp32 on the CPU against fp64 (both sides are fp32 with different
summation orders), floored at 1e-6 and never above 1e-5 (forward) or 2e-4 (gradients), the bars of test_genrec_gpu.py.
LayerNorm's y and dx are taken relative to each row's largest expected value, its mean relative to the row's largest
input, rstd relative to itself; dw, db and the cross-attention tensors relative to the tensor's largest expected
value.  Every bar is measured on the restatement alone and printed next to the observed error.

Seen on the MI355X, largest error (largest bar) over all shapes and option sets: LayerNorm mean 2.2e-8, rstd 1.5e-7
(1.0e-6), y 3.0e-7 (1.8e-6), dx 3.0e-7 (1.8e-6), dw 2.5e-7 (1.2e-6), db 1.3e-7 (1.1e-6); cross-attention table 3.2e-7
(1.0e-6), CA 1.7e-7 (1.2e-6), g_wo 2.7e-7 (2.0e-6), g_bv 2.7e-7 (1.4e-6).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
FWD_CAP, GRAD_CAP = 1e-5, 2e-4
LN_EPS = float(np.float32(1e-5))
FILL = 7.0


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


def _np(t):
    return t.detach().cpu().numpy()


def _rel(got, want, scale=None):
    """Largest error relative to the tensor's largest expected value, or to scale (broadcast against want)."""
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want)
    if scale is None:
        scale = np.abs(want).max()
    scale = np.broadcast_to(np.asarray(scale, np.float64), err.shape)
    if (err[scale == 0] != 0).any():
        return float("inf")
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def _rows(want):
    return np.abs(np.asarray(want, np.float64)).max(axis=1, keepdims=True)


def _check(what, got, w64, w32, cap, tag, scale=None):
    bar = min(max(4 * _rel(w32, w64, scale), 1e-6), cap)
    err = _rel(got, w64, scale)
    print(f"{tag} {what}: relative error {err:.3e} (bar {bar:.3e})")
    assert np.isfinite(np.asarray(got)).all(), (tag, what)
    assert err <= bar, (tag, what, err, bar)


def _strided(a, on, pad=5):
    """A device copy of the 2-d array a: contiguous, or the leading columns of a table pad wider holding FILL."""
    a = torch.as_tensor(a)
    if not on:
        return a.to(DEV).contiguous()
    wide = torch.full((a.shape[0], a.shape[1] + pad), FILL, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return wide.to(DEV)[:, :a.shape[1]]


def _untouched(t):
    return t._base is None or bool((t._base[:, t.shape[1]:] == FILL).all())


# ------------------------------------------------------------------------------------------------ LayerNorm
# (gelu, b, keep, strided, accumulate_dx, accumulate_params)
LN_OPTIONS = ((0, None, False, False, 0, 0), (1, "matrix", True, True, 1, 1), (0, "row", False, True, 0, 1),
              (1, "row", True, False, 1, 0), (0, "matrix", False, True, 1, 1), (1, None, False, True, 0, 0))
LN_ROWS = (1, 3, 4, 5, 8, 9, 130)
LN_KEEP_SCALE = float(np.float32(1.0 / 0.9))


def _ln_inputs(rows, D):
    rng = np.random.default_rng(rows * 4096 + D)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    a = f(rows, D)
    if rows >= 3:
        a[rows // 2] = 0.5  # a constant row: variance 0 (where no b is added)
        a[rows - 1] *= 1e3
    return {"a": a, "bm": f(rows, D), "br": f(1, D), "keep": (rng.random((rows, D)) < 0.9).astype(np.uint8),
            "w": (1 + 0.1 * f(D)).astype(np.float32), "bias": 0.1 * f(D), "dy": f(rows, D), "dx0": f(rows, D),
            "dw0": f(D), "db0": f(D)}


def _ln_ref(x, gelu, bmode, keep, dtype):
    t = lambda k: torch.tensor(x[k], dtype=dtype)  # noqa: E731
    s = t("a")
    if bmode:
        bb = t("bm") if bmode == "matrix" else t("br")
        if keep:
            bb = bb * (t("keep") * torch.tensor(LN_KEEP_SCALE, dtype=dtype))
        s = s + bb
    s = s.detach().requires_grad_(True)
    w, bias = t("w").requires_grad_(True), t("bias").requires_grad_(True)
    D = s.shape[1]
    y = F.layer_norm(s, (D,), w, bias, LN_EPS)
    if gelu:
        y = F.gelu(y)  # the exact (erf) form
    mean = s.mean(1)
    rstd = 1 / torch.sqrt(((s - mean[:, None]) ** 2).mean(1) + torch.tensor(LN_EPS, dtype=dtype))
    g = torch.autograd.grad((y * t("dy")).sum(), [s, w, bias])
    r = {"s": s, "y": y, "mean": mean, "rstd": rstd, "dx": g[0], "dw": g[1], "db": g[2]}
    return {k: v.detach().numpy() for k, v in r.items()}


def _ln_case(rows, D):
    from gmr import _lib
    x = _ln_inputs(rows, D)
    d = {k: dev(x[k]) for k in ("w", "bias")}
    nparts = int(_lib.load().gmr_layernorm_parts_floats(rows, D))
    assert nparts == -(-rows // 8) * 2 * D
    nan = lambda *sh: torch.full(sh, float("nan"))  # noqa: E731
    for gelu, bmode, keep, strided, acc_dx, acc_p in LN_OPTIONS:
        tag = f"ln D={D} rows={rows} gelu={gelu} b={bmode} keep={keep} strided={strided} acc={acc_dx}{acc_p}"
        a, dy = _strided(x["a"], strided), _strided(x["dy"], strided, 9)
        b = None if not bmode else (_strided(x["bm"], strided, 3) if bmode == "matrix" else dev(x["br"]))
        km = _strided(x["keep"], strided, 11) if keep and bmode else None
        y, s_out = _strided(nan(rows, D), strided, 7), _strided(nan(rows, D), strided, 2)
        mean, rstd = nan(rows).to(DEV), nan(rows).to(DEV)
        ld = lambda v: v.stride(0) if v is not None else 0  # noqa: E731
        _call("gmr_layernorm_fwd", rows, D, _ptr(a), ld(a), _ptr(b), ld(b) if bmode == "matrix" else 0, _ptr(km), ld(km),
              LN_KEEP_SCALE, _ptr(d["w"]), _ptr(d["bias"]), LN_EPS, gelu, _ptr(y), ld(y), _ptr(s_out), ld(s_out),
              _ptr(mean), _ptr(rstd))
        dx = _strided(x["dx0"] if acc_dx else nan(rows, D), strided, 4)
        dw, db = (dev(x[k]) if acc_p else nan(D).to(DEV) for k in ("dw0", "db0"))
        parts = nan(nparts).to(DEV)
        _call("gmr_layernorm_bwd", rows, D, _ptr(s_out), ld(s_out), _ptr(mean), _ptr(rstd), _ptr(d["w"]), _ptr(d["bias"]),
              gelu, _ptr(dy), ld(dy), _ptr(dx), ld(dx), acc_dx, _ptr(parts), _ptr(dw), _ptr(db), acc_p)
        torch.cuda.synchronize()
        assert all(_untouched(v) for v in (a, dy, y, s_out, dx) + ((km,) if km is not None else ()))
        w64, w32 = (_ln_ref(x, gelu, bmode, keep and bmode, dt) for dt in (torch.float64, torch.float32))
        # s = a + keep scale b: a product and a sum
        added = np.abs(w64["s"] - x["a"])
        assert (np.abs(_np(s_out) - w64["s"]) <= 2 * U24 * (np.abs(x["a"]) + added) + 1e-37).all(), tag
        smax = _rows(w64["s"])[:, 0]
        _check("mean", _np(mean), w64["mean"], w32["mean"], FWD_CAP, tag, smax)
        _check("rstd", _np(rstd), w64["rstd"], w32["rstd"], FWD_CAP, tag, w64["rstd"])
        _check("y", _np(y), w64["y"], w32["y"], FWD_CAP, tag, _rows(w64["y"]))
        add = lambda k: x[k].astype(np.float64)  # noqa: E731
        wdx = w64["dx"] + (add("dx0") if acc_dx else 0)
        _check("dx", _np(dx), wdx, w32["dx"] + (x["dx0"] if acc_dx else np.float32(0)), GRAD_CAP, tag, _rows(wdx))
        for k, k0, got in (("dw", "dw0", dw), ("db", "db0", db)):
            _check(k, _np(got), w64[k] + (add(k0) if acc_p else 0), w32[k] + (x[k0] if acc_p else np.float32(0)),
                   GRAD_CAP, tag)


@pytest.mark.parametrize("D", [32, 64, 128, 256, 512, 1024])
def test_layernorm_fwd_bwd(D):
    for rows in LN_ROWS:
        _ln_case(rows, D)


@pytest.mark.parametrize("D", [64, 512])
def test_layernorm_fwd_bwd_1000_rows(D):
    _ln_case(1000, D)


def test_layernorm_rejects_other_widths():
    t = torch.zeros((4, 96), device=DEV)
    v = torch.zeros(96, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_layernorm_fwd"):
        _call("gmr_layernorm_fwd", 4, 96, _ptr(t), 96, None, 0, None, 0, 1.0, _ptr(v), _ptr(v), LN_EPS, 0, _ptr(t), 96,
              None, 0, _ptr(v), _ptr(v))


# ------------------------------------------------------------------------------------------------ adaLN
@pytest.mark.parametrize("rows,D", [(1, 64), (7, 48), (300, 512)])
def test_adaln_fwd_bwd(rows, D):
    T = 11
    rng = np.random.default_rng(rows + D)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    h0, g, S = f(rows, D), f(rows, D), f(T, 2 * D)
    t = rng.integers(0, T, rows)
    t[0] = T - 1
    dh0_, dg, dS = _strided(h0, True, 3), _strided(g, True, 6), _strided(S, True, 9)
    dt = dev(t, torch.int32)
    nan = lambda: torch.full((rows, D), float("nan"))  # noqa: E731
    h64, S64 = h0.astype(np.float64), S.astype(np.float64)
    for tt, t_arr in ((t, dt), (np.full(rows, 4), None)):
        h1 = _strided(nan(), True, 2)
        _call("gmr_adaln_fwd", rows, D, _ptr(dh0_), dh0_.stride(0), _ptr(t_arr), 4, _ptr(dS), dS.stride(0), _ptr(h1),
              h1.stride(0))
        shift, scale = S64[tt, :D], S64[tt, D:]
        # 1 + scale, the product, the sum
        bound = 3 * U24 * (np.abs(h64) * (1 + np.abs(scale)) + np.abs(shift)) + 1e-37
        assert (np.abs(_np(h1) - (h64 * (1 + scale) + shift)) <= bound).all()
        assert _untouched(h1)
    scale = S64[t, D:]
    dh0, prod = _strided(nan(), True, 4), _strided(nan(), True, 8)
    _call("gmr_adaln_bwd", rows, D, _ptr(dh0_), dh0_.stride(0), _ptr(dg), dg.stride(0), _ptr(dt), _ptr(dS), dS.stride(0),
          _ptr(dh0), dh0.stride(0), _ptr(prod), prod.stride(0))
    g64 = g.astype(np.float64)
    # dh0 = g (1 + scale): a sum and a product; prod = g h0: one product
    assert (np.abs(_np(dh0) - g64 * (1 + scale)) <= 2 * U24 * np.abs(g64) * (1 + np.abs(scale)) + 1e-37).all()
    assert (np.abs(_np(prod) - g64 * h64) <= U24 * np.abs(g64 * h64) + 1e-37).all()
    assert all(_untouched(v) for v in (dh0, prod, dh0_, dg, dS))


# ------------------------------------------------------------------------------------------------ cross-attention
P_KEEP = float(np.float32(0.75))
XATTN_ROWS = (1, 127, 128, 129, 1000)


def _xattn_ref(wo, bv, bo, keep, dca, nhead, dtype):
    t = lambda a: torch.tensor(a, dtype=dtype)  # noqa: E731
    D = wo.shape[0]
    Wo, b = t(wo).requires_grad_(True), t(bv).requires_grad_(True)
    bs = b / torch.tensor(P_KEEP, dtype=dtype)
    table = (Wo.view(D, nhead, D // nhead) * bs.view(1, nhead, D // nhead)).sum(2).t()  # P[h][j]
    Bc = t(keep).repeat_interleave(D // nhead, 1) * bs  # keep spread over the head's columns
    CA = Bc @ Wo.t() + t(bo)
    g = torch.autograd.grad((CA * t(dca)).sum(), [Wo, b])
    return [v.detach().numpy() for v in (table, CA, g[0], g[1])]


@pytest.mark.parametrize("D,nhead", [(64, 1), (64, 8), (96, 8), (512, 8), (512, 16)])
def test_xattn_table_fwd_bwd(D, nhead):
    from gmr import _lib
    L = 2
    stride = D * D + D + 13
    rng = np.random.default_rng(D + nhead)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    slab = np.full(L * stride, FILL, np.float32)
    wo, bv = [], []
    for l in range(L):
        wo.append(f(D, D) / np.float32(np.sqrt(D)))
        bv.append(f(D))
        slab[l * stride:l * stride + D * D] = wo[l].ravel()
        slab[l * stride + D * D:l * stride + D * D + D] = bv[l]
    dslab = dev(slab)
    P = torch.full((L, nhead, D), float("nan"), device=DEV)
    _call("gmr_xattn_table_f32", L, D, nhead, _ptr(dslab), _ptr(dslab[D * D:]), stride, P_KEEP, _ptr(P))
    bo = f(D)
    dbo = dev(bo)
    for rows in XATTN_ROWS + ((4097,) if D == 64 else ()):
        l = rows % L
        keep = (rng.random((rows, nhead)) < P_KEEP).astype(np.uint8)
        keep[rows // 2] = 0   # a row that keeps no head
        if nhead > 1:
            keep[:, 1] = 0    # a head that no row keeps
        dca = f(rows, D)
        km, ddca = _strided(keep, True, 3), _strided(dca, True, 5)
        CA = _strided(torch.full((rows, D), float("nan")), True, 7)
        _call("gmr_xattn_fwd_f32", rows, D, nhead, _ptr(P[l]), _ptr(dbo), P_KEEP, _ptr(km), None, km.stride(0), 0, 0, 0,
              _ptr(CA), CA.stride(0))
        g_wo0, g_bv0 = f(D, D), f(D)
        g_wo, g_bv = dev(g_wo0.copy()), dev(g_bv0.copy())
        nws = int(_lib.load().gmr_xattn_bwd_workspace_floats(rows, D, nhead))
        chunks = min(32, -(-rows // 128))
        assert nws == (chunks + 1) * nhead * D
        ws = torch.full((nws,), float("nan"), device=DEV)
        woff = l * stride
        _call("gmr_xattn_bwd_f32", rows, D, nhead, _ptr(ddca), ddca.stride(0), _ptr(km), km.stride(0),
              _ptr(dslab[woff:]), _ptr(dslab[woff + D * D:]), P_KEEP, _ptr(g_wo), _ptr(g_bv), _ptr(ws), nws)
        torch.cuda.synchronize()
        assert _untouched(CA) and _untouched(km) and _untouched(ddca)
        w64, w32 = (_xattn_ref(wo[l], bv[l], bo, keep, dca, nhead, dt) for dt in (torch.float64, torch.float32))
        tag = f"xattn D={D} nhead={nhead} rows={rows} layer={l}"
        _check("table", _np(P[l]), w64[0], w32[0], FWD_CAP, tag)
        _check("CA", _np(CA), w64[1], w32[1], FWD_CAP, tag)
        _check("g_wo", _np(g_wo), w64[2] + g_wo0, w32[2] + g_wo0, GRAD_CAP, tag)
        _check("g_bv", _np(g_bv), w64[3] + g_bv0, w32[3] + g_bv0, GRAD_CAP, tag)
    assert bool((dslab == dev(slab)).all())


@pytest.mark.parametrize("D,nhead", [(64, 8), (96, 8), (512, 16)])
def test_xattn_drawn_masks(D, nhead):
    rng = np.random.default_rng(D)
    P = dev(rng.standard_normal((nhead, D)).astype(np.float32))
    bo = dev(rng.standard_normal(D).astype(np.float32))
    rows, split, seed, step, row0 = 300, 129, 77, 5, 40
    ldm = nhead + 3

    def fwd(n, r0, mask_in=None):
        mask = torch.full((n, ldm), 9, dtype=torch.uint8, device=DEV)
        CA = torch.full((n, D), float("nan"), device=DEV)
        _call("gmr_xattn_fwd_f32", n, D, nhead, _ptr(P), _ptr(bo), P_KEEP, _ptr(mask_in), None if mask_in is not None
              else _ptr(mask), ldm, seed, step, r0, _ptr(CA), D)
        return _np(mask), _np(CA)

    m_all, ca_all = fwd(rows, row0)
    assert set(np.unique(m_all[:, :nhead])) == {0, 1} and (m_all[:, nhead:] == 9).all()
    frac = m_all[:, :nhead].mean()  # 300 x nhead Bernoulli(0.75) draws: five standard deviations
    assert abs(frac - P_KEEP) < 5 * np.sqrt(P_KEEP * (1 - P_KEEP) / (rows * nhead))
    _, ca_replay = fwd(rows, row0, dev(m_all))
    assert np.array_equal(ca_replay, ca_all)
    m1, ca1 = fwd(split, row0)
    m2, ca2 = fwd(rows - split, row0 + split)
    assert np.array_equal(np.concatenate([m1, m2]), m_all) and np.array_equal(np.concatenate([ca1, ca2]), ca_all)


def test_xattn_fwd_and_bwd_take_the_same_heads():
    """The backward holds 16 heads in registers; the forward and the table refuse what the backward cannot follow.
    All three return before a launch."""
    D, nhead = 64, 32
    t = torch.zeros((4, D), device=DEV)
    m = torch.ones((4, nhead), dtype=torch.uint8, device=DEV)
    P = torch.zeros((nhead, D), device=DEV)
    W = torch.zeros((D * D + D,), device=DEV)
    with pytest.raises(RuntimeError, match="gmr_xattn_table_f32"):
        _call("gmr_xattn_table_f32", 1, D, nhead, _ptr(W), _ptr(W[D * D:]), D * D + D, 1.0, _ptr(P))
    with pytest.raises(RuntimeError, match="gmr_xattn_fwd_f32"):
        _call("gmr_xattn_fwd_f32", 4, D, nhead, _ptr(P), _ptr(t), 1.0, _ptr(m), None, nhead, 0, 0, 0, _ptr(t), D)
    ws = torch.zeros((2 * nhead * D,), device=DEV)
    with pytest.raises(RuntimeError, match="gmr_xattn_bwd_f32"):
        _call("gmr_xattn_bwd_f32", 4, D, nhead, _ptr(t), D, _ptr(m), nhead, _ptr(W), _ptr(W[D * D:]), 1.0, _ptr(W),
              _ptr(W[D * D:]), _ptr(ws), 2 * nhead * D)
    torch.cuda.synchronize()
