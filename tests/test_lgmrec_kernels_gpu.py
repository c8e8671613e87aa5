"""The LGMRec kernels of csrc/lgmrec.hip by name, against fp64 torch on random data.

Bar per output: the largest error against fp64 is at most twice the largest error of the same computation done by fp32
torch on the CPU on the same inputs; both are printed.  Row counts 1, 15, 17, 53 and 4,103 (a workgroup's second trip,
more partial tiles than workgroups under a grid cap), H in {4, 5, 64}, packed and padded strides with NaN outside the
columns."""
import numpy as np
import pytest
import torch

from gmr import _lib
from gmr.kernels import ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, TAU = 64, 0.2
ROWS = [1, 15, 17, 53, 4103]
HS = [4, 5, 64]
CAP = 3   # a grid cap for the row kernels: at 4,103 rows 257 tiles (or 1,026 waves' rows) over 3 workgroups
SPLIT = {1: (0, 1), 15: (5, 10), 17: (6, 11), 53: (20, 33), 4103: (103, 4000)}   # N -> (U, I)


def _bar(got, ref64, ref32, what):
    got = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    ref64 = ref64.numpy() if torch.is_tensor(ref64) else np.asarray(ref64)
    ref32 = (ref32.numpy() if torch.is_tensor(ref32) else np.asarray(ref32)).astype(np.float64)
    assert np.isfinite(got).all(), what
    err, own = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    print(f"{what}: max abs error {err:.3e} (fp32 torch {own:.3e})")
    assert err <= 2 * own, (what, err, own)


def _dev(a, pad=0):
    """A device copy of a 2-D array; pad > 0: rows `pad` floats apart with NaN outside the columns."""
    a = torch.as_tensor(np.asarray(a))
    if not pad or a.dim() != 2:
        return a.to(DEV).contiguous()
    buf = torch.full((a.shape[0], pad), float("nan") if a.is_floating_point() else 0, dtype=a.dtype, device=DEV)
    v = buf[:, :a.shape[1]]
    v.copy_(a)
    return v


def _out(n, cols, pad=0):
    return torch.full((n, pad or cols), float("nan"), device=DEV)[:, :cols]


def _padded(n, H):
    return (n + H) % 2 == 1   # about half of the cases run on padded strides


def _csr(rng, U, I):
    """A user CSR with an empty row (the last), a row that holds item 1 alone (row 1) and, where it fits, a row of 300
    items (row 0); columns ascending."""
    rows = []
    for u in range(U):
        k = 300 if (u == 0 and I >= 300) else 0 if u == U - 1 else int(rng.integers(1, min(I, 9) + 1))
        rows.append(np.array([1]) if u == 1 else np.sort(rng.choice(I, k, replace=False)))
    rp = np.zeros(U + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32) if U and rp[-1] else np.zeros(0, np.int32)
    R = np.zeros((U, I))
    for u, r in enumerate(rows):
        R[u, r] = 1.0
    return rp, col, R


# ----------------------------------------------------------------------------- hyperedge rows
def hyper_ref(Lv, Lt, R, g, keep, p_keep, dtype):
    out = []
    for m, L in enumerate((Lv, Lt)):
        Li = torch.tensor(L, dtype=dtype)
        Lall = torch.cat([torch.tensor(R, dtype=dtype) @ Li, Li])
        S = torch.softmax((Lall + torch.tensor(g[m], dtype=dtype)) / TAU, dim=1)
        h = S if keep is None else S * torch.tensor(keep[m]).to(dtype) * (1.0 / p_keep)
        out.append((S, h))
    return torch.cat([out[0][0], out[1][0]], 1), torch.cat([out[0][1], out[1][1]], 1)


def hyper_run(U, I, H, Lv, Lt, rp, col, g=None, keep=None, p_keep=1.0, mode=0, seed=0, step=0, pad=False, cap=0):
    N = U + I
    ldh = 2 * H + 3 if pad else 2 * H
    S, h = _out(N, 2 * H, ldh), _out(N, 2 * H, ldh)
    lv, lt = _dev(Lv, H + 8 if pad else 0), _dev(Lt, H + 4 if pad else 0)
    rpd, cold = _dev(rp), _dev(col if len(col) else np.zeros(1, np.int32))
    gd = [_dev(x.astype(np.float32), H + 1 if pad else 0) for x in g] if g is not None else [None, None]
    kd = [_dev(x.astype(np.uint8), H + 1 if pad else 0) for x in keep] if keep is not None else [None, None]
    _lib.call("gmr_lgm_hyper_fwd", U, I, H, ptr(lv), lv.stride(0), ptr(lt), lt.stride(0), ptr(rpd), ptr(cold),
              ptr(gd[0]), ptr(gd[1]), gd[0].stride(0) if g is not None else 0, ptr(kd[0]), ptr(kd[1]),
              kd[0].stride(0) if keep is not None else 0, TAU, p_keep, mode, seed, step, ptr(S), ptr(h), ldh, cap,
              stream())
    return S, h


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", ROWS)
def test_hyper_fwd(N, H):
    U, I = SPLIT[N]
    rng = np.random.default_rng(100 * N + H)
    rp, col, R = _csr(rng, U, I)
    Lv, Lt = (rng.standard_normal((I, H)).astype(np.float32) for _ in range(2))
    if I > 1:
        Lv[1, 0] += 40.0      # logits more than 20 apart: probabilities of exactly 0 in fp32 (user row 1 holds item 1 alone)
    g = -np.log(-np.log(rng.uniform(1e-6, 1 - 1e-6, (2, N, H)))).astype(np.float32)
    keep = (rng.uniform(size=(2, N, H)) < 0.5).astype(np.uint8)
    keep[0, N - 1] = 0        # an all-dropped row
    pad = _padded(N, H)
    for kp, pk, mode in ((None, 1.0, 0), (keep, 0.5, 1)):
        S, h = hyper_run(U, I, H, Lv, Lt, rp, col, g, kp, pk, mode, pad=pad)
        r64, r32 = (hyper_ref(Lv, Lt, R, g, kp, pk, dt) for dt in (torch.float64, torch.float32))
        _bar(S, r64[0], r32[0], f"N {N} H {H} mode {mode}: S")
        _bar(h, r64[1], r32[1], f"N {N} H {H} mode {mode}: h")
        S1, h1 = hyper_run(U, I, H, Lv, Lt, rp, col, g, kp, pk, mode, pad=not pad, cap=1)
        assert torch.equal(S, S1) and torch.equal(h, h1)       # one workgroup, other strides: the same bits
    if I > 1:
        assert float(S[U + 1, 1]) == 0.0                       # the underflow is there
    # keep_rate = 1 draws no dropout whatever the mode says
    S2, h2 = hyper_run(U, I, H, Lv, Lt, rp, col, g, None, 1.0, 2, pad=pad)
    assert torch.equal(S2, h2)


def _draws(n, H, site, seed, step, p_keep):
    g = torch.empty((n, H), device=DEV)
    k = torch.empty((n, H), dtype=torch.uint8, device=DEV)
    _lib.call("gmr_lgm_draws", n, H, site, seed, step, p_keep, ptr(g), ptr(k), stream())
    return g, k


@pytest.mark.parametrize("H", HS)
def test_philox_draws_do_not_depend_on_the_tiling(H):
    U, I = 103, 4000
    rng = np.random.default_rng(H)
    rp, col, R = _csr(rng, U, I)
    Lv, Lt = (rng.standard_normal((I, H)).astype(np.float32) for _ in range(2))
    a = hyper_run(U, I, H, Lv, Lt, rp, col, p_keep=0.5, mode=2, seed=11, step=7)
    b = hyper_run(U, I, H, Lv, Lt, rp, col, p_keep=0.5, mode=2, seed=11, step=7, cap=3, pad=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = hyper_run(U, I, H, Lv, Lt, rp, col, p_keep=0.5, mode=2, seed=11, step=8)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1] != 0, c[1] != 0)
    # the draws are the ones gmr_lgm_draws reports: site 4 m for the users' Gumbel rows, + 2 for the items', + 1 dropout
    gs, ks = [], []
    for m in range(2):
        gu, ku = _draws(U, H, 4 * m, 11, 7, 0.5)
        gi, ki = _draws(I, H, 4 * m + 2, 11, 7, 0.5)
        gs.append(torch.cat([gu, gi]).cpu().numpy())
        ks.append(torch.cat([ku, ki]).cpu().numpy())
    d = hyper_run(U, I, H, Lv, Lt, rp, col, gs, ks, 0.5, 1)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])
    # an item row's draw does not depend on the number of users before it
    e = hyper_run(0, I, H, Lv, Lt, np.zeros(1, np.int32), np.zeros(0, np.int32), p_keep=0.5, mode=2, seed=11, step=7)
    assert torch.equal(e[0], a[0][U:]) and torch.equal(e[1], a[1][U:])


def test_philox_statistics():
    n, H, p = 8192, 64, 0.3
    cnt = n * H
    assert cnt >= 5e5
    for site in (0, 6):
        g, k = _draws(n, H, site, 5, 9, p)
        g = g.double().cpu().numpy()
        assert np.isfinite(g).all()
        var = np.pi ** 2 / 6
        mean_err, var_err = abs(g.mean() - 0.5772156649), abs(g.var() - var)
        share_err = abs(k.float().mean().item() - p)
        # sigma of the mean: sqrt(var / n); of the sample variance: sqrt((mu4 - var^2) / n), mu4 = 5.4 var^2 (Gumbel)
        print(f"site {site}: mean off {mean_err:.2e} (sigma {np.sqrt(var / cnt):.2e}), variance off {var_err:.2e} "
              f"(sigma {np.sqrt(4.4 * var ** 2 / cnt):.2e}), keep share off {share_err:.2e} "
              f"(sigma {np.sqrt(p * (1 - p) / cnt):.2e})")
        assert mean_err <= 5 * np.sqrt(var / cnt)
        assert var_err <= 5 * np.sqrt(4.4 * var ** 2 / cnt)
        assert share_err <= 5 * np.sqrt(p * (1 - p) / cnt)
    g2, k2 = _draws(n, H, 2, 5, 9, p)
    g0, k0 = _draws(n, H, 0, 5, 9, p)
    assert not torch.equal(g0, g2) and not torch.equal(k0, k2)


# ----------------------------------------------------------------------------- the reductions
def lat_run(A, Xv, Xt, H, cap=0):
    n = A.shape[0]
    ws = torch.full((int(_lib.load().gmr_lgm_lat_ws_floats(n, H)),), float("nan"), device=DEV)
    lat = _out(2 * H, D).contiguous()
    _lib.call("gmr_lgm_lat", n, ptr(A), A.stride(0), H, ptr(Xv), ptr(Xt), Xv.stride(0), ptr(ws), ws.numel(), cap,
              ptr(lat), stream())
    return lat


def lat_ref(A, Xv, Xt, H, dtype):
    A, Xv, Xt = (torch.tensor(x, dtype=dtype) for x in (A, Xv, Xt))
    return torch.cat([A[:, :H].T @ Xv, A[:, H:].T @ Xt])


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", ROWS)
def test_lat(n, H):
    rng = np.random.default_rng(7 * n + H)
    A = rng.uniform(0, 1, (n, 2 * H)).astype(np.float32)
    X = rng.standard_normal((n, 2 * D)).astype(np.float32)
    pad = _padded(n, H)
    Ad, Xd = _dev(A, 2 * H + 5 if pad else 0), _dev(X, 2 * D + 4 if pad else 0)
    # the backward's form: one table per modality; the forward's form: the same table for both
    for (xv, xt), (rv, rt), what in (((Xd[:, :D], Xd[:, D:]), (X[:, :D], X[:, D:]), "two tables"),
                                     ((Xd[:, :D], Xd[:, :D]), (X[:, :D], X[:, :D]), "one table")):
        lat = lat_run(Ad, xv, xt, H)
        _bar(lat, lat_ref(A, rv, rt, H, torch.float64), lat_ref(A, rv, rt, H, torch.float32), f"n {n} H {H} lat, {what}")
        for cap in (1, 7):   # bit-equal under two grid caps
            assert torch.equal(lat, lat_run(Ad, xv, xt, H, cap=cap)), (what, cap)
    # trailing rows with zero h leave the bits as they are
    A2 = np.concatenate([A, np.zeros((77, 2 * H), np.float32)])
    X2 = np.concatenate([X, rng.standard_normal((77, 2 * D)).astype(np.float32)])
    X2d = _dev(X2)
    assert torch.equal(lat_run(_dev(A2), X2d[:, :D], X2d[:, D:], H), lat_run(Ad, Xd[:, :D], Xd[:, D:], H))


# ----------------------------------------------------------------------------- rows of A M, the combine
def comb_ref(d, H, alpha, dtype):
    t = {k: torch.tensor(v, dtype=dtype) for k, v in d.items()}
    for k in ("mge", "h", "lat"):
        t[k].requires_grad_(True)
    lat = t["lat"].reshape(2, H, D)
    x = torch.cat([t["h"][:, :H] @ lat[0], t["h"][:, H:] @ lat[1]], 1)
    x.retain_grad()
    xv, xt = x[:, :D], x[:, D:]
    nrm = lambda x: x.norm(dim=1, keepdim=True).clamp_min(1e-12)  # noqa: E731
    mv, mt, g = t["mge"][:, :D], t["mge"][:, D:], xv + xt
    al = t["cge"] + mv / nrm(mv) + mt / nrm(mt) + alpha * g / nrm(g)
    (al * t["dall"]).sum().backward()
    o = {"all": al, "CLN": torch.cat([xv / nrm(xv), xt / nrm(xt)], 1), "nrmCL": torch.cat([nrm(xv), nrm(xt)]).reshape(-1),
         "nrm3": torch.cat([nrm(mv), nrm(mt), nrm(g)]).reshape(-1), "x": x, "dmge": t["mge"].grad,
         "dK": x.grad + t["dK0"]}
    return {k: v.detach().numpy() for k, v in o.items()}


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", ROWS)
def test_apply_and_combine(n, H):
    rng = np.random.default_rng(13 * n + H)
    alpha = 0.3
    d = {"cge": rng.standard_normal((n, D)), "mge": rng.standard_normal((n, 2 * D)), "h": rng.uniform(0, 2, (n, 2 * H)),
         "lat": rng.standard_normal((2 * H, D)), "dall": rng.standard_normal((n, D)),
         "dK0": rng.standard_normal((n, 2 * D))}
    d["h"][rng.uniform(size=d["h"].shape) < 0.5] = 0.0
    d["h"][n - 1] = 0.0                                    # an all-dropped row: ghe = 0, its norm clamped
    if n > 2:
        d["mge"][1, :D] = 0.0                              # and a modal view of zeros
    d = {k: v.astype(np.float32) for k, v in d.items()}
    r64, r32 = comb_ref(d, H, alpha, torch.float64), comb_ref(d, H, alpha, torch.float32)
    pad = _padded(n, H)
    hd, lat = _dev(d["h"], 2 * H + 3 if pad else 0), _dev(d["lat"])
    # apply, both modes
    want = [d["cge"].astype(np.float64) + r["x"][:, :D].astype(np.float64) + r["x"][:, D:] for r in (r64, r32)]
    applied = []
    for cap in (0, CAP):   # the default grid, then CAP workgroups: a workgroup's later trips, more tiles than workgroups
        Y = _out(n, 2 * D, 2 * D + 8 if pad else 0)
        _lib.call("gmr_lgm_apply", n, ptr(hd), hd.stride(0), H, ptr(lat), ptr(Y), Y.stride(0), 0, cap, stream())
        _bar(Y, r64["x"], r32["x"], f"n {n} H {H} apply, cap {cap}")
        Y1 = _dev(d["cge"], D + 4 if pad else 0)
        _lib.call("gmr_lgm_apply", n, ptr(hd), hd.stride(0), H, ptr(lat), ptr(Y1), Y1.stride(0), 1, cap, stream())
        _bar(Y1, want[0], want[1], f"n {n} H {H} apply, added, cap {cap}")
        applied.append((Y, Y1))
    assert torch.equal(applied[0][0], applied[1][0]) and torch.equal(applied[0][1], applied[1][1])
    # combine, forward
    cge, mge = _dev(d["cge"], D + 4 if pad else 0), _dev(d["mge"], 2 * D + 4 if pad else 0)
    al = _out(n, D, D + 8 if pad else 0)
    CLN, nrmCL, nrm3 = _out(n, 2 * D).contiguous(), _out(2, n).contiguous(), _out(3, n).contiguous()

    def fwd(cap):
        _lib.call("gmr_lgm_combine_fwd", n, ptr(cge), cge.stride(0), ptr(mge), mge.stride(0), ptr(hd), hd.stride(0), H,
                  ptr(lat), alpha, ptr(al), al.stride(0), ptr(CLN), ptr(nrmCL), ptr(nrm3), cap, stream())
        return [t.clone() for t in (al, CLN, nrmCL, nrm3)]

    first = fwd(0)
    for got, k in zip(first, ("all", "CLN", "nrmCL", "nrm3")):
        _bar(got.reshape(-1), r64[k].reshape(-1), r32[k].reshape(-1), f"n {n} H {H} combine {k}")
    assert all(torch.equal(a, b) for a, b in zip(first, fwd(2)))
    assert float(nrm3[2, n - 1]) == np.float32(1e-12) and not CLN[n - 1].any()
    # combine, backward
    dall = _dev(d["dall"], D + 4 if pad else 0)

    def bwd(cap):
        dK_, dmge_ = _dev(d["dK0"]), _out(n, 2 * D, 2 * D + 4 if pad else 0)
        _lib.call("gmr_lgm_combine_bwd", n, ptr(dall), dall.stride(0), ptr(mge), mge.stride(0), ptr(CLN), ptr(nrmCL),
                  ptr(nrm3), alpha, ptr(dmge_), dmge_.stride(0), ptr(dK_), cap, stream())
        return dmge_, dK_

    dmge, dK = bwd(0)
    capped = bwd(CAP)
    assert torch.equal(dmge, capped[0]) and torch.equal(dK, capped[1])     # CAP workgroups: the same bits
    # the rows with a clamped norm carry d y / 1e-12: they are held on their own, relative to their size, so that they
    # do not set the bar of the others
    big = (r64["nrm3"].reshape(3, n) <= 1e-12).any(0)     # row n - 1, row 1, and any row whose h came out all zero
    assert big[n - 1] and (n <= 2 or big[1])
    for got, k in ((dmge, "dmge"), (dK, "dK")):
        got = got.cpu().numpy()
        if (~big).any():
            _bar(got[~big], r64[k][~big], r32[k][~big], f"n {n} H {H} combine {k}")
        np.testing.assert_allclose(got[big], r64[k][big], rtol=1e-5, atol=2 * np.abs(r32[k][big] - r64[k][big]).max())


# ----------------------------------------------------------------------------- d h, the softmax backward
def dh_ref(d, H, p_keep, sbwd, dtype):
    t = {k: torch.tensor(v, dtype=dtype) for k, v in d.items()}
    M = t["M"].reshape(2, H, D)
    dh = torch.cat([t["X"][:, :D] @ M[0].T, t["X"][:, D:] @ M[1].T], 1) + t["acc"]
    if not sbwd:
        return dh.numpy()
    S, h = t["S"], t["h"]
    dS = torch.where(h != 0, dh * (1.0 / p_keep), torch.zeros_like(dh))
    out = []
    for m in range(2):
        s, ds = S[:, m * H:(m + 1) * H], dS[:, m * H:(m + 1) * H]
        out.append(s * (ds - (ds * s).sum(1, keepdim=True)) / TAU)
    return torch.cat(out, 1).numpy()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", ROWS)
def test_dh(n, H):
    rng = np.random.default_rng(17 * n + H)
    p_keep = 0.5
    z = rng.standard_normal((n, 2, H)) * 3
    z[0, 0, 0] += 200.0                                    # probabilities of exactly 0
    S = torch.softmax(torch.tensor(z, dtype=torch.float32), dim=2).numpy().reshape(n, 2 * H)
    assert (S == 0).any() or H == 1
    keep = rng.uniform(size=S.shape) < p_keep
    keep[n - 1] = False
    d = {"X": rng.standard_normal((n, 2 * D)), "M": rng.standard_normal((2 * H, D)),
         "acc": rng.standard_normal((n, 2 * H)), "S": S, "h": S * keep / p_keep}
    d = {k: np.asarray(v, np.float32) for k, v in d.items()}
    pad = _padded(n, H)
    X, M = _dev(d["X"], 2 * D + 4 if pad else 0), _dev(d["M"])
    acc, Sd, hd = (_dev(d[k], 2 * H + 3 if pad else 0) for k in ("acc", "S", "h"))
    first = {}
    for sbwd, cap in ((False, 0), (True, 0), (False, CAP), (True, CAP)):
        # CAP workgroups: every workgroup restages its LDS rows on later trips, and there are more tiles than workgroups
        out = _out(n, 2 * H, 2 * H + 1 if pad else 0)
        _lib.call("gmr_lgm_dh", n, ptr(X[:, :D]), ptr(X[:, D:]), X.stride(0), ptr(M), H, ptr(acc), acc.stride(0),
                  ptr(Sd) if sbwd else None, ptr(hd) if sbwd else None, hd.stride(0), p_keep, TAU, ptr(out),
                  out.stride(0), cap, stream())
        if cap == 0:
            first[sbwd] = out
        else:
            assert torch.equal(out, first[sbwd]), (sbwd, cap)
        _bar(out, dh_ref(d, H, p_keep, sbwd, torch.float64), dh_ref(d, H, p_keep, sbwd, torch.float32),
             f"n {n} H {H} dh, softmax backward {sbwd}")
    # without acc, in place on acc: the layer loop's accumulation
    zero = dict(d, acc=np.zeros_like(d["acc"]))
    out = _out(n, 2 * H)
    _lib.call("gmr_lgm_dh", n, ptr(X[:, :D]), ptr(X[:, D:]), X.stride(0), ptr(M), H, None, 0, None, None, 0, 1.0, TAU,
              ptr(out), out.stride(0), 0, stream())
    _bar(out, dh_ref(zero, H, 1.0, False, torch.float64), dh_ref(zero, H, 1.0, False, torch.float32), "dh, no acc")
    _lib.call("gmr_lgm_dh", n, ptr(X[:, :D]), ptr(X[:, D:]), X.stride(0), ptr(M), H, ptr(out), out.stride(0), None, None,
              0, 1.0, TAU, ptr(out), out.stride(0), CAP, stream())
    twice = dict(d, acc=dh_ref(zero, H, 1.0, False, torch.float64))
    _bar(out, dh_ref(twice, H, 1.0, False, torch.float64), 2 * dh_ref(zero, H, 1.0, False, torch.float32), "dh, in place")


# ----------------------------------------------------------------------------- d Lu to the items, the regulariser
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", ROWS)
def test_logit_bwd(N, H):
    from gmr import kernels as K
    U, I = SPLIT[N]
    rng = np.random.default_rng(19 * N + H)
    rp, col, R = _csr(rng, U, I)
    dL = rng.standard_normal((N, 2 * H)).astype(np.float32)
    pad = _padded(N, H)
    dLd = _dev(dL, 2 * H + 3 if pad else 0)
    if U:
        a = K.user_item_csr(U, I, _dev(rp), _dev(col if len(col) else np.zeros(1, np.int32))[:len(col)])
        at = K.csr_transpose(a)
        trp, tcol = at.rowptr, at.col
    else:
        trp, tcol = torch.zeros(I + 1, dtype=torch.int32, device=DEV), None
    def run(cap):
        ov_, ot_ = _out(I, H, H + 64 if pad else 0), _out(I, H, H + 6 if pad else 0)
        _lib.call("gmr_lgm_logit_bwd", U, I, H, ptr(dLd), dLd.stride(0), ptr(trp), ptr(tcol), ptr(ov_), ov_.stride(0),
                  ptr(ot_), ot_.stride(0), cap, stream())
        return ov_, ot_

    ov, ot = run(0)
    capped = run(CAP)
    assert torch.equal(ov, capped[0]) and torch.equal(ot, capped[1])       # CAP workgroups: the same bits
    refs = []
    for dt in (torch.float64, torch.float32):
        x, r = torch.tensor(dL, dtype=dt), torch.tensor(R, dtype=dt)
        refs.append(x[U:] + r.T @ x[:U])
    _bar(ov, refs[0][:, :H], refs[1][:, :H], f"N {N} H {H} d Li image")
    _bar(ot, refs[0][:, H:], refs[1][:, H:], f"N {N} H {H} d Li text")


@pytest.mark.parametrize("B", [1, 16, 100, 2048])
def test_reg(B):
    rng = np.random.default_rng(B)
    U, I = 23, 31
    al = rng.standard_normal((U + I, D)).astype(np.float32)
    idx = [rng.integers(0, n, B).astype(np.int32) for n in (U, I, I)]
    c0 = rng.standard_normal((3 * B, D)).astype(np.float32)
    coef = 1e-3 / B
    ald, cd, out = _dev(al, D + 4), _dev(c0, D + 8), torch.full((1,), float("nan"), device=DEV)
    ud, pd_, nd = (_dev(i) for i in idx)
    _lib.call("gmr_lgm_reg", B, U, ptr(ald), ald.stride(0), ptr(ud), ptr(pd_), ptr(nd), coef, ptr(cd), cd.stride(0),
              ptr(out), stream())
    refs = []
    for dt in (torch.float64, torch.float32):
        a = torch.tensor(al, dtype=dt, requires_grad=True)
        rows = [a[torch.as_tensor(idx[0].astype(np.int64))], a[U + torch.as_tensor(idx[1].astype(np.int64))],
                a[U + torch.as_tensor(idx[2].astype(np.int64))]]
        reg = coef * sum(r.norm() for r in rows)
        con = torch.cat([coef * r / r.norm() for r in rows]) + torch.tensor(c0, dtype=dt)
        refs.append((reg.detach().reshape(1), con.detach()))
    _bar(out, refs[0][0], refs[1][0], f"B {B} reg")
    _bar(cd, refs[0][1], refs[1][1], f"B {B} reg rows")


def test_argument_errors():
    x = torch.zeros(64, 256, device=DEV)
    for H in (0, 65):
        with pytest.raises(RuntimeError, match="hyper_num: 1..64"):
            _lib.call("gmr_lgm_dh", 8, ptr(x), ptr(x), 256, ptr(x), H, None, 0, None, None, 0, 1.0, TAU, ptr(x), 256,
                      0, stream())
        assert b"hyper_num" in _lib.load().gmr_last_error_string()
        assert _lib.load().gmr_lgm_lat_ws_floats(100, H) == 0
    assert _lib.load().gmr_lgm_lat_ws_floats(100, 4) == -(-100 // _lib.load().gmr_lgm_tile_rows()) * 8 * D
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.call("gmr_lgm_lat", 100, ptr(x), 256, 4, ptr(x), ptr(x), 256, ptr(x), 8, 0, ptr(x), stream())
