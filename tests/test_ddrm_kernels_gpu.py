"""The DDRM kernels of csrc/ddrm.hip by name, against the fp64 restatement of tests/ddrm_fixture.py: the fused
conditional-denoiser forward, the reverse chain and the row loss with its backward.

Bars: rtol 1e-5 against fp64, and next to it (sums of products cancel, so does x0 - out) an entry may be off by twice
the largest error of the same computation done by fp32 torch on the CPU against fp64, measured here (DESIGN section 2:
the rule for a bar that fp32 cannot hold)."""
import numpy as np
import pytest
import torch

import ddrm_fixture as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
T = 100
M = "item_reverse_model"
SCHED = F.schedule_ref(T, 1e-4, 5e-4, 5e-3)


def _lib():
    from gmr.utils import get_model
    get_model("DDRM")  # the feature under test: raises ValueError without it
    from gmr import _lib as lib
    return lib


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _stream():
    from gmr.kernels import stream
    return stream()


def R():
    return int(_lib().load().gmr_ddrm_tile_rows())


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _strided(a, pad):
    """a on the device as a view of a wider buffer (row stride = columns + pad), the pad filled with 7."""
    a = np.asarray(a)
    base = torch.full((a.shape[0], a.shape[1] + pad), 7, dtype=torch.as_tensor(a).dtype, device=DEV)
    base[:, :a.shape[1]] = dev(a)
    return base[:, :a.shape[1]]


def make_net(H, seed):
    """Random denoiser parameters (the restatement's names) and their device copies with the folded time table."""
    rng = np.random.default_rng(seed)
    P = {F.key(M + ".emb_layer.weight"): rng.standard_normal((64, 64)) * 0.12,
         F.key(M + ".emb_layer.bias"): rng.standard_normal(64) * 0.05,
         F.key(M + ".in_layers.0.weight"): rng.standard_normal((H, 192)) * 0.3,
         F.key(M + ".in_layers.0.bias"): rng.standard_normal(H) * 0.05,
         F.key(M + ".out_layers.0.weight"): rng.standard_normal((64, H)) * (0.8 / np.sqrt(H)),
         F.key(M + ".out_layers.0.bias"): rng.standard_normal(64) * 0.05}
    P = {k: v.astype(np.float32) for k, v in P.items()}

    def tens(dtype):
        return {n: torch.tensor(P[F.key(n)], dtype=dtype) for n in F.param_names() if n.startswith(M)}

    P64 = tens(torch.float64)
    emb = F.temb_ref(torch.arange(T), torch.float64) @ P64[M + ".emb_layer.weight"].T + P64[M + ".emb_layer.bias"]
    TB = emb @ P64[M + ".in_layers.0.weight"][:, 64:128].T + P64[M + ".in_layers.0.bias"]
    d = {"W1": dev(P[F.key(M + ".in_layers.0.weight")]), "W2": dev(P[F.key(M + ".out_layers.0.weight")]),
         "b2": dev(P[F.key(M + ".out_layers.0.bias")]), "TB": dev(TB.numpy().astype(np.float32))}
    return {"H": H, "tens": tens, "d": d}


def make_rows(N, seed, nx=23, nc=19):
    """N rows gathered (with duplicates) from an nx-row x table and an nc-row cond table, t with 0 and T - 1."""
    rng = np.random.default_rng(seed)
    c = {"X": (rng.standard_normal((nx, 64)) * 0.1).astype(np.float32),
         "C": (rng.standard_normal((nc, 64)) * 0.1).astype(np.float32),
         "ix": rng.integers(0, nx, N).astype(np.int32), "ic": rng.integers(0, nc, N).astype(np.int32),
         "t": rng.integers(0, T, N).astype(np.int32), "noise": rng.standard_normal((N, 64)).astype(np.float32),
         "keep": (rng.random((N, 64)) < 0.5).astype(np.uint8)}
    c["t"][0] = 0
    c["t"][-1] = T - 1
    if N > 2:
        c["ix"][1] = c["ix"][0]
        c["ic"][2] = c["ic"][0]
    return c


def fwd_ref(net, c, keep, dtype):
    P = net["tens"](dtype)
    t = torch.as_tensor(c["t"].astype(np.int64))
    x0 = torch.as_tensor(c["X"]).to(dtype)[c["ix"].astype(np.int64)]
    cond = torch.as_tensor(c["C"]).to(dtype)[c["ic"].astype(np.int64)]
    sa = F.f32_table(SCHED["sqrt_alphas_cumprod"], dtype)[t][:, None]
    s1 = F.f32_table(SCHED["sqrt_one_minus_alphas_cumprod"], dtype)[t][:, None]
    xt = sa * x0 + s1 * torch.as_tensor(c["noise"]).to(dtype)
    out, h, xd = F.dnn_ref(P, M, xt, cond, t, None if keep is None else torch.as_tensor(keep))
    return {"out": out.numpy(), "h": h.numpy(), "xd": xd.numpy(), "mse": ((x0 - out) ** 2).mean(1).numpy()}


def run_fwd(net, c, N, lo=0, noise=True, drop=None, keep=None, seed=5, step=0, row_off=None):
    """gmr_ddrm_denoise_fwd over rows lo..N of the case.  Returns out, h, xd, mse, keep_out (device)."""
    lib = _lib()
    H, d = net["H"], net["d"]
    n = N - lo
    X, C = _strided(c["X"], 8), _strided(c["C"], 16)
    ix, ic, t = dev(c["ix"][lo:N]), dev(c["ic"][lo:N]), dev(c["t"][lo:N])
    nz = _strided(c["noise"][lo:N], 4) if noise else None
    kp = _strided(keep[lo:N], 8) if keep is not None else None
    out, xd = _strided(np.zeros((n, 64), np.float32), 4), _strided(np.zeros((n, 64), np.float32), 12)
    h = _strided(np.zeros((n, H), np.float32), 4)
    ko = _strided(np.full((n, 64), 9, np.uint8), 8)
    mse = torch.full((n,), 7.0, device=DEV)
    sa, s1 = dev(SCHED["sqrt_alphas_cumprod"].astype(np.float32)), dev(SCHED["sqrt_one_minus_alphas_cumprod"].astype(np.float32))
    mode = {None: 0, "given": 1, "draw": 2}[drop]
    lib.call("gmr_ddrm_denoise_fwd", n, H, T, lo if row_off is None else row_off, _ptr(X), X.stride(0), _ptr(ix),
             _ptr(C), C.stride(0), _ptr(ic), _ptr(t), _ptr(sa), _ptr(s1), _ptr(nz), nz.stride(0) if noise else 0, mode,
             _ptr(kp), kp.stride(0) if kp is not None else 0, seed, step, 3, _ptr(d["W1"]), _ptr(d["TB"]),
             _ptr(d["W2"]), _ptr(d["b2"]), _ptr(out), out.stride(0), _ptr(xd), xd.stride(0), _ptr(ko), ko.stride(0),
             _ptr(h), h.stride(0), _ptr(mse), _stream())
    torch.cuda.synchronize()
    for v in (out, xd, h):
        assert float(v._base[:, v.shape[1]:].min()) == 7.0  # nothing written past a row
    return {"out": out, "h": h, "xd": xd, "mse": mse, "keep": ko}


def _bar(got, ref64, ref32, what):
    own = float(np.abs(ref32.astype(np.float64) - ref64).max())
    got = got.cpu().numpy().astype(np.float64)
    print(f"{what}: max abs error {np.abs(got - ref64).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(got, ref64, rtol=1e-5, atol=2 * own, err_msg=what)


# ----------------------------------------------------------------------------- fused forward
NETS = {}


def net_for(H):
    if H not in NETS:
        NETS[H] = make_net(H, 100 + H)
    return NETS[H]


@pytest.mark.parametrize("H", [300, 64, 20])
@pytest.mark.parametrize("nrel", ["1", "R-1", "R", "R+1", "2R+3"])
def test_fwd_against_fp64(H, nrel):
    r = R()
    N = {"1": 1, "R-1": r - 1, "R": r, "R+1": r + 1, "2R+3": 2 * r + 3}[nrel]
    net, c = net_for(H), make_rows(N, 7 * N + H)
    for drop, keep in (("given", c["keep"]), (None, None)):
        got = run_fwd(net, c, N, drop=drop, keep=keep)
        r64, r32 = fwd_ref(net, c, keep, torch.float64), fwd_ref(net, c, keep, torch.float32)
        for k in ("xd", "h", "out", "mse"):
            _bar(got[k], r64[k], r32[k], f"fwd N={N} H={H} drop={drop} {k}")
        if drop == "given":
            assert np.array_equal(got["xd"].cpu().numpy() == 0, (c["keep"] == 0) | (r64["xd"] == 0))
        assert float(got["keep"].min()) == 9  # keep_out is written only for drawn masks


def test_fwd_philox_draws():
    N, H = 1600, 20   # 102,400 elements
    net, c = net_for(H), make_rows(1600, 3)
    a = run_fwd(net, c, N, noise=False, drop="draw", seed=11, step=4)
    b = run_fwd(net, c, N, noise=False, drop="draw", seed=11, step=4)
    o = run_fwd(net, c, N, noise=False, drop="draw", seed=11, step=5)
    for k in ("out", "h", "xd", "mse", "keep"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["keep"], o["keep"]) and not torch.equal(a["xd"], o["xd"])
    keep = a["keep"].cpu().numpy()
    assert set(np.unique(keep)) == {0, 1}
    n = keep.size
    assert n >= 100000 and abs(keep.mean() - 0.5) <= 4 * np.sqrt(0.25 / n), keep.mean()
    assert abs(keep.mean(0) - 0.5).max() < 0.08  # every column draws
    assert np.array_equal(a["xd"].cpu().numpy() == 0, keep == 0)
    # the noise alone: xd = sa x0 + s1 n without dropout
    z = run_fwd(net, c, N, noise=False, drop=None, seed=11, step=4)["xd"].cpu().numpy().astype(np.float64)
    sa = SCHED["sqrt_alphas_cumprod"].astype(np.float32)[c["t"]][:, None].astype(np.float64)
    s1 = SCHED["sqrt_one_minus_alphas_cumprod"].astype(np.float32)[c["t"]][:, None].astype(np.float64)
    ok = c["t"] > 0  # at t = 0 the noise term is 3e-3 of the row and fp32 keeps few of its digits
    nz = ((z - sa * c["X"][c["ix"]]) / s1)[ok]
    assert abs(nz.mean()) <= 4 / np.sqrt(nz.size) and abs(nz.std() - 1) < 0.02, (nz.mean(), nz.std())
    assert np.array_equal(a["xd"].cpu().numpy()[keep == 1], (2 * z.astype(np.float32))[keep == 1])


@pytest.mark.parametrize("H", [300, 20])
def test_fwd_rows_do_not_depend_on_neighbours(H):
    r = R()
    N = 2 * r + 3
    net, c = net_for(H), make_rows(N, 9)
    full = run_fwd(net, c, N, noise=False, drop="draw", seed=21, step=2)
    for a in (5, r + 1):
        part = run_fwd(net, c, N, lo=a, noise=False, drop="draw", seed=21, step=2)
        for k in ("out", "h", "xd", "mse", "keep"):
            assert torch.equal(part[k], full[k][a:]), (a, k)


def test_fwd_rejects_width():
    lib = _lib()
    x = torch.zeros((4, 64), device=DEV)
    t = torch.zeros(4, dtype=torch.int32, device=DEV)
    for H in (0, 22, 1028):
        with pytest.raises(RuntimeError, match="hidden width"):
            lib.call("gmr_ddrm_denoise_fwd", 4, H, T, 0, _ptr(x), 64, None, _ptr(x), 64, None, _ptr(t), _ptr(x), _ptr(x),
                     None, 0, 0, None, 0, 0, 0, 0, _ptr(x), _ptr(x), _ptr(x), _ptr(x), _ptr(x), 64, None, 0, None, 0,
                     None, 0, None, _stream())


# ----------------------------------------------------------------------------- chain
def run_chain(net, xs, cond, ic, S, lo=0, step_noise=None, sigma=False, noise0=None, seed=5, step=1):
    lib = _lib()
    H, d = net["H"], net["d"]
    N = xs.shape[0]
    n = N - lo
    X, C = _strided(xs[lo:], 4), _strided(cond, 8)
    out = _strided(np.zeros((n, 64), np.float32), 4)
    f32 = lambda k: dev(SCHED[k].astype(np.float32))  # noqa: E731
    sg = dev(np.exp(0.5 * SCHED["posterior_log_variance_clipped"].astype(np.float32)).astype(np.float32))
    sn = dev(step_noise[:, lo:]) if step_noise is not None else None
    n0 = dev(noise0[lo:]) if noise0 is not None else None
    qa, qb = float(np.float32(SCHED["sqrt_alphas_cumprod"][-1])), float(np.float32(SCHED["sqrt_one_minus_alphas_cumprod"][-1]))
    icd, c1, c2 = dev(ic[lo:]), f32("posterior_mean_coef1"), f32("posterior_mean_coef2")  # held until the sync
    lib.call("gmr_ddrm_chain", n, H, T, S, lo, _ptr(X), X.stride(0), _ptr(n0), 64, qa, qb, _ptr(C), C.stride(0),
             _ptr(icd), _ptr(d["W1"]), _ptr(d["TB"]), _ptr(d["W2"]), _ptr(d["b2"]), _ptr(c1), _ptr(c2),
             _ptr(sg) if (sigma or sn is not None) else None, _ptr(sn), seed, step, 2, _ptr(out), out.stride(0), _stream())
    torch.cuda.synchronize()
    assert float(out._base[:, 64:].min()) == 7.0
    return out


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("S", [0, 1, 3, T])
@pytest.mark.parametrize("nrel", ["1", "R+1"])
def test_chain_against_fp64(nrel, S, noisy):
    N = 1 if nrel == "1" else R() + 1
    net = net_for(300)
    rng = np.random.default_rng(S + 10 * N)
    xs = (rng.standard_normal((N, 64)) * 0.1).astype(np.float32)
    cond = (rng.standard_normal((11, 64)) * 0.1).astype(np.float32)
    ic = rng.integers(0, 11, N).astype(np.int32)
    n0 = rng.standard_normal((N, 64)).astype(np.float32)
    sn = rng.standard_normal((S, N, 64)).astype(np.float32) if noisy and S else None
    got = run_chain(net, xs, cond, ic, S, step_noise=sn, noise0=n0)
    ref = {}
    for dt in (torch.float64, torch.float32):
        sa, s1 = F.f32_table(SCHED["sqrt_alphas_cumprod"], dt)[-1], F.f32_table(SCHED["sqrt_one_minus_alphas_cumprod"], dt)[-1]
        x = sa * torch.as_tensor(xs).to(dt) + s1 * torch.as_tensor(n0).to(dt)
        with torch.no_grad():
            ref[dt] = F.chain_ref(net["tens"](dt), x, torch.as_tensor(cond).to(dt)[ic.astype(np.int64)], S, SCHED,
                                  sn, dt).numpy()
    _bar(got, ref[torch.float64], ref[torch.float32], f"chain N={N} S={S} noisy={noisy}")
    if S == 0:  # a copy when no q_sample noise is given
        assert torch.equal(run_chain(net, xs, cond, ic, 0), dev(xs))


def test_chain_row_subset_and_philox():
    N = R() + 1
    net = net_for(300)
    rng = np.random.default_rng(2)
    xs = (rng.standard_normal((N, 64)) * 0.1).astype(np.float32)
    cond = (rng.standard_normal((N, 64)) * 0.1).astype(np.float32)
    ic = np.arange(N, dtype=np.int32)
    full = run_chain(net, xs, cond, ic, 3, sigma=True, seed=31, step=6)
    again = run_chain(net, xs, cond, ic, 3, sigma=True, seed=31, step=6)
    other = run_chain(net, xs, cond, ic, 3, sigma=True, seed=31, step=7)
    plain = run_chain(net, xs, cond, ic, 3)
    assert torch.equal(full, again) and not torch.equal(full, other) and not torch.equal(full, plain)
    part = run_chain(net, xs, cond, ic, 3, lo=3, sigma=True, seed=31, step=6)
    assert torch.equal(part, full[3:])
    # the drawn step noise is small against the row (sigma ~ 7e-5) but not nothing
    assert 1e-6 < float((full - plain).abs().max()) < 1e-2


# ----------------------------------------------------------------------------- row loss
def loss_case(B, seed):
    rng = np.random.default_rng(seed)
    U, I = 13, 17
    G = (rng.standard_normal((U + I, 64)) * 0.3).astype(np.float32)
    G[0] = 0
    G[0, 0] = 8          # user 0
    G[U:U + 3] = 0
    G[U, 0] = 5          # item 0: score +40 with user 0
    G[U + 1, 0] = -5     # item 1: score -40
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    special = [(0, 0, 1), (0, 1, 0), (0, 2, 2)]   # (pos, neg) scores (40, -40), (-40, 40), (0, 0)
    for b, (u, p, n) in enumerate(special[:B]):
        users[b], pos[b], neg[b] = u, p, n
    if B > 8:
        users[5] = users[6] = users[4]
        pos[7] = pos[6]
        neg[8] = neg[4]
    out_u = (G[users] + rng.standard_normal((B, 64)) * 0.05).astype(np.float32)
    out_i = (G[U + pos] + rng.standard_normal((B, 64)) * 0.05).astype(np.float32)
    return U, G, users.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32), out_u, out_i, np.float32(0.37)


def loss_ref(case, alpha, beta, rw, dtype):
    U, G, users, pos, neg, out_u, out_i, reg = case
    g = torch.as_tensor(G).to(dtype)
    leaf = lambda a: a.clone().requires_grad_(True)  # noqa: E731
    u, p, n = leaf(g[users.astype(np.int64)]), leaf(g[U + pos.astype(np.int64)]), leaf(g[U + neg.astype(np.int64)])
    ou, oi = leaf(torch.as_tensor(out_u).to(dtype)), leaf(torch.as_tensor(out_i).to(dtype))
    rg = torch.tensor(float(reg), dtype=dtype, requires_grad=True)
    loss, w, sp, rec = F.row_loss_ref(u, p, n, ou, oi, rg, alpha, beta, rw)
    gr = torch.autograd.grad(loss, [u, p, n, ou, oi, rg], allow_unused=True)
    z = lambda x, like: (torch.zeros_like(like) if x is None else x).numpy()  # noqa: E731
    lb = (w * ((1 - alpha) * (sp + rw * rg) + alpha * rec)).detach().numpy()
    return {"loss": loss.item(), "w": w.numpy(), "sp": sp.detach().numpy(), "rec": rec.detach().numpy(), "lb": lb,
            "contrib": np.concatenate([z(gr[0], u), z(gr[1], p), z(gr[2], n)]), "dou": z(gr[3], ou),
            "doi": z(gr[4], oi), "coef": float(z(gr[5], rg)),
            "mse_u": ((u - ou) ** 2).mean(1).detach().numpy(), "mse_i": ((p - oi) ** 2).mean(1).detach().numpy()}


def run_loss(case, alpha, beta, rw, mse_u, mse_i):
    lib = _lib()
    U, G, users, pos, neg, out_u, out_i, reg = case
    B = len(users)
    Gd, ou, oi = _strided(G, 8), _strided(out_u, 4), _strided(out_i, 12)
    terms, loss = torch.full((4, B), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)
    contrib = _strided(np.zeros((3 * B, 64), np.float32), 4)
    dou, doi = torch.empty((B, 64), device=DEV), torch.empty((B, 64), device=DEV)
    ud, pd, nd = dev(users), dev(pos), dev(neg)  # held until the sync
    mu, mi, rg = dev(mse_u.astype(np.float32)), dev(mse_i.astype(np.float32)), dev(np.asarray([reg], np.float32))
    lib.call("gmr_ddrm_loss_fwd_bwd", B, U, _ptr(Gd), Gd.stride(0), _ptr(ud), _ptr(pd), _ptr(nd), _ptr(ou),
             ou.stride(0), _ptr(oi), oi.stride(0), _ptr(mu), _ptr(mi), _ptr(rg), alpha, beta, rw, 1.0 / B,
             _ptr(terms), _ptr(loss), _ptr(contrib), contrib.stride(0), _ptr(dou), _ptr(doi), _stream())
    torch.cuda.synchronize()
    assert float(contrib._base[:, 64:].min()) == 7.0 and float(loss[3]) == 7.0
    return {"terms": terms, "loss": loss, "contrib": contrib, "dou": dou, "doi": doi}


@pytest.mark.parametrize("alpha,beta", [(0.1, 0.1), (0.1, 1.0), (0.0, 0.1), (0.0, 1.0)])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_row_loss_against_fp64(B, alpha, beta):
    rw = 0.01
    case = loss_case(B, 40 + B)
    r64, r32 = loss_ref(case, alpha, beta, rw, torch.float64), loss_ref(case, alpha, beta, rw, torch.float32)
    got = run_loss(case, alpha, beta, rw, r64["mse_u"], r64["mse_i"])
    again = run_loss(case, alpha, beta, rw, r64["mse_u"], r64["mse_i"])
    for k in got:
        assert torch.equal(got[k], again[k]), k
    terms = got["terms"].cpu().numpy().astype(np.float64)
    assert np.isfinite(terms).all()
    U, G, users, pos, neg = case[:5]
    ps = (G[users].astype(np.float64) * G[U + pos]).sum(1)
    assert ps[0] == 40 and (B < 3 or (ps[1] == -40 and ps[2] == 0))
    for i, k in enumerate(("w", "sp", "rec", "lb")):
        np.testing.assert_allclose(terms[i], r64[k], rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(float(got["loss"][0]), r64["loss"], rtol=1e-5)
    np.testing.assert_allclose(float(got["loss"][1]), r64["coef"], rtol=1e-5)
    np.testing.assert_allclose(float(got["loss"][2]), r64["coef"] / B, rtol=1e-5)
    for k in ("contrib", "dou", "doi"):
        _bar(got[k], r64[k], r32[k], f"loss B={B} alpha={alpha} beta={beta} {k}")
