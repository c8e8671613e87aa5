"""The GRCN kernels of csrc/grcn.hip by name, against fp64 torch on random data.

Bar per output: the largest error against fp64 is at most twice the largest error of the same computation done by fp32
torch on the CPU on the same inputs; both are printed.  Node counts 1, 15, 17, 53 and 4,103 (a workgroup's second trip,
more rows than waves under a grid cap), split into users and items as tests/test_lgmrec_kernels_gpu.py does; the user
lists hold an empty row, a row of one neighbour (alpha is exactly 1 and ds exactly 0) and, where it fits, a row of 300
neighbours (more neighbours than lanes); n_layers in {0, 1, 3}; packed and padded strides with NaN outside the
columns; the default grid and a cap of 3 workgroups agree bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import grcn_fixture as F
from gmr import _lib
from gmr.kernels import ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64
NODES = [1, 15, 17, 53, 4103]
LAYERS = [0, 1, 3]
CAP = 3
SPLIT = {1: (0, 1), 15: (5, 10), 17: (6, 11), 53: (20, 33), 4103: (103, 4000)}   # N -> (U, I)


def _bar(got, ref64, ref32, what):
    got = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    ref64 = ref64.numpy() if torch.is_tensor(ref64) else np.asarray(ref64)
    ref32 = (ref32.numpy() if torch.is_tensor(ref32) else np.asarray(ref32)).astype(np.float64)
    assert np.isfinite(got).all(), what
    if got.size == 0:
        return
    err, own = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    print(f"{what}: max abs error {err:.3e} (fp32 torch {own:.3e})")
    assert err <= 2 * own, (what, err, own)


def _dev(a, pad=0):
    """A device copy; pad > 0 (2-D floats): rows `pad` floats further apart with NaN outside the columns."""
    a = torch.as_tensor(np.asarray(a))
    if not pad or a.dim() != 2:
        return a.to(DEV).contiguous()
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=a.dtype, device=DEV)
    v = buf[:, :a.shape[1]]
    v.copy_(a)
    return v


def _out(n, cols, pad=0):
    return torch.full((max(n, 1), cols + pad), float("nan"), device=DEV)[:n, :cols]


class Graph:
    """A user CSR with an empty row (the last), a row that holds item 1 alone (row 1) and, where it fits, a row of 300
    items (row 0); its CSC and the position maps, on the host (int64) and on the device (int32)."""

    def __init__(self, rng, U, I):
        lists = []
        for u in range(U):
            k = 300 if (u == 0 and I >= 300) else 0 if u == U - 1 else int(rng.integers(1, min(I, 9) + 1))
            lists.append(np.array([1]) if u == 1 else np.sort(rng.choice(I, k, replace=False)))
        self.U, self.I, self.N = U, I, U + I
        self.rp = np.zeros(U + 1, np.int64)
        self.rp[1:] = np.cumsum([len(r) for r in lists])
        self.cols = np.concatenate(lists).astype(np.int64) if U and self.rp[-1] else np.zeros(0, np.int64)
        self.rows = np.repeat(np.arange(U), np.diff(self.rp))
        E = self.E = len(self.cols)
        self.order = np.lexsort((self.rows, self.cols))          # csc2csr
        self.inv = np.empty(E, np.int64)
        self.inv[self.order] = np.arange(E)                      # csr2csc
        self.trp = np.zeros(I + 1, np.int64)
        np.cumsum(np.bincount(self.cols, minlength=I), out=self.trp[1:])
        self.tcol = self.rows[self.order]
        i32 = lambda a: _dev(np.concatenate([a, [0]]).astype(np.int32))  # noqa: E731  (never an empty tensor)
        self.d = {k: i32(getattr(self, k)) for k in ("rp", "cols", "trp", "tcol", "order", "inv")}
        self.args = (U, I, E, ptr(self.d["rp"]), ptr(self.d["cols"]), ptr(self.d["trp"]), ptr(self.d["tcol"]))
        self.maps = (ptr(self.d["inv"]), ptr(self.d["order"]))
        self.t = {k: torch.as_tensor(getattr(self, k)) for k in ("rows", "cols", "order", "inv", "tcol")}
        # the 2E directed edges in the kernels' layout: [user-destination, CSR order | item-destination, CSC order]
        self.dst = torch.cat([self.t["rows"], U + self.t["cols"][self.t["order"]]])
        self.src = torch.cat([U + self.t["cols"], self.t["tcol"]])


def _unit(rng, n, cols):
    x = rng.standard_normal((n, cols)).astype(np.float32)
    for b in range(cols // D):
        x[:, D * b:D * b + D] /= np.maximum(np.linalg.norm(x[:, D * b:D * b + D], axis=1, keepdims=True), 1e-12)
    return x


def _blocks(x, M, dtype):
    """The M 64-column blocks of a table at `dtype`."""
    t = torch.as_tensor(np.asarray(x)).to(dtype)
    return [t[:, D * m:D * m + D] for m in range(M)]


# ----------------------------------------------------------------------------- routing forward
def route_ref(P0, Fm, g, R, M, dtype):
    """(P tables (R + 1) x U x 64 M, nrmY R x M x U)."""
    rows, cols = g.t["rows"], g.t["cols"]
    tabs, nrm = [[] for _ in range(R + 1)], [[] for _ in range(R)]
    for p, f in zip(_blocks(P0, M, dtype), _blocks(Fm, M, dtype)):
        tabs[0].append(p)
        for r in range(R):
            h, _ = F.attend(p, f, rows, cols)
            y = p + h
            nrm[r].append(y.norm(dim=1).clamp_min(F.EPS))
            p = y / nrm[r][-1][:, None]
            tabs[r + 1].append(p)
    P = torch.stack([torch.cat(t, dim=1) for t in tabs])
    return P, (torch.stack([torch.stack(n) for n in nrm]) if R else torch.zeros((0, M, g.U), dtype=dtype))


def route_run(g, P0, Fm, R, M, pad=0, cap=0, messages=1):
    U = g.U
    P = torch.full((R + 1, max(U, 1), D * M + pad), float("nan"), device=DEV)
    P[0, :U, :D * M] = torch.as_tensor(P0)
    Fd = _dev(Fm, pad)
    nrm = torch.full((max(R, 1), M, max(U, 1)), float("nan"), device=DEV)[:, :, :U].contiguous()
    _lib.call("gmr_grcn_route_fwd", U, R, M, messages, ptr(g.d["rp"]), ptr(g.d["cols"]), ptr(Fd), Fd.stride(0), ptr(P),
              P.stride(1), P.stride(0), ptr(nrm), cap, stream())
    return P[:, :U, :D * M], nrm[:R]


def _inputs(N, M, seed, zero_row=True):
    U, I = SPLIT[N]
    rng = np.random.default_rng(seed)
    g = Graph(rng, U, I)
    P0, Fm = _unit(rng, U, D * M), _unit(rng, I, D * M)
    if zero_row and U > 2:
        P0[2] = 0.0           # a zero preference row: the norm is clamped, the scores are 0, alpha is uniform
    return rng, g, P0, Fm


@pytest.mark.parametrize("R", LAYERS)
@pytest.mark.parametrize("N", NODES)
def test_route_fwd(N, R):
    M = 1 if N == 17 else 2
    rng, g, P0, Fm = _inputs(N, M, 10 * N + R)
    pad = 4 * ((N + R) % 2)
    P, nrm = route_run(g, P0, Fm, R, M, pad=pad)
    (P64, n64), (P32, n32) = (route_ref(P0, Fm, g, R, M, dt) for dt in (torch.float64, torch.float32))
    assert torch.equal(P[0].cpu(), torch.as_tensor(P0))
    if g.U and R:
        _bar(P[1:], P64[1:], P32[1:], f"N {N} R {R}: p^1..p^R")
        _bar(nrm, n64, n32, f"N {N} R {R}: norms")
    P1, nrm1 = route_run(g, P0, Fm, R, M, pad=4 - pad, cap=CAP)
    assert torch.equal(P, P1) and torch.equal(nrm, nrm1)
    # without messages a round only normalises the row again
    P2, _ = route_run(g, P0, Fm, R, M, messages=0)
    want = torch.as_tensor(P0).double()
    for r in range(1, R + 1):
        for m in range(M):
            sl = slice(D * m, D * m + D)
            want[:, sl] = want[:, sl] / want[:, sl].norm(dim=1, keepdim=True).clamp_min(1e-12)
        np.testing.assert_allclose(P2[r].cpu().numpy(), want.numpy(), rtol=0, atol=1e-6)


# ----------------------------------------------------------------------------- final attention
def attn_ref(Pm, Fm, g, M, dtype):
    """(rep N x 64 M, alpha M x 2E)."""
    rows, cols, order = g.t["rows"], g.t["cols"], g.t["order"]
    reps, als = [], []
    for p, f in zip(_blocks(Pm, M, dtype), _blocks(Fm, M, dtype)):
        hu, a = F.attend(p, f, rows, cols)
        hi, b = F.attend(f, p, cols, rows)
        reps.append(torch.cat([p + hu, f + hi]))
        als.append(torch.cat([a, b[order]]))
    return torch.cat(reps, dim=1), torch.stack(als)


def attn_run(g, Pm, Fm, M, pad=0, cap=0):
    Pd, Fd = _dev(Pm, pad), _dev(Fm, pad)
    rep = _out(g.N, D * M, pad)
    alpha = torch.full((M, 2 * g.E + 1), float("nan"), device=DEV)[:, :2 * g.E].contiguous()
    _lib.call("gmr_grcn_attn_fwd", *g.args[:3], M, *g.args[3:], ptr(Pd), Pd.stride(0), ptr(Fd), Fd.stride(0), ptr(rep), rep.stride(0),
              ptr(alpha), cap, stream())
    return rep, alpha


@pytest.mark.parametrize("N", NODES)
def test_attn_fwd(N):
    M = 1 if N == 17 else 2
    rng, g, Pm, Fm = _inputs(N, M, 20 * N)
    pad = 4 * (N % 2)
    rep, alpha = attn_run(g, Pm, Fm, M, pad=pad)
    (r64, a64), (r32, a32) = (attn_ref(Pm, Fm, g, M, dt) for dt in (torch.float64, torch.float32))
    _bar(rep, r64, r32, f"N {N}: rep")
    _bar(alpha, a64, a32, f"N {N}: alpha")
    if g.U > 2:
        e0, e1 = g.rp[1], g.rp[2]
        assert e1 - e0 == 1 and bool((alpha[:, e0] == 1.0).all())                  # one neighbour: exactly 1
        z0, z1 = g.rp[2], g.rp[3]
        assert bool((alpha[:, z0:z1] == alpha[:, z0:z0 + 1]).all())                # the zero row: uniform
        np.testing.assert_allclose(alpha[:, z0].cpu().numpy(), 1.0 / (z1 - z0), rtol=1e-6)
    rep1, alpha1 = attn_run(g, Pm, Fm, M, pad=4 - pad, cap=CAP)
    assert torch.equal(rep, rep1) and torch.equal(alpha, alpha1)


# ----------------------------------------------------------------------------- refine
def _refine_inputs(rng, g, M):
    """alpha (M x 2E, in (0, 1]) and conf (N x M) with every margin of the fp64 values at least 1e-3."""
    alpha = rng.uniform(0.05, 1.0, (M, 2 * g.E)).astype(np.float32)
    conf = (rng.choice([-1.0, 1.0], (g.N, M)) * rng.uniform(1.0, 2.0, (g.N, M))).astype(np.float32)
    src = g.src.numpy()
    for _ in range(50):
        val = alpha.astype(np.float64).T * conf.astype(np.float64)[src]
        bad = np.abs(val[:, 0] - val[:, -1]) < 2e-3 if M == 2 else np.zeros(len(src), bool)
        if not bad.any():
            break
        alpha[1, bad] = np.minimum(alpha[1, bad] * np.float32(1.5), np.float32(4.0))
    return alpha, conf


def refine_ref(alpha, conf, g, M, dtype):
    a, c = torch.as_tensor(alpha).to(dtype), torch.as_tensor(conf).to(dtype)
    val = a.t() * c[g.src]
    mx, arg = val.max(dim=1)
    return torch.relu(mx), arg, val


def refine_run(g, alpha, conf, M, pad=0, cap=0):
    ad, cd = _dev(alpha), _dev(conf, pad)
    n2 = 2 * g.E + 1
    W, WT = torch.full((n2,), float("nan"), device=DEV), torch.full((n2,), float("nan"), device=DEV)
    arg = torch.full((n2,), -7, dtype=torch.int32, device=DEV)
    _lib.call("gmr_grcn_refine_fwd", *g.args[:3], M, *g.args[3:], *g.maps, ptr(ad), ptr(cd), cd.stride(0), ptr(W),
              ptr(WT), ptr(arg), cap, stream())
    return W[:2 * g.E], WT[:2 * g.E], arg[:2 * g.E]


@pytest.mark.parametrize("N", NODES)
def test_refine_fwd(N):
    M = 1 if N == 17 else 2
    U, I = SPLIT[N]
    rng = np.random.default_rng(30 * N)
    g = Graph(rng, U, I)
    alpha, conf = _refine_inputs(rng, g, M)
    w64, arg64, val64 = refine_ref(alpha, conf, g, M, torch.float64)
    w32, _, _ = refine_ref(alpha, conf, g, M, torch.float32)
    if g.E:   # the margins the exact comparison rests on
        assert float(val64.max(dim=1)[0].abs().min()) >= 1e-3
        assert M == 1 or float((val64[:, 0] - val64[:, 1]).abs().min()) >= 1e-3
    W, WT, arg = refine_run(g, alpha, conf, M, pad=(N % 2))
    assert np.array_equal((arg & 1).cpu().numpy(), arg64.numpy())                       # the argmax, every edge
    assert np.array_equal((arg < 2).cpu().numpy(), (val64.max(dim=1)[0] > 0).numpy())   # the sign, every edge
    assert bool((W[arg >= 2] == 0).all())
    _bar(W, w64, w32, f"N {N}: w")
    E = g.E
    Wc = W.cpu()
    want = torch.empty_like(Wc)
    want[E + g.t["inv"]] = Wc[:E]
    want[g.t["order"]] = Wc[E:]
    assert torch.equal(WT.cpu(), want)                                                  # the transposed positions
    if E:
        assert 0.1 < float((arg >= 2).float().mean()) < 0.9 and (M == 1 or 0.2 < float((arg & 1).float().mean()) < 0.8)
    W1, WT1, arg1 = refine_run(g, alpha, conf, M, pad=1 - (N % 2), cap=CAP)
    assert torch.equal(W, W1) and torch.equal(WT, WT1) and torch.equal(arg, arg1)


def refine_bwd_ref(alpha, conf, arg, dw, g, M, dtype):
    a, c, d = (torch.as_tensor(np.asarray(x)).to(dtype) for x in (alpha, conf, dw))
    arg = torch.as_tensor(arg).long()
    dal, dconf = torch.zeros_like(a), torch.zeros_like(c)
    for m in range(M):
        sel = (arg == m).to(dtype) * d
        dal[m] = sel * c[g.src, m]
        dconf[:, m].index_add_(0, g.src, sel * a[m])
    return dal, dconf


@pytest.mark.parametrize("N", NODES)
def test_refine_bwd(N):
    M = 1 if N == 17 else 2
    U, I = SPLIT[N]
    rng = np.random.default_rng(31 * N)
    g = Graph(rng, U, I)
    alpha, conf = _refine_inputs(rng, g, M)
    _, _, arg = refine_run(g, alpha, conf, M)
    dw = rng.standard_normal(2 * g.E).astype(np.float32)

    def run(pad, cap):
        ad, cd, dwd = _dev(alpha), _dev(conf, pad), _dev(np.concatenate([dw, [0]]).astype(np.float32))
        dal = torch.full((M, 2 * g.E + 1), float("nan"), device=DEV)[:, :2 * g.E].contiguous()
        dconf = _out(g.N, M, pad)
        argd = torch.cat([arg, arg.new_zeros(1)])
        _lib.call("gmr_grcn_refine_bwd", *g.args[:3], M, *g.args[3:], *g.maps, ptr(ad), ptr(cd), cd.stride(0), ptr(argd),
                  ptr(dwd), ptr(dal), ptr(dconf), dconf.stride(0), cap, stream())
        return dal, dconf

    dal, dconf = run(N % 2, 0)
    (a64, c64), (a32, c32) = (refine_bwd_ref(alpha, conf, arg.cpu(), dw, g, M, dt) for dt in (torch.float64, torch.float32))
    _bar(dal, a64, a32, f"N {N}: dalpha")
    _bar(dconf, c64, c32, f"N {N}: dconf")
    dal1, dconf1 = run(1 - N % 2, CAP)
    assert torch.equal(dal, dal1) and torch.equal(dconf, dconf1)


# ----------------------------------------------------------------------------- the sampled product
@pytest.mark.parametrize("N", NODES)
def test_dw(N):
    U, I = SPLIT[N]
    rng = np.random.default_rng(40 * N)
    g = Graph(rng, U, I)
    x, x1, dx1, gr = (rng.standard_normal((g.N, D)).astype(np.float32) for _ in range(4))

    def run(pad, cap):
        t = [_dev(a, pad) for a in (x, x1, dx1, gr)]
        dw = torch.full((2 * g.E + 1,), float("nan"), device=DEV)
        _lib.call("gmr_grcn_dw", *g.args, ptr(t[0]), t[0].stride(0), ptr(t[1]), t[1].stride(0), ptr(t[2]),
                  t[2].stride(0), ptr(t[3]), t[3].stride(0), ptr(dw), cap, stream())
        return dw[:2 * g.E]

    def ref(dtype):
        a, b, c, d = (torch.as_tensor(v).to(dtype) for v in (x, x1, dx1, gr))
        return (a[g.src] * c[g.dst]).sum(1) + (b[g.src] * d[g.dst]).sum(1)

    dw = run(4 * (N % 2), 0)
    _bar(dw, ref(torch.float64), ref(torch.float32), f"N {N}: dw")
    assert torch.equal(dw, run(4 - 4 * (N % 2), CAP))


# ----------------------------------------------------------------------------- attention backward
def attn_bwd_ref(Pm, Fm, alpha, dalpha, drep, g, M, dtype):
    """(ds M x 2E, dxd N x 64 M) of the destination pass."""
    rows, cols, order, U, E = g.t["rows"], g.t["cols"], g.t["order"], g.U, g.E
    al, dal = torch.as_tensor(alpha).to(dtype), torch.as_tensor(dalpha).to(dtype)
    dss, outs = [], []
    for m, (p, f, dh) in enumerate(zip(_blocks(Pm, M, dtype), _blocks(Fm, M, dtype), _blocks(drep, M, dtype))):
        parts = []
        for xd, xs, di, si, a, da, dhd in ((p, f, rows, cols, al[m, :E], dal[m, :E], dh[:U]),
                                           (f, p, cols[order], rows[order], al[m, E:], dal[m, E:], dh[U:])):
            t = (dhd[di] * xs[si]).sum(1) + da
            tbar = torch.zeros(xd.shape[0], dtype=dtype).index_add_(0, di, a * t)
            ds = a * (t - tbar[di])
            parts.append((ds, dhd + torch.zeros_like(xd).index_add_(0, di, ds[:, None] * xs[si])))
        dss.append(torch.cat([parts[0][0], parts[1][0]]))
        outs.append(torch.cat([parts[0][1], parts[1][1]]))
    return torch.stack(dss), torch.cat(outs, dim=1)


@pytest.mark.parametrize("N", NODES)
def test_attn_bwd_dst(N):
    M = 1 if N == 17 else 2
    rng, g, Pm, Fm = _inputs(N, M, 50 * N)
    _, alpha = attn_run(g, Pm, Fm, M)
    alpha = alpha.cpu().numpy()
    dalpha = rng.standard_normal((M, 2 * g.E)).astype(np.float32)
    drep = rng.standard_normal((g.N, D * M)).astype(np.float32)

    def run(pad, cap):
        Pd, Fd, dr = _dev(Pm, pad), _dev(Fm, pad), _dev(drep, pad)
        e = lambda a: _dev(np.concatenate([a, np.zeros((M, 1), np.float32)], axis=1))[:, :2 * g.E].contiguous()  # noqa: E731
        ad, dad = e(alpha), e(dalpha)
        ds = torch.full((M, 2 * g.E + 1), float("nan"), device=DEV)[:, :2 * g.E].contiguous()
        dxd = _out(g.N, D * M, pad)
        _lib.call("gmr_grcn_attn_bwd_dst", *g.args[:3], M, *g.args[3:], ptr(Pd), Pd.stride(0), ptr(Fd), Fd.stride(0),
                  ptr(ad), ptr(dad), ptr(dr), dr.stride(0), ptr(ds), ptr(dxd), dxd.stride(0), cap, stream())
        return ds, dxd

    ds, dxd = run(4 * (N % 2), 0)
    (s64, x64), (s32, x32) = (attn_bwd_ref(Pm, Fm, alpha, dalpha, drep, g, M, dt) for dt in (torch.float64, torch.float32))
    _bar(ds, s64, s32, f"N {N}: ds")
    _bar(dxd, x64, x32, f"N {N}: dxd")
    if g.U > 2:
        assert bool((ds[:, g.rp[1]] == 0.0).all())                                  # one neighbour: ds is exactly 0
    ds1, dxd1 = run(4 - 4 * (N % 2), CAP)
    assert torch.equal(ds, ds1) and torch.equal(dxd, dxd1)


def route_bwd_ref(P, nrmY, Fm, dpR, pref, nrm0, regtab, dense, g, R, M, dtype):
    """(RA, RD: R x M x E; DY: R x U x 64 M; dpref: U x 64 M)."""
    rows, cols, U = g.t["rows"], g.t["cols"], g.U
    Pt, nY, n0 = torch.as_tensor(P).to(dtype), torch.as_tensor(nrmY).to(dtype), torch.as_tensor(nrm0).to(dtype)
    RA, RD = torch.zeros((R, M, g.E), dtype=dtype), torch.zeros((R, M, g.E), dtype=dtype)
    DY, outs = torch.zeros((R, U, D * M), dtype=dtype), []
    for m, (f, dp, pf, rg) in enumerate(zip(_blocks(Fm, M, dtype), _blocks(dpR, M, dtype), _blocks(pref, M, dtype),
                                            _blocks(regtab, M, dtype))):
        sl = slice(D * m, D * m + D)
        for r in range(R - 1, -1, -1):
            dy = F.normalize_bwd(Pt[r + 1][:, sl], nY[r, m][:, None], dp)
            pr = Pt[r][:, sl]
            al = F.seg_softmax((pr[rows] * f[cols]).sum(1), rows, U)
            t = (dy[rows] * f[cols]).sum(1)
            ds = al * (t - torch.zeros(U, dtype=dtype).index_add_(0, rows, al * t)[rows])
            RA[r, m], RD[r, m], DY[r][:, sl] = al, ds, dy
            dp = dy + torch.zeros_like(dy).index_add_(0, rows, ds[:, None] * f[cols])
        outs.append(F.normalize_bwd(Pt[0][:, sl], n0[m][:, None], dp) + dense[m] * pf + rg)
    return RA, RD, DY, torch.cat(outs, dim=1)


@pytest.mark.parametrize("R", LAYERS)
@pytest.mark.parametrize("N", NODES[1:])
def test_route_bwd_dst(N, R):
    """The inputs are the forward kernel's own tables and norms, so both torch runs start from the same fp32 values; no
    zero preference row here (its gradient is the incoming one times 1e12 on both sides, which tests nothing)."""
    M = 1 if N == 17 else 2
    rng, g, _, Fm = _inputs(N, M, 60 * N + R, zero_row=False)
    U, E = g.U, g.E
    pref = (rng.standard_normal((U, D * M)) * 0.3).astype(np.float32)
    nrm0 = np.stack([np.linalg.norm(pref[:, D * m:D * m + D].astype(np.float64), axis=1) for m in range(M)]).astype(np.float32)
    P0 = np.concatenate([pref[:, D * m:D * m + D] / nrm0[m][:, None] for m in range(M)], axis=1).astype(np.float32)
    P, nrmY = route_run(g, P0, Fm, R, M)
    P, nrmY = P.cpu().numpy(), nrmY.cpu().numpy()
    dpR, regtab = (rng.standard_normal((U, D * M)).astype(np.float32) for _ in range(2))
    dense = [0.25, 0.0]

    def run(pad, cap):
        Pd = torch.full((R + 1, U, D * M + pad), float("nan"), device=DEV)
        Pd[:, :, :D * M] = torch.as_tensor(P)
        Fd, dpd, rgd, pfd = _dev(Fm, pad), _dev(dpR, pad), _dev(regtab, pad), _dev(pref)
        nY = _dev(np.concatenate([nrmY.reshape(-1), [0]]).astype(np.float32))
        RA, RD = (torch.full((max(R, 1) * M * E + 1,), float("nan"), device=DEV) for _ in range(2))
        DY = torch.full((max(R, 1), U, D * M), float("nan"), device=DEV)
        out = [_out(U, D, pad) for _ in range(M)]
        pf = [pfd[:, D * m:D * m + D] for m in range(M)]
        n0d = _dev(nrm0)
        _lib.call("gmr_grcn_route_bwd_dst", U, E, R, M, 1, ptr(g.d["rp"]), ptr(g.d["cols"]), ptr(Fd), Fd.stride(0), ptr(Pd),
                  Pd.stride(1), Pd.stride(0), ptr(nY), ptr(dpd), dpd.stride(0), ptr(RA), ptr(RD), ptr(DY), ptr(pf[0]),
                  ptr(pf[-1]), pfd.stride(0), ptr(n0d), ptr(rgd), rgd.stride(0), dense[0], dense[1], ptr(out[0]),
                  ptr(out[-1]), out[0].stride(0), cap, stream())
        return (RA[:R * M * E].view(R, M, E), RD[:R * M * E].view(R, M, E), DY[:R], torch.cat(out, dim=1))

    got = run(4 * ((N + R) % 2), 0)
    r64, r32 = (route_bwd_ref(P, nrmY, Fm, dpR, pref, nrm0, regtab, dense, g, R, M, dt)
                for dt in (torch.float64, torch.float32))
    for a, b, c, k in zip(got, r64, r32, ("alpha^r", "ds^r", "dy^r", "d preference")):
        if a.numel():
            _bar(a, b, c, f"N {N} R {R}: {k}")
    if R:
        assert bool((got[0][:, :, g.rp[1]] == 1.0).all()) and bool((got[1][:, :, g.rp[1]] == 0.0).all())
    for a, b in zip(got, run(4 - 4 * ((N + R) % 2), CAP)):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- the source pass
@pytest.mark.parametrize("N", NODES[1:])
def test_bwd_src(N):
    """Both uses: the users over their CSR rows with one term, the items over their CSC rows with four."""
    M = 1 if N == 17 else 2
    U, I = SPLIT[N]
    rng = np.random.default_rng(70 * N)
    g = Graph(rng, U, I)
    E = g.E
    for n, n_dst, ptr_k, idx_k, pos_k, idx_t, pos_t, T in ((U, I, "rp", "cols", "inv", g.t["cols"], g.t["inv"], 1),
                                                           (I, U, "trp", "tcol", "order", g.t["tcol"], g.t["order"], 4)):
        own = torch.as_tensor(np.repeat(np.arange(n), np.diff(getattr(g, ptr_k))))
        A, DS = (rng.standard_normal((T, M, E)).astype(np.float32) for _ in range(2))
        DH, XD = (rng.standard_normal((T, n_dst, D * M)).astype(np.float32) for _ in range(2))
        base = rng.standard_normal((n, D * M)).astype(np.float32)

        def run(pad, cap):
            Ad, DSd = (_dev(np.concatenate([a.reshape(-1), [0]]).astype(np.float32)) for a in (A, DS))
            DHd, XDd = [_dev(a, pad) for a in DH], [_dev(a, pad) for a in XD]
            out = _dev(base, pad)
            PA, LA = ctypes.c_void_p * T, ctypes.c_int64 * T
            fl = 4 * M * E
            _lib.call("gmr_grcn_bwd_src", n, M, T, ptr(g.d[ptr_k]), ptr(g.d[idx_k]), ptr(g.d[pos_k]),
                      PA(*[Ad.data_ptr() + fl * t for t in range(T)]), PA(*[DSd.data_ptr() + fl * t for t in range(T)]),
                      LA(*[E] * T), PA(*[a.data_ptr() for a in DHd]), LA(*[a.stride(0) for a in DHd]),
                      PA(*[a.data_ptr() for a in XDd]), LA(*[a.stride(0) for a in XDd]), ptr(out), out.stride(0), cap,
                      stream())
            return out

        def ref(dtype):
            out = torch.as_tensor(base).to(dtype).clone()
            for t in range(T):
                for m in range(M):
                    sl = slice(D * m, D * m + D)
                    a, d = torch.as_tensor(A[t, m]).to(dtype)[pos_t], torch.as_tensor(DS[t, m]).to(dtype)[pos_t]
                    dh, xd = torch.as_tensor(DH[t]).to(dtype)[:, sl], torch.as_tensor(XD[t]).to(dtype)[:, sl]
                    out[:, sl] += torch.zeros((n, D), dtype=dtype).index_add_(
                        0, own, a[:, None] * dh[idx_t] + d[:, None] * xd[idx_t])
            return out

        got = run(4 * (N % 2), 0)
        _bar(got, ref(torch.float64), ref(torch.float32), f"N {N}: {n} source rows, {T} terms")
        assert torch.equal(got, run(4 - 4 * (N % 2), CAP))


# ----------------------------------------------------------------------------- loss rows
def loss_ref(res, Eid, pref, users, pos, neg, U, M, inv, rw, dtype):
    r, e, p = (torch.as_tensor(x).to(dtype) for x in (res, Eid, pref))
    u, ps, ng = (torch.as_tensor(x).long() for x in (users, pos, neg))
    B, Wd = len(u), D * (1 + M)
    ru, rp, rn = r[u], r[U + ps], r[U + ng]
    s = (ru * (rp - rn)).sum(1)
    c = (-inv * torch.sigmoid(-s))[:, None]
    k1 = 1.0 / (128.0 * B)
    terms = torch.cat([-torch.log(torch.sigmoid(s)),
                       k1 * (2 * (e[u] ** 2).sum(1) + (e[U + ps] ** 2).sum(1) + (e[U + ng] ** 2).sum(1)
                             + 2 * (p[u] ** 2).sum(1))])
    z = torch.zeros((B, D * M), dtype=dtype)
    contrib = torch.cat([torch.cat([c * (rp - rn), 4 * k1 * rw * e[u], 4 * k1 * rw * p[u]], 1),
                         torch.cat([c * ru, 2 * k1 * rw * e[U + ps], z], 1),
                         torch.cat([-c * ru, 2 * k1 * rw * e[U + ng], z], 1)])
    assert contrib.shape[1] == Wd + D + D * M
    return terms, contrib


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_loss_rows(B, M):
    U, I = 20, 33
    rng = np.random.default_rng(80 + B + M)
    Wd, CW = D * (1 + M), D * (2 + 2 * M)
    res = rng.standard_normal((U + I, Wd)).astype(np.float32) * 0.4
    Eid = rng.standard_normal((U + I, D)).astype(np.float32)
    pref = rng.standard_normal((U, D * M)).astype(np.float32)
    users, pos, neg = (rng.integers(0, n, B).astype(np.int32) for n in (U, I, I))
    if B > 4:
        users[3], pos[4] = users[1], pos[2]
    inv, rw = 1.0 / B, 0.1

    def run(pad, cap):
        rd, ed, pd = _dev(res, pad), _dev(Eid, pad), _dev(pref, pad)
        ud, psd, ngd = _dev(users), _dev(pos), _dev(neg)
        terms = torch.full((2 * B,), float("nan"), device=DEV)
        contrib = _out(3 * B, CW, pad)
        _lib.call("gmr_grcn_loss_rows", B, U, M, ptr(rd), rd.stride(0), ptr(ed), ed.stride(0), ptr(pd),
                  ptr(pd[:, D * (M - 1):]), pd.stride(0), ptr(ud), ptr(psd), ptr(ngd), inv, rw,
                  ptr(terms), ptr(contrib), contrib.stride(0), cap, stream())
        return terms, contrib

    terms, contrib = run(4 * (B % 2), 0)
    (t64, c64), (t32, c32) = (loss_ref(res, Eid, pref, users, pos, neg, U, M, inv, rw, dt)
                              for dt in (torch.float64, torch.float32))
    _bar(terms, t64, t32, f"B {B} M {M}: terms")
    _bar(contrib, c64, c32, f"B {B} M {M}: contrib")
    t1, c1 = run(4 - 4 * (B % 2), 1)
    assert torch.equal(terms, t1) and torch.equal(contrib, c1)


def test_bad_arguments_raise():
    x = torch.zeros((8, 128), device=DEV)
    i = torch.zeros(16, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="modalities"):
        _lib.call("gmr_grcn_route_fwd", 4, 1, 3, 1, ptr(i), ptr(i), ptr(x), 128, ptr(x), 128, 1024, ptr(x), 0, stream())
    with pytest.raises(RuntimeError, match="n_layers"):
        _lib.call("gmr_grcn_route_fwd", 4, 8, 2, 1, ptr(i), ptr(i), ptr(x), 128, ptr(x), 128, 1024, ptr(x), 0, stream())
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("gmr_grcn_attn_fwd", 2, 2, 0, 2, ptr(i), ptr(i), ptr(i), ptr(i), ptr(x), 127, ptr(x), 128, ptr(x), 128,
                  ptr(x), 0, stream())
    assert _lib.load().gmr_grcn_max_layers() == 7 and _lib.load().gmr_grcn_max_blocks() >= CAP
