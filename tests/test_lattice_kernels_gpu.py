"""The LATTICE graph kernels (csrc/lattice.hip) by name against a plain torch statement of what each computes, in
fp64 with autograd: rtol 1e-5 against fp64 with an atol of twice fp32 torch's own error (test_mgcn_kernels_gpu's
bar), measured here and printed.  Shapes: I in {1, k, 63, 65, 257} x k in {1, 5, 10} x M in {1, 2} (no launch is
capped: every grid grows with I), tables with a row stride above 64 and NaN outside their columns.  Constructed cases:
lists that share columns, an item nobody lists, a hub every row lists in both modalities (its incoming list is
longer than a wave's trip), a row whose sum is exactly 0, equal modal weights, bad arguments; two runs give the same
bits."""
import functools

import numpy as np
import pytest
import torch

from lattice_fixture import DEV, bar

pytestmark = pytest.mark.gpu

LD, LAM = 80, 0.7
SHAPES = [(I, k, M) for k in (1, 5, 10) for I in sorted({1, k, 63, 65, 257}) for M in (1, 2)]
OUTS = {"gmr_lat_edge_fwd": ("v", "r", "s", "col"), "gmr_lat_adj_fwd": ("val",), "gmr_lat_sddmm": ("dA", "dA2"),
        "gmr_lat_bwd_ds": ("dr",), "gmr_lat_bwd_da": ("dv", "parts"), "gmr_lat_dw_reduce": ("dmw",),
        "gmr_lat_bwd_dn": ("dn",)}


def make_data(I, k, M, kind="random"):
    rng = np.random.default_rng(1000 * I + 10 * k + M)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    n = [np.abs(rng.standard_normal((I, 64))) + 0.05 for _ in range(M)]  # positive rows: every row sum is positive
    n = [f32(x / np.linalg.norm(x, axis=1, keepdims=True)) for x in n]
    if I == 1:
        # one item: L is the constant 1 - lambda (I = k = M = 1) or depends on the weights alone, and the backward is
        # a difference of equal terms.  fp32 torch returns exactly 0 there when v rounds to 1, so "twice its error" is
        # no bar at all; four entries of 0.5 make v = 1 exact in every summation order, for torch and for the kernel
        n = [np.zeros((1, 64), np.float32) for _ in range(M)]
        for x in n:
            x[0, rng.choice(64, 4, replace=False)] = 0.5
    pick = lambda hi: np.stack([rng.choice(hi, k, replace=hi < k) for _ in range(I)])  # noqa: E731
    hi = I - 1 if kind == "unlisted" and I > 1 else I
    idx = [pick(hi) for _ in range(M)]
    if kind == "shared" and M == 2:
        idx[1][:] = idx[0]                      # every row's image and text lists share all their columns
    if kind == "hub":
        for x in idx:
            x[:, 0] = 0                         # item 0 in every row, in both modalities
    d = {"I": I, "k": k, "M": M, "n": n, "idx": [x.astype(np.int32) for x in idx],
         "mw": f32([0.3, 0.3] if kind == "equal" else rng.standard_normal(2)),
         "oidx": rng.integers(0, I, (I, M * k)).astype(np.int32), "oval": f32(rng.random((I, M * k)) + 0.1),
         "g": f32(rng.standard_normal((I, 64))), "h": f32(rng.standard_normal((I, 64))),
         "h2": f32(rng.standard_normal((I, 64))), "dA_up": f32(rng.standard_normal((I, 2 * M * k)))}
    if kind == "rzero":
        assert (I, k) == (3, 2)
        e = np.eye(64, dtype=np.float32)
        d["n"] = [np.stack([e[0], -e[0], e[1]]) for _ in range(M)]     # unnormalised on purpose
        d["idx"] = [np.asarray([[0, 1], [1, 2], [2, 0]], np.int32) for _ in range(M)]
        d["mw"] = f32([0.2, 0.2])
    return d


def _s_of(r):
    zero = r == 0
    return torch.where(zero, torch.zeros_like(r), torch.where(zero, torch.ones_like(r), r).pow(-0.5))


def reference(d, dtype):
    """Every kernel's outputs in plain torch at `dtype` ({name: numpy})."""
    I, k, M = d["I"], d["k"], d["M"]
    Mk = M * k
    t = lambda a: torch.tensor(a, dtype=dtype)  # noqa: E731
    idx = [torch.as_tensor(x.astype(np.int64)) for x in d["idx"]]
    n = [t(x).requires_grad_() for x in d["n"]]
    oval, dA_up = t(d["oval"]), t(d["dA_up"])
    mw = t(d["mw"]).requires_grad_()
    w = torch.softmax(mw, 0) if M == 2 else [torch.ones((), dtype=dtype)]
    v = [(n[m][:, None, :] * n[m][idx[m]]).sum(-1) for m in range(M)]
    vl = [x.detach().clone().requires_grad_() for x in v]

    def values(r_leaf=None):
        a = [w[m] * vl[m] for m in range(M)]
        r = sum(x.sum(-1) for x in a) if r_leaf is None else r_leaf
        s = _s_of(r)
        val = torch.cat([(1 - LAM) * (s[:, None] * a[m] * s[idx[m]]) for m in range(M)] +
                        [LAM * (w[m] * oval[:, m * k:(m + 1) * k]) for m in range(M)], dim=1)
        return val, r, s

    val, r, s = values()
    leaves = vl + ([mw] if M == 2 else [])
    grads = torch.autograd.grad((val * dA_up).sum(), leaves, retain_graph=True)
    dv = list(grads[:M])
    rl = r.detach().clone().requires_grad_()
    dr, = torch.autograd.grad((values(rl)[0] * dA_up).sum(), [rl], retain_graph=True)
    dn = torch.autograd.grad(sum((v[m] * dv[m]).sum() for m in range(M)), n)
    da = [dv[m] / w[m].detach() for m in range(M)]
    parts = torch.zeros((I, 2), dtype=dtype)
    for m in range(M):
        parts[:, m] = (da[m] * vl[m].detach()).sum(-1) + LAM * (oval[:, m * k:(m + 1) * k] *
                                                             dA_up[:, Mk + m * k:Mk + (m + 1) * k]).sum(-1)
    col = torch.cat(idx + [torch.as_tensor(d["oidx"].astype(np.int64))], dim=1)
    g, h, h2 = t(d["g"]), t(d["h"]), t(d["h2"])
    dA = (g[:, None, :] * h[col]).sum(-1)
    out = {"v": torch.cat(vl, 1), "r": r, "s": s, "col": col[:, :Mk], "val": val, "dA": dA,
           "dA2": dA + (g[:, None, :] * h2[col]).sum(-1), "dr": dr, "dv": torch.cat(dv, 1), "parts": parts,
           "dn": torch.cat(dn, 1)}
    if M == 2:
        out["dmw"] = grads[M]
    return {k_: x.detach().numpy() for k_, x in out.items()}


def _table(blocks):
    """[I x 64] * M as the column blocks of one NaN-filled I x (M LD) buffer: row stride above 64."""
    I, M = blocks[0].shape[0], len(blocks)
    buf = torch.full((I, M * LD), float("nan"), device=DEV)
    for m, b in enumerate(blocks):
        buf[:, LD * m:LD * m + 64] = torch.as_tensor(b).to(DEV)
    return buf, [buf[:, LD * m:LD * m + 64] for m in range(M)]


def run_device(d):
    """Every kernel once, in the model's order ({name: device tensor})."""
    from gmr import _lib
    from gmr.kernels import ptr, stream
    from gmr.lattice import incoming_lists
    I, k, M = d["I"], d["k"], d["M"]
    Mk, R = M * k, 2 * M * k
    dev = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    f = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
    nbuf, n = _table(d["n"])
    idx = [dev(x) for x in d["idx"]]
    mw, oval, dA_up = dev(d["mw"]), dev(d["oval"]), dev(d["dA_up"])
    mwp = ptr(mw) if M == 2 else None
    ldc = R + 3
    col = torch.full((I, ldc), -1, dtype=torch.int32, device=DEV)
    col[:, Mk:R] = dev(d["oidx"])
    v, r, s, val = f(I, Mk), f(I), f(I), f(I, R)
    n1, i1 = n[M - 1], idx[M - 1]
    _lib.call("gmr_lat_edge_fwd", I, k, M, ptr(n[0]), n[0].stride(0), ptr(idx[0]), k, ptr(n1), n1.stride(0), ptr(i1), k,
              mwp, ptr(v), ptr(col), ldc, ptr(r), ptr(s), stream())
    _lib.call("gmr_lat_adj_fwd", I, k, M, ptr(v), ptr(s), ptr(col), ldc, ptr(oval), mwp, LAM, ptr(val), stream())
    gbuf, (g, h, h2) = _table([d["g"], d["h"], d["h2"]])
    dA, dA2 = f(I, R), f(I, R)
    for out, src, acc in ((dA, h, 0), (dA2, h, 0), (dA2, h2, 1)):
        _lib.call("gmr_lat_sddmm", I, R, ptr(col), ldc, ptr(g), g.stride(0), ptr(src), src.stride(0), acc, ptr(out),
                  stream())
    in_ptr, in_edge = incoming_lists(col[:, :Mk], M, k)
    dr, dv, parts, dmw = f(I), f(I, Mk), f(I, 2), f(2)
    _lib.call("gmr_lat_bwd_ds", I, k, M, ptr(dA_up), ptr(v), ptr(r), ptr(s), ptr(col), ldc, ptr(in_ptr), ptr(in_edge),
              mwp, LAM, ptr(dr), stream())
    _lib.call("gmr_lat_bwd_da", I, k, M, ptr(dA_up), ptr(v), ptr(s), ptr(dr), ptr(col), ldc, ptr(oval), mwp, LAM,
              ptr(dv), ptr(parts), stream())
    if M == 2:
        _lib.call("gmr_lat_dw_reduce", I, ptr(parts), ptr(mw), ptr(dmw), stream())
    dnbuf, dn = _table([np.full((I, 64), np.nan, np.float32)] * M)
    _lib.call("gmr_lat_bwd_dn", I, k, M, ptr(dv), ptr(n[0]), n[0].stride(0), ptr(n1), n1.stride(0), ptr(col), ldc,
              ptr(in_ptr), ptr(in_edge), ptr(dn[0]), dn[0].stride(0), ptr(dn[M - 1]), dn[M - 1].stride(0), stream())
    torch.cuda.synchronize()
    assert torch.isnan(dnbuf[:, 64:LD]).all() and (col[:, R:] == -1).all()  # nothing outside the columns is written
    out = {"v": v, "r": r, "s": s, "col": col[:, :Mk], "val": val, "dA": dA, "dA2": dA2, "dr": dr, "dv": dv,
           "parts": parts if M == 2 else torch.cat([parts[:, :1], torch.zeros_like(parts[:, :1])], 1),
           "dn": torch.cat(dn, 1), "in_ptr": in_ptr}
    if M == 2:
        out["dmw"] = dmw
    return out


@functools.lru_cache(maxsize=None)
def case(I, k, M, kind="random"):
    d = make_data(I, k, M, kind)
    return d, run_device(d), reference(d, torch.float64), reference(d, torch.float32)


def _check(name, I, k, M, kind="random"):
    d, got, r64, r32 = case(I, k, M, kind)
    for key in OUTS[name]:
        if key == "dmw" and M == 1:
            continue
        what = f"{name} {key} I={I} k={k} M={M} {kind}"
        if key == "col":
            assert np.array_equal(got[key].cpu().numpy(), r64[key]), what
        else:
            bar(got[key], r64[key], r32[key], what)


# the softmax backward exists with two modalities only
@pytest.mark.parametrize("name,I,k,M", [(name, *sh) for name in OUTS for sh in SHAPES
                                        if not (name == "gmr_lat_dw_reduce" and sh[2] == 1)])
def test_kernel(name, I, k, M):
    _check(name, I, k, M)


@pytest.mark.parametrize("name", list(OUTS))
@pytest.mark.parametrize("kind", ["shared", "unlisted", "hub"])
def test_constructed(name, kind):
    _check(name, 257, 5, 2, kind)
    d, got, *_ = case(257, 5, 2, kind)
    cnt = np.diff(got["in_ptr"].cpu().numpy())
    if kind == "unlisted":
        assert cnt[256] == 0 and cnt[257 + 256] == 0       # nobody lists the last item
    if kind == "hub":
        assert cnt[0] >= 257 and cnt[257] >= 257           # every row lists item 0: more than a wave's 64 lanes
    if kind == "shared":
        assert np.array_equal(d["idx"][0], d["idx"][1])


@pytest.mark.parametrize("M", [1, 2])
def test_zero_row_sum(M):
    """n_0 = e_1, n_1 = -e_1, idx_0 = {0, 1}: r_0 is exactly 0, so s_0 = 0, the learned part of row 0 is 0 and its dr
    is 0; nothing is NaN."""
    d, got, r64, r32 = case(3, 2, M, "rzero")
    assert got["r"][0].item() == 0.0 and got["s"][0].item() == 0.0 and got["dr"][0].item() == 0.0
    assert (got["val"][0, :M * 2] == 0).all()
    for key, x in got.items():
        if x.is_floating_point():
            assert torch.isfinite(x).all(), key
    for name in OUTS:
        _check(name, 3, 2, M, "rzero")


def test_equal_modal_weights_give_exact_halves():
    d, got, *_ = case(65, 5, 2, "equal")
    want = np.float32(LAM) * (np.float32(0.5) * d["oval"])
    assert np.array_equal(got["val"][:, 10:].cpu().numpy(), want)


@pytest.mark.parametrize("I,k,M,kind", [(257, 10, 2, "random"), (257, 5, 2, "hub"), (63, 5, 1, "random")])
def test_two_runs_give_the_same_bits(I, k, M, kind):
    d, got, *_ = case(I, k, M, kind)
    again = run_device(d)
    for key, x in got.items():
        assert torch.equal(x, again[key]), key


def test_bad_arguments_raise():
    from gmr import _lib
    from gmr.kernels import ptr, stream
    I, k, M = 8, 2, 2
    d = make_data(I, k, M)
    nbuf, n = _table(d["n"])
    idx = [torch.as_tensor(x).to(DEV) for x in d["idx"]]
    z = torch.zeros((I, 64), device=DEV)
    zi = torch.zeros((I, 64), dtype=torch.int32, device=DEV)

    def edge(k=k, M=M, ldn=n[0].stride(0), v=z, ldc=8, n0=n[0], mw=z):
        _lib.call("gmr_lat_edge_fwd", I, k, M, ptr(n0), ldn, ptr(idx[0]), 2, ptr(n[1]), n[1].stride(0), ptr(idx[1]), 2,
                  ptr(mw), ptr(v), ptr(zi), ldc, ptr(z), ptr(z), stream())

    edge()
    for bad in (dict(k=65), dict(k=0), dict(M=3), dict(ldn=60), dict(ldn=66), dict(v=None), dict(ldc=3),
                dict(n0=nbuf[:, 1:65]), dict(mw=None)):
        with pytest.raises(RuntimeError, match="gmr_lat_edge_fwd"):
            edge(**bad)
    with pytest.raises(RuntimeError, match="gmr_lat_adj_fwd"):
        _lib.call("gmr_lat_adj_fwd", I, k, M, ptr(z), ptr(z), ptr(zi), 3, ptr(z), ptr(z), LAM, ptr(z), stream())
    with pytest.raises(RuntimeError, match="gmr_lat_sddmm"):
        _lib.call("gmr_lat_sddmm", I, 8, ptr(zi), 64, ptr(z), 60, ptr(z), 64, 0, ptr(z), stream())
    with pytest.raises(RuntimeError, match="gmr_lat_sddmm"):
        _lib.call("gmr_lat_sddmm", 0, 8, ptr(zi), 64, ptr(z), 64, ptr(z), 64, 0, ptr(z), stream())
    with pytest.raises(RuntimeError, match="gmr_lat_bwd_ds"):
        _lib.call("gmr_lat_bwd_ds", I, k, M, ptr(z), ptr(z), ptr(z), ptr(z), ptr(zi), 64, None, ptr(zi), ptr(z), LAM,
                  ptr(z), stream())
    with pytest.raises(RuntimeError, match="gmr_lat_bwd_da"):
        _lib.call("gmr_lat_bwd_da", I, 65, M, ptr(z), ptr(z), ptr(z), ptr(z), ptr(zi), 64, ptr(z), ptr(z), LAM, ptr(z),
                  ptr(z), stream())
    with pytest.raises(RuntimeError, match="gmr_lat_dw_reduce"):
        _lib.call("gmr_lat_dw_reduce", I, ptr(z), None, ptr(z), stream())
    with pytest.raises(RuntimeError, match="gmr_lat_bwd_dn"):
        _lib.call("gmr_lat_bwd_dn", I, k, M, ptr(z), ptr(z), 64, ptr(z), 64, ptr(zi), 64, ptr(zi), ptr(zi), ptr(z), 64,
                  ptr(z), 62, stream())
