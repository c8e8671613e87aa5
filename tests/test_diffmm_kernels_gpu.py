"""The DiffMM rec-step row kernels and the batch plumbing of csrc/diffmm.hip (lines 1-936), every entry point called
by name through _lib.call against tests/diffmm_kernels_ref.py (fp64; autograd in double for the backward kernels; one
strict fp32 restatement of the sorted scatter; np.sort for the plan).

Outputs start as NaN in buffers that end with three sentinel rows (and, where the ABI takes a leading dimension, a
pad of sentinel columns); the sentinels are asserted untouched.  In-place and cleared buffers are checked for exactly
what was and was not written.

Bars, none of them tuned to a kernel:
  exact (bits)   sort_batch_keys against np.sort; scatter_sorted_f32 against the fp32 slot-order restatement;
                 gather_rows; dg; every cleared or untouched region; every kernel against a second run of itself;
                 the fused forms against the separate launches they replaced (final_bwd2 / final_bwd / cl_bwd,
                 cl_bwd2 / cl_bwd, assemble2 / assemble + normalize_rows_bwd, bpr_sqnorm / bpr_fwd_bwd + sqnorm_part,
                 loss_total / sum + sqnorm + sum + sum, loss_mw / loss_total + mw_grad + sum; scatter_sorted_nbwd /
                 scatter_sorted + normalize_rows_bwd onto a zero dK only: onto anything else the fused kernel's last
                 step is one fused multiply-add where the separate launches round twice, and both are held to fp64)
  sums           |got - ref| <= (n + 2) 2^-24 sum|terms|, n = the terms on the longest chain, counted beside each
                 assertion; the fp64 accumulators: one 2^-24 per (float) cast or fp32 add and n 2^-53 sum|terms|
  pointwise      k 2^-24 times the magnitude of the terms, k = roundings + 1, counted beside each assertion; a row
                 with a clamped norm (the result is g / 1e-12) is held relative to |g| / 1e-12 by the same formula
  transcendentals (expf / logf / sqrtf in softmax2, bpr_rows, row_softmax and the norms): DESIGN section 2's rule -
                 at most twice the largest error of the same computation in fp32 numpy (kernel order of operations)
                 on the same inputs, both figures printed

Seen on the MI355X, kernel (fp32 numpy restatement), largest error against fp64:
  combine_fwd M        n = 1: 9.6e-8 .. 1.3e-7 (the same); n = 4101: 4.2e-7 .. 8.6e-7 (4.2e-7 .. 9.5e-7); at most 1.32
                       times the restatement's (n = 17, mw = (3, -2): 5.1e-7 against 3.8e-7)
  final_fwd            Emb 7.2e-8 .. 1.17e-7 of the terms (9.4e-8 .. 1.17e-7); nrm 9.0e-9 .. 1.14e-7 of nrm
                       (5.1e-8 .. 1.17e-7)
  cl_fwd               CLN 1.8e-8 .. 8.1e-8, nrm 4.0e-8 .. 1.12e-7 of nrm (the restatement's to the digit)
  mw_grad              4.18e-8 (4.18e-8) of sum|partials|, over all its cases
  bpr_fwd_bwd          loss B = 1: 2.1e-9; 16, 17: 6.2e-7; 37: 8.4e-7; 1000: 2.06e-6; contributions 1.8e-11 .. 8.1e-8
                       (the restatement's to the digit).  Before bpr_rows took its log in double the loss of the x = -100
                       row, -logf(1e-10f), was 3.19e-6 off (1.7 ulp) against numpy's 6.2e-7, and the bar failed at
                       B = 16, 17, 37
  row_softmax          P 0 .. 9.3e-10 (8.3e-11 .. 9.3e-10 over the 1000 rows); lse 3.0e-8 .. 5.6e-7 (2.4e-7 ..
                       5.9e-7).  Before row_softmax_kernel took its log in double lse was 1.12e-6 off at 1000 x 255
                       (2.3 ulp) against numpy's 3.3e-7, and the bar failed at every row count
  sums                 the largest share of a bound: the 40-slot run through scatter_sorted_nbwd 0.46 (both forms);
                       assemble's dE0 1.36e-6, 0.31; final_bwd's partials at most 0.03; loss_total 4.8e-7 of 1.4e-6
  pointwise            at most 0.65 of a bound (combine_fwd's E at 4101 rows; contrast_rows' contributions)
The whole file takes 3.4 s.
"""
import numpy as np
import pytest
import torch

import diffmm_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
U53 = 2.0 ** -53
TINY = 1e-37
FILL = 7.0
NAN = float("nan")
ROWS = [1, 15, 16, 17, 333, 4101]
BATCH = [1, 16, 17, 37, 1000]
MWS = [(0.0, 0.0), (3.0, -2.0), (80.0, -80.0)]


def f32(v):
    return float(np.float32(v))


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _call(name, *args):
    from gmr import _lib
    from gmr.kernels import stream
    return _lib.call(name, *args, stream())


def _ptr(t):
    """The device pointer of t; of an empty view (no item rows), the pointer of the buffer it starts."""
    from gmr.kernels import ptr
    return ptr(t if t is None or t.numel() else t._base)


def _np(t):
    return t.detach().cpu().numpy()


def _guarded(a, pad=0, extra=3):
    """A device copy of a (1-D or 2-D) at the start of a buffer with `extra` more rows and, for 2-D, rows `pad`
    elements longer; everything outside the copy holds FILL."""
    a = torch.as_tensor(a)
    shape = (a.shape[0] + extra,) + ((a.shape[1] + pad,) if a.dim() == 2 else ())
    buf = torch.full(shape, FILL, dtype=a.dtype, device=DEV)
    v = buf[:a.shape[0], :a.shape[1]] if a.dim() == 2 else buf[:a.shape[0]]
    v.copy_(a)
    return v


def _nan(*shape, pad=0, dtype=torch.float32):
    return _guarded(torch.full(shape, NAN, dtype=dtype), pad)


def _guard_ok(*views):
    for v in views:
        m = v._base.clone()
        m[tuple(slice(0, s) for s in v.shape)] = FILL
        assert bool((m == FILL).all()), "a sentinel row or pad column was written"


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same(a, b, what=""):
    """Bit equality of two tensors (or two tuples of them); NaN equals NaN, -0 differs from 0."""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
        return
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _sum_ok(got, ref, terms, n, what, extra=0.0):
    """The running-error bound of a length-n fp32 sum: |got - ref| <= (n + 2) 2^-24 sum|terms| (+ extra)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), what
    bound = (n + 2) * U24 * np.asarray(terms, np.float64) + extra + TINY
    bad = np.abs(got - ref) > bound
    assert not bad.any(), (what, n, float(np.abs(got - ref)[bad].max()), float(np.broadcast_to(bound, bad.shape)[bad].min()),
                           int(bad.sum()))
    ratio = float((np.abs(got - ref) / bound).max()) if got.size else 0.0
    print(f"{what}: largest error {float(np.abs(got - ref).max()) if got.size else 0.0:.3e}, {ratio:.3f} of its bound")
    return ratio


def _pt_ok(got, ref, mag, k, what, extra=0.0):
    """Pointwise: |got - ref| <= k 2^-24 mag (+ extra), k = roundings + 1."""
    return _sum_ok(got, ref, mag, k - 2, what, extra)


def _transc_ok(got, ref64, restated32, what, scale=None):
    """at most twice the fp32 restatement's largest error against fp64 (in units of scale)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert np.isfinite(got).all(), what
    s = 1.0 if scale is None else np.asarray(scale, np.float64) + TINY
    own = float((np.abs(np.asarray(restated32, np.float64) - ref64) / s).max()) if ref64.size else 0.0
    err = float((np.abs(got - ref64) / s).max()) if ref64.size else 0.0
    print(f"{what}: kernel {err:.3e} (fp32 numpy {own:.3e})")
    assert err <= 2 * own, (what, err, own)
    return err, own


def _rand(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _edge_rows(x, rng):
    """In place, from 8 rows up: two exactly-zero rows (one the last: in the last partial block), a row of norm about
    1e-20, one of about 1e18, and one of about 5e-13 (clamped, yet x / 1e-12 is of order one: the only kind of row
    on which dropping the projection term shows)."""
    n = x.shape[0]
    if n >= 8:
        x[n - 1] = 0
        x[n // 2] = 0
        x[1] *= np.float32(1e-21)
        x[2] *= np.float32(1e17)
        x[3] *= np.float32(6e-14)
    return x


def _unit(z, slope=1.0):
    """fp32 y = normalize(leaky(z)) and the clamped norms, rounded from fp64 (what a forward hands the backward)."""
    y, nv = R.normalize_rows(R.leaky(z, slope) if slope != 1.0 else z)
    return y.astype(np.float32), nv.astype(np.float32)


def _nbwd_bound(g, e_g, y, nv, slope_abs=1.0):
    """Elementwise bound of (g - y <y, g>) / nv in fp32 given y, nv rounded to fp32 and g carrying the error e_g.
    g path: nv's rounding, 1 / nv, the subtraction, the scaling, the slope: 5 roundings, k = 6.  dp y path: y
    rounded (twice: it enters dp and the product), dp a chain of n = 8 (four lane terms, four butterfly levels:
    n + 2 = 10), the product, the subtraction, 1 / nv, nv's rounding, the scaling, the slope: 18.  e_g goes through
    the same linear map."""
    g, y, nv = np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(y, np.float64)), np.asarray(nv, np.float64)[:, None]
    S = (y * g).sum(1, keepdims=True)
    lin = (e_g + y * (y * e_g).sum(1, keepdims=True)) if np.ndim(e_g) else 0.0
    return slope_abs * (U24 * (6 * g + 18 * y * S) + lin) / nv


def _twice(run):
    a = run()
    _same(a, run(), "a second run gave other bits")
    return a


# ------------------------------------------------------------------------------------------------ combine_fwd
@pytest.mark.parametrize("n", ROWS)
def test_combine_fwd(n):
    rng = np.random.default_rng(n)
    G, H, Qi, Qt = (_rand(rng, n, 128) for _ in range(4))
    lam = f32(0.37)
    d_H, d_Qi, d_Qt = dev(H), dev(Qi), dev(Qt)
    for mw in MWS:
        d_mw = dev(np.array(mw, np.float32))

        def run():
            d_G, M = _guarded(G), _nan(n, 64)
            _call("gmr_dmm_combine_fwd", n, _ptr(d_G), _ptr(d_H), _ptr(d_Qi), _ptr(d_Qt), _ptr(d_mw), lam, _ptr(M))
            _guard_ok(d_G, M)
            return d_G, M

        d_G, M = _twice(run)
        E64, M64 = R.combine_fwd(G, H, Qi, Qt, mw, lam)
        A = np.abs(np.concatenate([Qi[:, :64], Qt[:, :64]], 1)).astype(np.float64)
        # E = fma(lam, a, g + h): two roundings, k = 3
        _pt_ok(_np(d_G), E64, np.abs(G.astype(np.float64)) + np.abs(H) + lam * A, 3, f"E n={n}")
        _transc_ok(_np(M), M64, R.combine_fwd(G, H, Qi, Qt, mw, lam, np.float32)[1], f"combine M n={n} mw={mw}")


# ------------------------------------------------------------------------------------------------ final_fwd
@pytest.mark.parametrize("n", ROWS)
def test_final_fwd(n):
    rng = np.random.default_rng(10 + n)
    M, L = _edge_rows(_rand(rng, n, 64), rng), _rand(rng, n, 64)
    ris = f32(0.7)
    d_M, d_L = dev(M), dev(L)

    def run():
        Emb, nrm = _nan(n, 64), _nan(n)
        _call("gmr_dmm_final_fwd", n, _ptr(d_M), _ptr(d_L), ris, _ptr(Emb), _ptr(nrm))
        _guard_ok(Emb, nrm)
        return Emb, nrm

    Emb, nrm = _twice(run)
    E64, n64 = R.final_fwd(M, L, ris)
    E32, n32 = R.final_fwd(M, L, ris, np.float32)
    mag = np.abs(M.astype(np.float64)) + np.abs(L) + ris * np.abs(M) / n64[:, None]
    _transc_ok(_np(Emb), E64, E32, f"final_fwd Emb n={n}", mag)
    _transc_ok(_np(nrm), n64, n32, f"final_fwd nrm n={n}", n64)
    if n >= 8:  # the zero rows, the 1e-20 row and the 5e-13 row are clamped: exactly 1e-12f
        assert (_np(nrm)[[n - 1, n // 2, 1, 3]] == np.float32(1e-12)).all()
        np.testing.assert_array_equal(_np(Emb)[n - 1], L[n - 1])


# ------------------------------------------------------------------------------------------------ cl_fwd
def _cl_inputs(n, rng):
    Qi, Qt, K2 = (_rand(rng, n, 128) for _ in range(3))
    c8 = np.float32(1e-8)
    if n >= 8:
        for Q, h, rows in ((Qi, 0, (n - 1, n // 2)), (Qt, 64, (n - 1,))):  # K + 1e-8 == 0: Q = 0, K2 = -1e-8f
            for r in rows:
                Q[r, 64:] = 0
                K2[r, h:h + 64] = -c8
        Qi[2, 64:] *= np.float32(1e17)
        for Q, h in ((Qi, 0), (Qt, 64)):  # K + 1e-8 of norm about 5e-13 (the sum is exact: Sterbenz)
            Q[3, 64:] = 0
            K2[3, h:h + 64] = -c8 + (rng.standard_normal(64) * 6e-14).astype(np.float32)
    return Qi, Qt, K2


@pytest.mark.parametrize("n", ROWS + [7, 8, 9])
def test_cl_fwd(n):
    rng = np.random.default_rng(20 + n)
    Qi, Qt, K2 = _cl_inputs(n, rng)
    d = [dev(v) for v in (Qi, Qt, K2)]

    def run():
        CLN, nrm = _nan(n, 128), _nan(2 * n)
        _call("gmr_dmm_cl_fwd", n, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(CLN), _ptr(nrm))
        _guard_ok(CLN, nrm)
        return CLN, nrm

    CLN, nrm = _twice(run)
    C64, n64 = R.cl_fwd(Qi, Qt, K2)
    C32, n32 = R.cl_fwd(Qi, Qt, K2, np.float32)
    _transc_ok(_np(CLN), C64, C32, f"cl_fwd CLN n={n}")
    _transc_ok(_np(nrm), n64, n32, f"cl_fwd nrm n={n}", n64)
    if n >= 8:
        g = _np(nrm)
        assert (g[[n - 1, n // 2, 3, n + n - 1, n + 3]] == np.float32(1e-12)).all()
        assert (_np(CLN)[n - 1] == 0).all() and (_np(CLN)[n // 2, :64] == 0).all()
        assert 0.05 < np.abs(_np(CLN)[3]).max() < 10  # the 5e-13 rows: of order one after the clamp


# ------------------------------------------------------------------------------------------------ final_bwd
def _partials(n):
    from gmr import _lib
    return int(_lib.load().gmr_dmm_final_bwd_partials(n))


@pytest.mark.parametrize("n", ROWS)
def test_final_bwd(n):
    rng = np.random.default_rng(30 + n)
    dEmb, T1, M = _rand(rng, n, 64), _rand(rng, n, 64), _edge_rows(_rand(rng, n, 64), rng)
    E = _rand(rng, n, 128)
    ris, lam = f32(0.7), f32(0.37)
    y64, nv64 = R.normalize_rows(M)
    nrm = nv64.astype(np.float32)
    npart = _partials(n)
    assert npart == 2 * -(-n // 16)
    d_T1, d_M, d_nrm, d_E = dev(T1), dev(M), dev(nrm), dev(E)
    # dM = g + t + (ris / nv) (g - dp y).  g + t and the last add: k = 3.  g path of the third term: nv's rounding,
    # ris / nv, the subtraction, the scaling, the add: k = 6.  dp y path: y = m (1 / nv) enters twice (three roundings
    # each: nv, 1 / nv, the product), dp a chain of n = 8 (n + 2 = 10), the product, the subtraction, ris / nv
    # (two), the scaling, the add: 22.
    g, t = np.abs(dEmb.astype(np.float64)), np.abs(T1.astype(np.float64))
    S = (np.abs(y64) * g).sum(1, keepdims=True)
    e_dm = U24 * (3 * (g + t) + ris / nv64[:, None] * (6 * g + 22 * np.abs(y64) * S))
    for mw in MWS:
        d_mw = dev(np.array(mw, np.float32))

        def run():
            d_dEmb, dE, part = _guarded(dEmb), _nan(n, 128), _nan(npart)
            _call("gmr_dmm_final_bwd", n, _ptr(d_dEmb), _ptr(d_T1), _ptr(d_M), _ptr(d_nrm), ris, _ptr(d_E), _ptr(d_mw),
                  _ptr(dE), _ptr(part))
            _guard_ok(d_dEmb, dE, part)
            np.testing.assert_array_equal(_np(d_dEmb), dEmb)
            return dE, part

        dE, part = _twice(run)
        dM64, dE64, dw64, _ = R.final_bwd(dEmb, T1, M, ris, E, mw)
        w = np.array(R.softmax2(mw))
        # dE = w dM: softmax2's w is four roundings (the subtraction, expf at 1 ulp, the sum, the division), the
        # product one more: k = 6 over |w dM|, next to w e_dm
        wcol = np.repeat(w, 64)[None, :]
        _pt_ok(_np(dE), dE64, np.abs(dE64), 6, f"final_bwd dE n={n} mw={mw}", wcol * np.concatenate([e_dm, e_dm], 1))
        # the partials, summed in fp64 here: each is a chain of n = 12 (four lane terms, six butterfly levels, the two
        # adds of the four wave partials) over |e dm|, on top of |e| e_dm
        got = _np(part).astype(np.float64).reshape(-1, 2).sum(0)
        for h in (0, 1):
            Eh = np.abs(E[:, 64 * h:64 * h + 64].astype(np.float64))
            _sum_ok(got[h], dw64[h], (Eh * np.abs(dM64)).sum(), 12, f"final_bwd partials n={n} half={h}", (Eh * e_dm).sum())
        # the fused form: the same dE and partials; Ri / Rt left halves as cl_bwd with left = 1 writes them
        z = dev(np.zeros((n, 128), np.float32))
        Ri0, Rt0 = _nan(n, 128), _nan(n, 128)
        _call("gmr_dmm_cl_bwd", n, _ptr(z), _ptr(z), _ptr(dE), lam, _ptr(Ri0), _ptr(Rt0))
        for clear in (0, 1):
            for with_r in (False, True):
                d_dEmb, dE2, part2 = _guarded(dEmb), _nan(n, 128), _nan(npart)
                Ri, Rt = _guarded(np.full((n, 128), FILL, np.float32)), _guarded(np.full((n, 128), FILL, np.float32))
                _call("gmr_dmm_final_bwd2", n, _ptr(d_dEmb), _ptr(d_T1), _ptr(d_M), _ptr(d_nrm), ris, _ptr(d_E),
                      _ptr(d_mw), _ptr(dE2), _ptr(part2), clear, lam, _ptr(Ri) if with_r else None,
                      _ptr(Rt) if with_r else None)
                _same((dE2, part2), (dE, part), f"final_bwd2 clear={clear} R={with_r}")
                _guard_ok(d_dEmb, dE2, part2, Ri, Rt)
                if clear:
                    _same(d_dEmb, torch.zeros_like(d_dEmb), "dEmb cleared")
                else:
                    np.testing.assert_array_equal(_np(d_dEmb), dEmb)
                for R_, R0 in ((Ri, Ri0), (Rt, Rt0)):
                    assert bool((R_[:, 64:] == FILL).all())
                    if with_r:
                        _same(R_[:, :64], R0[:, :64], "Ri / Rt left halves")
                    else:
                        assert bool((R_ == FILL).all())


# ------------------------------------------------------------------------------------------------ mw_grad
def test_mw_grad():
    """dmw = w (dw - <w, dw>), dw the sums of final_bwd's partials.  Two outputs a case, so the rule's figures are
    taken over every case of this test, in units of sum|partials|."""
    rng = np.random.default_rng(40)
    worst, own_worst, cases = 0.0, 0.0, []
    for nparts in (1, 2, 21, 256, 257, 600):  # 257 = the partials of 4101 rows: past one pass of the 256 threads
        parts = _rand(rng, nparts, 2)
        d_parts = _guarded(parts.reshape(-1))
        dw64 = parts.astype(np.float64).sum(0)
        dw32 = [R.block_sum(parts[:, h], np.float32) for h in (0, 1)]
        scale = np.abs(parts).sum()
        for mw in MWS:
            d_mw = dev(np.array(mw, np.float32))
            want = R.mw_grad(dw64, mw)
            for acc in (0, 1):
                old = _rand(rng, 2) if acc else np.full(2, np.nan, np.float32)

                def run():
                    dmw = _guarded(old)
                    _call("gmr_dmm_mw_grad", nparts, _ptr(d_parts), _ptr(d_mw), _ptr(dmw), acc)
                    _guard_ok(dmw, d_parts)
                    return dmw

                got = _np(_twice(run)).astype(np.float64)
                assert np.isfinite(got).all()
                g32 = R.mw_grad_closed(dw32, mw, np.float32)
                ref, rest = (want + old, (g32 + old).astype(np.float32)) if acc else (want, g32)
                s = scale + (np.abs(old).max() if acc else 0.0)
                cases.append((nparts, mw, acc, float(np.abs(got - ref).max() / s), float(np.abs(rest - ref).max() / s)))
                worst, own_worst = max(worst, cases[-1][3]), max(own_worst, cases[-1][4])
    print(f"mw_grad: kernel {worst:.3e} (fp32 numpy {own_worst:.3e}) of sum|partials|")
    assert worst <= 2 * own_worst, [c for c in cases if c[3] > 2 * own_worst]


# ------------------------------------------------------------------------------------------------ dg
NU = [(1, 0), (1, 1), (17, 0), (17, 17), (333, 100), (4101, 4090)]


@pytest.mark.parametrize("n,U", NU + [(7, 3), (8, 8), (9, 0)])
def test_dg(n, U):
    rng = np.random.default_rng(50 + n + U)
    dE, T2 = _rand(rng, n, 128), _rand(rng, n, 128)
    want = R.dg(dE, T2, U)
    T2[U:] = np.nan  # a read of an item row of T2 shows
    d_dE, d_T2 = dev(dE), dev(T2)

    def run():
        dG = _nan(n, 128)
        _call("gmr_dmm_dg", n, U, _ptr(d_dE), _ptr(d_T2), _ptr(dG))
        _guard_ok(dG)
        return dG

    _same(_twice(run), dev(want), "dg")  # one fp32 addition: exact


# ------------------------------------------------------------------------------------------------ cl_bwd
@pytest.mark.parametrize("n", ROWS)
def test_cl_bwd(n):
    rng = np.random.default_rng(60 + n)
    dK, T, dE = (_rand(rng, n, 128) for _ in range(3))
    lam = f32(0.37)
    d_T, d_dE = dev(T), dev(dE)

    def run():
        d_dK, Ri, Rt = _guarded(dK), _nan(n, 128), _nan(n, 128)
        _call("gmr_dmm_cl_bwd", n, _ptr(d_dK), _ptr(d_T), _ptr(d_dE), lam, _ptr(Ri), _ptr(Rt))
        _guard_ok(d_dK, Ri, Rt)
        np.testing.assert_array_equal(_np(d_dK), dK)
        return Ri, Rt

    Ri0, Rt0 = _twice(run)
    wi, wt = R.cl_bwd(dK, T, dE, lam)
    mag = lambda h: np.concatenate([lam * np.abs(dE[:, h:h + 64]), np.abs(dK[:, h:h + 64]).astype(np.float64)  # noqa: E731
                                    + np.abs(T[:, h:h + 64])], 1)
    _pt_ok(_np(Ri0), wi, mag(0), 2, f"cl_bwd Ri n={n}")  # one product or one addition: k = 2
    _pt_ok(_np(Rt0), wt, mag(64), 2, f"cl_bwd Rt n={n}")
    for clear in (0, 1):
        for left in (0, 1):
            d_dK = _guarded(dK)
            Ri, Rt = _guarded(np.full((n, 128), FILL, np.float32)), _guarded(np.full((n, 128), FILL, np.float32))
            _call("gmr_dmm_cl_bwd2", n, _ptr(d_dK), _ptr(d_T), _ptr(d_dE) if left else None, lam, _ptr(Ri), _ptr(Rt),
                  clear, left)
            _guard_ok(d_dK, Ri, Rt)
            for R_, R0 in ((Ri, Ri0), (Rt, Rt0)):
                _same(R_[:, 64:], R0[:, 64:], f"cl_bwd2 right halves clear={clear} left={left}")
                if left:
                    _same(R_[:, :64], R0[:, :64], "cl_bwd2 left halves")
                else:
                    assert bool((R_[:, :64] == FILL).all())
            _same(d_dK[:, 64:], dev(dK[:, 64:]), "dK[:, 64:] is never written")
            _same(d_dK[:, :64], torch.zeros((n, 64), device=DEV) if clear else dev(dK[:, :64]), "dK[:, :64]")


# ------------------------------------------------------------------------------------------------ assemble
@pytest.mark.parametrize("n,U", NU)
def test_assemble(n, U):
    rng = np.random.default_rng(70 + n + U)
    I = n - U
    T2, T3, Ri, Rt = (_rand(rng, n, 128) for _ in range(4))
    E0 = _rand(rng, n, 64)
    reg2, slope = f32(0.03), f32(0.2)
    Z = np.concatenate([_edge_rows(_rand(rng, I, 64), rng), _edge_rows(_rand(rng, I, 64), rng)], 1)
    (yi, ni), (yt, nt) = _unit(Z[:, :64], slope), _unit(Z[:, 64:], slope)
    NF, nrmF = np.concatenate([yi, yt], 1), np.concatenate([ni, nt])
    d = [dev(v) for v in (T2, T3, Ri, Rt, E0)]
    d_NF, d_nrmF = _guarded(NF), _guarded(nrmF)

    def plain(d_T3):
        dE0, dNF = _nan(n, 64), _nan(I, 128)
        _call("gmr_dmm_assemble", n, U, _ptr(d[0]), _ptr(d_T3), _ptr(d[2]), _ptr(d[3]), _ptr(d[4]), reg2, _ptr(dE0),
              _ptr(dNF))
        _guard_ok(dE0, dNF)
        return dE0, dNF

    dE0, dNF = _twice(lambda: plain(d[1]))
    a = lambda v: np.abs(v.astype(np.float64))  # noqa: E731
    # dE0: seven terms on a user row (six table halves and reg2 E0), five on an item row: n = 7
    hsum = lambda v: a(v[:, :64]) + a(v[:, 64:])  # noqa: E731
    t_u = hsum(T3[:U]) + hsum(Ri[:U]) + hsum(Rt[:U]) + reg2 * a(E0[:U])
    t_i = hsum(T2[U:]) + a(Ri[U:, :64]) + a(Rt[U:, :64]) + reg2 * a(E0[U:])
    w0, wNF = R.assemble(T2, T3, Ri, Rt, E0, reg2, U)
    _sum_ok(_np(dE0), w0, np.concatenate([t_u, t_i]), 7, f"assemble dE0 n={n} U={U}")
    g_mag = np.concatenate([a(T3[U:, :64]) + a(Ri[U:, 64:]), a(T3[U:, 64:]) + a(Rt[U:, 64:])], 1)
    _pt_ok(_np(dNF), wNF, g_mag, 2, f"assemble dNF n={n} U={U}")  # one addition: k = 2

    # the separate launches assemble2 replaced: assemble, then the normalize backward with the slope on each half
    def separate(d_T3):
        dE0s, dNFs = plain(d_T3)
        if I:
            for h in (0, 1):
                _call("gmr_normalize_rows_bwd_f32", I, 64, _ptr(d_NF[:, 64 * h:]), 128, _ptr(d_nrmF[h * I:]),
                      _ptr(dNFs[:, 64 * h:]), 128, _ptr(dNFs[:, 64 * h:]), 128, slope, 0)
            _guard_ok(dNFs)
        return dE0s, dNFs

    T3n = T3.copy()
    T3n[:U] = np.nan  # t3u_from_t2 = 1: a read of T3's user rows shows
    T3c = T3.copy()
    T3c[:U] = T2[:U]  # what the separate launches need in their place
    dK0 = _rand(rng, n, 128)
    d_T3n, d_T3c = dev(T3n), dev(T3c)
    for flag in (0, 1):
        sep = separate(d_T3c if flag else d[1])
        for with_clear in (False, True):

            def fused():
                dE0f, dNFf, dKc = _nan(n, 64), _nan(I, 128), _guarded(dK0)
                _call("gmr_dmm_assemble2", n, U, _ptr(d[0]), _ptr(d_T3n if flag else d[1]), _ptr(d[2]),
                      _ptr(d[3]), _ptr(d[4]), reg2, _ptr(dE0f), _ptr(dNFf), _ptr(d_NF), _ptr(d_nrmF), slope,
                      _ptr(dKc) if with_clear else None, flag)
                _guard_ok(dE0f, dNFf, dKc, d_NF, d_nrmF)
                _same(dKc[:, 64:], dev(dK0[:, 64:]), "dK_clear[:, 64:] is never written")
                _same(dKc[:, :64], torch.zeros((n, 64), device=DEV) if with_clear else dev(dK0[:, :64]), "dK_clear")
                return dE0f, dNFf

            got = _twice(fused)
            _same(got, sep, f"assemble2 against assemble + normalize_rows_bwd, t3u_from_t2={flag}")
        if I:
            w0f, wNFf = R.assemble(T2, T3, Ri, Rt, E0, reg2, U, bool(flag))
            if flag:
                t_uf = hsum(T2[:U]) + hsum(Ri[:U]) + hsum(Rt[:U]) + reg2 * a(E0[:U])
                _sum_ok(_np(got[0]), w0f, np.concatenate([t_uf, t_i]), 7, "assemble2 dE0 from T2's user rows")
            want = R.assemble_projection(wNFf, Z, slope)
            for h, nv in ((0, ni), (1, nt)):
                c = slice(64 * h, 64 * h + 64)
                # g = T3 + R: one rounding, e_g = 2^-24 |terms|; then the bound of the normalize backward
                bound = _nbwd_bound(wNFf[:, c], U24 * g_mag[:, c], NF[:, c], nv)
                _pt_ok(_np(got[1])[:, c], want[:, c], 0.0, 2, f"assemble2 dNF half {h} n={n} U={U}", bound)


# ------------------------------------------------------------------------------------------------ BPR rows
@pytest.fixture(scope="module")
def bpr_pool():
    """One batch of 1000 rows; every case takes its first B.  Rows 0 .. 4 have x = 0 (pos == neg), about +30, -30,
    +100 and -100; row 15 repeats the user of row 7; rows 5 and 6 take the first user and the first and last item.
    Read-only."""
    rng = np.random.default_rng(80)
    U, I, B = 50, 80, 1000
    Emb = (0.3 * rng.standard_normal((U + I, 64))).astype(np.float32)
    users, pos, neg = (rng.integers(0, hi, B).astype(np.int32) for hi in (U, I, I))
    neg[0] = pos[0]
    for b, x in ((1, 30.0), (2, -30.0), (3, 100.0), (4, -100.0)):  # p = q + x a / |a|^2: <a, p> - <a, q> ~ x
        users[b], pos[b], neg[b] = U - b, I - 2 * b, I - 2 * b + 1
        a64 = Emb[users[b]].astype(np.float64)
        Emb[U + pos[b]] = (Emb[U + neg[b]] + x * a64 / (a64 * a64).sum()).astype(np.float32)
    users[15] = users[7]
    users[5], pos[5], neg[6] = 0, I - 1, 0
    return U, I, Emb, users, pos, neg


@pytest.mark.parametrize("B", BATCH)
def test_bpr(B, bpr_pool):
    from gmr import _lib
    U, I, Emb, users, pos, neg = bpr_pool
    users, pos, neg = users[:B], pos[:B], neg[:B]
    inv_norm = f32(1.0 / (B + 3))  # not 1 / B: the rows of a global batch
    d_Emb, d_u, d_p, d_n = _guarded(Emb), dev(users), dev(pos), dev(neg)

    def run():
        loss, contrib = _nan(B), _nan(3 * B, 64)
        _call("gmr_bpr_fwd_bwd", B, U, _ptr(d_Emb), _ptr(d_u), _ptr(d_p), _ptr(d_n), _ptr(loss), _ptr(contrib), inv_norm)
        _guard_ok(loss, contrib, d_Emb)
        return loss, contrib

    loss, contrib = _twice(run)
    l64, c64, x64 = R.bpr(Emb, U, users, pos, neg, inv_norm)
    l32, c32, _ = R.bpr(Emb, U, users, pos, neg, inv_norm, np.float32)
    assert x64[0] == 0 and (B < 16 or np.allclose(x64[1:5], [30, -30, 100, -100], rtol=1e-5))
    _transc_ok(_np(loss), l64, l32, f"bpr loss B={B}")
    _transc_ok(_np(contrib), c64, c32, f"bpr contrib B={B}")
    # the fused launch: the BPR rows and the squared-norm partials of a table, against the two launches
    n_sq = (U + I) * 64
    g = int(_lib.load().gmr_sqnorm_nparts(n_sq))
    assert g == R.sqnorm_nparts(n_sq) == 5
    parts0 = _nan(g, dtype=torch.float64)
    _call("gmr_sqnorm_part_f32", n_sq, _ptr(d_Emb), _ptr(parts0))

    def fused():
        loss2, contrib2, parts = _nan(B), _nan(3 * B, 64), _nan(g, dtype=torch.float64)
        _call("gmr_dmm_bpr_sqnorm", B, U, _ptr(d_Emb), _ptr(d_u), _ptr(d_p), _ptr(d_n), _ptr(loss2), _ptr(contrib2),
              inv_norm, n_sq, _ptr(d_Emb), _ptr(parts))
        _guard_ok(loss2, contrib2, parts, parts0)
        return loss2, contrib2, parts

    _same(_twice(fused), (loss, contrib, parts0), "bpr_sqnorm against bpr_fwd_bwd + sqnorm_part_f32")


# ------------------------------------------------------------------------------------------------ row softmax
SOFTMAX_COEF = f32(0.013)
_softmax_pool = {}


def _softmax_case(cols):
    """1000 rows of `cols` logits with |L| <= 1 / temp, their fp64 softmax and the fp32 restatement's; built once
    per width, every case takes its first rows."""
    if cols not in _softmax_pool:
        L = np.clip(2 * _rand(np.random.default_rng(90 + cols), 1000, cols), -5, 5)
        _softmax_pool[cols] = (L,) + R.row_softmax(L, SOFTMAX_COEF) + R.row_softmax(L, SOFTMAX_COEF, np.float32)
    return _softmax_pool[cols]


@pytest.mark.parametrize("rows", BATCH)
def test_row_softmax(rows):
    """The restatement's largest error is taken over all 1000 rows of the width, of which the case is the first
    `rows`: with one column the true lse is L itself, a float, and a restatement that returns it has no error at
    all to double on a case of one row."""
    for cols in (1, 255, 257, 1000):  # one pass of the 256 threads, its tail, and four passes
        Lp, P64, s64, P32, s32 = _softmax_case(cols)
        L = Lp[:rows]

        def run():
            d_L, lse = _guarded(L, pad=5), _nan(rows)
            _call("gmr_row_softmax_f32", rows, cols, _ptr(d_L), d_L.stride(0), SOFTMAX_COEF, _ptr(lse))
            _guard_ok(d_L, lse)
            return d_L, lse

        P, lse = _twice(run)
        for got, ref, rest, what in ((P, P64, P32, "P"), (lse, s64, s32, "lse")):
            g = _np(got).astype(np.float64)
            assert np.isfinite(g).all()
            err, own = float(np.abs(g - ref[:rows]).max()), float(np.abs(rest - ref).max())
            print(f"row_softmax {what} {rows}x{cols}: kernel {err:.3e} (fp32 numpy, 1000 rows {own:.3e})")
            assert err <= 2 * own, (what, rows, cols, err, own)


# ------------------------------------------------------------------------------------------------ contrast rows
@pytest.mark.parametrize("B", BATCH)
def test_contrast_rows(B):
    rng = np.random.default_rng(100 + B)
    N, off = 90, 40
    CLN = np.concatenate([_unit(_rand(rng, N, 64))[0], _unit(_rand(rng, N, 64))[0]], 1)
    nodes = rng.integers(0, N - off, B).astype(np.int32)
    nodes[0] = N - off - 1  # the last table row
    if B > 1:
        nodes[1], nodes[-1] = 0, nodes[0]
    lse = (6 + _rand(rng, B)).astype(np.float32)
    inv_temp, coef = f32(5.0), f32(0.013)
    left = _rand(rng, B, 64)  # dp1 as the GEMM left it
    c0 = np.concatenate([left, np.full((B, 64), np.nan, np.float32)], 1)
    d_CLN, d_nodes, d_lse = _guarded(CLN), dev(nodes), dev(lse)

    def run():
        loss, contrib = _nan(B), _guarded(c0, pad=8)
        _call("gmr_contrast_rows", B, _ptr(d_CLN), _ptr(d_nodes), off, _ptr(d_lse), inv_temp, coef, _ptr(loss),
              _ptr(contrib), contrib.stride(0))
        _guard_ok(loss, contrib, d_CLN)
        return loss, contrib

    loss, contrib = _twice(run)
    l64, c64 = R.contrast_rows(CLN, nodes, off, lse, inv_temp, coef, left)
    r = CLN[off + nodes].astype(np.float64)
    p1, p2 = np.abs(r[:, :64]), np.abs(r[:, 64:])
    # loss = lse - d / temp: d a chain of n = 8 over |p1 p2| (n + 2 = 10), then the product and the subtraction: 12
    _pt_ok(_np(loss), l64, np.abs(lse) + inv_temp * (p1 * p2).sum(1), 12, f"contrast loss B={B}")
    k = coef * inv_temp
    # left: k = -coef / temp rounds, then one fma onto dp1: k = 3; right: two products: k = 3
    _pt_ok(_np(contrib), c64, np.concatenate([np.abs(left) + k * p2, k * p1], 1), 3, f"contrast contrib B={B}")


# ------------------------------------------------------------------------------------------------ gather rows
@pytest.mark.parametrize("B", BATCH)
def test_gather_rows(B):
    rng = np.random.default_rng(110 + B)
    rows, off = 60, 7
    for cols in (4, 64, 128, 192):
        src = _rand(rng, rows, cols)
        idx = rng.integers(0, rows - off, B).astype(np.int32)
        idx[0] = rows - off - 1
        idx[-1] = 0 if B > 1 else idx[-1]
        d_src, d_idx = _guarded(src, pad=4), dev(idx)

        def run():
            out = _nan(B, cols, pad=8)
            _call("gmr_gather_rows_f32", B, cols, _ptr(d_src), d_src.stride(0), _ptr(d_idx), off, _ptr(out), out.stride(0))
            _guard_ok(out, d_src)
            return out

        _same(_twice(run), dev(src[off + idx]), f"gather_rows B={B} cols={cols}")


# ------------------------------------------------------------------------------------------------ sorted scatter
TABLE = 20


def _run_keys(rng, last_run):
    """One key 40 times, runs of exactly 8, 9, 16 and 17, key 0, singles, and the largest table row `last_run`
    times: its run ends on the last word of an unpadded plan.  Shuffled: slots of a run are not adjacent."""
    keys = [5] * 40 + [0] * 8 + [2] * 9 + [7] * 16 + [11] * 17 + [3, 4, 6, 8] + [TABLE - 1] * last_run
    return rng.permutation(np.array(keys, np.int32))


def _vals(rng, n, cols):
    """Rows whose magnitudes span seven decades, so that any other order of a run's sum gives other bits."""
    return (rng.standard_normal((n, cols)) * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(np.float32)


def _scatter(plan, n, cols, d_x, dst0):
    dst = _guarded(dst0, pad=8)
    _call("gmr_scatter_sorted_f32", n, cols, _ptr(plan), _ptr(d_x), d_x.stride(0), _ptr(dst), dst.stride(0))
    _guard_ok(dst, d_x)
    return dst


@pytest.mark.parametrize("cols", [4, 64, 128, 192])
@pytest.mark.parametrize("last_run,padded", [(8, False), (9, False), (8, True), (9, True)])
def test_scatter_sorted_runs(cols, last_run, padded):
    rng = np.random.default_rng(120 + cols + last_run)
    keys = _run_keys(rng, last_run)
    plan = R.plan_of(keys, 128 if padded else None)  # padded: passed with n = plan.numel(), ~0 words after the last run
    assert (plan[len(keys) - 1] >> np.uint64(32)) == TABLE - 1 and (padded or len(plan) == len(keys))
    x, dst0 = _vals(rng, len(keys), cols), _rand(rng, TABLE, cols)
    d_plan, d_x = dev(plan.view(np.int64)), _guarded(x, pad=4)
    dst = _twice(lambda: _scatter(d_plan, len(plan), cols, d_x, dst0))
    want = R.scatter_sorted_f32(plan, x, dst0)
    _same(dst, dev(want), f"scatter_sorted cols={cols} last run {last_run} padded={padded}")
    none = np.setdiff1d(np.arange(TABLE), keys)  # rows with no key: bit-unchanged
    assert len(none) and np.array_equal(_np(dst)[none].view(np.uint32), dst0[none].view(np.uint32))


@pytest.mark.parametrize("B", BATCH)
def test_scatter_sorted_batches(B):
    rng = np.random.default_rng(130 + B)
    keys = rng.integers(0, 10, B).astype(np.int32)  # B = 1000: runs of about a hundred slots, a dozen 8-word reads
    keys[0] = TABLE - 1
    plan = R.plan_of(keys)
    x, dst0 = _vals(rng, B, 64), _rand(rng, TABLE, 64)
    d_plan, d_x = dev(plan.view(np.int64)), _guarded(x, pad=4)
    dst = _twice(lambda: _scatter(d_plan, B, 64, d_x, dst0))
    _same(dst, dev(R.scatter_sorted_f32(plan, x, dst0)), f"scatter_sorted B={B}")


def test_scatter_inputs_tell_orders_apart():
    """The run inputs above give other bits when a run is summed backwards: the exact comparison pins the order."""
    rng = np.random.default_rng(120 + 64 + 8)
    keys = _run_keys(rng, 8)
    plan = R.plan_of(keys)
    x, dst0 = _vals(rng, len(keys), 64), _rand(rng, TABLE, 64)
    slot = (plan & np.uint64(0xFFFFFFFF)).astype(np.int64)
    back = plan.copy()
    key = plan >> np.uint64(32)
    for k in np.unique(key):  # the same runs, slots descending
        m = key == k
        back[m] = (k << np.uint64(32)) | slot[m][::-1].astype(np.uint64)
    a, b = R.scatter_sorted_f32(plan, x, dst0), R.scatter_sorted_f32(back, x, dst0)
    assert not np.array_equal(a[5], b[5]) and not np.array_equal(a[2], b[2])


@pytest.mark.parametrize("padded", [False, True])
def test_scatter_sorted_nbwd(padded):
    rng = np.random.default_rng(140 + padded)
    N = TABLE
    keys = _run_keys(rng, 9)
    plan = R.plan_of(keys, 128 if padded else None)
    K = _rand(rng, N, 128)
    K[5, :64] = 0     # the 40-slot run: a zero image row
    K[0, 64:] = 0     # a zero text row
    K[7] *= np.float32(6e-14)   # both halves of norm about 5e-13: clamped, y of order one
    K[11] *= np.float32(1e-21)
    K[N - 1] *= np.float32(1e17)
    (yi, ni), (yt, nt) = _unit(K[:, :64]), _unit(K[:, 64:])
    y, nrm = np.concatenate([yi, yt], 1), np.concatenate([ni, nt])
    x, dK0 = _vals(rng, len(keys), 128), _rand(rng, N, 128)
    d_plan, d_x, d_y, d_nrm = dev(plan.view(np.int64)), _guarded(x, pad=8), _guarded(y), _guarded(nrm)

    def fused(start):
        dK = _guarded(start)
        _call("gmr_scatter_sorted_nbwd_f32", len(plan), _ptr(d_plan), _ptr(d_x), d_x.stride(0), _ptr(d_y), _ptr(d_nrm), N,
              _ptr(dK))
        _guard_ok(dK, d_x, d_y, d_nrm)
        return dK

    # the separate launches: the sorted scatter (cols = 128) into zeros, then the normalize backward added per half
    tmp = _scatter(d_plan, len(plan), 128, d_x, np.zeros((N, 128), np.float32))

    def separate(start):
        dK2 = _guarded(start)
        for h in (0, 1):
            _call("gmr_normalize_rows_bwd_f32", N, 64, _ptr(d_y[:, 64 * h:]), 128, _ptr(d_nrm[h * N:]),
                  _ptr(tmp[:, 64 * h:]), tmp.stride(0), _ptr(dK2[:, 64 * h:]), 128, 1.0, 1)
        _guard_ok(dK2, tmp)
        return dK2

    # onto a zero dK the two forms give the same bits: the run sums and the normalize backward are one expression.
    # Onto anything else the fused kernel ends in one fused multiply-add, dK + (1 / nrm) (s - y <y, s>) (read from
    # its code object), where the separate launches round the product and then the sum: both are held to fp64.
    zero = np.zeros((N, 128), np.float32)
    _same(_twice(lambda: fused(zero)), separate(zero), "scatter_sorted_nbwd against scatter_sorted + normalize_rows_bwd")
    dK = _twice(lambda: fused(dK0))
    none = np.setdiff1d(np.arange(N), keys)
    assert len(none) and np.array_equal(_np(dK)[none].view(np.uint32), dK0[none].view(np.uint32))
    s64, terms, longest = R.scatter_index_add(plan, x, np.zeros((N, 128)))
    assert longest == 40
    for form, got in (("fused", dK), ("separate", separate(dK0))):
        for h, nv in ((0, ni), (1, nt)):
            c = slice(64 * h, 64 * h + 64)
            nb = R.normalize_bwd(K[:, c], s64[:, c])
            # s: a run of r slots is a chain of n = r; then the normalize backward's bound, and the add onto dK: k = 2
            bound = _nbwd_bound(s64[:, c], (longest + 2) * U24 * terms[:, c], y[:, c], nv)
            _pt_ok(_np(got)[:, c], dK0[:, c] + nb, np.abs(dK0[:, c]) + np.abs(nb), 2, f"{form} nbwd half {h}", bound)
    assert 1e9 < np.abs(_np(dK)[5, :64]).max()  # the clamped rows did get g / 1e-12


# ------------------------------------------------------------------------------------------------ sort
def _sort(keys, offs, key_add, nk, pow2, out_stride):
    nb = len(offs) - 1
    d_keys, d_offs, d_add = dev(keys), dev(np.asarray(offs, np.int64)), dev(np.asarray(key_add, np.int32))
    out = _guarded(np.full((nb, out_stride), 7, np.int64))
    _call("gmr_sort_batch_keys", nb, _ptr(d_keys), _ptr(d_offs), _ptr(d_add), nk, keys.shape[1], _ptr(out), out_stride,
          pow2)
    _guard_ok(out)
    return out


@pytest.mark.parametrize("nk,ln", [(2, 1), (3, 1), (3, 37), (2, 2048), (3, 2730), (1, 5)])
def test_sort_batch_keys(nk, ln):
    rng = np.random.default_rng(150 + nk + ln)
    pow2 = 1 << max(1, (nk * ln - 1).bit_length())
    assert pow2 == {(2, 1): 2, (3, 1): 4, (3, 37): 128, (2, 2048): 4096, (3, 2730): 8192, (1, 5): 8}[(nk, ln)]
    stride = ln + 3  # a key row longer than the batch: the three after it are never read into the plan
    keys = rng.integers(0, 50, (nk, stride)).astype(np.int32)
    keys[0, 0], keys[nk - 1, ln - 1] = 0, 2 ** 31 - 101  # key 0, and with key_add the largest row an int32 holds
    key_add = [0, 100, 100][:nk] if nk > 1 else [100]
    out = _twice(lambda: _sort(keys, [0, ln], key_add, nk, pow2, pow2))
    want = R.sort_batch_keys(keys, [0, ln], key_add, nk, pow2)
    _same(out, dev(want.view(np.int64)), f"sort nk={nk} len={ln}")
    assert int(want[0, nk * ln - 1] >> np.uint64(32)) == 2 ** 31 - 1


def test_sort_batch_keys_batches():
    """Three batches in one call: 37 keys, none, 16 (a short last one); rows of pow2 + 8 words, the gap untouched."""
    rng = np.random.default_rng(160)
    offs, nk, pow2 = [0, 37, 37, 53], 3, 128
    keys = rng.integers(0, 9, (nk, 53)).astype(np.int32)
    out = _twice(lambda: _sort(keys, offs, [0, 100, 100], nk, pow2, pow2 + 8))
    want = R.sort_batch_keys(keys, offs, [0, 100, 100], nk, pow2, pow2 + 8, fill=np.uint64(7))
    _same(out, dev(want.view(np.int64)), "sort, three batches")
    assert bool((out[:, pow2:] == 7).all()) and bool((out[1, :pow2] == -1).all())


# ------------------------------------------------------------------------------------------------ reductions
@pytest.fixture(scope="module")
def big():
    """2 * 1024 * 2048 + 77 floats that every reduction case slices: read-only."""
    x = np.random.default_rng(170).standard_normal(2 * 1024 * 2048 + 77).astype(np.float32)
    return x, dev(x), x.astype(np.float64)


RED = [0, 1, 255, 256, 257, 3001]
SQN = RED + [2047, 2048, 2049, 2 * 1024 * 2048 + 77]


def _cast_bound(v, old, acc, n, terms):
    """One 2^-24 for the (float) cast, one for the fp32 add when accumulating, n 2^-53 sum|terms| before them."""
    return (U24 * (abs(v) + (abs(old + v) if acc else 0.0)) + (n + 8) * U53 * terms) * (1 + 1e-6) + TINY


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", RED)
def test_sum_f32(n, acc, big):
    x, d_x, x64 = big
    scale, old = f32(0.37), np.float32(1.5) if acc else np.float32(np.nan)

    def run():
        out = _guarded(np.array([old], np.float32))
        _call("gmr_sum_f32", n, _ptr(d_x), scale, _ptr(out), acc)
        _guard_ok(out)
        return out

    got = float(_twice(run)[0])
    v = x64[:n].sum() * scale
    ref = v + (float(old) if acc else 0.0)
    # a thread's chain is ceil(n / 256) terms, six butterfly levels, two adds: n = ceil(n / 256) + 8
    assert abs(got - ref) <= _cast_bound(v, float(old) if acc else 0.0, acc, -(-n // 256), np.abs(x64[:n]).sum() * scale)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", RED)
def test_sum_f64(n, acc, big):
    x64 = big[2]
    d_x = dev(x64[:max(n, 1)])
    scale, old = 0.37, 1.5 if acc else np.nan

    def run():
        out = _guarded(np.array([old]))
        _call("gmr_sum_f64", n, _ptr(d_x), scale, _ptr(out), acc)
        _guard_ok(out)
        return out

    got = float(_twice(run)[0])
    v = x64[:n].sum() * scale
    ref = v + (old if acc else 0.0)
    # all in fp64: the chain (ceil(n / 256) + 8), the scaling and the add
    assert abs(got - ref) <= (-(-n // 256) + 8 + 2) * U53 * (np.abs(x64[:n]).sum() * scale + abs(ref)) + TINY


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", SQN)
def test_sqnorm_f32(n, acc, big):
    from gmr import _lib
    x, d_x, x64 = big
    g = int(_lib.load().gmr_sqnorm_nparts(n))
    assert g == R.sqnorm_nparts(n)
    assert (n > 1024 * 2048) == (n == SQN[-1])  # past the 1024-block cap: the grid-stride loop takes a second turn
    scale, old = f32(0.37), np.float32(1.5) if acc else np.float32(np.nan)

    def parts_only():
        ws = _nan(g, dtype=torch.float64)
        _call("gmr_sqnorm_part_f32", n, _ptr(d_x), _ptr(ws))
        _guard_ok(ws)
        return ws

    ws = _twice(parts_only)
    want = R.sqnorm_parts(x64[:n], g)
    # a thread adds ceil(n / (256 g)) squares (each rounded once), then six butterfly levels and two adds
    chain = -(-n // (256 * g)) + 8 + 1
    assert (np.abs(_np(ws) - want) <= (chain + 2) * U53 * want + TINY).all()

    def run():
        out, ws2 = _guarded(np.array([old], np.float32)), _nan(1024, dtype=torch.float64)
        _call("gmr_sqnorm_f32", n, _ptr(d_x), scale, _ptr(out), acc, _ptr(ws2))
        _guard_ok(out, ws2)
        _same(ws2[:g], ws, "sqnorm_f32's partials are sqnorm_part_f32's")
        assert bool(torch.isnan(ws2[g:]).all())
        return out

    got = float(_twice(run)[0])
    v = want.sum() * scale
    ref = v + (float(old) if acc else 0.0)
    # the final sum of g partials: ceil(g / 256) + 8 more fp64 terms on the chain
    assert abs(got - ref) <= _cast_bound(v, float(old) if acc else 0.0, acc, chain + -(-g // 256) + 8, v)


# ------------------------------------------------------------------------------------------------ the loss sums
@pytest.mark.parametrize("B", BATCH)
def test_loss_total_and_loss_mw(B, big):
    rng = np.random.default_rng(180 + B)
    _, d_x, x64 = big
    n_sq = 5000
    g = R.sqnorm_nparts(n_sq)
    bpr, cu, ci = (0.7 + _rand(rng, B)).astype(np.float32), (6 + _rand(rng, B)).astype(np.float32), _rand(rng, B)
    inv_nr, reg, ssl = f32(1.0 / (B + 3)), f32(1e-3), f32(0.013 / (B + 3))
    d_bpr, d_cu, d_ci = dev(bpr), dev(cu), dev(ci)
    parts = _nan(g, dtype=torch.float64)
    _call("gmr_sqnorm_part_f32", n_sq, _ptr(d_x), _ptr(parts))

    def total():
        out = _nan(1)
        _call("gmr_dmm_loss_total", B, _ptr(d_bpr), inv_nr, _ptr(parts), g, reg, _ptr(d_cu), _ptr(d_ci), ssl, _ptr(out))
        _guard_ok(out)
        return out

    out = _twice(total)
    # the four reductions it replaced
    sep, ws = _nan(1), _nan(1024, dtype=torch.float64)
    _call("gmr_sum_f32", B, _ptr(d_bpr), inv_nr, _ptr(sep), 0)
    _call("gmr_sqnorm_f32", n_sq, _ptr(d_x), reg, _ptr(sep), 1, _ptr(ws))
    _call("gmr_sum_f32", B, _ptr(d_cu), ssl, _ptr(sep), 1)
    _call("gmr_sum_f32", B, _ptr(d_ci), ssl, _ptr(sep), 1)
    _guard_ok(sep)
    _same(out, sep, "loss_total against sum, sqnorm, sum, sum")
    ref, t = R.loss_total(bpr, inv_nr, R.sqnorm_parts(x64[:n_sq], g), reg, cu, ci, ssl)
    # four (float) casts, one 2^-24 of each addend, and three fp32 adds of at most sum|addends| each; the fp64 chains
    # below them add n 2^-53
    mag = sum(abs(v) for v in t)
    assert abs(float(out[0]) - ref) <= (4 * U24 + (B + n_sq) * U53) * mag * (1 + 1e-6)
    print(f"loss_total B={B}: {abs(float(out[0]) - ref):.3e} of the bound {4 * U24 * mag:.3e}")
    for nmw in (1, 257):
        mwp = _rand(rng, 2 * nmw)
        d_mwp = dev(mwp)
        for mw in MWS:
            d_mw = dev(np.array(mw, np.float32))
            dmw0 = _nan(2)
            _call("gmr_dmm_mw_grad", nmw, _ptr(d_mwp), _ptr(d_mw), _ptr(dmw0), 0)
            acc0 = _guarded(np.array([2.5], np.float32))
            _call("gmr_sum_f32", 1, _ptr(out), 1.0, _ptr(acc0), 1)
            for with_acc in (False, True):

                def fused():
                    o, dmw, acc = _nan(1), _nan(2), _guarded(np.array([2.5], np.float32))
                    _call("gmr_dmm_loss_mw", B, _ptr(d_bpr), inv_nr, _ptr(parts), g, reg, _ptr(d_cu), _ptr(d_ci), ssl,
                          _ptr(o), _ptr(acc) if with_acc else None, nmw, _ptr(d_mwp), _ptr(d_mw), _ptr(dmw))
                    _guard_ok(o, dmw, acc)
                    return o, dmw, acc

                o, dmw, acc = _twice(fused)
                _same((o, dmw), (out, dmw0), f"loss_mw against loss_total + mw_grad nmw={nmw} mw={mw}")
                _same(acc, acc0 if with_acc else dev(np.array([2.5], np.float32)), "loss_mw acc against sum_f32")
