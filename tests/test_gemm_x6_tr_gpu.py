"""TN / NN split-bf16 GEMM calls read their m- / n-contiguous operands in place (gemm_x6.hip TrTile: float4 granules
along m / n, [k][row] bf16 planes in LDS, fragments through transposed LDS reads).  The fragments are the ones the
k-contiguous path reads, so three calls must agree bit for bit: the in-place call, the same call with
tile | GMR_GEMM_X6_COPY (operands copied k-contiguous into the workspace first) and the NT call on host-made
k-contiguous copies.  Shapes are the smallest that reach every path: one tile and more than one per dimension,
ragged edges, no full k tile, a partial last k tile, split-K slabs, operands that must fall back to the copies."""
import numpy as np
import pytest
import torch

from test_kernels_gpu import X6, DEV, K, _dev, _rng  # noqa: F401  (K: fixture)

pytestmark = pytest.mark.gpu

COPY = 1 << 29  # GMR_GEMM_X6_COPY (include/gmr.h)
TILES = (128, 256128, 128256)
LAYOUTS = [(1, 0), (0, 0)]  # (trans_a, trans_b): TN, NN
NAN = np.float32(np.nan)


def _bits(t):
    return t.view(torch.int32)


def _r4(n):
    return (n + 3) // 4 * 4


_BASE = {}


def _data(M, N, Kd):
    """a [M][Kd], b [N][Kd]: slices of one random pair made once per process"""
    if not _BASE:
        rng = _rng(71)
        _BASE["a"] = rng.standard_normal((300, 1000)).astype(np.float32)
        _BASE["b"] = rng.standard_normal((260, 1000)).astype(np.float32)
    return _BASE["a"][:M, :Kd], _BASE["b"][:N, :Kd]


def _kc(x):
    """x [rows][Kd] k-contiguous on the device, rows padded to 16 bytes"""
    return _dev(np.pad(x, ((0, 0), (0, (-x.shape[1]) % 4))))[:, :x.shape[1]]


def _mn(x, how):
    """x [rows][Kd] stored m- / n-contiguous: a [Kd][rows] device view.  Everything around the view is NaN.
    padded: ld = rows rounded up to 4 (read in place; the last granule straddles the end into the padding);
    unpadded: ld = rows (copied unless rows is a multiple of 4); offset: the view starts one column into its
    buffer (not 16-byte aligned: copied); sub: columns 8 .. 8 + rows of a wider buffer (in place, ld > rows)"""
    rows, Kd = x.shape
    if how == "unpadded":
        return _dev(x.T)
    lead, ld = {"padded": (0, _r4(rows)), "offset": (1, _r4(rows) + 4), "sub": (8, _r4(rows) + 72)}[how]
    buf = np.full((Kd, ld), NAN, dtype=np.float32)
    buf[:, lead:lead + rows] = x.T
    return _dev(buf)[:, lead:lead + rows]


def _three(K, a, b, ta, tile, split=1, how="padded", mk_c=None, **kw):
    """C of the in-place call, of the same call with GMR_GEMM_X6_COPY, and of the NT call on k-contiguous copies"""
    M, N = a.shape[0], b.shape[0]
    A = _mn(a, how) if ta else _kc(a)
    B = _mn(b, how)
    outs = []
    for AA, BB, t_a, t_b, flag in ((A, B, bool(ta), False, 0), (A, B, bool(ta), False, COPY),
                                   (_kc(a), _kc(b), False, True, 0)):
        C = mk_c() if mk_c else torch.full((M, N), 7.0, device=DEV)
        K.gemm(AA, BB, C, trans_a=t_a, trans_b=t_b, tile=tile | X6 | flag, split_k=split, **kw)
        outs.append(C)
    return outs


def _same(outs, what):
    assert not torch.isnan(outs[0]).any(), what  # (no padding value reached C)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), ("in place vs copy", what)
    assert torch.equal(_bits(outs[0]), _bits(outs[2])), ("in place vs NT", what)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_inplace_copy_nt_bit_equal(K, tile, ta, tb):
    for M, N in ((128, 128), (132, 260), (300, 200)):
        for Kd in (1, 31, 32, 33, 64, 97, 1000):
            a, b = _data(M, N, Kd)
            for split in ((1, 2) if Kd in (97, 1000) else (1,)):
                _same(_three(K, a, b, ta, tile, split), (tile, ta, M, N, Kd, split))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("how", ["padded", "unpadded", "offset", "sub"])
def test_ragged_rows_and_fallbacks(K, tile, ta, tb, how):
    """M = 130 / N = 257 (not multiples of 4) with NaN all around the operands: padded rows and column sub-views
    are read in place (granules straddle into the NaN), unpadded rows and a view off 16-byte alignment fall back
    to the copies; same bits either way and no NaN in C"""
    for Kd, split in ((33, 1), (97, 2)):
        a, b = _data(130, 257, Kd)
        _same(_three(K, a, b, ta, tile, split, how), (tile, ta, how, Kd, split))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_epilogues(K, tile, ta, tb):
    """DTANH with aux (the denoiser backward's NN call; leaves through the LDS epilogue, which reuses the stage
    buffers) and NONE into a C with ldc > N (the columns beside C stay untouched)"""
    M, N, Kd = 132, 260, 97
    a, b = _data(M, N, Kd)
    aux = _dev(np.tanh(_rng(73).standard_normal((M, N))).astype(np.float32))
    _same(_three(K, a, b, ta, tile, epi=K.EPI_DTANH, aux=aux, alpha=0.5), (tile, ta, "dtanh"))
    wide = []

    def mk_c():
        wide.append(torch.full((M, N + 12), 7.0, device=DEV))
        return wide[-1][:, :N]

    _same(_three(K, a, b, ta, tile, mk_c=mk_c), (tile, ta, "ldc"))
    for w in wide:
        assert (w[:, N:] == 7.0).all()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_edge_values(K, tile, ta, tb):
    """test_pipelined_edge_values' inputs (|x| up to FLT_MAX, subnormals, -0; then inf / NaN operands): the in-place
    and the copy path agree on every bit that is not a NaN and on where the NaNs are"""
    M, N, Kd = 64, 64, 256
    rng = _rng(39)
    a = rng.standard_normal((M, Kd)).astype(np.float32)
    b = (rng.standard_normal((N, Kd)) * 1e-30).astype(np.float32)
    a[3, :] = np.float32(3.3999e38) * np.sign(a[3, :])
    a[5, 7] = np.float32(np.finfo(np.float32).max)
    a[7, ::3] = np.float32(1e-41) * np.sign(a[7, ::3])
    a[9, ::2] = np.float32(-0.0)
    b[11, ::5] = np.float32(-0.0)
    outs = _three(K, a, b, ta, tile)
    assert torch.isfinite(outs[0]).all()
    _same(outs, (tile, ta, "finite"))
    a2 = a.copy()
    a2[0, 0], a2[1, 1], a2[2, 2] = np.inf, -np.inf, np.nan
    b2 = (np.abs(b) + 1e-31).astype(np.float32)
    inpl, copy, nt = _three(K, a2, b2, ta, tile)
    for other in (copy, nt):
        nan = torch.isnan(inpl)
        assert torch.equal(nan, torch.isnan(other))
        assert torch.equal(_bits(inpl)[~nan], _bits(other)[~nan])
    assert torch.isnan(inpl[2]).all() and not torch.isnan(inpl[3:]).any()  # (the NaN row, and only rows 0 - 2)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_against_fp64(K, tile, ta, tb):
    """and it is the product: both paths skipping a tile would still agree with each other.  Positive operands, so
    no sum cancels and a relative bound alone holds: fp32-accurate sums of K = 1,000 terms sit near 1e-7"""
    a, b = _data(300, 200, 1000)
    a, b = np.abs(a) + np.float32(0.25), np.abs(b) + np.float32(0.25)
    ref = torch.as_tensor(a.astype(np.float64) @ b.astype(np.float64).T, device=DEV)
    for split in (1, 2):
        outs = _three(K, a, b, ta, tile, split)
        _same(outs, (tile, ta, split))
        torch.testing.assert_close(outs[0].double(), ref, rtol=1e-4, atol=0.0)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_workspace_bound(K, tile, ta, tb, monkeypatch):
    """gmr_gemm_workspace_floats of a call is enough for it (the call runs on a workspace of exactly that size, in
    place and copying) and the in-place call's is not larger than the copy plan's"""
    from gmr import _lib
    lib = _lib.load()
    sizes = []
    monkeypatch.setattr(K, "workspace", lambda n, device, tag="gemm": (sizes.append(n),
                                                                        torch.zeros(n, device=device))[1])
    for (M, N, Kd, split), how in (((132, 260, 97, 2), "padded"), ((130, 257, 33, 1), "padded"),
                                   ((130, 257, 97, 2), "unpadded"), ((300, 200, 1000, 1), "sub")):
        need = [int(lib.gmr_gemm_workspace_floats(ta, tb, M, N, Kd, tile | X6 | f, split)) for f in (0, COPY)]
        assert 0 < need[0] <= need[1]
        a, b = _data(M, N, Kd)
        del sizes[:]
        _same(_three(K, a, b, ta, tile, split, how), (tile, ta, M, N, Kd, split, how))
        assert sizes[:2] == need, (sizes, need)
