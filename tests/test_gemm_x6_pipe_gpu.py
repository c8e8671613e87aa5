"""The pipelined k loop of the split-bf16 GEMM (tile | GMR_GEMM_X6_PIPE1, gemm_x6.hip PIPE 1): the next k tile is
split into the free LDS buffer between the MFMAs of the current one.  Same plan, same plane images, same MFMA
order as the plain loop, so every output is the plain loop's bit for bit; the shapes are the smallest that reach
every path of the loop (no full k tile, the fetch clamp at 1 / 2 / 3 tiles, a partial last tile, split-K slabs,
ragged edges, more than one tile per dimension)."""
import numpy as np
import pytest
import torch

from test_kernels_gpu import X6, F32, X6_RATIO, X6_FLOOR, X6_ABS, DEV, K, _dev, _rng  # noqa: F401  (K: fixture)

pytestmark = pytest.mark.gpu

PIPE1 = 1 << 28  # GMR_GEMM_X6_PIPE1 (include/gmr.h)
TILES = (128, 256128, 128256)


def _bits(t):
    return t.view(torch.int32)


def _operands(rng, M, N, Kd):
    """k-contiguous A [M][Kd], B [N][Kd] with rows padded to 16 bytes (the split kernel's float4 granules)"""
    pad = lambda x: np.pad(x, ((0, 0), (0, (-x.shape[1]) % 4))).astype(np.float32)  # noqa: E731
    a = rng.standard_normal((M, Kd)).astype(np.float32)
    b = rng.standard_normal((N, Kd)).astype(np.float32)
    return _dev(pad(a))[:, :Kd], _dev(pad(b))[:, :Kd]


def _pair(K, A, B, M, N, tile, **kw):
    """the same call on the plain and on the pipelined loop; C starts from the same (non-zero) image"""
    init = kw.pop("init", None)
    outs = []
    for flag in (0, PIPE1):
        C = init.clone() if init is not None else torch.full((M, N), 7.0, device=DEV)
        if kw.get("aux") == "C":
            K.gemm(A, B, C, tile=tile | X6 | flag, **dict(kw, aux=C))
        else:
            K.gemm(A, B, C, tile=tile | X6 | flag, **kw)
        outs.append(C)
    return outs


@pytest.mark.parametrize("tile", TILES)
def test_pipelined_equals_plain_bit_exact(K, tile):
    rng = _rng(61)
    for M, N in ((128, 128), (130, 257), (300, 200)):
        for Kd in (1, 31, 32, 33, 64, 97, 1000):
            A, B = _operands(rng, M, N, Kd)
            for split in ((1, 2) if Kd in (97, 1000) else (1,)):
                plain, piped = _pair(K, A, B, M, N, tile, trans_b=True, split_k=split)
                assert torch.equal(_bits(plain), _bits(piped)), (tile, M, N, Kd, split)
                if Kd == 97 and split == 1:  # and it is the product (a pipelined loop that skipped a tile would
                    ref = A.double() @ B.double().t()  # still have to match the plain one; this pins both)
                    torch.testing.assert_close(piped.double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("tile", TILES)
def test_pipelined_epilogues_bit_exact(K, tile):
    """BIAS_TANH with a per-row bias index, the in-place POSTERIOR (the LDS epilogue reuses the stage buffers after
    the loop) and SCALE_BIAS, at a ragged shape with a partial last k tile"""
    rng = _rng(62)
    M, N, Kd, T = 130, 257, 97, 5
    A, B = _operands(rng, M, N, Kd)
    eb = _dev(rng.standard_normal((T, N)).astype(np.float32))
    t = _dev(rng.integers(0, T, size=M), torch.int32)
    bias = _dev(rng.standard_normal(N).astype(np.float32))
    aux = _dev(rng.standard_normal((M, N)).astype(np.float32))
    acc = A.double() @ B.double().t()
    cases = (
        (dict(epi=K.EPI_BIAS_TANH, bias=eb, bias_row=t, ld_bias=N), None, torch.tanh(acc + eb.double()[t.long()])),
        (dict(epi=K.EPI_POSTERIOR, bias=bias, aux="C", slope=0.25, beta=0.75), aux,
         0.25 * (acc + bias.double()) + 0.75 * aux.double()),
        (dict(epi=K.EPI_SCALE_BIAS, bias=bias, slope=0.25), None, 0.25 * (acc + bias.double())),
    )
    for kw, init, want in cases:
        plain, piped = _pair(K, A, B, M, N, tile, trans_b=True, init=init, **kw)
        assert torch.equal(_bits(plain), _bits(piped)), (tile, kw["epi"])
        torch.testing.assert_close(piped.double(), want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("tile", TILES)
def test_pipelined_fp32_accuracy(K, tile):
    """test_gemm_x6_fp32_accuracy's bar through the pipelined loop: the error against an fp64 product is within
    X6_RATIO of the fp32-input MFMA kernel's on the same operands (+ X6_FLOOR) and below X6_ABS, with row scales
    spanning 2^-20 .. 2^20, K not a multiple of 32 or 4, and split-K slabs"""
    rng = _rng(37)
    for M, N, Kd, split in ((300, 200, 1000, 1), (19, 33, 7, 1), (640, 384, 1001, 2)):
        a = rng.standard_normal((M, Kd)) * np.exp2(rng.integers(-20, 21, size=(M, 1)))
        b = rng.standard_normal((N, Kd))
        pad = lambda x: np.pad(x, ((0, 0), (0, (-x.shape[1]) % 4))).astype(np.float32)  # noqa: E731
        A, B = _dev(pad(a))[:, :Kd], _dev(pad(b))[:, :Kd]
        a64, b64 = A.double(), B.double()
        ref, scale = a64 @ b64.t(), a64.abs() @ b64.abs().t()
        err = {}
        for flag in (X6 | PIPE1, F32):
            C = torch.empty(M, N, device=DEV)
            K.gemm(A, B, C, trans_b=True, tile=tile | flag, split_k=split)
            err[flag] = ((C.double() - ref).abs() / scale).max().item()
        assert err[X6 | PIPE1] <= X6_RATIO * err[F32] + X6_FLOOR, (M, N, Kd, split, err)
        assert err[X6 | PIPE1] <= X6_ABS, (M, N, Kd, split, err)


@pytest.mark.parametrize("tile", TILES)
def test_pipelined_edge_values(K, tile):
    """test_gemm_x6_edge_values' inputs (|x| up to FLT_MAX, inf / NaN) plus subnormals and -0 through the pipelined
    loop: finite and accurate where the values are finite, non-finite exactly where the fp32-MFMA kernel is, and the
    plain loop's bits throughout (NaN payloads included)"""
    M, N, Kd = 64, 64, 256
    rng = _rng(39)
    a = rng.standard_normal((M, Kd)).astype(np.float32)
    b = (rng.standard_normal((N, Kd)) * 1e-30).astype(np.float32)
    a[3, :] = np.float32(3.3999e38) * np.sign(a[3, :])   # above bf16's max: RN would give inf
    a[5, 7] = np.float32(np.finfo(np.float32).max)
    a[7, ::3] = np.float32(1e-41) * np.sign(a[7, ::3])    # subnormals
    a[9, ::2] = np.float32(-0.0)
    b[11, ::5] = np.float32(-0.0)
    A, B = _dev(a), _dev(b)
    ref = torch.as_tensor(a.astype(np.float64) @ b.astype(np.float64).T, device=DEV)
    scale = torch.as_tensor(np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T, device=DEV)
    plain, piped = _pair(K, A, B, M, N, tile, trans_b=True)
    assert torch.equal(_bits(plain), _bits(piped))
    assert torch.isfinite(piped).all()
    assert (((piped.double() - ref).abs()) / scale).max().item() <= X6_ABS
    a2 = a.copy()
    a2[0, 0], a2[1, 1], a2[2, 2] = np.inf, -np.inf, np.nan
    b2 = (np.abs(b) + 1e-31).astype(np.float32)
    plain, piped = _pair(K, _dev(a2), _dev(b2), M, N, tile, trans_b=True)
    assert torch.equal(_bits(plain), _bits(piped))
    C32 = torch.empty(M, N, device=DEV)
    K.gemm(_dev(a2), _dev(b2), C32, trans_b=True, tile=128 | F32)
    assert torch.equal(torch.isfinite(piped), torch.isfinite(C32))
    fin = torch.isfinite(C32)
    sc2 = torch.as_tensor(np.abs(np.nan_to_num(a2, posinf=0, neginf=0)).astype(np.float64) @ b2.astype(np.float64).T,
                          device=DEV)
    assert ((piped - C32).double().abs()[fin] / sc2[fin]).max().item() <= 2 * X6_ABS


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ta,tb", [(1, 0), (0, 0)])
def test_pipelined_tn_nn_bit_exact(K, tile, ta, tb):
    """TN / NN calls with the flag run as NT on the k-contiguous copies of their operands, through the pipelined
    loop: the unflagged call's bits"""
    rng = _rng(63)
    M, N, Kd = 257, 130, 97
    pad = lambda x: np.pad(x, ((0, 0), (0, (-x.shape[1]) % 4)))  # noqa: E731
    a = rng.standard_normal((M, Kd)).astype(np.float32)
    b = rng.standard_normal((N, Kd)).astype(np.float32)
    A = _dev(pad(a.T))[:, :M] if ta else _dev(pad(a))[:, :Kd]
    B = _dev(pad(b.T))[:, :N]
    plain, piped = _pair(K, A, B, M, N, tile, trans_a=bool(ta), trans_b=bool(tb))
    assert torch.equal(_bits(plain), _bits(piped)), (tile, ta, tb)
    torch.testing.assert_close(piped.double(), A.double().t() @ B.double() if ta else A.double() @ B.double(),
                               rtol=1e-4, atol=1e-4)
