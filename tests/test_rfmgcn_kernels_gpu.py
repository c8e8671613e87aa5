"""The entry point RFMGCN adds, by name, against the fp64 restatement of tests/rfmgcn_fixture.py (prior_ref).

  gmr_rf_view_prior   (U, I) = (1, 1) both priors exactly zero; (5, 3) smaller than a row group; (37, 41) the item
                      segment starts mid-block; (128, 128) exactly one block per segment; (129, 127) one row into a
                      second user block and a short item block; (300, 1100) 3 + 9 blocks, both last blocks short.
                      a, b and prior as views of one 128-wide table (the model's layout), as views of a 192-wide
                      table, and contiguous.  The columns past the 64 and the row after N keep a sentinel; the output is
                      filled with NaN beforehand; two runs are bit-identical.

Bar (the rule of test_rfbm3_kernels_gpu.py): rtol 1e-5 against fp64, and next to it an entry may be off by twice the
largest error in its column of the same formula done by fp32 torch on the CPU against fp64, measured here and printed.

The contamination case draws the user rows around +100 and the item rows around -100: one row of the other segment in
a segment's mean moves it by 200 / rows, so every |prior| below 10 says that no block straddled row U."""
import ctypes

import numpy as np
import pytest
import torch

import rfmgcn_fixture as RM

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64
SENT = 7.25
# (2049, 1): 17 user blocks, one more than the sixteen chains of the mean kernel, beside a one-row item segment
SHAPES = [(1, 1), (5, 3), (37, 41), (128, 128), (129, 127), (300, 1100), (2049, 1)]
LAYOUTS = ["model", "wide", "contiguous"]


def _call(name, *args):
    from gmr import _lib
    from gmr.kernels import stream
    return _lib.call(name, *args, stream())


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _ws(U, I, fill=float("nan")):
    from gmr import _lib
    n = int(_lib.load().gmr_rf_view_prior_ws_floats(U, I))
    assert n == ((U + 127) // 128 + (I + 127) // 128 + 2) * D
    return torch.full((n,), fill, device=DEV)


def _run(a_np, b_np, U, I, layout, fill):
    """The kernel on the given layout; prior pre-filled with `fill`, its spare columns and the row after N with SENT.
    Returns (prior N x 64, the whole output table) as numpy."""
    N = U + I
    if layout == "model":      # a, b the two column blocks of one 128-wide table; prior in a 128-wide table
        ab = torch.as_tensor(np.concatenate([a_np, b_np], axis=1)).to(DEV)
        a, b, lda, ldp = ab[:, :D], ab[:, D:], 128, 128
    elif layout == "wide":     # 192-wide: a first, b last, the middle block unused; prior the middle block of another
        w = np.full((N, 192), SENT, np.float32)
        w[:, :D], w[:, 128:] = a_np, b_np
        ab = torch.as_tensor(w).to(DEV)
        a, b, lda, ldp = ab[:, :D], ab[:, 128:], 192, 192
    else:
        ab = None
        a, b, lda, ldp = torch.as_tensor(a_np).to(DEV), torch.as_tensor(b_np).to(DEV), D, D
    out = torch.full((N + 1, ldp), SENT, device=DEV)
    c0 = D if layout == "wide" else 0
    out[:N, c0:c0 + D] = fill
    prior = out[:N, c0:c0 + D]
    ws = _ws(U, I)
    _call("gmr_rf_view_prior", U, I, _ptr(a), lda, _ptr(b), lda, _ptr(prior), ldp, _ptr(ws))
    torch.cuda.synchronize()
    full = out.cpu().numpy()
    # nothing outside the N x 64 block is written
    keep = np.ones_like(full, bool)
    keep[:N, c0:c0 + D] = False
    assert (full[keep] == SENT).all(), "a sentinel was overwritten"
    return full[:N, c0:c0 + D]


def _refs(a_np, b_np, U):
    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = RM.prior_ref(torch.tensor(a_np, dtype=dt), torch.tensor(b_np, dtype=dt), U).numpy()
    return ref[torch.float64], ref[torch.float32].astype(np.float64)


def _check(got, a_np, b_np, U, what):
    r64, r32 = _refs(a_np, b_np, U)
    own = np.abs(r32 - r64).max(axis=0)
    err = np.abs(got.astype(np.float64) - r64)
    print(f"{what}: max abs error {err.max():.3e} (fp32 torch {own.max():.3e})")
    assert np.isfinite(got).all(), what
    assert (err <= 1e-5 * np.abs(r64) + 2 * own[None, :]).all(), what
    return r64


@pytest.mark.parametrize("U,I", SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_view_prior(U, I, layout):
    rng = np.random.default_rng(1000 * U + I)
    a = (rng.standard_normal((U + I, D)) + 0.5).astype(np.float32)  # a mean next to the spread
    b = (rng.standard_normal((U + I, D)) * 0.5 - 0.25).astype(np.float32)
    got = _run(a, b, U, I, layout, float("nan"))
    _check(got, a, b, U, f"prior U={U} I={I} {layout}")
    if (U, I) == (1, 1):
        assert not got.any()  # a single row is its own mean
    # a second run over other leftovers: bit-identical
    assert np.array_equal(got, _run(a, b, U, I, layout, -3.0))


@pytest.mark.parametrize("U,I", SHAPES[1:])
def test_view_prior_segments_do_not_mix(U, I):
    rng = np.random.default_rng(7 * U + I)
    off = np.concatenate([np.full((U, 1), 100.0), np.full((I, 1), -100.0)])
    a = (off + rng.standard_normal((U + I, D))).astype(np.float32)
    b = (off + rng.standard_normal((U + I, D))).astype(np.float32)
    got = _run(a, b, U, I, "model", float("nan"))
    assert np.isfinite(got).all() and np.abs(got).max() < 10, np.abs(got).max()
    # Next to fp64 the values only say how fp32 rounds a mean of numbers near 100, which the per-column rule above
    # cannot judge: a column's error is here one rounding of its mean, shared by all its rows, so fp32 torch's own
    # error in that column is one draw of the same size and may be any fraction of the kernel's (seen on the MI355X at
    # (37, 41): 2.0e-5 against 2.1e-5 over the table, yet a column at 2.0e-5 against 0.65e-5).  The bound is the
    # worst case of the kernel's own order instead: an entry passes 7 additions in its row group, 15 over the groups,
    # 2 + 15 over the sixteen chains of block partials (up to 17 blocks: at most two per chain), then the rounding of
    # a + b, of the division and of the subtraction: 42 <= 48 half-ulps at the magnitude of Z.  It is 3e-4 here; one
    # foreign row would move a mean by 200 / rows >= 0.18.
    r64, _ = _refs(a, b, U)
    zmax = float(np.abs(0.5 * (a.astype(np.float64) + b)).max())
    err = np.abs(got.astype(np.float64) - r64).max()
    print(f"contamination U={U} I={I}: max abs error {err:.3e} (bound {48 * 2.0 ** -24 * zmax:.3e})")
    assert err <= 48 * 2.0 ** -24 * zmax


def test_view_prior_bad_args():
    U, I = 5, 3
    ab = torch.zeros((U + I, 128), device=DEV)
    prior = torch.full((U + I, D), SENT, device=DEV)
    ws = _ws(U, I, 0.0)
    ok = [U, I, _ptr(ab), 128, _ptr(ab[:, D:]), 128, _ptr(prior), D, _ptr(ws)]
    _call("gmr_rf_view_prior", *ok)
    torch.cuda.synchronize()
    assert not prior.any()
    prior.fill_(SENT)
    off1 = ctypes.c_void_p(ab.data_ptr() + 4)  # one float in: not 16-byte aligned
    for pos, val in ((0, 0), (1, 0), (4, None), (3, 66), (5, 66), (7, 66), (7, 32), (2, off1), (6, None), (8, None)):
        bad = list(ok)
        bad[pos] = val
        with pytest.raises(RuntimeError, match="gmr_rf_view_prior"):
            _call("gmr_rf_view_prior", *bad)
    torch.cuda.synchronize()
    assert bool((prior == SENT).all())  # the argument error comes before any launch
    from gmr import _lib
    assert int(_lib.load().gmr_rf_view_prior_ws_floats(0, 3)) == -1
    assert int(_lib.load().gmr_rf_view_prior_ws_floats(3, 0)) == -1
