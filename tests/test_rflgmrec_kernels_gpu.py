"""The kernels RFLGMRec adds, called by name past the tiny golden shape.

  gmr_rf_view_sum_prior  (U, I) = (1, 1) both priors exactly zero; (127, 129) and (128, 128) around the 128-row block;
                         (300, 1100) 3 + 9 blocks with both last blocks short.  a and b the two column blocks of one
                         128-wide table, prior a 64-column block of a 68-wide NaN-filled table, the workspace
                         NaN-filled.
                         Against torch fp64 of Z = a + b at the project's bar: rtol 1e-5 with an atol of twice fp32 CPU
                         torch's own error on the same formula.  Two runs bit-equal; bad arguments raise by name.
  gmr_rf_sample_mix      C = 128, L = 2, 3 steps, N = 1, 31, 32, 33, 97 (one row, a short tile, a full tile, a tile and
                         one row, three tiles and one row), base at strides 64 and 128, out a 64-column block of a
                         68-wide NaN-filled table.  The result is base + ratio * z with z the plain entry's fp32 rows,
                         formed in fp64, within one fp32 rounding of the sum: |err| <= 2^-23 (|base| + |ratio z|)
                         elementwise (derived: the fused kernel rounds the sum once; 2^-24 of |result| <= |base| +
                         |ratio z| would do for the fused multiply-add alone, 2^-23 also covers a separate product).
                         ratio = 0 returns base bit for bit; the ratio is read from the device at run time.
"""
import numpy as np
import pytest
import torch

import rflgmrec_fixture as RL

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D, C = 128, 64, 128
NAN = float("nan")


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


# ------------------------------------------------------------------------------------------------ the prior
def _views(U, I, seed):
    """One N x 128 table [a | b]: unit spread around column means of about 0.5, the two segments' means 2 apart."""
    rng = np.random.default_rng(seed)
    N = U + I
    tab = rng.standard_normal((N, 2 * D)) + 0.5
    tab[:, :D] += np.where(np.arange(N) < U, 1.5, -0.5)[:, None]
    return tab.astype(np.float32)


def _run_prior(U, I, tab):
    from gmr import _lib
    N = U + I
    t = dev(tab)
    prior = torch.full((N, 68), NAN, device=DEV)
    n = int(_lib.load().gmr_rf_view_sum_prior_ws_floats(U, I))
    assert n == (-(-U // 128) + -(-I // 128) + 2) * 64 == int(_lib.load().gmr_rf_view_prior_ws_floats(U, I))
    ws = torch.full((n,), NAN, device=DEV)
    _call("gmr_rf_view_sum_prior", U, I, _ptr(t), 128, _ptr(t[:, D:]), 128, _ptr(prior), 68, _ptr(ws))
    return prior.cpu().numpy()


@pytest.mark.parametrize("U,I", [(1, 1), (127, 129), (128, 128), (300, 1100)])
def test_view_sum_prior(U, I):
    tab = _views(U, I, U + I)
    got = _run_prior(U, I, tab)
    assert np.isnan(got[:, D:]).all()   # nothing outside the block is written
    prior = got[:, :D]
    want = {}
    for dt in (torch.float64, torch.float32):
        t = torch.tensor(tab, dtype=dt)
        want[dt] = RL.prior_ref(t[:, :D], t[:, D:], U).numpy().astype(np.float64)
    w = want[torch.float64]
    own = float(np.abs(want[torch.float32] - w).max())
    err = np.abs(prior - w)
    print(f"view sum prior U={U} I={I}: max abs error {err.max():.3e} (fp32 torch {own:.3e}; largest |prior| "
          f"{np.abs(w).max():.3f})")
    np.testing.assert_allclose(prior, w, rtol=1e-5, atol=2 * own)
    if U == 1 and I == 1:
        assert not prior.any()   # a single row is its own mean
    else:
        z = tab[:, :D].astype(np.float64) + tab[:, D:]
        assert np.abs(prior - (z - z.mean(0))).max() > 0.1    # one mean over all N rows is another table
        assert np.abs(prior - 0.5 * w).max() > 0.1            # and so is the mean of the views (gmr_rf_view_prior)
    assert np.array_equal(_run_prior(U, I, tab)[:, :D], prior)   # fixed-order sums, no float atomics


def test_view_sum_prior_rejects_bad_arguments():
    from gmr import _lib
    U, I = 5, 3
    N = U + I
    tab = torch.ones((N, 128), device=DEV)
    prior = torch.full((N, 68), NAN, device=DEV)
    ws = torch.full((int(_lib.load().gmr_rf_view_sum_prior_ws_floats(U, I)),), NAN, device=DEV)
    p, pp, pw = tab.data_ptr(), prior.data_ptr(), ws.data_ptr()   # byte addresses
    ok = [U, I, p, 128, p + 256, 128, pp, 68, pw]
    for i, v in ((0, 0), (1, 0),                                  # an empty segment
                 (2, None), (4, None), (6, None), (8, None),      # null pointers
                 (2, p + 4), (4, p + 260), (6, pp + 8), (8, pw + 4),   # misaligned
                 (3, 126), (5, 130), (7, 70),                     # strides that are no multiple of 4
                 (3, 60), (5, 32), (7, 60)):                      # too narrow
        args = list(ok)
        args[i] = v
        with pytest.raises(RuntimeError, match="gmr_rf_view_sum_prior"):
            _call("gmr_rf_view_sum_prior", *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(prior).all()) and bool(torch.isnan(ws).all())
    assert int(_lib.load().gmr_rf_view_sum_prior_ws_floats(0, 3)) == -1
    assert int(_lib.load().gmr_rf_view_sum_prior_ws_floats(3, 0)) == -1
    _call("gmr_rf_view_sum_prior", *ok)
    assert bool(torch.isfinite(prior[:, :D]).all())


# ------------------------------------------------------------------------------------------------ the sampler's mix
def _generator(N, seed, L=2):
    """An RFGenerator at C = 128 on N = U + I rows with its LayerNorm weights and biases away from 1 / 0."""
    from gmr.rf import RFGenerator
    torch.manual_seed(seed)
    gen = RFGenerator(N // 2, N - N // 2, C, DEV, n_layers=L, dropout=0.1, sampling_steps=3, n_negatives=7)
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for (name, sh), v in zip(gen.specs, gen.param_views()):
            if len(sh) == 1:
                v.add_(dev((0.1 * rng.standard_normal(sh)).astype(np.float32)))
    return gen


def _mix(gen, N, cond, z0, base, ldb, ratio, n_steps=3):
    """gmr_rf_sample_mix by name: base a view of stride ldb, out columns 0..63 of a NaN-filled N x 68 table."""
    bw = torch.full((N, ldb), 1e30, device=DEV)
    bw[:, :D] = base
    outw = torch.full((N, 68), NAN, device=DEV)
    _call("gmr_rf_sample_mix", N, H, C, gen.L, n_steps, _ptr(z0), D, _ptr(cond), C, _ptr(gen.slab.data), _ptr(bw), ldb,
          _ptr(ratio), _ptr(outw), 68)
    return outw


@pytest.mark.parametrize("ldb", [64, 128])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 97])
def test_sample_mix(N, ldb):
    gen = _generator(N, 10 + N)
    rng = np.random.default_rng(3 * N + ldb)
    cond = dev(rng.standard_normal((N, C)).astype(np.float32))
    z0 = dev(rng.standard_normal((N, D)).astype(np.float32))
    base = dev((2.0 * rng.standard_normal((N, D))).astype(np.float32))
    ratio = torch.tensor([0.2], dtype=torch.float32, device=DEV)
    z = torch.full((N, D), NAN, device=DEV)
    _call("gmr_rf_sample", N, H, C, gen.L, 3, _ptr(z0), D, _ptr(cond), C, _ptr(gen.slab.data), _ptr(z), D)
    assert bool(torch.isfinite(z).all())
    outw = _mix(gen, N, cond, z0, base, ldb, ratio)
    assert bool(torch.isnan(outw[:, D:]).all())   # the padding columns are not written
    out = outw[:, :D].double().cpu().numpy()
    r = float(ratio.item())   # the fp32 value the kernel reads
    b64, rz = base.double().cpu().numpy(), r * z.double().cpu().numpy()
    err = np.abs(out - (b64 + rz))
    bound = 2.0 ** -23 * (np.abs(b64) + np.abs(rz))
    print(f"sample mix N={N} ldb={ldb}: max err / bound {np.max(err / bound):.3f}, max abs err {err.max():.3e}")
    assert (err <= bound).all()
    assert float((outw[:, :D] - base).abs().max()) > 1e-2    # the rows did move
    # ratio = 0: base bit for bit
    ratio.zero_()
    assert torch.equal(_mix(gen, N, cond, z0, base, ldb, ratio)[:, :D], base)
    # the scalar is read on the device at run time: another value, another table, the same host-side arguments
    ratio.fill_(-1.5)
    out2 = _mix(gen, N, cond, z0, base, ldb, ratio)[:, :D].double().cpu().numpy()
    rz2 = -1.5 * z.double().cpu().numpy()
    assert (np.abs(out2 - (b64 + rz2)) <= 2.0 ** -23 * (np.abs(b64) + np.abs(rz2))).all()
    assert np.abs(out2 - out).max() > 1e-2


def test_generate_with_base_fused_and_composed():
    """RFGenerator.generate(base=): the fused entry and the composed copy + axpy path give the same table within the
    two roundings of the composed one next to the sampler's own fused-against-composed spread."""
    N = 97
    gen = _generator(N, 5)
    rng = np.random.default_rng(5)
    cond = dev(rng.standard_normal((N, C)).astype(np.float32))
    z0 = dev(rng.standard_normal((N, D)).astype(np.float32))
    wide = dev(rng.standard_normal((N, 2 * D)).astype(np.float32))
    base = wide[:, D:]   # a strided view, as cge never is but E's blocks may be
    z = gen.generate(cond, z0=z0)
    a = gen.generate(cond, z0=z0, base=base, out=torch.full((N, D), NAN, device=DEV))
    want = base.double() + gen.inference_mix_ratio * z.double()
    assert float((a.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    zc = gen.generate(cond, z0=z0, fused=False)
    b = gen.generate(cond, z0=z0, base=base, out=torch.full((N, D), NAN, device=DEV), fused=False)
    wantc = base.double() + gen.inference_mix_ratio * zc.double()
    assert float((b.double() - wantc).abs().max()) <= 2.0 ** -22 * float(wantc.abs().max())
    gen._ratio.fill_(0.5)   # what a captured graph would see: the device scalar, not the Python attribute
    c = gen.generate(cond, z0=z0, base=base)
    assert float((c.double() - (base.double() + 0.5 * z.double())).abs().max()) <= 2.0 ** -22 * float(c.abs().max())
    with pytest.raises(ValueError, match="base"):
        gen.generate(cond, z0=z0, base=wide)


def test_sample_mix_rejects_bad_arguments():
    N = 8
    gen = _generator(N, 0)
    z0, cond = torch.zeros((N, D), device=DEV), torch.zeros((N, C), device=DEV)
    base = torch.zeros((N, 128), device=DEV)
    out = torch.full((N, 68), NAN, device=DEV)
    ratio = torch.tensor([0.2], device=DEV)
    pb, po = base.data_ptr(), out.data_ptr()
    ok = [N, H, C, 2, 1, _ptr(z0), D, _ptr(cond), C, _ptr(gen.slab.data), pb, 128, _ptr(ratio), po, 68]
    for i, v in ((10, None), (12, None),           # a null base, a null ratio
                 (11, 60), (11, 66), (14, 66),     # a stride below 64, strides that are no multiple of 4
                 (10, pb + 4), (13, po + 8),       # misaligned
                 (10, po),                         # base aliasing out
                 (1, 256), (2, 96)):               # the plain entry's own checks
        args = list(ok)
        args[i] = v
        with pytest.raises(RuntimeError, match="gmr_rf_sample_mix"):
            _call("gmr_rf_sample_mix", *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    _call("gmr_rf_sample_mix", *ok)
    assert bool(torch.isfinite(out[:, :D]).all()) and bool(torch.isnan(out[:, D:]).all())
