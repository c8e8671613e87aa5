"""The width-taking RF entry points (csrc/rf.hip gmr_rf_*_w, csrc/rf_prior.hip gmr_rf_center_segments) by name, at the
widths RFGRCN runs (128 and 192) and at shapes past its golden record, against torch fp64 of the same formula
(tests/rf_fixture.py, tests/rfbm3_fixture.py: their formulas take the widths from the tensors).

Bars, the project's three: the sampler bar (4x the fp32 CPU run's error against the fp64 run, absolute, floored at
1e-6 of the largest value), the gradient bar (the same rule relative to the parameter's largest gradient, floored at
1e-6) and the table bar (rtol 1e-5, atol 2e-6); losses at rtol 1e-5.  Every test prints what it saw next to its bar.

Seen on the MI355X (largest over the cases of each test):
  centring              max abs error 3.1e-07 on entries up to 5 (table bar: 1e-5 |x| + 2e-6)
  sampler, fused        8.8e-07 at a bar of 4.3e-06 ((128, 128), L 2, 1 step); composed 4.7e-07; the mix 2.5e-07 at its
                        bar of 1.7e-06
  head                  V 1.2e-07 of the largest entry (fp32 torch 1.2e-07 .. 1.5e-07), the clamped rows included
  head, zero prior      V, pred and row parts equal to the plain head's bit for bit at 128 and 192
  InfoNCE contrib       2.7e-07 of the largest entry at a bar of 1.0e-06 (the floor)
  train step (192)      worst gradient 5.0e-07 of the parameter's largest at a bar of 1.0e-06; losses to seven digits
  train step (128)      worst gradient 7.7e-07 at a bar of 1.2e-06
"""
import numpy as np
import pytest
import torch

import rf_fixture as R
import rfbm3_fixture as RB
import rfgrcn_fixture as RG

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 1.0e30
H = 128
PAIRS = [(128, 128), (192, 192)]


def _lib():
    from gmr import _lib as lib
    return lib


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _stream():
    from gmr.kernels import stream
    return stream()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _block(n, width, lead, trail, fill):
    """An n x width column block (from column `lead`) of a table filled with `fill`; returns (table, view)."""
    tab = torch.full((n, lead + width + trail), fill, dtype=torch.float32, device=DEV)
    return tab, tab[:, lead:lead + width]


def _slab(P, C, L, D):
    """The packed parameters of {name: array} in gmr.rf.param_specs order, 16-byte aligned on the device."""
    from gmr.rf import param_specs
    flat = np.concatenate([np.asarray(P[n], np.float32).reshape(-1) for n, _ in param_specs(C, L, D)])
    assert flat.size == int(_lib().load().gmr_rf_param_floats_w(D, C, L))
    return _dev(flat)


# ------------------------------------------------------------------------------------------------ packed layout
def test_param_floats_w():
    from gmr.rf import param_specs
    lib = _lib().load()
    for D, C in [(64, 64), (64, 128), (64, 192), (128, 128), (192, 192)]:
        for L in range(1, 5):
            want = sum(int(np.prod(sh)) for _, sh in param_specs(C, L, D))
            assert int(lib.gmr_rf_param_floats_w(D, C, L)) == want, (D, C, L)
            if D == 64:
                assert int(lib.gmr_rf_param_floats(C, L)) == want
    assert int(lib.gmr_rf_param_floats_w(192, 192, 2)) == 166848 and int(lib.gmr_rf_param_floats_w(128, 128, 2)) == 142208
    for D, C, L in [(192, 128, 2), (128, 192, 2), (96, 96, 2), (256, 256, 2), (192, 192, 0), (192, 192, 5),
                    (128, 128, 0), (128, 128, 5)]:
        assert int(lib.gmr_rf_param_floats_w(D, C, L)) == -1, (D, C, L)


# ------------------------------------------------------------------------------------------------ centring
@pytest.mark.parametrize("W", [64, 128, 192])
@pytest.mark.parametrize("U,I", [(1, 1), (127, 129), (128, 128), (300, 2100)])
def test_center_segments(W, U, I):
    lib = _lib()
    N = U + I
    rng = np.random.default_rng(U * 1000 + W)
    x = rng.standard_normal((N, W)).astype(np.float32)
    x[:U] += 1.0   # the two segments' means differ by 2
    x[U:] -= 1.0
    stab, src = _block(N, W, 64, 4, SENT)
    src.copy_(_dev(x))
    ptab, prior = _block(N, W, 4, 8, NAN)
    ws = torch.zeros(int(lib.load().gmr_rf_center_segments_ws_floats(U, I, W)), dtype=torch.float32, device=DEV)
    lib.call("gmr_rf_center_segments", U, I, W, _ptr(src), src.stride(0), _ptr(prior), prior.stride(0), _ptr(ws),
             _stream())
    got = prior.cpu().numpy()
    x64 = torch.tensor(x, dtype=torch.float64)
    want = RG.prior_ref(x64, U).numpy()
    err = float(np.abs(got - want).max())
    print(f"centring W {W} U {U} I {I}: max abs error {err:.3e} (table bar rtol 1e-5, atol 2e-6)")
    np.testing.assert_allclose(got, want, **RG.TABLE)
    if (U, I) == (1, 1):
        assert not got.any(), "a segment of one row is its own mean"
    else:
        assert abs(float(want[:U].mean())) < 1e-9 and float((x64[:U].mean(0) - x64[U:].mean(0)).abs().min()) > 1.0
    out = ptab.cpu().numpy()
    assert np.isnan(out[:, :4]).all() and np.isnan(out[:, 4 + W:]).all(), "nothing outside the block is written"
    assert bool((stab[:, :64] == SENT).all()) and bool((stab[:, 64 + W:] == SENT).all())
    again = torch.full_like(ptab, NAN)
    lib.call("gmr_rf_center_segments", U, I, W, _ptr(src), src.stride(0), _ptr(again[:, 4:]), again.stride(0), _ptr(ws),
             _stream())
    assert torch.equal(again[:, 4:4 + W], prior), "two runs are bit-identical"


def test_center_segments_rejects_bad_arguments():
    lib = _lib()
    x = torch.zeros((8, 192), dtype=torch.float32, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float32, device=DEV)
    assert int(lib.load().gmr_rf_center_segments_ws_floats(4, 4, 96)) == -1
    assert int(lib.load().gmr_rf_center_segments_ws_floats(0, 4, 64)) == -1
    for U, I, W, lds in [(4, 4, 96, 192), (0, 8, 64, 192), (4, 4, 192, 128), (4, 4, 64, 190)]:
        with pytest.raises(RuntimeError, match="gmr_rf_center_segments"):
            lib.call("gmr_rf_center_segments", U, I, W, _ptr(x), lds, _ptr(x), 192, _ptr(ws), _stream())


# ------------------------------------------------------------------------------------------------ sampler
NS = [1, 31, 32, 33, 97]


@pytest.fixture(scope="module")
def sampler_refs():
    """{(D, L, n_steps): (P, cond, z0, base, ref64, ref32)} at N = 97, computed once; a row's result does not depend
    on N, so the first N rows are the reference of every smaller N."""
    refs = {}

    def get(D, L, n_steps):
        key = (D, L, n_steps)
        if key not in refs:
            rng = np.random.default_rng(100 * D + 10 * L + n_steps)
            P = RG.random_params(rng, D, L, D)
            cond = rng.standard_normal((97, D)).astype(np.float32)
            z0 = rng.standard_normal((97, D)).astype(np.float32)
            base = rng.standard_normal((97, D)).astype(np.float32)
            r64 = RG.generate_ref(P, cond, z0, n_steps, L, torch.float64)
            r32 = RG.generate_ref(P, cond, z0, n_steps, L, torch.float32)
            refs[key] = (P, cond, z0, base, r64, r32)
        return refs[key]

    return get


@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("D,C", PAIRS)
def test_sample_w(sampler_refs, D, C, L, n_steps):
    from gmr.rf import RFGenerator
    lib = _lib()
    P, cond, z0, base, r64, r32 = sampler_refs(D, L, n_steps)
    bar = RG.sampler_bar(r32, r64)
    slab = _slab(P, C, L, D)
    ratio = torch.tensor([0.2], dtype=torch.float32, device=DEV)
    worst = {"fused": 0.0, "composed": 0.0, "mix": 0.0}
    # the mix rounds base + ratio z once more: 0.2 of the sampler bar next to one fp32 rounding of the mixed value
    mix_bar = 0.2 * bar + 2.0 ** -23 * float((np.abs(base) + np.abs(cond) + 0.2 * np.abs(r64)).max())
    for N in NS:
        ctab, cv = _block(N, C, 8, 4, SENT)
        cv.copy_(_dev(cond[:N]))
        z = _dev(z0[:N])
        otab, out = _block(N, D, 4, 12, NAN)
        lib.call("gmr_rf_sample_w", N, H, D, C, L, n_steps, _ptr(z), z.stride(0), _ptr(cv), cv.stride(0), _ptr(slab),
                 _ptr(out), out.stride(0), _stream())
        got = out.cpu().numpy().astype(np.float64)
        worst["fused"] = max(worst["fused"], float(np.abs(got - r64[:N]).max()))
        full = otab.cpu().numpy()
        assert np.isnan(full[:, :4]).all() and np.isnan(full[:, 4 + D:]).all() and np.isfinite(got).all(), N
        # the composed sampler of a generator of this N (the comparison path), through RFGenerator at width D
        gen = RFGenerator(N, 0, C, DEV, n_layers=L, dropout=0.0, sampling_steps=n_steps, embedding_dim=D)
        gen.load_reference_state(P)
        comp = gen.generate(cv.contiguous(), z0=z, n_steps=n_steps, fused=False).cpu().numpy().astype(np.float64)
        worst["composed"] = max(worst["composed"], float(np.abs(comp - r64[:N]).max()))
        assert np.abs(comp - got).max() <= 2 * bar, N
        fz = gen.generate(cv, z0=z, n_steps=n_steps, fused=True)
        assert torch.equal(fz, out.contiguous()), "RFGenerator.generate at width D is this launch"
        # the mix as the epilogue: base = cond (the model's case) and a base of its own
        for bv in (cv, _block(N, D, 12, 4, SENT)[1]):
            if bv is not cv:
                bv.copy_(_dev(base[:N]))
            mtab, mix = _block(N, D, 8, 8, NAN)
            lib.call("gmr_rf_sample_mix_w", N, H, D, C, L, n_steps, _ptr(z), z.stride(0), _ptr(cv), cv.stride(0),
                     _ptr(slab), _ptr(bv), bv.stride(0), _ptr(ratio), _ptr(mix), mix.stride(0), _stream())
            want = bv.cpu().numpy().astype(np.float64) + np.float64(np.float32(0.2)) * r64[:N]
            worst["mix"] = max(worst["mix"], float(np.abs(mix.cpu().numpy() - want).max()))
            mf = mtab.cpu().numpy()
            assert np.isnan(mf[:, :8]).all() and np.isnan(mf[:, 8 + D:]).all()
            # the epilogue is one fused multiply-add on the rows the plain launch writes
            fma = torch.addcmul(bv.double(), out.double(), ratio.double()).float()
            assert float((mix - fma).abs().max()) <= 1e-6 * float(fma.abs().max())
        assert bool((ctab[:, :8] == SENT).all()) and bool((ctab[:, 8 + C:] == SENT).all())
    print(f"sampler ({D}, {C}) L {L} steps {n_steps}: fused {worst['fused']:.3e}, composed {worst['composed']:.3e}, "
          f"mix {worst['mix']:.3e} (sampler bar {bar:.3e}, mix bar {mix_bar:.3e})")
    assert worst["fused"] <= bar and worst["composed"] <= bar and worst["mix"] <= mix_bar


@pytest.mark.parametrize("C", [64, 128, 192])
def test_sample_w_at_64_is_the_old_entry(C):
    lib = _lib()
    rng = np.random.default_rng(C)
    L, n_steps, N = 2, 3, 97
    slab = _slab(RG.random_params(rng, C, L, 64), C, L, 64)
    cond, z0, base = (_dev(rng.standard_normal((N, w)).astype(np.float32)) for w in (C, 64, 64))
    ratio = torch.tensor([0.2], dtype=torch.float32, device=DEV)
    a, b, c, d = (torch.full((N, 64), NAN, dtype=torch.float32, device=DEV) for _ in range(4))
    lib.call("gmr_rf_sample", N, H, C, L, n_steps, _ptr(z0), 64, _ptr(cond), C, _ptr(slab), _ptr(a), 64, _stream())
    lib.call("gmr_rf_sample_w", N, H, 64, C, L, n_steps, _ptr(z0), 64, _ptr(cond), C, _ptr(slab), _ptr(b), 64, _stream())
    lib.call("gmr_rf_sample_mix", N, H, C, L, n_steps, _ptr(z0), 64, _ptr(cond), C, _ptr(slab), _ptr(base), 64,
             _ptr(ratio), _ptr(c), 64, _stream())
    lib.call("gmr_rf_sample_mix_w", N, H, 64, C, L, n_steps, _ptr(z0), 64, _ptr(cond), C, _ptr(slab), _ptr(base), 64,
             _ptr(ratio), _ptr(d), 64, _stream())
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(c, d)


def test_sample_w_rejects_bad_widths():
    lib = _lib()
    x = torch.zeros((32, 256), dtype=torch.float32, device=DEV)
    for D, C in [(192, 128), (128, 192), (96, 96), (256, 256)]:
        with pytest.raises(RuntimeError, match="gmr_rf_sample_w"):
            lib.call("gmr_rf_sample_w", 32, H, D, C, 2, 1, _ptr(x), 256, _ptr(x), 256, _ptr(x), _ptr(x), 256, _stream())
    with pytest.raises(RuntimeError, match="gmr_rf_sample_w"):   # the row stride of out below the width
        lib.call("gmr_rf_sample_w", 32, H, 192, 192, 2, 1, _ptr(x), 256, _ptr(x), 256, _ptr(x), _ptr(x), 128, _stream())


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("D", [128, 192])
def test_interp_head_losses_w(D, N):
    lib = _lib()
    rng = np.random.default_rng(10 * D + N)
    x1 = rng.standard_normal((N, D)).astype(np.float32)
    x0 = rng.standard_normal((N, D)).astype(np.float32)
    t = rng.random((N, 1)).astype(np.float32)
    xt_in = rng.standard_normal((N, D)).astype(np.float32)
    v_in = (0.5 * rng.standard_normal((N, D))).astype(np.float32)
    pr = rng.standard_normal((N, D)).astype(np.float32)
    if N >= 3:
        x1[1] = 0.0      # a zero X1 row and a zero Xt row: the norm clamps
        xt_in[2] = 0.0
    _, X1 = _block(N, D, 64, 0, SENT)        # row stride 192 (D = 128) / 256 (D = 192) inside a wider table
    assert X1.stride(0) == D + 64
    X1.copy_(_dev(x1))
    _, prior = _block(N, D, 4, 4, SENT)
    prior.copy_(_dev(pr))
    X0, tt = _dev(x0), _dev(t.reshape(N))
    # interp
    Xt = torch.full((N, D), NAN, dtype=torch.float32, device=DEV)
    lib.call("gmr_rf_interp_w", N, D, _ptr(X1), X1.stride(0), _ptr(X0), _ptr(tt), _ptr(Xt), _stream())
    c64 = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    want = (c64(t) * c64(x1) + (1 - c64(t)) * c64(x0)).numpy()
    np.testing.assert_allclose(Xt.cpu().numpy(), want, **RG.TABLE)
    # the head, with and without the prior, on an Xt of its own (the zero row)
    for with_prior in (False, True):
        V, Xi = _dev(v_in.copy()), _dev(xt_in)
        pred = torch.full((N, D), NAN, dtype=torch.float32, device=DEV)
        parts = torch.full((N,), NAN, dtype=torch.float64, device=DEV)
        if with_prior:
            lib.call("gmr_rf_head_prior_fwd_w", N, D, _ptr(V), _ptr(Xi), _ptr(X1), X1.stride(0), _ptr(X0), _ptr(tt),
                     _ptr(prior), prior.stride(0), 0.2, 0.1, _ptr(pred), _ptr(parts), _stream())
        else:
            lib.call("gmr_rf_head_fwd_w", N, D, _ptr(V), _ptr(Xi), _ptr(X1), X1.stride(0), _ptr(X0), _ptr(tt), 0.1,
                     _ptr(pred), _ptr(parts), _stream())
        res = {}
        for dt in (torch.float64, torch.float32):
            c = lambda a: torch.tensor(a, dtype=dt)  # noqa: E731
            res[dt] = [x.numpy().astype(np.float64) for x in
                       RB.head_ref(c(v_in), c(xt_in), c(x1), c(x0), c(t), c(pr) if with_prior else None)]
        (v64, p64, s64), (v32, p32, s32) = res[torch.float64], res[torch.float32]
        gv, gp, gs = V.cpu().numpy(), pred.cpu().numpy(), parts.cpu().numpy()
        # a clamped row is of the order 1e7: the table bar's rtol carries it
        print(f"head D {D} N {N} prior {with_prior}: V rel {np.abs(gv - v64).max() / np.abs(v64).max():.3e}, "
              f"fp32 torch {np.abs(v32 - v64).max() / np.abs(v64).max():.3e}")
        own = 2 * np.abs(v32 - v64)   # next to fp32 torch's own distance on the clamped rows
        assert (np.abs(gv - v64) <= 1e-5 * np.abs(v64) + 2e-6 + own).all()
        assert (np.abs(gp - p64) <= 1e-5 * np.abs(p64) + 2e-6 + 2 * np.abs(p32 - p64)).all()
        assert (np.abs(gs - s64) <= 1e-5 * np.abs(s64) + 2 * np.abs(s32 - s64)).all()
        # losses: the mean over N D entries
        loss = torch.full((3,), NAN, dtype=torch.float32, device=DEV)
        clp = torch.tensor([0.5, 1.5], dtype=torch.float64, device=DEV)
        lib.call("gmr_rf_losses_w", N, D, _ptr(parts), 1, _ptr(clp), 0.5, _ptr(loss), _stream())
        rf = gs.sum() / (N * D)
        np.testing.assert_allclose(loss.cpu().numpy(), [rf, 2.0, rf + 1.0], rtol=1e-5)
        # the head's backward
        dp = (rng.standard_normal((N, D)) / (N * D)).astype(np.float32)
        dV, dpd = torch.full((N, D), NAN, dtype=torch.float32, device=DEV), _dev(dp)
        lib.call("gmr_rf_head_bwd_w", N, D, _ptr(V), _ptr(X1), X1.stride(0), _ptr(X0), _ptr(tt), _ptr(dpd), _ptr(dV),
                 _stream())
        # differences and a sum that may cancel: rtol 1e-5 of the result next to 1e-6 (a few fp32 roundings) of the
        # operands V, X1, X0 at the scale 2 / (N D) and of the dpred term
        ta = 2 * (gv.astype(np.float64) - (x1.astype(np.float64) - x0)) / (N * D)
        tb = (1 - t.astype(np.float64)) * dp
        ops = 2 * (np.abs(gv) + np.abs(x1) + np.abs(x0)).astype(np.float64) / (N * D) + np.abs(tb)
        assert (np.abs(dV.cpu().numpy() - (ta + tb)) <= 1e-5 * np.abs(ta + tb) + 1e-6 * ops).all()


@pytest.mark.parametrize("N", [1, 5, 130])
@pytest.mark.parametrize("D", [128, 192])
def test_head_w_zero_prior_is_head_fwd_w(D, N):
    """An all-zero prior adds an exact zero: the prior head's V, pred and row parts are the plain head's bit for bit,
    the rows with a clamped norm included (as tests/test_rfbm3_kernels_gpu.py asks of the 64-wide head)."""
    lib = _lib()
    rng = np.random.default_rng(D + N)
    x1, x0, xt, v = (rng.standard_normal((N, D)).astype(np.float32) for _ in range(4))
    xt[0] = 0.0
    _, X1 = _block(N, D, 64, 0, SENT)
    X1.copy_(_dev(x1))
    X0, Xt, tt = _dev(x0), _dev(xt), _dev(rng.random(N).astype(np.float32))
    zero = torch.zeros((N, D + 64), dtype=torch.float32, device=DEV)[:, 64:]
    outs = []
    for with_prior in (False, True):
        V = _dev(v.copy())
        pred = torch.full((N, D), NAN, dtype=torch.float32, device=DEV)
        parts = torch.full((N,), NAN, dtype=torch.float64, device=DEV)
        if with_prior:
            lib.call("gmr_rf_head_prior_fwd_w", N, D, _ptr(V), _ptr(Xt), _ptr(X1), X1.stride(0), _ptr(X0), _ptr(tt),
                     _ptr(zero), zero.stride(0), 0.2, 0.1, _ptr(pred), _ptr(parts), _stream())
        else:
            lib.call("gmr_rf_head_fwd_w", N, D, _ptr(V), _ptr(Xt), _ptr(X1), X1.stride(0), _ptr(X0), _ptr(tt), 0.1,
                     _ptr(pred), _ptr(parts), _stream())
        outs.append((V, pred, parts))
    for a, b, what in zip(*outs, ("V", "pred", "row parts")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), what


def _infonce_ref(pred, T, idx, neg, temp, dtype):
    """Per-anchor losses and d loss_b / d pred[idx[b]] of rf_fixture.infonce's formula."""
    a = torch.tensor(pred[idx], dtype=dtype, requires_grad=True)
    Tt = torch.tensor(T, dtype=dtype)
    Fn = torch.nn.functional
    an = Fn.normalize(a, dim=1)
    pos = torch.exp((an * Fn.normalize(Tt[idx], dim=1)).sum(-1) / temp)
    tn = Fn.normalize(Tt[neg], dim=1)
    ns = torch.exp(torch.bmm(an.unsqueeze(1), tn.transpose(1, 2)).squeeze(1) / temp)
    l = -torch.log(pos / (pos + ns.sum(1)))
    l.sum().backward()
    return l.detach().numpy().astype(np.float64), a.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("n_neg", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("D", [128, 192])
def test_infonce_w_injected(D, n_neg):
    lib = _lib()
    rng = np.random.default_rng(7 * D + n_neg)
    n, off, B, temp, coef = 50, 13, 9, 0.2, 0.37
    pred = rng.standard_normal((off + n, D)).astype(np.float32)
    T = rng.standard_normal((off + n, D)).astype(np.float32)
    idx = rng.integers(0, n, B)
    idx[4] = idx[1]                                  # an anchor twice
    raw = rng.integers(0, n, (B, n_neg))
    raw[2, 0] = idx[2]                               # a negative equal to the positive: the next row
    raw[6, n_neg - 1] = idx[6]
    neg = R.collide(raw, idx, n)
    _, Tv = _block(off + n, D, 64, 0, SENT)          # the target at row stride D + 64, as X1 is
    Tv.copy_(_dev(T))
    P, idx_d, raw_d = _dev(pred), _dev(idx.astype(np.int32)), _dev(raw.astype(np.int32))
    parts = torch.full((B,), NAN, dtype=torch.float64, device=DEV)
    ctab, contrib = _block(B, D, 4, 4, NAN)
    lib.call("gmr_rf_infonce_sampled_fwd_bwd_w", B, n, D, _ptr(P), D, _ptr(Tv), Tv.stride(0), off, _ptr(idx_d), n_neg,
             _ptr(raw_d), 0, 0, 0, 1.0 / temp, coef, _ptr(parts), _ptr(contrib), contrib.stride(0), _stream())
    l64, g64 = _infonce_ref(pred[off:], T[off:], idx, neg, temp, torch.float64)
    l32, g32 = _infonce_ref(pred[off:], T[off:], idx, neg, temp, torch.float32)
    np.testing.assert_allclose(parts.cpu().numpy(), l64, rtol=1e-5, atol=2 * float(np.abs(l32 - l64).max()))
    bar = RG.grad_bar(g32, g64)
    err = R.rel_to_max(contrib.cpu().numpy() / coef, g64)
    print(f"InfoNCE D {D} n_neg {n_neg}: contrib error {err:.3e} of the largest entry (gradient bar {bar:.3e})")
    assert err <= bar
    full = ctab.cpu().numpy()
    assert np.isnan(full[:, :4]).all() and np.isnan(full[:, 4 + D:]).all()


@pytest.mark.parametrize("n_neg", [1, 17, 40])
@pytest.mark.parametrize("D", [128, 192])
def test_infonce_w_draws_the_indices_of_the_64_wide_kernel(D, n_neg):
    """Rows that are zero past column 64 have the same norms, dots and column norms at every width, so with
    Philox-drawn negatives the wide kernel's losses and its first 64 contrib columns are the 64-wide kernel's exactly
    when both drew the same indices for the key (any other index changes them at the order of 1)."""
    lib = _lib()
    rng = np.random.default_rng(D + n_neg)
    n, B, temp = 50, 12, 0.2
    pred = torch.zeros((n, D), dtype=torch.float32, device=DEV)
    T = torch.zeros((n, D), dtype=torch.float32, device=DEV)
    pred[:, :64] = _dev(rng.standard_normal((n, 64)).astype(np.float32))
    T[:, :64] = _dev(rng.standard_normal((n, 64)).astype(np.float32))
    idx = _dev(rng.integers(0, n, B).astype(np.int32))
    out = []
    for W, name in ((D, "gmr_rf_infonce_sampled_fwd_bwd_w"), (64, "gmr_rf_infonce_sampled_fwd_bwd")):
        parts = torch.full((B,), NAN, dtype=torch.float64, device=DEV)
        contrib = torch.full((B, W), NAN, dtype=torch.float32, device=DEV)
        width = (W,) if W != 64 else ()
        lib.call(name, B, n, *width, _ptr(pred), D, _ptr(T), D, 0, _ptr(idx), n_neg, None, 1234, 5, 3, 1.0 / temp, 1.0,
                 _ptr(parts), _ptr(contrib), W, _stream())
        out.append((parts.cpu().numpy(), contrib.cpu().numpy()))
    (pw, cw), (p6, c6) = out
    assert np.isfinite(pw).all() and np.isfinite(cw).all()
    np.testing.assert_allclose(pw, p6, rtol=1e-6)
    np.testing.assert_allclose(cw[:, :64], c6, rtol=1e-5, atol=1e-6 * float(np.abs(c6).max()))
    assert not cw[:, 64:].any()


# ------------------------------------------------------------------------------------------------ the train step
@pytest.mark.parametrize("D,C", [(192, 192), (128, 128)])
def test_generator_train_step_at_width(D, C):
    """RFGenerator(embedding_dim = condition_dim = D).train_step at U = 700, I = 900 (N = 1,600: 50 sampler tiles, 400
    head blocks), B = 300 with repeated anchors, 40 negatives (three rounds of 16 slots, the last short), dropout 0.1
    with injected masks and draws; X1 and cond are one table, as in the model."""
    from gmr.rf import RFGenerator
    U, I, B, n_neg, L, p, lr = 700, 900, 300, 40, 2, 0.1, 1e-3
    N = U + I
    rng = np.random.default_rng(D)
    P0 = RG.random_params(rng, C, L, D)
    gen = RFGenerator(U, I, C, DEV, n_layers=L, dropout=p, learning_rate=lr, n_negatives=n_neg, embedding_dim=D)
    gen.load_reference_state(P0)
    tab = rng.standard_normal((N, D)).astype(np.float32)
    prior = RG.prior_ref(torch.tensor(tab), U).numpy()
    users, pos = rng.integers(0, U, B), rng.integers(0, I, B)
    users[5], pos[9] = users[2], pos[3]
    dr = {"X0": rng.standard_normal((N, D)).astype(np.float32), "t": rng.random((N, 1)).astype(np.float32),
          "neg_items": R.collide(rng.integers(0, I, (B, n_neg)), pos, I).astype(np.int32),
          "neg_users": R.collide(rng.integers(0, U, (B, n_neg)), users, U).astype(np.int32)}
    masks = {s: (rng.random((N, H)) >= p).astype(np.uint8) for s in R.drop_sites(L)}
    X1 = _dev(tab)
    loss = gen.train_step(X1, X1, _dev(users.astype(np.int32)), _dev(pos.astype(np.int32)),
                          masks={s: _dev(m) for s, m in masks.items()}, prior=_dev(prior),
                          **{k: _dev(v) for k, v in dr.items()})
    res = {}
    for dt in (torch.float64, torch.float32):
        Pt = {n: torch.tensor(v, dtype=dt, requires_grad=True) for n, v in P0.items()}
        c = lambda a: torch.tensor(a, dtype=dt)  # noqa: E731
        li = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
        r = RB.train_losses(Pt, c(tab), c(dr["X0"]), c(dr["t"]), c(tab), c(prior), li(users), li(pos),
                            li(dr["neg_items"]), li(dr["neg_users"]), U, L,
                            masks={s: torch.tensor(m) for s, m in masks.items()}, p=p)
        res[dt] = (r, R.grads_of(Pt, r["total"]))
    (r64, g64), (_, g32) = res[torch.float64], res[torch.float32]
    terms = loss.cpu().numpy()
    print(f"train step ({D}, {C}): rf {terms[0]:.7f} ({r64['rf_loss'].item():.7f}), cl {terms[1]:.7f} "
          f"({r64['cl_loss'].item():.7f})")
    np.testing.assert_allclose(terms[0], r64["rf_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(terms[1], r64["cl_loss"].item(), rtol=1e-5)
    np.testing.assert_allclose(terms[2], r64["total"].item(), rtol=1e-5)
    worst = (0.0, 0.0, 0.0)
    eps, wd = 1e-8, 0.01
    for (name, _), got, pv in zip(gen.specs, gen.grad_views(), gen.param_views()):
        want = g64[name].numpy()
        bar = RG.grad_bar(g32[name].numpy(), want)
        err = R.rel_to_max(got.cpu().numpy(), want)
        worst = max(worst, (err / bar, err, bar))
        assert err <= bar, (name, err, bar)
        # the first AdamW step from the fp64 gradient (mhat = g, sqrt(vhat) = |g|): an element moves by
        # lr g / (|g| + eps), so gradients within dg move it by at most lr min(2, dg / (|g| + eps)) (rfbm3_fixture.p1_bound)
        p0 = P0[name].astype(np.float64)
        p1 = p0 * (1 - lr * wd) - lr * want / (np.abs(want) + eps)
        dg = 1e-4 * np.abs(want) + bar * np.abs(want).max()
        bound = 1e-5 * np.abs(p1) + lr * np.minimum(2.0, dg / (np.abs(want) + 1e-8))
        assert (np.abs(pv.cpu().numpy() - p1) <= bound).all(), name
        assert not np.array_equal(pv.cpu().numpy(), P0[name])
    print(f"train step ({D}, {C}): worst gradient error {worst[1]:.3e} of the parameter's largest (bar {worst[2]:.3e})")
    assert gen.step_ctr == 1 and gen._w["contrib"].shape == (2 * B, D) and gen._w["pred"].shape == (N, D)
