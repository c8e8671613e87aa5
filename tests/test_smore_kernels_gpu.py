"""The SMORE kernels of csrc/smore.hip by name, against fp64 row restatements with autograd (tests/smore_fixture.py:
real cosine / sine matrices, no torch.fft).

Bars (the rule of test_mgcn_kernels_gpu.py): rtol 1e-5 against fp64, and next to it an entry may be off by twice the
largest error of the same computation done by fp32 torch on the CPU against fp64, measured here and printed."""
import functools

import numpy as np
import pytest
import torch

import smore_fixture as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
P_DROP = 0.1


def _lib():
    from gmr.utils import get_model
    get_model("SMORE")  # the feature under test: raises ValueError without it
    from gmr import _lib as lib
    return lib


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _stream():
    from gmr.kernels import stream
    return stream()


def TR():
    return int(_lib().load().gmr_smore_tile_rows())


def MB():
    return int(_lib().load().gmr_smore_max_blocks())


def rows_of(rel):
    tr, mb = TR(), MB()
    return {"1": 1, "TR-1": tr - 1, "TR+1": tr + 1, "3TR+5": 3 * tr + 5, "2nd trip": mb * tr + 7}[rel]


ROWS = ["1", "TR-1", "TR+1", "3TR+5", "2nd trip"]


def mat(x, ld=None):
    """x (n x w array) as the first w columns of a NaN-filled n x ld device tensor."""
    w = x.shape[1]
    t = torch.full((x.shape[0], ld or w), float("nan"), device=DEV)
    t[:, :w] = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t[:, :w]


def vec(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def nan(n, cols=64, ld=None):
    return torch.full((n, ld or cols), float("nan"), device=DEV)[:, :cols]


def _bar(got, ref64, ref32, what):
    F.bar(got, ref64, ref32, what)


# ----------------------------------------------------------------------------------------------- spectrum
SW = ("Wgv", "bgv", "Wgt", "bgt", "Wgf", "bgf")
S_OUT = ("S", "conv", "g", "P", "dE", "z", "dV", "dT", "dWi", "dWt", "dWf")


def spec_data(n, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    d = {k: (rng.standard_normal((n, 64)) * 0.7).astype(np.float32) for k in ("V", "T", "E", "dE0")}
    d["dP"] = (rng.standard_normal((n, 192)) * 0.7).astype(np.float32)
    for k in ("Wi", "Wt", "Wf"):
        d[k] = rng.standard_normal((33, 2)).astype(np.float32)
    rw = np.random.default_rng(7 + seed)
    for k in SW:
        d[k] = (rw.standard_normal((64, 64) if k.startswith("W") else (64,)) * (0.3 if k.startswith("W") else 0.2)
                ).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def spec_refs(n):
    d = spec_data(n)
    return d, F.spectrum_rows_ref(d, torch.float64), F.spectrum_rows_ref(d, torch.float32)


def spec_run(d, n=None, wide=False, accumulate=True):
    """gmr_smore_spectrum_fwd, then gmr_smore_spectrum_bwd on what it saved; every output starts as NaN.  wide: every
    row stride above the columns."""
    lib = _lib()
    m = d["V"].shape[0]
    n = m if n is None else n
    ld1, ld2, ld3 = (192, 192, 256) if wide else (64, 128, 192)
    V, T, E = (mat(d[k], ld1) for k in ("V", "T", "E"))
    dP = mat(d["dP"], ld3)
    W = {k: (mat(d[k], ld1) if k.startswith("W") else vec(d[k])) for k in SW}
    cw = {k: vec(d[k]) for k in ("Wi", "Wt", "Wf")}
    o = {"S": nan(m, 128, ld2), "conv": nan(m, 192, ld3), "g": nan(m, 192, ld3), "P": nan(m, 192, ld3),
         "z": nan(m, 192, ld3), "dV": nan(m, 64, ld1), "dT": nan(m, 64, ld1),
         "dE": mat(d["dE0"], ld1) if accumulate else nan(m, 64, ld1)}
    for k in ("dWi", "dWt", "dWf"):
        o[k] = torch.full((33, 2), float("nan"), device=DEV)
    nws = int(lib.load().gmr_smore_spectrum_ws_floats(n))
    ws = torch.full((nws,), float("nan"), device=DEV)
    lib.call("gmr_smore_spectrum_fwd", n, _ptr(V), ld1, _ptr(T), ld1, _ptr(E), ld1, _ptr(cw["Wi"]), _ptr(cw["Wt"]),
             _ptr(cw["Wf"]), *[_ptr(W[k]) for k in SW], ld1, _ptr(o["S"]), ld2, _ptr(o["conv"]), ld3, _ptr(o["g"]), ld3,
             _ptr(o["P"]), ld3, _stream())
    lib.call("gmr_smore_spectrum_bwd", n, _ptr(dP), ld3, _ptr(o["g"]), ld3, _ptr(E), ld1, _ptr(o["S"]), ld2,
             _ptr(cw["Wi"]), _ptr(cw["Wt"]), _ptr(cw["Wf"]), _ptr(W["Wgv"]), _ptr(W["Wgt"]), _ptr(W["Wgf"]), ld1,
             _ptr(o["dE"]), ld1, int(accumulate), _ptr(o["z"]), ld3, _ptr(o["dV"]), _ptr(o["dT"]), ld1, _ptr(ws), nws,
             _ptr(o["dWi"]), _ptr(o["dWt"]), _ptr(o["dWf"]), _stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("rel", ROWS)
def test_spectrum_against_fp64(rel, wide):
    n = rows_of(rel)
    d, r64, r32 = spec_refs(n)
    got = spec_run(d, wide=wide)
    for k in S_OUT:
        _bar(got[k].reshape(r64[k].shape), r64[k], r32[k], f"spectrum n={n} wide={wide} {k}")
    for k in ("dWi", "dWt", "dWf"):
        g = got[k].cpu().numpy()
        assert g[0, 1] == 0.0 and g[32, 1] == 0.0, k


def test_twiddles():
    lib = _lib()
    fwd, inv = nan(64), nan(64)
    lib.call("gmr_smore_twiddles", _ptr(fwd), _ptr(inv), _stream())
    torch.cuda.synchronize()
    C, S, ck = (x.numpy() for x in F.trig())
    want_f = np.concatenate([C, -S[1:32]])                       # F[j][n]: 33 cosine rows, 31 sine rows
    cj = np.concatenate([ck, ck[1:32]])
    f, g = fwd.cpu().numpy(), inv.cpu().numpy()
    assert np.array_equal(f, want_f.astype(np.float32))           # computed in double, rounded once
    assert np.array_equal(g, (want_f * cj[:, None]).T.astype(np.float32))
    assert np.all(np.abs(f[[0, 32]]) == 0.125) and np.all(f[:, 0][:33] == 0.125) and not f[33:, 0].any()


def test_spectrum_identity_filter_returns_the_rows():
    n = 3 * TR() + 5
    d = dict(spec_data(n))
    for k in ("Wi", "Wt", "Wf"):
        d[k] = np.tile(np.float32([1, 0]), (33, 1))
    got = spec_run(d)
    r64, r32 = F.spectrum_rows_ref(d, torch.float64), F.spectrum_rows_ref(d, torch.float32)
    conv = got["conv"].cpu().numpy()
    np.testing.assert_allclose(r64["conv"][:, :128], np.concatenate([d["V"], d["T"]], 1).astype(np.float64), atol=1e-14)
    _bar(conv[:, :64], d["V"].astype(np.float64), r32["conv"][:, :64], "W = 1: image_conv against V")
    _bar(conv[:, 64:128], d["T"].astype(np.float64), r32["conv"][:, 64:128], "W = 1: text_conv against T")


def test_spectrum_imaginary_parts_of_the_real_bins_are_not_read():
    n = TR() + 1
    d = dict(spec_data(n))
    base = spec_run(d)
    for k in ("Wi", "Wt", "Wf"):
        d[k] = d[k].copy()
        d[k][0, 1], d[k][32, 1] = 5.0, -3.0
    got = spec_run(d)
    for k in S_OUT:
        assert torch.equal(got[k], base[k]), k
    for k in ("dWi", "dWt", "dWf"):
        g = got[k].cpu().numpy()
        assert g[0, 1] == 0.0 and g[32, 1] == 0.0 and not np.signbit(g[[0, 32], 1]).any(), k


def test_spectrum_impulse_and_zero_row():
    n = TR() + 3
    d = dict(spec_data(n))
    d["V"], d["T"], d["dP"] = d["V"].copy(), d["T"].copy(), d["dP"].copy()
    d["V"][2] = 0
    d["V"][2, 0] = 1            # an impulse e_0: a flat spectrum of 1/8
    d["T"][4] = 0               # a zero T row: no fusion signal, and no dV from the fusion term
    d["dP"][4, :64] = 0
    got = {k: v.cpu().numpy() for k, v in spec_run(d).items()}
    assert np.all(got["S"][2, :33] == 0.125) and not got["S"][2, 33:64].any()
    assert not got["S"][4, 64:].any() and not got["conv"][4, 64:].any()
    assert not got["dV"][4].any()
    assert np.abs(got["dT"][4]).max() > 0


def test_spectrum_repeats_and_fixed_order():
    tr = TR()
    n1, n2 = 3 * tr + 5, MB() * tr + 7
    d = dict(spec_data(n2))
    d["dP"] = d["dP"].copy()
    d["dP"][n1:] = 0            # the rows past the shared prefix add zeros to the filter gradients
    full, again = spec_run(d), spec_run(d)
    short = spec_run(d, n=n1)
    for k in S_OUT:
        assert torch.equal(full[k], again[k]), k
    for k in ("S", "conv", "g", "P", "dE", "z", "dV", "dT"):
        assert torch.equal(full[k][:n1], short[k][:n1]), k
        assert bool(torch.isnan(short[k][n1:]).all()) or k == "dE", k   # rows past n are not written
    for k in ("dWi", "dWt", "dWf"):     # more partials than workgroups against four tiles: the same bits
        assert torch.equal(full[k], short[k]), k
        assert np.abs(full[k].cpu().numpy()).max() > 0


# ----------------------------------------------------------------------------------------------- fuser
F_OUT = ("side", "all", "saved", "dabf", "dc", "z")


def fuse_data(n, seed=0):
    rng = np.random.default_rng(200 + n + seed)
    d = {k: (rng.standard_normal((n, 64)) * 0.7).astype(np.float32) for k in ("c", "dall", "dside", "dcin")}
    d["abf"] = (rng.standard_normal((n, 192)) * 0.7).astype(np.float32)
    rw = np.random.default_rng(11 + seed)
    for k in F.FUSE_W:
        d[k] = (rw.standard_normal((64, 64) if k.startswith("W") else (64,)) * (0.3 if k.startswith("W") else 0.2)
                ).astype(np.float32)
    return d


def keep_of(n, seed=3):
    return (np.random.default_rng(seed).random((n, 192)) >= P_DROP).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def fuse_refs(n, masked):
    d = fuse_data(n)
    keep, p = (keep_of(n), P_DROP) if masked else (None, 0.0)
    return d, keep, F.fuse_rows_ref(d, torch.float64, keep, p), F.fuse_rows_ref(d, torch.float32, keep, p)


def fuse_run(d, n=None, wide=False, keep=None, p=0.0, mode=None, seed=0, step=0, grads=(True, True)):
    """gmr_smore_fuse_fwd, then gmr_smore_fuse_bwd on the rows it saved; every output starts as NaN."""
    lib = _lib()
    m = d["c"].shape[0]
    n = m if n is None else n
    ld1, ld3, ld7 = (192, 256, 512) if wide else (64, 192, 448)
    abf, c, dall = mat(d["abf"], ld3), mat(d["c"], ld1), mat(d["dall"], ld1)
    dsc = mat(np.concatenate([d["dside"], d["dcin"]], 1), 2 * ld1 if wide else 128)
    W = {k: (mat(d[k], ld1) if k.startswith("W") else vec(d[k])) for k in F.FUSE_W}
    o = {"side": nan(m, 64, ld1), "all": nan(m, 64, ld1), "saved": nan(m, 448, ld7), "dabf": nan(m, 192, ld3),
         "dc": nan(m, 64, ld1), "z": nan(m, 448, ld7)}
    mode = (0 if p == 0 else 1 if keep is not None else 2) if mode is None else mode
    kp = None
    if keep is not None:
        kp = torch.zeros((m, 256 if wide else 192), dtype=torch.uint8, device=DEV)
        kp[:, :192] = torch.as_tensor(keep).to(DEV)
    lib.call("gmr_smore_fuse_fwd", n, _ptr(abf), ld3, _ptr(c), ld1, *[_ptr(W[k]) for k in F.FUSE_W], ld1, p, mode,
             _ptr(kp) if kp is not None else None, kp.stride(0) if kp is not None else 0, seed, step, _ptr(o["side"]),
             _ptr(o["all"]), ld1, _ptr(o["saved"]), ld7, _stream())
    lib.call("gmr_smore_fuse_bwd", n, _ptr(dall), ld1, _ptr(dsc) if grads[0] else None,
             _ptr(dsc[:, 64:]) if grads[1] else None, dsc.stride(0), _ptr(abf), ld3, _ptr(o["saved"]), ld7, p,
             *[_ptr(W[k]) for k in ("Wv1", "Wv2", "Wt1", "Wt2", "Wi", "Wt", "Wf")], ld1, _ptr(o["dabf"]), ld3,
             _ptr(o["dc"]), ld1, _ptr(o["z"]), ld7, _stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rel", ROWS)
def test_fuser_against_fp64(rel, masked):
    """Without dropout at the packed strides; with injected masks at strides above the columns."""
    n = rows_of(rel)
    d, keep, r64, r32 = fuse_refs(n, masked)
    got = fuse_run(d, wide=masked, keep=keep, p=P_DROP if masked else 0.0)
    for k in F_OUT:
        _bar(got[k], r64[k], r32[k], f"fuser n={n} masked={masked} {k}")
    sv = got["saved"].cpu().numpy()
    assert np.abs(sv[:, 128:192].astype(np.float64).sum(1) - 1).max() <= 1e-6      # the softmax rows sum to 1
    assert np.abs(sv[:, 192:256].astype(np.float64).sum(1) - 1).max() <= 1e-6
    if masked:      # the injected masks, exactly, in the saved gate rows
        assert np.array_equal(sv[:, 256:] != 0, keep != 0)


def test_fuser_null_direct_gradients_are_zero():
    d = fuse_data(TR() + 1)
    got = fuse_run(d, grads=(False, False))
    want = fuse_run(dict(d, dside=np.zeros_like(d["dside"]), dcin=np.zeros_like(d["dcin"])))
    for k in F_OUT:
        assert torch.equal(got[k], want[k]), k


def test_fuser_rows_do_not_depend_on_the_call():
    tr = TR()
    d = fuse_data(3 * tr + 5)
    keep = keep_of(3 * tr + 5)
    full, again = fuse_run(d, keep=keep, p=P_DROP), fuse_run(d, keep=keep, p=P_DROP)
    short = fuse_run(d, n=tr + 1, keep=keep, p=P_DROP)
    for k in F_OUT:
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k][:tr + 1], short[k][:tr + 1]), k
        assert bool(torch.isnan(short[k][tr + 1:]).all()), k


def test_fuser_large_logits_stay_finite():
    """Pre-softmax entries of +80 and -80 (tanh saturated to 1 by the bias, a row of Wv2 / Wt2 of +-80 / 64)."""
    d = dict(fuse_data(41))
    for b, w in (("bv1", "Wv2"), ("bt1", "Wt2")):
        d[b] = np.full(64, 100.0, np.float32)
        d[w] = d[w].copy()
        d[w][0], d[w][1] = 80.0 / 64, -80.0 / 64
    got = {k: v.cpu().numpy() for k, v in fuse_run(d).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    sv = got["saved"]
    assert np.all(sv[:, :128] == 1) and np.all(sv[:, 128] > 0.999) and np.all(sv[:, 129] <= 1e-30)
    assert np.abs(sv[:, 128:192].astype(np.float64).sum(1) - 1).max() <= 1e-6
    r64, r32 = F.fuse_rows_ref(d, torch.float64), F.fuse_rows_ref(d, torch.float32)
    for k in F_OUT:
        _bar(got[k], r64[k], r32[k], f"fuser +-80 {k}")


# ----------------------------------------------------------------------------------------------- dropout
def _gates(o):
    return o["saved"][:, 256:].cpu().numpy()


def test_dropout_masks_from_philox():
    tr, mb = TR(), MB()
    n1, n2 = mb * tr + 7, mb * tr + 3 * tr + 12     # both past one trip of the grid, different grids per row
    d = fuse_data(n2)
    sig = _gates(fuse_run(d))                       # p = 0: the sigmoid rows, nothing drawn
    a = _gates(fuse_run(d, p=P_DROP, seed=5, step=3))
    scale = np.float32(1) / (np.float32(1) - np.float32(P_DROP))
    kept = a != 0
    assert np.array_equal(a[kept], (sig * scale)[kept])          # saved gate / sigmoid is 0 or 1 / (1 - p)
    cnt = kept.size
    assert cnt == 3 * n2 * 64
    share = kept.mean()
    print(f"kept share {share:.5f} over {cnt} draws (5 sigma: {5 * np.sqrt(0.09 / cnt):.5f})")
    assert abs(share - 0.9) <= 5 * np.sqrt(0.09 / cnt)
    for blk in range(3):                                         # the three gates draw different masks
        assert not np.array_equal(kept[:, 64 * blk:64 * blk + 64], kept[:, 64 * ((blk + 1) % 3):][:, :64])
    assert torch.equal(fuse_run(d, p=P_DROP, seed=5, step=3)["saved"], fuse_run(d, p=P_DROP, seed=5, step=3)["saved"])
    b = _gates(fuse_run(d, n=n1, p=P_DROP, seed=5, step=3))      # another row count: the same mask on the shared rows
    assert np.array_equal(a[:n1], b[:n1])
    nxt = _gates(fuse_run(d, p=P_DROP, seed=5, step=4)) != 0
    other = _gates(fuse_run(d, p=P_DROP, seed=6, step=3)) != 0
    for m_ in (nxt, other):                                      # step + 1 and another seed: other masks
        agree = (m_ == kept).mean()                              # independent masks agree on 0.9^2 + 0.1^2
        assert abs(agree - 0.82) <= 5 * np.sqrt(0.82 * 0.18 / cnt), agree
    ev = fuse_run(d, p=P_DROP, mode=0)                           # evaluation: nothing dropped
    assert np.array_equal(_gates(ev), sig)


# ----------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_raise():
    """A status and the entry point's error string (gmr_last_error_string: "<function>: <what>"), never a launch."""
    lib = _lib()
    d = spec_data(8)
    x, x3 = mat(d["V"]), mat(d["dP"])
    w, bias, cw = mat(d["Wgv"]), vec(d["bgv"]), vec(d["Wi"])
    o2, o3 = nan(8, 128), [nan(8, 192) for _ in range(3)]
    good = [8, _ptr(x), 64, _ptr(x), 64, _ptr(x), 64, _ptr(cw), _ptr(cw), _ptr(cw), _ptr(w), _ptr(bias), _ptr(w),
            _ptr(bias), _ptr(w), _ptr(bias), 64, _ptr(o2), 128, _ptr(o3[0]), 192, _ptr(o3[1]), 192, _ptr(o3[2]), 192,
            _stream()]
    lib.call("gmr_smore_spectrum_fwd", *good)
    for i, v in ((0, 0), (1, None), (2, 60), (2, 66), (7, None), (11, None), (16, 32), (18, 64), (20, 128), (23, None),
                 (1, _ptr(x.view(-1)[1:]))):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError, match=r"\): gmr_smore_spectrum_fwd: \w"):
            lib.call("gmr_smore_spectrum_fwd", *bad)
    nws = int(lib.load().gmr_smore_spectrum_ws_floats(8))
    ws, dw = torch.zeros(nws, device=DEV), [torch.zeros((33, 2), device=DEV) for _ in range(3)]
    z, dv, de = nan(8, 192), nan(8, 128), nan(8)
    good = [8, _ptr(x3), 192, _ptr(o3[1]), 192, _ptr(x), 64, _ptr(o2), 128, _ptr(cw), _ptr(cw), _ptr(cw), _ptr(w),
            _ptr(w), _ptr(w), 64, _ptr(de), 64, 0, _ptr(z), 192, _ptr(dv), _ptr(dv[:, 64:]), 128, _ptr(ws), nws,
            _ptr(dw[0]), _ptr(dw[1]), _ptr(dw[2]), _stream()]
    lib.call("gmr_smore_spectrum_bwd", *good)
    for i, v in ((0, 0), (1, None), (2, 64), (8, 64), (9, None), (15, 60), (16, None), (20, 128), (24, None),
                 (25, nws - 1), (26, None)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError, match=r"\): gmr_smore_spectrum_bwd: \w"):
            lib.call("gmr_smore_spectrum_bwd", *bad)
    sv, zf, kp = nan(8, 448), nan(8, 448), torch.ones((8, 192), dtype=torch.uint8, device=DEV)
    good = [8, _ptr(x3), 192, _ptr(x), 64, _ptr(w), _ptr(bias), _ptr(w), _ptr(w), _ptr(bias), _ptr(w), _ptr(w),
            _ptr(bias), _ptr(w), _ptr(bias), _ptr(w), _ptr(bias), 64, 0.1, 1, _ptr(kp), 192, 0, 0, _ptr(o3[0]),
            _ptr(o3[0][:, 64:]), 192, _ptr(sv), 448, _stream()]
    lib.call("gmr_smore_fuse_fwd", *good)
    for i, v in ((0, 0), (1, None), (2, 128), (4, 62), (6, None), (17, 32), (18, 1.0), (19, 3), (20, None), (21, 64),
                 (24, None), (28, 256)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError, match=r"\): gmr_smore_fuse_fwd: \w"):
            lib.call("gmr_smore_fuse_fwd", *bad)
    sv.fill_(0.25)
    good = [8, _ptr(x), 64, None, None, 64, _ptr(x3), 192, _ptr(sv), 448, 0.1, _ptr(w), _ptr(w), _ptr(w), _ptr(w),
            _ptr(w), _ptr(w), _ptr(w), 64, _ptr(o3[1]), 192, _ptr(o3[0]), 192, _ptr(zf), 448, _stream()]
    lib.call("gmr_smore_fuse_bwd", *good)
    for i, v in ((0, 0), (1, None), (2, 65), (7, 64), (9, 192), (10, -0.5), (11, None), (18, 60), (20, 64), (23, None),
                 (24, 192)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError, match=r"\): gmr_smore_fuse_bwd: \w"):
            lib.call("gmr_smore_fuse_bwd", *bad)
    torch.cuda.synchronize()
