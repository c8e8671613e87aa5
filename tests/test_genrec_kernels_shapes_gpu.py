"""The GenRecV1 rec-step kernels (csrc/genrec.hip) past the tiny fixture (U = 97, I = 61, batch 24), called through
_lib.call against fp64 references on the CPU (torch autograd where a backward is checked).

  gmr_bn_fwd / _bwd   16 row slots per block, at most 256 blocks, finalize kernels with 16 part groups per column:
                        rows 1          no second row: biased variance kept in run_var, x_hat == 0, dz == 0
                        rows 15, 16, 17 one slot empty / one block exactly / a second block holding one row
                        rows 250        P = 16: every part group of the finalize kernels holds one part
                        rows 272        P = 17: group 0 takes the second step of the 16-group stride (p += 16)
                        rows 4096       16 x 256 exactly: the block cap, one pass, every slot full
                        rows 4097       only slot 0 of block 0 wraps into a second grid-stride pass
                        rows 8200       8200 = 2 x 4096 + 8: slots 0..7 of block 0 make three passes, the rest two
                      every (act, post, keep, layout) at rows 17 and 4097 with the accumulate flags alternating so
                      that every act and every post meets both; four option sets at the other row counts.  Layout:
                      z, y, dy, dz, aux, out2 contiguous, or columns 64..127 of 192-wide tables whose other columns
                      must come back untouched (every ld a multiple of 4: the kernels load float4).  post 3's
                      backward goes through da / v / dv, post 2's through mul.  eval mode, an offset-column case
                      (eight columns with mean 1e3, standard deviation 1e-1), run-to-run determinism.
  content fwd / bwd   n = 1, 17, 1000, 16400: 16400 x 16 threads pass the 1024-block cap (n > 16384), so the
                      grid-stride loop makes a second pass and block_sum_parts takes four steps of p += 256;
                      origin / generation weights 0.3 apart and 60 apart (softmax saturated)
  fusion fwd / bwd    n = 1, 17, 1000 with rows whose aI - aT is +-60
  mul64 / dot64       rows 1, 17, 16400 (the same cap), operands as views of 192-wide tables
  nce_rows[_off]      cols 1, 63, 64, 65 (a wave short of / exactly / past 64 lanes), 255, 256, 257 (the 256-thread
                      stride), 1000, ld = cols + 3; logits of a few units, logits spread over +-60, and +-100
                      (exp(60) is still finite in fp32, exp(100) is not: only the last overflows without the
                      max-subtraction) with one row near -100 throughout and one near +100 throughout
  bpr_logsigmoid      B = 1, 15, 16, 17, 1000 (16 rows per block), repeated users, x reaching +-100
  nce_pairs/_combine  nterms 1..4, Bg = 50, (row0, B) = (0, 50), (0, 20), (13, 20), (30, 20); tab, ct, dts wider

Leaky-ReLU inputs are drawn, then moved, so that no pre-activation of the fp64 reference has |v| < 1e-3 (asserted on
the reference); no element is left out of any comparison.

Bars.  Element-wise kernels (content forward and combine, fusion, mul64, bpr, the nce gradient rows, eval-mode BN):
a few fp32 roundings, counted and stated at each check.  Everything behind a sum (BN statistics, outputs and
gradients, dow / dgw, dot64, fusion's daI, the nce loss): 4 x the error of the same torch formula in fp32 on the CPU
against fp64 (both sides are fp32 with different summation orders), relative to the tensor's largest expected value,
floored at 1e-6 of it and never above the bars of test_genrec_gpu.py (forward 1e-5, gradients 2e-4).  Every such bar
is measured on the restatement alone and printed next to the observed error.  nce_pairs / nce_combine are a copy
and a fixed-order sum: bit for bit against numpy fp32 adding in the kernel's order.

Seen on the MI355X, largest error (largest bar) over all row counts and option sets: BN mean 4.6e-8, invstd 4.9e-8,
run_mean 7.9e-8, run_var 6.1e-8, rowdot 1.8e-7 (bars 1.0e-6, the floor); y 1.9e-7 (2.7e-6), out2 1.3e-7 (1.0e-6),
dz 2.5e-7 (1.6e-6), dw 2.2e-7 (2.6e-6), db 2.1e-7 (1.5e-6), dv 1.2e-7 (1.0e-5).  Offset columns: mean 3.0e-8, invstd
4.6e-8 (2.0e-6), y 1.0e-7 against the 1e-5 cap (the fp32 restatement is 1.4e-4 off there: before the forward
kept the residual of the fp32 mean, y carried the same 1e-4); the backward still normalises with the saved fp32
mean, so with the sigmoid set dz is 1.1e-4, dw 1.8e-4 and db 4.4e-5 off against the 2e-4 cap, with the leaky set
dz 1.0e-6 (1.0e-5), dw 3.0e-5 (2e-4).  content dow 5.3e-7 (2.3e-6), dgw 2.2e-6 (2.0e-5); fusion daI 1.4e-7 (1.0e-6);
dot64 8.3e-7 (1.0e-5, at 17 rows where the sum nearly cancels), 8.6e-9 at 16400 rows; nce loss 6.7e-8 (1.0e-6).
dv of post 3 under a keep mask used to sum the unmasked activation (no caller combines the two); the keep sets of
post 3 here are what showed it, and the backward now sums what the forward's row dot multiplied.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24  # half an ulp of 1: one fp32 rounding, relative
FWD_CAP, GRAD_CAP = 1e-5, 2e-4
EPS, MOM, SLOPE = float(np.float32(1e-5)), float(np.float32(0.1)), float(np.float32(0.2))
KEEP_SCALE = float(np.float32(1.0 / 0.8))


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


def _np(t):
    return t.detach().cpu().numpy()


def _rel(got, want):
    """Largest error relative to the tensor's largest expected value; an all-zero expectation must be met exactly."""
    want = np.asarray(want, np.float64)
    err, top = np.abs(np.asarray(got, np.float64) - want).max(), np.abs(want).max()
    return float(err / top) if top > 0 else (0.0 if err == 0 else float("inf"))


def _bar(w32, w64, cap):
    return min(max(4 * _rel(w32, w64), 1e-6), cap)


def _check(what, got, w64, w32, cap, tag, seen=None):
    bar, err = _bar(w32, w64, cap), _rel(got, w64)
    print(f"{tag} {what}: error relative to max {err:.3e} (bar {bar:.3e})")
    assert np.isfinite(np.asarray(got)).all(), (tag, what)
    assert err <= bar, (tag, what, err, bar)
    if seen is not None:
        seen.append((err, bar))


FILL = 7.0


def _table(a, strided):
    """A rows x 64 device tensor: contiguous, or columns 64..127 of a 192-wide table filled with FILL elsewhere."""
    a = torch.as_tensor(a)
    if not strided:
        return a.to(DEV).contiguous()
    wide = torch.full((a.shape[0], 192), FILL, dtype=a.dtype)
    wide[:, 64:128] = a
    return wide.to(DEV)[:, 64:128]


def _untouched(t):
    """The neighbours of a strided view still hold FILL."""
    if t._base is None:
        return True
    b = t._base
    return bool((b[:, :64] == FILL).all()) and bool((b[:, 128:] == FILL).all())


# ------------------------------------------------------------------------------------------------ BatchNorm1d
BN_ROWS_FULL = (17, 4097)
BN_ROWS_REDUCED = (1, 15, 16, 250, 272, 4096, 8200)
# (act, post, keep, strided, accumulate): every act, post, layout and flag once
BN_REDUCED = ((1, 0, True, True, 0), (2, 2, False, False, 1), (3, 3, False, True, 1), (0, 1, True, False, 0))
_bn_cache = {}


def _bn_pre64(z, w, b):
    z = z.astype(np.float64)
    mean = z.mean(0)
    std = np.sqrt(((z - mean) ** 2).mean(0) + EPS)
    return (z - mean) / std * w + b, std


def _bn_inputs(rows, offset=False):
    key = (rows, offset)
    if key in _bn_cache:
        return _bn_cache[key]
    rng = np.random.default_rng(1000 + rows + (7 if offset else 0))
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    z = f(rows, 64) * np.exp(0.5 * f(64)) + f(64)
    if offset:
        z[:, 3::8] = 1e3 + 1e-1 * f(rows, 8)
    w = (1 + 0.2 * f(64)).astype(np.float32)
    w[5] = -w[5]
    b = f(64)
    b = (np.sign(b) * (0.05 + 0.3 * np.abs(b))).astype(np.float32)  # rows = 1: the pre-activation is b itself
    assert np.abs(w).min() > 0.2
    for _ in range(50):  # move the few elements whose leaky pre-activation sits next to the kink
        v, std = _bn_pre64(z, w, b)
        bad = np.abs(v) < 2e-3
        if not bad.any() or rows == 1:
            break
        step = np.where(v >= 0, 1.0, -1.0) * np.sign(w) * 0.02 * std
        z = np.where(bad, z.astype(np.float64) + step, z).astype(np.float32)
    x = {"z": z, "w": w, "b": b, "aux": f(rows, 64), "dy": f(rows, 64), "da": f(rows), "v": f(64),
         "keep": (rng.random((rows, 64)) < 0.8).astype(np.uint8), "rs": np.array([0.7], np.float32),
         "run_mean": 0.3 * f(64), "run_var": (0.5 + rng.random(64)).astype(np.float32),
         "dz0": f(rows, 64), "dw0": f(64), "db0": f(64), "dv0": f(64)}
    _bn_cache[key] = x
    return x


def _act(a, v):
    return [v, F.leaky_relu(v, SLOPE), torch.sigmoid(v), torch.tanh(v)][a]


def _bn_ref(x, act, post, keep, dtype, train=True):
    """The layer and its post op in dtype, and the gradients of sum(upstream * output)."""
    t = lambda k: torch.tensor(x[k], dtype=dtype)  # noqa: E731
    z, w, b, v = (t(k).requires_grad_(True) for k in ("z", "w", "b", "v"))
    n = z.shape[0]
    eps, mom = torch.tensor(EPS, dtype=dtype), torch.tensor(MOM, dtype=dtype)
    if train:
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
    else:
        mean, var = t("run_mean"), t("run_var")
    invstd = 1 / torch.sqrt(var + eps)
    pre = (z - mean) * invstd * w + b
    if act == 1 and train and dtype == torch.float64:  # the backward differentiates there; the forward is continuous
        assert bool((pre.abs() >= 1e-3).all()), "a leaky pre-activation of the reference sits on the kink"
    y = _act(act, pre)
    if keep:
        y = y * (t("keep") * torch.tensor(KEEP_SCALE, dtype=dtype))
    r = {"y": y, "mean": mean, "invstd": invstd}
    if post == 0:
        out = y
    elif post == 1:
        out = r["out2"] = t("rs") * t("aux") + y
    elif post == 2:
        out = r["out2"] = t("aux") * y
    else:
        out = r["rowdot"] = y @ v
    if train:
        unbiased = var * n / (n - 1) if n > 1 else var  # one row: the kernel keeps the biased value (torch raises)
        r["run_mean"] = (1 - mom) * t("run_mean") + mom * mean
        r["run_var"] = (1 - mom) * t("run_var") + mom * unbiased
        loss = (out * (t("da") if post == 3 else t("dy"))).sum()
        g = torch.autograd.grad(loss, [z, w, b] + ([v] if post == 3 else []))
        r.update(dz=g[0], dw=g[1], db=g[2])
        if post == 3:
            r["dv"] = g[3]
    return {k: a.detach().numpy() for k, a in r.items()}


def _bn_run(x, act, post, keep, strided, acc, train=True, backward=True):
    from gmr import _lib
    rows = x["z"].shape[0]
    nparts = int(_lib.load().gmr_bn_parts_doubles(rows))
    assert nparts == 192 * min(-(-rows // 16), 256)
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
    d = {k: dev(x[k]) for k in ("w", "b", "v", "da", "rs", "run_mean", "run_var")}
    z, aux, dy = (_table(x[k], strided) for k in ("z", "aux", "dy"))
    km = _table(x["keep"], strided) if keep else None
    ld = lambda a: a.stride(0) if a is not None else 0  # noqa: E731
    parts = torch.full((nparts,), float("nan"), dtype=torch.float64, device=DEV)
    y, out2 = _table(nan(rows, 64).cpu(), strided), (_table(nan(rows, 64).cpu(), strided) if post in (1, 2) else None)
    rowdot = nan(rows) if post == 3 else None
    mean, invstd = nan(64), nan(64)
    _call("gmr_bn_fwd_f32", rows, _ptr(z), ld(z), int(train), EPS, MOM, _ptr(d["run_mean"]), _ptr(d["run_var"]),
          _ptr(parts), _ptr(mean), _ptr(invstd), _ptr(d["w"]), _ptr(d["b"]), act, SLOPE, _ptr(km), ld(km), KEEP_SCALE,
          _ptr(y), ld(y), post, _ptr(d["v"] if post == 3 else aux) if post else None, ld(aux) if post in (1, 2) else 0,
          _ptr(d["rs"]) if post == 1 else None, _ptr(out2), ld(out2), _ptr(rowdot))
    out = {"y": y, "mean": mean, "invstd": invstd, "run_mean": d["run_mean"], "run_var": d["run_var"]}
    if out2 is not None:
        out["out2"] = out2
    if rowdot is not None:
        out["rowdot"] = rowdot
    views = [z, aux, dy, y] + ([out2] if out2 is not None else []) + ([km] if keep else [])
    if backward:
        base = (lambda k: dev(x[k])) if acc else (lambda k: nan(*x[k].shape))  # noqa: E731
        dz = _table(x["dz0"] if acc else nan(rows, 64).cpu(), strided)
        dw, db, dv = base("dw0"), base("db0"), (base("dv0") if post == 3 else None)
        parts.fill_(float("nan"))
        sums = nan(128)
        _call("gmr_bn_bwd_f32", rows, _ptr(z), ld(z), _ptr(mean), _ptr(invstd), _ptr(d["w"]), _ptr(d["b"]), act, SLOPE,
              _ptr(km), ld(km), KEEP_SCALE, _ptr(dy) if post != 3 else None, ld(dy) if post != 3 else 0,
              _ptr(aux) if post == 2 else None, ld(aux) if post == 2 else 0, _ptr(d["da"]) if post == 3 else None,
              _ptr(d["v"]) if post == 3 else None, _ptr(parts), _ptr(sums), _ptr(dw), _ptr(db), _ptr(dv), acc, _ptr(dz),
              ld(dz), acc)
        out.update(dz=dz, dw=dw, db=db)
        if post == 3:
            out["dv"] = dv
        views.append(dz)
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in views), "a kernel wrote beside its 64 columns"
    return {k: _np(a) for k, a in out.items()}


def _bn_check(x, act, post, keep, strided, acc, seen=None):
    rows = x["z"].shape[0]
    tag = f"bn rows={rows} act={act} post={post} keep={keep} strided={strided} acc={acc}"
    got = _bn_run(x, act, post, keep, strided, acc)
    w64 = _bn_ref(x, act, post, keep, torch.float64)
    w32 = _bn_ref(x, act, post, keep, torch.float32)
    for k in ("mean", "invstd", "run_mean", "run_var", "y", "out2", "rowdot"):
        if k in w64:
            _check(k, got[k], w64[k], w32[k], FWD_CAP, tag, seen)
    for k, k0 in (("dz", "dz0"), ("dw", "dw0"), ("db", "db0"), ("dv", "dv0")):
        if k in w64:
            add = x[k0].astype(np.float64) if acc else 0.0  # accumulate 0: the NaN the buffer held is gone
            _check(k, got[k], w64[k] + add, w32[k] + (x[k0] if acc else np.float32(0)), GRAD_CAP, tag, seen)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("rows", BN_ROWS_FULL)
def test_bn_every_option(rows, act):
    x = _bn_inputs(rows)
    i = 0
    for post in range(4):
        for keep in (True, False):
            for strided in (True, False):
                _bn_check(x, act, post, keep, strided, (i + post + act) & 1)
                i += 1  # over the 16 sets of one act, and over the four acts of one post, both flags occur


@pytest.mark.parametrize("rows", BN_ROWS_REDUCED)
def test_bn_rows(rows):
    x = _bn_inputs(rows)
    for act, post, keep, strided, acc in BN_REDUCED:
        _bn_check(x, act, post, keep, strided, acc)
    if rows == 1:
        got = _bn_run(x, 1, 0, False, False, 0)
        assert np.array_equal(got["mean"], x["z"][0]) and not got["dz"].any()
        assert np.array_equal(got["invstd"], np.full(64, np.float32(1.0 / np.sqrt(np.float64(EPS)))))


def test_bn_offset_columns():
    """Eight columns with mean 1e3 and standard deviation 1e-1: q / n - mean^2 loses nine digits, which the fp64
    partials have to spare and fp32 ones have not; the fp32 mean alone is 3e-5 off, 3e-4 of a standard deviation,
    which the forward's x_hat must not carry (the kernel keeps the mean's rounding residual for it)."""
    x = _bn_inputs(4097, offset=True)
    assert np.allclose(x["z"][:, 3::8].mean(0), 1e3, atol=0.02) and np.allclose(x["z"][:, 3::8].std(0), 0.1, atol=0.01)
    _bn_check(x, 1, 0, True, True, 0)
    _bn_check(x, 2, 2, False, False, 1)


@pytest.mark.parametrize("rows", BN_ROWS_FULL)
def test_bn_eval_mode(rows):
    """train = 0: the running statistics normalise, and come back bit for bit."""
    x = _bn_inputs(rows)
    rm, rv = x["run_mean"].astype(np.float64), x["run_var"].astype(np.float64)
    for act, post, keep, strided, _ in BN_REDUCED:
        got = _bn_run(x, act, post, keep, strided, 0, train=False, backward=False)
        assert np.array_equal(got["run_mean"], x["run_mean"]) and np.array_equal(got["run_var"], x["run_var"])
        assert np.array_equal(got["mean"], x["run_mean"])
        w64 = _bn_ref(x, act, post, keep, torch.float64, train=False)
        # invstd: add, square root, divide
        assert (np.abs(got["invstd"] - w64["invstd"]) <= 3 * U24 * w64["invstd"]).all()
        # element-wise: invstd's three roundings, the subtraction, two products and the sum make seven on the
        # pre-activation, carried through an activation of slope <= 1 whose own value adds a few ulp, then the keep
        # scale: 16 x 2^-24 x (|w x_hat| + |b| + |y|)
        xh = (x["z"].astype(np.float64) - rm) / np.sqrt(rv + EPS)
        bound = 16 * U24 * (np.abs(xh * x["w"]) + np.abs(x["b"]) + np.abs(w64["y"])) * KEEP_SCALE
        assert (np.abs(got["y"] - w64["y"]) <= bound).all(), (rows, act, post)
        if "out2" in w64:  # one product, or a product and a sum, more
            b2 = bound * (np.abs(x["aux"]) if post == 2 else 1.0) + 2 * U24 * np.abs(w64["out2"]) + \
                (2 * U24 * np.abs(0.7 * x["aux"]) if post == 1 else 0.0)
            assert (np.abs(got["out2"] - w64["out2"]) <= b2).all(), (rows, act, post)
        if "rowdot" in w64:  # 64 products, 3 + 4 levels of adds
            b3 = (np.abs(x["v"]) * bound).sum(1) + 9 * U24 * (np.abs(w64["y"]) * np.abs(x["v"])).sum(1)
            assert (np.abs(got["rowdot"] - w64["rowdot"]) <= b3).all(), (rows, act, post)


def test_bn_is_deterministic():
    x = _bn_inputs(8200)
    for act, post, keep, strided, acc in BN_REDUCED:
        a, b = (_bn_run(x, act, post, keep, strided, acc) for _ in range(2))
        for k in ("mean", "invstd", "dw", "db", "dz", "y"):
            assert np.array_equal(a[k], b[k]), (act, post, k)


def test_bn_bwd_rejects_unaligned_ld():
    """Every table of the backward is read as float4: a leading dimension that is no multiple of 4 (or below 64) is
    an argument error, returned before anything is launched."""
    rows = 5
    t = {k: torch.zeros((rows, 68), device=DEV) for k in ("z", "dy", "dz", "mul")}
    v = {k: torch.ones(128 if k == "sums" else 64, device=DEV) for k in ("mean", "invstd", "w", "b", "sums", "dw", "db")}
    parts = torch.zeros(192, dtype=torch.float64, device=DEV)

    def bwd(ldz=68, lddy=68, lddz=68, ldmul=68, mul=True, act=1):
        _call("gmr_bn_bwd_f32", rows, _ptr(t["z"]), ldz, _ptr(v["mean"]), _ptr(v["invstd"]), _ptr(v["w"]), _ptr(v["b"]),
              act, SLOPE, None, 0, 1.0, _ptr(t["dy"]), lddy, _ptr(t["mul"]) if mul else None, ldmul, None, None,
              _ptr(parts), _ptr(v["sums"]), _ptr(v["dw"]), _ptr(v["db"]), None, 0, _ptr(t["dz"]), lddz, 0)

    bwd()
    bwd(mul=False, ldmul=0)
    for bad in (dict(ldz=66), dict(lddy=67), dict(lddz=65), dict(ldmul=66), dict(ldz=60), dict(lddz=0), dict(act=4)):
        with pytest.raises(RuntimeError, match="gmr_bn_bwd_f32"):
            bwd(**bad)
    a = torch.zeros((rows, 68), device=DEV)
    out = torch.zeros(1, device=DEV)
    p2 = torch.zeros(1024, dtype=torch.float64, device=DEV)
    _call("gmr_dot64_f32", rows, _ptr(a), 68, _ptr(a), 68, _ptr(p2), 1.0, _ptr(out), 0)
    for lda, ldb in ((66, 68), (68, 67)):
        with pytest.raises(RuntimeError, match="gmr_dot64_f32"):
            _call("gmr_dot64_f32", rows, _ptr(a), lda, _ptr(a), ldb, _ptr(p2), 1.0, _ptr(out), 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ content
def _softmax2(a, b):
    m = max(a, b)
    ea, eb = np.exp(np.float64(a) - m), np.exp(np.float64(b) - m)
    return ea / (ea + eb), eb / (ea + eb)


@pytest.mark.parametrize("gap", [0.3, 60.0, -60.0])
@pytest.mark.parametrize("n", [1, 17, 1000, 16400])
def test_content_fwd_bwd(n, gap):
    from gmr import _lib
    rng = np.random.default_rng(n + int(abs(gap)) + (1 if gap < 0 else 0))
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    x = {k: f(n, 64) for k in ("E", "A1", "A2", "dC", "T1", "T2", "dE0")}
    ow, gw = np.float32(0.4), np.float32(0.4 - gap)
    dow0, dgw0, reg2 = np.float32(0.37), np.float32(-1.21), float(np.float32(1e-3))
    d = {k: dev(v) for k, v in x.items()}
    dow_, dgw_ = dev(np.array([ow])), dev(np.array([gw]))
    C = torch.full((n, 64), float("nan"), device=DEV)
    _call("gmr_gr_content_fwd", n, _ptr(d["E"]), _ptr(d["A1"]), _ptr(d["A2"]), _ptr(dow_), _ptr(dgw_), _ptr(C))
    nparts = int(_lib.load().gmr_gr_parts(n))
    assert nparts >= 2 * min(-(-n * 16 // 256), 1024)
    parts = torch.full((nparts,), float("nan"), dtype=torch.float64, device=DEV)
    dE, go, gg = dev(x["dE0"].copy()), dev(np.array([dow0])), dev(np.array([dgw0]))
    _call("gmr_gr_content_bwd", n, _ptr(d["E"]), _ptr(d["A1"]), _ptr(d["A2"]), _ptr(d["dC"]), _ptr(d["T1"]),
          _ptr(d["T2"]), _ptr(dow_), _ptr(dgw_), reg2, _ptr(parts), _ptr(dE), _ptr(go), _ptr(gg))

    def ref(dtype):
        t = lambda k: torch.tensor(x[k], dtype=dtype)  # noqa: E731
        E = t("E").requires_grad_(True)
        o = torch.tensor(float(ow), dtype=dtype, requires_grad=True)
        g = torch.tensor(float(gw), dtype=dtype, requires_grad=True)
        w = torch.softmax(torch.stack([o, g]), 0)
        Cr = w[0] * ((E + t("A1")) * 0.5) + w[1] * ((E + t("A2")) * 0.5)
        wd = w.detach()  # T_k = A_k^T dC: the path through the propagated tables, which the caller computed
        loss = (Cr * t("dC")).sum() + 0.5 * ((wd[0] * t("T1") + wd[1] * t("T2")) * E).sum() + \
            0.5 * torch.tensor(reg2, dtype=dtype) * (E * E).sum()
        gr = torch.autograd.grad(loss, [E, o, g])
        base = torch.tensor([dow0, dgw0]).to(dtype)
        return Cr.detach().numpy(), (gr[0] + t("dE0")).numpy(), (gr[1] + base[0]).item(), (gr[2] + base[1]).item()

    w64, w32 = ref(torch.float64), ref(torch.float32)
    w0, w1 = _softmax2(ow, gw)
    e, a1, a2, dc = (x[k].astype(np.float64) for k in ("E", "A1", "A2", "dC"))
    # the weights: subtract, exp, add, divide (4 roundings); each term a sum, a halving (exact), a product; one sum: 8
    bound = 8 * U24 * (w0 * np.abs(e + a1) / 2 + w1 * np.abs(e + a2) / 2) + 1e-37
    assert (np.abs(_np(C) - w64[0]) <= bound).all()
    # dE = old + ((w0 (dC + T1) + w1 (dC + T2)) / 2) + reg2 E: the weights' 4, two sums, two products, three sums: 12
    t1, t2 = x["T1"].astype(np.float64), x["T2"].astype(np.float64)
    bound = 12 * U24 * (np.abs(x["dE0"]) + w0 * np.abs(dc + t1) / 2 + w1 * np.abs(dc + t2) / 2 + reg2 * np.abs(e)) + 1e-37
    assert (np.abs(_np(dE) - w64[1]) <= bound).all()
    tag = f"content n={n} gap={gap}"
    _check("dow", _np(go), w64[2], w32[2], GRAD_CAP, tag)
    _check("dgw", _np(gg), w64[3], w32[3], GRAD_CAP, tag)


# ------------------------------------------------------------------------------------------------ fusion
@pytest.mark.parametrize("n", [1, 17, 1000])
def test_fusion_fwd_bwd(n):
    rng = np.random.default_rng(50 + n)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    x = {k: f(n, 64) for k in ("IMG", "TXT", "PI", "PT", "dS")}
    x["PI"], x["PT"] = 1 / (1 + np.exp(-x["PI"])), 1 / (1 + np.exp(-x["PT"]))  # the prefer gates are sigmoids
    aI, aT = f(n), f(n)
    aI[::5] += 60.0 * np.where(np.arange(len(aI[::5])) % 2 == 0, 1, -1)  # saturated rows, both ways
    if n == 1:
        aI[0] = aT[0] + 0.5
    d = {k: dev(v) for k, v in x.items()}
    daI_, daT_ = dev(aI), dev(aT)
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
    SIDE, alpha = nan(n, 64), nan(n)
    _call("gmr_gr_fusion_fwd", n, _ptr(d["IMG"]), _ptr(d["TXT"]), _ptr(daI_), _ptr(daT_), _ptr(d["PI"]), _ptr(d["PT"]),
          _ptr(SIDE), _ptr(alpha))
    o = {k: nan(n, 64) for k in ("dIMG", "dTXT", "dPI", "dPT")}
    gI, gT = nan(n), nan(n)
    _call("gmr_gr_fusion_bwd", n, _ptr(d["IMG"]), _ptr(d["TXT"]), _ptr(alpha), _ptr(d["PI"]), _ptr(d["PT"]), _ptr(d["dS"]),
          _ptr(o["dIMG"]), _ptr(o["dTXT"]), _ptr(gI), _ptr(gT), _ptr(o["dPI"]), _ptr(o["dPT"]))
    ak = _np(alpha)

    def ref(dtype, alpha_in=None):
        t = lambda a: torch.tensor(a, dtype=dtype)  # noqa: E731
        im, tx, pi, pt = (t(x[k]).requires_grad_(True) for k in ("IMG", "TXT", "PI", "PT"))
        ai = t(aI).requires_grad_(True)
        a = torch.softmax(torch.stack([ai, t(aT)], 1), 1)[:, 0] if alpha_in is None else \
            t(alpha_in).requires_grad_(True)
        com = a[:, None] * im + (1 - a[:, None]) * tx
        side = (pi * (im - com) + pt * (tx - com) + com) / 4
        g = torch.autograd.grad((side * t(x["dS"])).sum(), [im, tx, pi, pt, ai if alpha_in is None else a])
        return [a.detach().numpy(), side.detach().numpy()] + [v.numpy() for v in g]

    w64, w32 = ref(torch.float64), ref(torch.float32)
    gap = np.abs(aI.astype(np.float64) - aT)
    a64 = w64[0]
    # subtract (half an ulp of the gap, times the softmax's slope a (1 - a)), exp, add, divide
    assert (np.abs(ak - a64) <= U24 * (4 * a64 + 2 * gap * a64 * (1 - a64)) + 1e-37).all()
    im, tx, pi, pt, ds = (x[k].astype(np.float64) for k in ("IMG", "TXT", "PI", "PT", "dS"))
    a = a64[:, None]
    com = a * np.abs(im) + (1 - a) * np.abs(tx)
    # alpha's 4 roundings, COM (two products, a sum), two differences, two products, two sums, the quarter: 12; and
    # the rounding of aI - aT, which moves each weight by the gap times the other weight
    bound = 12 * U24 * (pi * (np.abs(im) + com) + pt * (np.abs(tx) + com) + com) / 4 + 1e-37
    bound = bound + U24 * gap[:, None] * a * (1 - a) * (np.abs(im) + np.abs(tx)) * (1 + pi + pt) / 4
    assert (np.abs(_np(SIDE) - w64[1]) <= bound).all()
    # the backward from the alpha it was given (the kernel's own fp32 one), so alpha's rounding is no error of its
    wk = ref(torch.float64, ak)
    a = ak.astype(np.float64)[:, None]
    com = a * np.abs(im) + (1 - a) * np.abs(tx)
    g = np.abs(ds) / 4
    slack = 8 * U24  # at most: 1 - a, COM's three, a difference, two products, a sum
    checks = {"dPI": (wk[4], g * (np.abs(im) + com)), "dPT": (wk[5], g * (np.abs(tx) + com)),
              "dIMG": (wk[2], g * pi + a * g * (1 + pi + pt)), "dTXT": (wk[3], g * pt + (1 - a) * g * (1 + pi + pt))}
    for k, (want, mag) in checks.items():
        assert (np.abs(_np(o[k]) - want) <= slack * mag + 1e-37).all(), k
    # daI: 64 terms summed per row, through the softmax
    _check("daI", _np(gI), w64[6], w32[6], GRAD_CAP, f"fusion n={n}")
    assert np.array_equal(_np(gT), -_np(gI))


# ------------------------------------------------------------------------------------------------ mul64 / dot64
@pytest.mark.parametrize("rows", [1, 17, 16400])
def test_mul64_dot64(rows):
    rng = np.random.default_rng(70 + rows)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    a, b, old = f(rows, 64), f(rows, 64), f(rows, 64)
    scale = float(np.float32(-0.37))
    da, db = _table(a, True), _table(b, True)
    want = scale * a.astype(np.float64) * b
    for acc in (0, 1):
        out = _table(old if acc else np.full((rows, 64), np.nan, np.float32), True)
        _call("gmr_mul64_f32", rows, _ptr(da), 192, _ptr(db), 192, _ptr(out), 192, scale, acc)
        # two products and, accumulating, a sum
        bound = 3 * U24 * (np.abs(want) + acc * np.abs(old)) + 1e-37
        assert (np.abs(_np(out) - (want + acc * old.astype(np.float64))) <= bound).all()
        assert _untouched(out) and _untouched(da) and _untouched(db)
    parts = torch.full((1024,), float("nan"), dtype=torch.float64, device=DEV)
    w64 = (a.astype(np.float64) * b).sum() * scale
    w32 = (torch.tensor(a) * torch.tensor(b)).sum().item() * np.float32(scale)
    dc = dev(b)  # one strided, one contiguous operand
    for acc in (0, 1):
        base = np.float32(3.25)
        res = []
        for _ in range(2):
            out = dev(np.array([base if acc else np.nan], np.float32))
            _call("gmr_dot64_f32", rows, _ptr(da), 192, _ptr(dc), 64, _ptr(parts), scale, _ptr(out), acc)
            res.append(_np(out))
        assert np.array_equal(res[0], res[1])
        _check("dot64", res[0], np.array([w64 + acc * base]), np.array([np.float32(w32) + acc * base]), FWD_CAP,
               f"rows={rows} acc={acc}")


# ------------------------------------------------------------------------------------------------ InfoNCE rows
NCE_COLS = [1, 63, 64, 65, 255, 256, 257, 1000]


def _nce_logits(cols, spread):
    rng = np.random.default_rng(cols + int(spread))
    if spread == 0:
        L = 3.0 * rng.standard_normal((cols, cols))
    else:
        L = rng.uniform(-spread, spread, (cols, cols))
        L[:, 0] = spread                                         # for every other row, a logit at the top
        L[0, :] = rng.uniform(-spread, -spread + 5, cols)       # a row at the bottom throughout
        L[cols // 2, :] = rng.uniform(spread - 5, spread, cols)  # and one at the top
    return L.astype(np.float32)


def _nce_square(L32, coef):
    cols = L32.shape[0]
    ld = cols + 3
    buf = torch.full((cols, ld), FILL)
    buf[:, :cols] = torch.tensor(L32)
    buf = buf.to(DEV)
    loss = torch.full((cols,), float("nan"), device=DEV)
    _call("gmr_nce_rows_f32", cols, _ptr(buf), ld, coef, _ptr(loss))
    return _np(buf), _np(loss)


@pytest.mark.parametrize("spread", [0, 60, 100])
@pytest.mark.parametrize("cols", NCE_COLS)
def test_nce_rows(cols, spread):
    L32 = _nce_logits(cols, spread)
    L64 = torch.tensor(L32, dtype=torch.float64)
    lse = torch.logsumexp(L64, 1)
    want = (lse - L64.diagonal()).numpy()
    w32 = (torch.logsumexp(torch.tensor(L32), 1) - torch.tensor(L32).diagonal()).numpy()
    tag = f"nce cols={cols} spread={spread}"
    kept, loss0 = _nce_square(L32, 0.0)
    assert np.array_equal(kept[:, :cols], L32) and (kept[:, cols:] == FILL).all()  # coef = 0 leaves L as it was
    _check("loss", loss0, want, w32, FWD_CAP, tag)
    coef = float(np.float32(0.013))
    grad, loss1 = _nce_square(L32, coef)
    assert np.array_equal(loss0, loss1) and (grad[:, cols:] == FILL).all()
    sm = torch.softmax(L64, 1).numpy()
    wantg = coef * (sm - np.eye(cols))
    # lse = m + log S: S's sum (ceil(cols / 256) + 8 adds), the logarithm, the sum rounded at |lse|; l - lse rounded
    # at |l - lse|; exp; the product; and on the diagonal the difference, rounded below coef
    lse_, l_ = lse.numpy()[:, None], L32.astype(np.float64)
    bound = coef * U24 * (sm * (2 * np.abs(lse_) + np.abs(l_ - lse_) + 24) + np.eye(cols)) + 1e-37
    assert np.isfinite(grad).all()
    assert (np.abs(grad[:, :cols] - wantg) <= bound).all(), tag
    assert (np.abs(grad[:, :cols].astype(np.float64).sum(1)) <= bound.sum(1)).all(), tag  # softmax - e_diag sums to 0


@pytest.mark.parametrize("cols", NCE_COLS)
def test_nce_rows_off_is_the_square_rows(cols):
    """A rank's rows [d, d + rows) against all cols keys equal the same rows of the square call, bit for bit."""
    L32 = _nce_logits(cols, 60)
    coef = float(np.float32(0.013))
    for c in (0.0, coef):
        sq, sq_loss = _nce_square(L32, c)
        rows = max(1, min(cols // 3, 40))
        for d in sorted({0, min(5, cols - rows), cols - rows}):
            ld = cols + 3
            buf = torch.full((rows, ld), FILL)
            buf[:, :cols] = torch.tensor(L32[d:d + rows])
            buf = buf.to(DEV)
            loss = torch.full((rows,), float("nan"), device=DEV)
            _call("gmr_nce_rows_off_f32", rows, cols, _ptr(buf), ld, d, c, _ptr(loss))
            assert np.array_equal(_np(loss), sq_loss[d:d + rows]), (cols, d, c)
            assert np.array_equal(_np(buf), sq[d:d + rows]), (cols, d, c)


# ------------------------------------------------------------------------------------------------ BPR log-sigmoid
@pytest.mark.parametrize("B", [1, 15, 16, 17, 1000])
def test_bpr_logsigmoid(B):
    U, I = 37, 53
    rng = np.random.default_rng(90 + B)
    C = rng.standard_normal((U + I, 64)).astype(np.float32)
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    users[B // 2:] = users[: B - B // 2]  # repeated users
    neg[0] = (pos[0] + 1) % I
    C[U + pos[0]] = 1.2 * np.sign(C[users[0]])  # x = 2.4 sum |u|, about 120; the swapped sample gives -120
    C[U + neg[0]] = -C[U + pos[0]]
    if B > 1:
        pos[1], neg[1], users[1] = neg[0], pos[0], users[0]
    inv = float(np.float32(1.0 / B))
    loss = torch.full((B,), float("nan"), device=DEV)
    contrib = torch.full((3 * B + 1, 64), float("nan"), device=DEV)
    contrib[3 * B] = FILL
    dC, du, dp, dn = dev(C), dev(users, torch.int32), dev(pos, torch.int32), dev(neg, torch.int32)
    _call("gmr_bpr_logsigmoid_f32", B, U, _ptr(dC), _ptr(du), _ptr(dp), _ptr(dn), _ptr(loss), _ptr(contrib), inv)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)  # noqa: E731
    u, p, q = t(C[users]), t(C[U + pos]), t(C[U + neg])  # the gathered rows: gradients before any scatter
    xx = (u * p).sum(1) - (u * q).sum(1)
    rows = F.softplus(-xx)
    gu, gp, gq = torch.autograd.grad((rows * inv).sum(), [u, p, q])
    x_ = xx.detach().numpy()
    assert np.abs(x_).max() > 100 and (B == 1 or (x_.min() < -100 and x_.max() > 100))
    # x: per lane four products and four adds, the difference, four butterfly levels: 10 roundings of the terms' sizes
    ud, pd, qd = u.detach().numpy(), p.detach().numpy(), q.detach().numpy()
    dx_ = 10 * U24 * (np.abs(ud * pd) + np.abs(ud * qd)).sum(1)
    sig = 1 / (1 + np.exp(x_))  # |d softplus(-x) / dx|
    got = _np(loss)
    assert np.isfinite(got).all()
    # softplus's own value: exp, log1p, max, sum
    assert (np.abs(got - rows.detach().numpy()) <= sig * dx_ + 4 * U24 * rows.detach().numpy() + 1e-37).all()
    # dx = -inv / (1 + exp(x)): d log|dx| / dx = sigmoid(x) <= 1; exp, sum, divide; then a difference and a product
    got = _np(contrib)
    rel = (dx_ + 6 * U24)[:, None]
    for k, (want, mag) in enumerate(((gu, np.abs(pd - qd)), (gp, np.abs(ud)), (gq, np.abs(ud)))):
        blk = got[k * B:(k + 1) * B]
        assert (np.abs(blk - want.numpy()) <= rel * (sig * inv)[:, None] * mag + 1e-37).all(), "UPN"[k]
    assert (got[3 * B] == FILL).all()


# ------------------------------------------------------------------------------------------------ nce pairs / combine
@pytest.mark.parametrize("row0,B", [(0, 50), (0, 20), (13, 20), (30, 20)])
@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
def test_nce_pairs_and_combine(nterms, row0, B):
    Bg, tab, ct, dts = 50, 57, B + 3, 61
    terms = [(0, 1), (2, 3), (0, 3), (2, 1)][:nterms] if nterms != 3 else [(1, 1), (0, 1), (3, 0)]
    i1 = (ctypes.c_int32 * 4)(*([a for a, _ in terms] + [0] * (4 - nterms)))
    i2 = (ctypes.c_int32 * 4)(*([b for _, b in terms] + [0] * (4 - nterms)))
    i1p, i2p = ctypes.cast(i1, ctypes.c_void_p), ctypes.cast(i2, ctypes.c_void_p)
    rng = np.random.default_rng(nterms * 100 + row0 + B)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    nv, contrib, dT = f(4, tab, 64), f(4, ct, 128), f(4, dts, 64)
    cln = torch.full((4, ct, 128), FILL, device=DEV)
    dnv, dcontrib, ddT = dev(nv), dev(contrib), dev(dT)
    _call("gmr_nce_pairs_f32", nterms, B, Bg, row0, i1p, i2p, _ptr(dnv), tab, _ptr(cln), ct)
    want = np.full((4, ct, 128), np.float32(FILL))
    for k, (a, b) in enumerate(terms):
        want[k, :B, :64], want[k, :B, 64:] = nv[a, row0:row0 + B], nv[b, row0:row0 + B]
    assert np.array_equal(_np(cln), want)  # rows past B and terms past nterms keep the sentinel
    g = torch.full((4, tab, 64), FILL, device=DEV)
    _call("gmr_nce_combine_f32", nterms, B, Bg, row0, i1p, i2p, _ptr(dcontrib), ct, _ptr(ddT), dts, _ptr(g), tab)
    want = np.full((4, tab, 64), np.float32(FILL))
    want[:, :Bg] = 0
    for j in range(4):
        for k, (a, b) in enumerate(terms):  # term order; within a term: dP, then dT, then the positive part
            if a == j:
                want[j, row0:row0 + B] = want[j, row0:row0 + B] + contrib[k, :B, :64]
            if b == j:
                want[j, :Bg] = want[j, :Bg] + dT[k, :Bg]
                want[j, row0:row0 + B] = want[j, row0:row0 + B] + contrib[k, :B, 64:]
    assert want.dtype == np.float32
    assert np.array_equal(_np(g), want)  # rows past Bg keep the sentinel
