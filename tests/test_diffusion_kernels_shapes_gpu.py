"""The diffusion row kernels of csrc/diffusion.hip, called by name through _lib.call at shapes past the fixtures,
against fp64 numpy / torch references built here and tests/philox_ref.py for everything drawn.

Every 2-D operand sits in a buffer whose rows are longer than the logical width (the pad holds 7.0 and is asserted
untouched); outputs start as NaN (or -7 for integers), so an unwritten in-range entry fails.

Bars, none of them tuned to a kernel:
  exact        densify, transpose, every integer draw, keep masks, history bookkeeping, a call in two row0 halves
               against the whole, sparse_hidden's h against sparse_pre's, a repeated call against itself
  sums         |got - ref| <= (n + 2) 2^-24 sum|terms| (sum|terms| in fp64), n = the terms on the longest chain
               including the fixed-order partial combines, stated beside each assertion
  pointwise    k 2^-24 times the magnitude of the terms, k = roundings + 1, counted beside each assertion
  transcendentals (tanh; cos / sin / exp of the time embedding; log / sqrt / sincos of Box-Muller): DESIGN section 2's
               rule - the kernel may be off from fp64 by at most twice the largest error of the same computation in
               fp32 numpy on the same inputs, both figures printed

Seen on the MI355X, kernel (fp32 numpy restatement), largest absolute error against fp64:
  Box-Muller eps       I = 37: 1.05e-6 (1.04e-6); I = 1103: 1.20e-6 (1.20e-6)
  time embedding       T = 1: 0 (0); T <= 7: 2.9e-8 .. 2.8e-7 (3.2e-8 .. 3.1e-7); T = 100: 6.5e-7 (6.5e-7);
                       T = 1000, E = 64: 3.57e-5 (3.57e-5) - the fp32 rounding of the angle t exp(..), shared by both
  tanh, sparse h       H = 4: 3.6e-8 (3.6e-8); H = 1020 .. 2052: 5.6e-8 .. 7.6e-8 (5.7e-8 .. 5.9e-8)
  tanh, tanh_bias      1 x 4: 3.2e-8 (3.4e-8); 300 x 1000: 8.1e-8 (6.0e-8); 4099 x 4100: 8.4e-8 (6.0e-8)
The kernel's figure is at most 1.39 times the restatement's in any case; every sum and pointwise bar held as derived.
"""
import numpy as np
import pytest
import torch

import philox_ref
from oracle import model_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
TINY = 1e-37
FILL = 7.0


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
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


def _strided(a, pad):
    """A device copy of the 2-D array a inside a buffer whose rows are `pad` elements longer, the pad holding FILL."""
    a = torch.as_tensor(a)
    buf = torch.full((a.shape[0], a.shape[1] + pad), FILL, dtype=a.dtype, device=DEV)
    v = buf[:, :a.shape[1]]
    v.copy_(a)
    return v


def _nan(rows, cols, pad):
    return _strided(torch.full((rows, cols), float("nan")), pad)


def _pads_ok(*views):
    return all(bool((v._base[:, v.shape[1]:] == FILL).all()) for v in views)


def _sum_ok(got, ref, terms, n, what):
    """The running-error bound of a length-n fp32 sum: |got - ref| <= (n + 2) 2^-24 sum|terms|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), what
    bound = (n + 2) * U24 * np.asarray(terms, np.float64) + TINY
    bad = np.abs(got - ref) > bound
    assert not bad.any(), (what, n, float(np.abs(got - ref)[bad].max()), float(bound[bad].min()), int(bad.sum()))


def _transc_ok(got, ref64, restated32, what):
    """at most twice the fp32 restatement's largest error against fp64."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    own = float(np.abs(np.asarray(restated32, np.float64) - ref64).max()) if ref64.size else 0.0
    err = float(np.abs(got - ref64).max()) if ref64.size else 0.0
    print(f"{what}: kernel {err:.3e} (fp32 numpy {own:.3e})")
    assert err <= 2 * own, (what, err, own)
    return err, own


def _csr(I, degs, rng):
    """A train CSR of len(degs) users with the given degrees (capped at I), items ascending; and its dense 0/1 rows."""
    degs = [min(int(d), I) for d in degs]
    items = [np.sort(rng.choice(I, d, replace=False)) for d in degs]
    uptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    uitems = (np.concatenate(items) if sum(degs) else np.zeros(0)).astype(np.int32)
    X = np.zeros((len(degs), I))
    for u, it in enumerate(items):
        X[u, it] = 1
    pad = np.zeros(4, np.int32)  # the item array is never empty on the device
    return dev(uptr), dev(np.concatenate([uitems, pad])), X


def _users(U, B, rng):
    """B users, permuted, the first repeated as the last when B > 1."""
    u = rng.permutation(U)[np.arange(B) % U].astype(np.int32)
    if B > 1:
        u[-1] = u[0]
    return u


# ------------------------------------------------------------------------------------------------ densify
@pytest.mark.parametrize("I", [1, 3, 37, 256, 1103])
def test_densify(I):
    rng = np.random.default_rng(I)
    U = 300
    degs = [(0, 1, 64, 65, 200)[u % 5] for u in range(U)]  # above 64: the second pass of the 64-thread item loop
    uptr, uitems, X = _csr(I, degs, rng)
    for B in (1, 5, 300):
        for given in (True, False):
            users = _users(U, B, rng) if given else np.arange(B, dtype=np.int32)
            x, d_users = _nan(B, I, 3), dev(users)
            _call("gmr_diff_densify", B, I, _ptr(d_users) if given else None, _ptr(uptr), _ptr(uitems), _ptr(x),
                  x.stride(0))
            np.testing.assert_array_equal(_np(x), X[users])
            assert _pads_ok(x)


# ------------------------------------------------------------------------------------------------ sample_t
def _t_ref(seed, step, row0, B, T):
    w = philox_ref.philox(seed ^ 0xA5A5A5A5, step, row0 + np.arange(B, dtype=np.uint64))
    return ((w[:, 0].astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.int32)


def _sample_t(B, T, seed, step, row0):
    t = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
    _call("gmr_diff_sample_t", B, T, seed, step, row0, _ptr(t))
    assert int(t[B]) == -7
    return _np(t[:B])


@pytest.mark.parametrize("T", [1, 5, 1000])
def test_sample_t(T):
    seed, step, row0 = 0x1234567890ABCDEF, 7, 40
    for B in (1, 255, 256, 257, 5000):
        got = _sample_t(B, T, seed, step, row0)
        np.testing.assert_array_equal(got, _t_ref(seed, step, row0, B, T))
        if B > 1:
            k = B // 2 + 1
            halves = np.concatenate([_sample_t(k, T, seed, step, row0), _sample_t(B - k, T, seed, step, row0 + k)])
            np.testing.assert_array_equal(halves, got)
    if T == 1000:
        assert len(np.unique(got)) > 900


# ------------------------------------------------------------------------------------------------ q_sample
QS_DEGS = (0, 1, 64, 65, 300)


def _qsample(B, I, users, uptr, uitems, t, sa, s1, noise, keep, kp, dropout, seed, step, row0):
    x = _nan(B, I, 5)
    ld = lambda v: v.stride(0) if v is not None else 0  # noqa: E731
    _call("gmr_diff_qsample", B, I, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(t), _ptr(sa), _ptr(s1), _ptr(noise),
          ld(noise), _ptr(keep), ld(keep), kp, dropout, seed, step, row0, _ptr(x), x.stride(0))
    assert _pads_ok(x)
    return x


@pytest.mark.parametrize("I", [1, 3, 37, 1103])
def test_qsample_injected(I):
    rng = np.random.default_rng(100 + I)
    T, kp = 7, float(np.float32(0.8))
    uptr, uitems, X = _csr(I, QS_DEGS, rng)
    sa = rng.uniform(0.1, 1.0, T).astype(np.float32)
    s1 = rng.uniform(0.1, 1.0, T).astype(np.float32)
    kscale = np.float64(np.float32(1) / np.float32(kp))  # kp at its fp32 value, as is its correctly rounded inverse
    for B in (1, 19):
        users = _users(len(QS_DEGS), B, rng)
        if B > 1:
            users[1] = 4  # the degree-300 user is in every batch
        t = rng.integers(0, T, B).astype(np.int32)
        noise = rng.standard_normal((B, I)).astype(np.float32)
        keep = (rng.random((B, I)) < kp).astype(np.float32)
        d_noise, d_keep = _strided(noise, 2), _strided(keep, 7)
        a = sa[t].astype(np.float64)[:, None] * X[users]
        b = s1[t].astype(np.float64)[:, None] * noise
        for dropout in (0, 1):
            x = _qsample(B, I, dev(users), uptr, uitems, dev(t), dev(sa), dev(s1), d_noise, d_keep, kp, dropout, 1, 2, 0)
            f = keep * kscale if dropout else 1.0
            # three roundings: s1 eps, the sum (one when the two contract), the product with keep / kp: k = 4
            got = _np(x).astype(np.float64)
            assert np.isfinite(got).all()
            assert (np.abs(got - (a + b) * f) <= 4 * U24 * (np.abs(a) + np.abs(b)) * f + TINY).all(), (B, dropout)
        assert _pads_ok(d_noise, d_keep)


def _box_muller(words, dtype):
    """gmr::box_muller of the word pairs (w0, w1), (w2, w3) -> the four columns of a quad, in dtype."""
    u = philox_ref.u32_to_unit(words).astype(dtype)  # exact in fp32
    two_pi = np.float32(6.283185307179586) if dtype == np.float32 else np.float64(2 * np.pi)
    out = np.empty(u.shape, dtype)
    for k in (0, 2):
        r = np.sqrt(dtype(-2) * np.log(u[:, k]))
        ang = two_pi * u[:, k + 1]
        out[:, k], out[:, k + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


def _draw_ref(seed, step, row0, B, I):
    """eps (fp64 and its fp32 restatement) and the uniform behind the keep mask of rows row0 .. row0 + B."""
    c4n = (I + 3) // 4
    off = ((np.arange(B, dtype=np.uint64)[:, None] + np.uint64(row0)) << np.uint64(24)) ^ np.arange(c4n, dtype=np.uint64)
    we = philox_ref.philox(seed, 2 * step, off.ravel())
    wk = philox_ref.philox(seed, 2 * step + 1, off.ravel())
    sh = lambda a: a.reshape(B, c4n * 4)[:, :I]  # noqa: E731
    return sh(_box_muller(we, np.float64)), sh(_box_muller(we, np.float32)), sh(philox_ref.u32_to_unit(wk))


@pytest.mark.parametrize("I", [37, 1103])  # I % 4 != 0: the tail of the dense kernel's quad
def test_qsample_philox(I):
    rng = np.random.default_rng(200 + I)
    B, T, kp = 19, 7, float(np.float32(0.8))
    seed, step, row0 = 0xC0FFEE1234, 11, 1000
    uptr, uitems, X = _csr(I, QS_DEGS, rng)  # 37 of 37 and 300 of 1103 items: every lane position c & 3
    users = _users(len(QS_DEGS), B, rng)
    users[1], users[2] = 4, 3
    d_users = dev(users)
    one, zero = dev(np.ones(1, np.float32)), dev(np.zeros(1, np.float32))
    t0 = dev(np.zeros(B, np.int32))
    # sqrt_ac = 0, sqrt_1mac = 1, no dropout: x = 0 + 1 eps exactly, from the dense draw and from the per-item draw
    eps = _qsample(B, I, d_users, uptr, uitems, t0, zero, one, None, None, 1.0, 0, seed, step, row0)
    e64, e32, uk = _draw_ref(seed, step, row0, B, I)
    got = _np(eps).astype(np.float64)
    _transc_ok(got, e64, e32, f"box_muller I={I}")
    n = got.size  # mean and variance of N(0, 1) within five standard errors
    assert abs(got.mean()) <= 5 / np.sqrt(n) and abs(got.var() - 1) <= 5 * np.sqrt(2 / n)
    keep = (uk <= np.float32(kp)).astype(np.float32)
    assert abs(keep.mean() - kp) <= 5 * np.sqrt(kp * (1 - kp) / n)
    # the real call against the injected call fed that eps and that mask
    sa, s1 = dev(rng.uniform(0.1, 1.0, T).astype(np.float32)), dev(rng.uniform(0.1, 1.0, T).astype(np.float32))
    t = dev(rng.integers(0, T, B).astype(np.int32))
    real = _qsample(B, I, d_users, uptr, uitems, t, sa, s1, None, None, kp, 1, seed, step, row0)
    d_eps, d_keep = _strided(_np(eps), 3), _strided(keep, 6)
    inj = _qsample(B, I, d_users, uptr, uitems, t, sa, s1, d_eps, d_keep, kp, 1, seed ^ 99, step + 1, 0)
    np.testing.assert_array_equal(_np(real), _np(inj))
    assert (_np(real)[keep == 0] == 0).all() and (_np(real)[keep == 1] != 0).any()
    # injected noise with the drawn mask, and the drawn noise with the injected mask
    np.testing.assert_array_equal(
        _np(_qsample(B, I, d_users, uptr, uitems, t, sa, s1, d_eps, None, kp, 1, seed, step, row0)), _np(real))
    np.testing.assert_array_equal(
        _np(_qsample(B, I, d_users, uptr, uitems, t, sa, s1, None, d_keep, kp, 1, seed, step, row0)), _np(real))
    k = 9
    h1 = _qsample(k, I, d_users[:k], uptr, uitems, t[:k], sa, s1, None, None, kp, 1, seed, step, row0)
    h2 = _qsample(B - k, I, d_users[k:], uptr, uitems, t[k:], sa, s1, None, None, kp, 1, seed, step, row0 + k)
    np.testing.assert_array_equal(np.concatenate([_np(h1), _np(h2)]), _np(real))


# ------------------------------------------------------------------------------------------------ importance draw of t
def _imp_inputs(T, Hn):
    rng = np.random.default_rng(T * 31 + Hn)
    return rng.uniform(0.05, 2.0, (T, Hn))


def _imp_replica(hist, up, seed, step, row0, B):
    """The kernel's full-history branch in fp64: sequential sums, the 53-bit uniform, the first cdf edge above u."""
    T, Hn = hist.shape
    m = np.zeros(T)
    for j in range(Hn):
        m = m + hist[:, j] * hist[:, j]
    pall = np.sqrt(m / Hn)
    tot = np.cumsum(pall)[-1]  # np.cumsum adds in order
    pall = pall / tot * (1.0 - up) + up / T
    cdf = np.cumsum(pall)
    w = philox_ref.philox(seed ^ 0x5EED5EED, step, row0 + np.arange(B, dtype=np.uint64)).astype(np.uint64)
    k53 = (w[:, 0] << np.uint64(21)) ^ (w[:, 1] >> np.uint64(11))
    u = k53.astype(np.float64) * (1.0 / 9007199254740992.0) * cdf[T - 1]
    t = np.minimum(np.searchsorted(cdf, u, side="right"), T - 1)
    gap = float(np.abs(u[:, None] - cdf[None, :T - 1]).min() / cdf[T - 1]) if T > 1 else 1.0
    return t.astype(np.int32), pall, gap


IMP_KEY = (0xBADC0DE, 3, 17)  # seed, step, row0: no u within 1e-12 of a cdf edge at any (T, hist_len) below


def test_importance_replica_is_decided_on_the_cpu():
    """The device may contract m += h h into an fma, moving a cdf edge by an ulp: no u may lie that close to one."""
    for T in (1, 100, 1024):
        for Hn in (1, 10, 16):
            assert _imp_replica(_imp_inputs(T, Hn), 0.001, *IMP_KEY, 5000)[2] > 1e-12, (T, Hn)


@pytest.mark.parametrize("Hn", [1, 10, 16])
@pytest.mark.parametrize("T", [1, 100, 1024])
def test_sample_t_importance(T, Hn):
    seed, step, row0 = IMP_KEY
    B, up = 5000, 0.001  # past one 1024-thread stride
    hist = _imp_inputs(T, Hn)
    d_hist = dev(hist)

    def draw(count):
        t = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        pt = torch.full((B,), float("nan"), device=DEV)
        d_count = dev(count)
        _call("gmr_diff_sample_t_importance", B, T, Hn, _ptr(d_hist), _ptr(d_count), up, seed, step, row0, _ptr(t),
              _ptr(pt))
        return _np(t), _np(pt)

    count = np.full(T, Hn, np.int32)
    count[T // 2] = Hn - 1
    t, pt = draw(count)  # a history not yet full: gmr_diff_sample_t's draw at the same key, pt = 1
    np.testing.assert_array_equal(t, _sample_t(B, T, seed, step, row0))
    assert (pt == 1).all()
    want_t, pall, gap = _imp_replica(hist, up, seed, step, row0, B)
    assert gap > 1e-12
    t, pt = draw(np.full(T, Hn, np.int32))
    np.testing.assert_array_equal(t, want_t)
    np.testing.assert_allclose(pall, model_ref.importance_pt_all(hist, up), rtol=1e-13)
    want_pt = pall[want_t] * T
    # pt = (float)(pall T): fp64 up to the order of its sums, then one rounding to fp32
    assert (np.abs(pt.astype(np.float64) - want_pt) <= (U24 + 1e-13) * want_pt).all()


def test_sample_t_importance_rejects():
    B = 8
    hist = torch.ones((1025, 17), dtype=torch.float64, device=DEV)
    count = torch.ones(1025, dtype=torch.int32, device=DEV)
    t = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    pt = torch.zeros(B, device=DEV)
    for T, Hn in ((1025, 10), (100, 0), (100, 17)):
        with pytest.raises(RuntimeError, match="gmr_diff_sample_t_importance"):
            _call("gmr_diff_sample_t_importance", B, T, Hn, _ptr(hist), _ptr(count), 0.001, 1, 1, 0, _ptr(t), _ptr(pt))
    torch.cuda.synchronize()
    assert (t == -7).all()


# ------------------------------------------------------------------------------------------------ history update
@pytest.mark.parametrize("Hn", [16, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 16384])
def test_history_update(B, Hn):
    T = 1024
    rng = np.random.default_rng(B + Hn)
    t = rng.integers(20, T, B).astype(np.int32)
    hist = rng.standard_normal((T, Hn))
    count = rng.integers(0, Hn + 1, T).astype(np.int32)
    many = np.zeros(0, np.int64)
    if B >= 65:  # one timestep matched more than hist_len times, across the last two 64-row ballots
        many = B - 1 - np.unique(np.linspace(0, 64, Hn + 4).astype(np.int64))
        t[many] = 13
        assert many.min() < B - 64 <= many.max() and len(many) > Hn
        count[13] = Hn // 2
    rows = [r for r in rng.permutation(B) if r not in set(many.tolist())]
    seen = min(3, Hn)
    for i, delta in enumerate((-1, 0, 1)):  # c + seen = hist_len - 1, hist_len, hist_len + 1
        if len(rows) >= seen:
            t[[rows.pop() for _ in range(seen)]] = 10 + i
            count[10 + i] = min(max(Hn + delta - seen, 0), Hn)
    if len(rows) >= 5:
        t[[rows.pop() for _ in range(5)]] = -1  # padding rows
    assert (t == 13).sum() == len(many)
    loss = rng.standard_normal(B)
    live = t >= 0
    want_h, want_c = model_ref.lt_history_update(hist, count, t[live], loss[live])
    d_hist, d_count, d_t, d_loss = dev(hist), dev(count), dev(t), dev(loss)
    _call("gmr_diff_history_update", B, T, Hn, _ptr(d_t), _ptr(d_loss), _ptr(d_hist), _ptr(d_count))
    np.testing.assert_array_equal(_np(d_count), want_c)
    np.testing.assert_array_equal(_np(d_hist), want_h)


def test_history_update_rejects_batch():
    B, T, Hn = 16385, 8, 4
    t = torch.zeros(B, dtype=torch.int32, device=DEV)
    loss = torch.ones(B, dtype=torch.float64, device=DEV)
    hist = torch.full((T, Hn), 3.0, dtype=torch.float64, device=DEV)
    count = torch.zeros(T, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_diff_history_update"):
        _call("gmr_diff_history_update", B, T, Hn, _ptr(t), _ptr(loss), _ptr(hist), _ptr(count))
    torch.cuda.synchronize()
    assert (hist == 3.0).all() and (count == 0).all()


# ------------------------------------------------------------------------------------------------ time bias
def _temb(T, E, dtype):
    """The sinusoidal table as time_bias_kernel writes it, evaluated in dtype (fp32: the same operations in order)."""
    half = E // 2
    out = np.zeros((T, E), dtype)
    if half:
        j = np.arange(half).astype(dtype)
        c = np.float32(-9.210340371976184) if dtype == np.float32 else dtype(-np.log(10000.0))
        a = np.arange(T).astype(dtype)[:, None] * np.exp(c * j / dtype(half))[None, :]
        out[:, :half], out[:, half:2 * half] = np.cos(a), np.sin(a)
    return out


@pytest.mark.parametrize("T,E,H", [(5, 10, 1000), (100, 10, 300), (1, 1, 1), (3, 9, 255), (7, 63, 257), (1000, 64, 256)])
def test_time_bias(T, E, H):
    rng = np.random.default_rng(T + E + H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    embW, embB, b1 = f(E, E), f(E), f(H)
    t64, t32 = _temb(T, E, np.float64), _temb(T, E, np.float32)
    for off in (37, 1104):
        ldw = off + E + 5
        W1 = f(H, ldw)
        d = [dev(v) for v in (embW, embB, W1, b1)]
        EB, temb, emb = (torch.full(s, float("nan"), device=DEV) for s in ((T, H), (T, E), (T, E)))
        _call("gmr_diff_time_bias", T, E, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), ldw, off, _ptr(d[3]), H, _ptr(EB),
              _ptr(temb), _ptr(emb))
        g_temb, g_emb = _np(temb), _np(emb)
        _transc_ok(g_temb, t64, t32, f"temb T={T} E={E}")
        if E % 2:
            assert (g_temb[:, E - 1] == 0).all()  # the odd-E pad column
        # emb[t][i] = sum_j emb_W[i][j] temb[t][j] + emb_b[i] from the kernel's own temb: an fma chain of E terms and
        # the bias add, E + 1 roundings: n = E
        k64 = g_temb.astype(np.float64)
        _sum_ok(g_emb, k64 @ embW.T.astype(np.float64) + embB, np.abs(k64) @ np.abs(embW.T).astype(np.float64)
                + np.abs(embB), E, "emb")
        # EB[t][h] = sum_j emb[t][j] W1[h][off + j] + b1[h] from the kernel's own emb: n = E
        k64, w64 = g_emb.astype(np.float64), W1[:, off:off + E].astype(np.float64)
        _sum_ok(_np(EB), k64 @ w64.T + b1, np.abs(k64) @ np.abs(w64.T) + np.abs(b1), E, "EB")
        EB2 = torch.full((T, H), float("nan"), device=DEV)
        _call("gmr_diff_time_bias", T, E, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), ldw, off, _ptr(d[3]), H, _ptr(EB2), None,
              None)
        assert torch.equal(EB, EB2)


def test_time_bias_rejects_width():
    T, H, ldw = 2, 4, 80
    z = torch.zeros((65 * 65,), device=DEV)
    W1 = torch.zeros((H, ldw), device=DEV)
    EB = torch.full((T, H), 3.0, device=DEV)
    for E in (0, 65):
        with pytest.raises(RuntimeError, match="gmr_diff_time_bias"):
            _call("gmr_diff_time_bias", T, E, _ptr(z), _ptr(z), _ptr(W1), ldw, 4, _ptr(z), H, _ptr(EB), None, None)
    torch.cuda.synchronize()
    assert (EB == 3.0).all()


# ------------------------------------------------------------------------------------------------ time backward
def _time_bwd_case(T, E, H, few):
    assert (T * E <= 64) == few
    rng = np.random.default_rng(T * 1000 + E * 7 + H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    off = 37 if H % 2 else 1104
    ldw = off + E + 3
    S, temb, emb, W1 = f(T, H), f(T, E), f(T, E), f(H, ldw)
    S64, te64, em64, W64 = (v.astype(np.float64) for v in (S, temb, emb, W1[:, off:off + E]))
    demb = S64 @ W64                      # T x E, never leaves the kernel
    ademb = np.abs(S64) @ np.abs(W64)
    # demb[t][i] over h.  FEW: a lane's longest chain is a0's (one term per 256 columns, then one per 64 in the tail:
    # at most ceil(H / 64)), two adds of the four chains, six butterfly levels.  Else: a0 takes H / 4 terms and a
    # tail of up to three, then the two adds.
    n_demb = -(-H // 64) + 2 + 6 if few else H // 4 + 3 + 2
    d = [dev(v) for v in (S, temb, emb, W1)]
    for acc in (0, 1):
        dW1_0, db1_0, dWe_0, dbe_0 = f(H, ldw), f(H), f(E, E), f(E)
        if not acc:
            dW1_0[:, off:off + E] = np.nan
            db1_0[:], dWe_0[:], dbe_0[:] = np.nan, np.nan, np.nan
        o = [dev(v.copy()) for v in (dW1_0, db1_0, dWe_0, dbe_0)]
        _call("gmr_diff_time_bwd", T, E, H, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), ldw, off, _ptr(o[0]),
              _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), acc)
        dW1, db1, dWe, dbe = (_np(v) for v in o)
        old = lambda v: v.astype(np.float64) if acc else 0.0  # noqa: E731
        tag = f"T={T} E={E} H={H} acc={acc}"
        # dW1[h][off + j] = sum_t S[t][h] emb[t][j]: an fma chain over t, n = T (+ 1: the accumulate add)
        _sum_ok(dW1[:, off:off + E], S64.T @ em64 + old(dW1_0[:, off:off + E]),
                np.abs(S64.T) @ np.abs(em64) + np.abs(old(dW1_0[:, off:off + E])), T + acc, "dW1 " + tag)
        np.testing.assert_array_equal(dW1[:, :off], dW1_0[:, :off])
        np.testing.assert_array_equal(dW1[:, off + E:], dW1_0[:, off + E:])
        # db1[h] = sum_t S[t][h]: n = T (+ 1)
        _sum_ok(db1, S64.sum(0) + old(db1_0), np.abs(S64).sum(0) + np.abs(old(db1_0)), T + acc, "db1 " + tag)
        # d emb_W[i][j] = sum_t demb[t][i] temb[t][j]: the chain over t on top of demb's own error; to first order
        # (n_demb + 2) + (T + 2) roundings: n = n_demb + T + 2 (+ 1), over the terms |S W1| |temb|
        _sum_ok(dWe, demb.T @ te64 + old(dWe_0), ademb.T @ np.abs(te64) + np.abs(old(dWe_0)), n_demb + T + 2 + acc,
                "d_emb_W " + tag)
        # d emb_b[i] = sum_t demb[t][i]: the same count
        _sum_ok(dbe, demb.sum(0) + old(dbe_0), ademb.sum(0) + np.abs(old(dbe_0)), n_demb + T + 2 + acc,
                "d_emb_b " + tag)


@pytest.mark.parametrize("T,E", [(5, 10), (1, 64), (4, 16)])
def test_time_bwd_few(T, E):
    for H in (4, 63, 64, 65, 255, 256, 257, 320, 1000):
        _time_bwd_case(T, E, H, True)


@pytest.mark.parametrize("T,E", [(5, 13), (100, 10), (234, 64)])
def test_time_bwd_many(T, E):
    for H in (1, 3, 5, 300, 1001):
        _time_bwd_case(T, E, H, False)


def test_time_bwd_rejected_call_adds_nothing():
    """T E too large for the LDS staging: the call raises before any launch, so nothing was accumulated."""
    T, E, H, off = 300, 64, 8, 5
    ldw = off + E + 3
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    d = [dev(v) for v in (f(T, H), f(T, E), f(T, E), f(H, ldw))]
    init = (f(H, ldw), f(H), f(E, E), f(E))
    o = [dev(v.copy()) for v in init]
    with pytest.raises(RuntimeError, match="gmr_diff_time_bwd"):
        _call("gmr_diff_time_bwd", T, E, H, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), ldw, off, _ptr(o[0]),
              _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), 1)
    torch.cuda.synchronize()
    for got, want in zip(o, init):
        np.testing.assert_array_equal(_np(got), want)


# ------------------------------------------------------------------------------------------------ loss rows
@pytest.mark.parametrize("I", [1, 41, 257, 1103])
def test_loss_rows(I):
    rng = np.random.default_rng(300 + I)
    B, T = 19, 6
    uptr, uitems, X = _csr(I, (0, 300, 5, 1, 17, 300), rng)  # 300 (at I = 1103): the second pass of the bitmap fill
    users = _users(6, B, rng)
    users[1], users[2] = 0, 1
    t = rng.integers(0, T, B).astype(np.int32)
    wtab = rng.uniform(0.2, 3.0, T)
    ptv = rng.uniform(0.5, 2.0, B).astype(np.float32)
    pred = (X[users] + 0.3 * rng.standard_normal((B, I))).astype(np.float32)
    gs = np.float32(1.0 / 31.0)
    d64 = pred.astype(np.float64) - X[users]
    mse = (d64 ** 2).sum(1) / I
    w = wtab[t]
    du, dt_, dw, d_pt = dev(users), dev(t), dev(wtab), dev(ptv)
    n = -(-I // 256) + 8  # a lane's fma chain, six butterfly levels, the two adds of the four wave partials
    for with_pt in (False, True):
        div = ptv.astype(np.float64) if with_pt else np.ones(B)
        for with_loss in (False, True):
            for write in (0, 1):
                out = _strided(pred, 4 - I % 4 + 8)
                o_mse, o_diff, o_loss = (torch.full((B,), float("nan"), dtype=torch.float64, device=DEV) for _ in "abc")
                _call("gmr_diff_loss_rows", B, I, _ptr(du), _ptr(uptr), _ptr(uitems), _ptr(dt_), _ptr(dw),
                      _ptr(d_pt) if with_pt else None, _ptr(out), out.stride(0), float(gs), _ptr(o_mse), _ptr(o_diff),
                      _ptr(o_loss) if with_loss else None, write)
                # the sum bound (d = pred - x0 rounds once, which the + 2 covers twice over in d d); the fp64 scalings
                # after it add a few 2^-53
                for got, scale, what in ((o_mse, 1.0, "mse"), (o_diff, w, "diff"), (o_loss, w / div, "loss")):
                    if what == "loss" and not with_loss:
                        assert torch.isnan(got).all()
                        continue
                    _sum_ok(_np(got), mse * scale, mse * scale * (1 + 1e-9), n, f"{what} I={I}")
                if write:
                    # four roundings: ca to fp32, ca grad_scale, d = pred - x0, ca d: k = 5
                    ca = (w / div * 2.0 / I) * np.float64(gs)
                    want = ca[:, None] * d64
                    assert (np.abs(_np(out) - want) <= 5 * U24 * np.abs(want) + TINY).all()
                else:
                    np.testing.assert_array_equal(_np(out), pred)
                assert _pads_ok(out)


def test_loss_rows_rejects():
    """An item count past the LDS bitmap, and a row stride below I: both return before a launch; the buffers have the
    true sizes, so a library without the checks stays inside them too."""
    I = 480001
    uptr, uitems = dev(np.zeros(3, np.int32)), dev(np.zeros(4, np.int32))
    users, t = dev(np.zeros(2, np.int32)), dev(np.zeros(2, np.int32))
    wtab = dev(np.ones(1))
    o = [torch.full((2,), float("nan"), dtype=torch.float64, device=DEV) for _ in "abc"]
    out = torch.full((1, I), 0.5, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_diff_loss_rows"):
        _call("gmr_diff_loss_rows", 1, I, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(t), _ptr(wtab), None, _ptr(out), I,
              1.0, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), 1)
    small = torch.full((2, 8), 0.5, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_diff_loss_rows"):
        _call("gmr_diff_loss_rows", 2, 8, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(t), _ptr(wtab), None, _ptr(small),
              4, 1.0, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), 1)
    torch.cuda.synchronize()
    assert (out == 0.5).all() and (small == 0.5).all() and all(torch.isnan(v).all() for v in o)


def test_row_strides_below_the_width_are_rejected():
    """gmr_diff_qsample, gmr_diff_densify and gmr_diff_gc_rows: B = 2 rows of I = 8 (or 64) in buffers of 2 x I, called
    with half the stride; every check returns before a launch."""
    B, I = 2, 8
    uptr, uitems = dev(np.zeros(3, np.int32)), dev(np.zeros(4, np.int32))
    users, t = dev(np.zeros(B, np.int32)), dev(np.zeros(B, np.int32))
    tab = dev(np.ones(1, np.float32))
    x, aux = torch.full((B, I), 0.5, device=DEV), torch.ones((B, I), device=DEV)
    for ldx, ldn, ldk in ((4, I, I), (I, 4, I), (I, I, 4)):
        with pytest.raises(RuntimeError, match="gmr_diff_qsample"):
            _call("gmr_diff_qsample", B, I, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(t), _ptr(tab), _ptr(tab),
                  _ptr(aux), ldn, _ptr(aux), ldk, 0.5, 1, 1, 1, 0, _ptr(x), ldx)
    with pytest.raises(RuntimeError, match="gmr_diff_densify"):
        _call("gmr_diff_densify", B, I, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(x), 4)
    iE, Z = torch.ones((4, 64), device=DEV), torch.ones((B, 64), device=DEV)
    G = torch.full((B, 64), 0.5, device=DEV)
    gc = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    for lde, ldz, ldg in ((32, 64, 64), (64, 32, 64), (64, 64, 32)):
        with pytest.raises(RuntimeError, match="gmr_diff_gc_rows"):
            _call("gmr_diff_gc_rows", B, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(iE), lde, _ptr(Z), ldz, 1.0, _ptr(G),
                  ldg, _ptr(gc))
    torch.cuda.synchronize()
    assert (x == 0.5).all() and (G == 0.5).all() and torch.isnan(gc).all()


# ------------------------------------------------------------------------------------------------ gc rows
@pytest.mark.parametrize("B", [1, 3, 4, 5, 300])
def test_gc_rows(B):
    rng = np.random.default_rng(400 + B)
    nI = 600
    degs = (0, 1, 500, 7, 1, 500)
    uptr, uitems, X = _csr(nI, degs, rng)
    users = _users(len(degs), B, rng)
    if B >= 3:
        users[:3] = (0, 2, 1)
    iE = rng.standard_normal((nI, 64)).astype(np.float32)
    Z = rng.standard_normal((B, 64)).astype(np.float32)
    gscale = np.float32(0.37)
    d_iE, d_Z, d_users = _strided(iE, 4), _strided(Z, 8), dev(users)
    y = X[users] @ iE.astype(np.float64)
    A = X[users] @ np.abs(iE).astype(np.float64) + np.abs(Z)
    dref = Z - y
    deg = X[users].sum(1)[:, None]
    for with_G in (False, True):
        G = _nan(B, 64, 12)
        gc = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
        _call("gmr_diff_gc_rows", B, _ptr(d_users), _ptr(uptr), _ptr(uitems), _ptr(d_iE), d_iE.stride(0), _ptr(d_Z),
              d_Z.stride(0), float(gscale), _ptr(G) if with_G else None, G.stride(0), _ptr(gc))
        # d = Z - sum of deg item rows, added in order: a chain of n = deg + 1 terms; e_d bounds its error
        e_d = (deg + 1 + 2) * U24 * A
        if with_G:
            # G = gscale d: one more rounding, inside the + 2
            assert (np.abs(_np(G) - np.float64(gscale) * dref) <= np.float64(gscale) * e_d + TINY).all()
        else:
            assert torch.isnan(G).all()
        # gc = sum_lane d^2 / 64: every term moves by 2 |d| e_d (+ e_d^2), and the sum of 64 squares takes the
        # product's rounding and six butterfly levels: n = 7 over d^2
        bound = ((2 * np.abs(dref) * e_d + e_d ** 2).sum(1) + (7 + 2) * U24 * (dref ** 2).sum(1)) / 64 + TINY
        assert (np.abs(_np(gc) - (dref ** 2).sum(1) / 64) <= bound).all()
        assert _pads_ok(G, d_iE, d_Z)


# ------------------------------------------------------------------------------------------------ column sums
def _colsum(x, group, n_groups, out, acc):
    _call("gmr_colsum_f32", x.shape[0], x.shape[1], _ptr(x), x.stride(0), _ptr(group), n_groups, _ptr(out), acc)


def _colsum_case(rows, cols, n_groups, rng, n):
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    d_x = _strided(x, 3)
    x64 = x.astype(np.float64)
    if n_groups == 1:
        group, d_group = np.zeros(rows, np.int64), None
    else:  # group n_groups - 1 stays empty; -1, n_groups and n_groups + 3 are outside and ignored
        pool = np.concatenate([np.arange(n_groups - 1), [-1, n_groups, n_groups + 3]])
        group = pool[rng.integers(0, len(pool), rows)]
        d_group = dev(group, torch.int32)
    onehot = (group[None, :] == np.arange(n_groups)[:, None]).astype(np.float64)
    ref, terms = onehot @ x64, onehot @ np.abs(x64)
    for acc in (0, 1):
        out0 = rng.standard_normal((n_groups, cols)).astype(np.float32) if acc else np.full((n_groups, cols), np.nan,
                                                                                            np.float32)
        out = torch.cat([dev(out0).reshape(-1), torch.full((5,), FILL, device=DEV)])
        _colsum(d_x, d_group, n_groups, out, acc)
        got = _np(out[:-5]).reshape(n_groups, cols)
        assert (out[-5:] == FILL).all() and _pads_ok(d_x)
        old = out0.astype(np.float64) if acc else 0.0
        _sum_ok(got, ref + old, terms + np.abs(old), n(rows) + acc, f"colsum {rows}x{cols} g={n_groups} acc={acc}")
        empty = onehot.sum(1) == 0
        if empty.any():  # an empty group: 0, or unchanged
            np.testing.assert_array_equal(got[empty], out0[empty] if acc else np.zeros_like(got[empty]))
    return got


# colsum_kernel: wave w adds rows w, w + 16, ... (ceil(rows / 16) terms), then the 16 wave partials in order
N_COLSUM = lambda rows: -(-rows // 16) + 16  # noqa: E731
# colsum_grouped_kernel: rows w, w + 4, ... and the two adds of the four wave partials
N_GROUPED = lambda rows: -(-rows // 4) + 2  # noqa: E731


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 1000])
def test_colsum_one_group(rows):
    rng = np.random.default_rng(rows)
    for cols in (1, 63, 64, 65, 300):
        _colsum_case(rows, cols, 1, rng, N_COLSUM)


@pytest.mark.parametrize("n_groups", [2, 5, 8, 9, 100])
def test_colsum_groups(n_groups):
    rng = np.random.default_rng(n_groups)
    for rows, cols in ((17, 65), (1000, 300)):
        _colsum_case(rows, cols, n_groups, rng, N_COLSUM if n_groups <= 8 else N_GROUPED)


@pytest.fixture(scope="module")
def wide_base():
    """One 5000 x 2048 matrix (rows of 2052) that every split-colsum case slices: read-only."""
    x = np.random.default_rng(77).standard_normal((5000, 2052)).astype(np.float32)
    return x, dev(x)


def _colsum_split(x, out, acc, ws, ws_floats=None):
    _call("gmr_colsum_split_f32", x.shape[0], x.shape[1], _ptr(x), x.stride(0), _ptr(out), acc, _ptr(ws),
          ws.numel() if ws_floats is None else ws_floats)


# colsum_wide_kernel: a lane adds rows rr, rr + 64, ... (ceil(rows / 64) terms), then the 64 slot partials in order
N_WIDE = lambda rows: -(-rows // 64) + 64  # noqa: E731
# split + finish: a wave adds every fourth row of its ceil(rows / 32) rows, two adds, then the 32 partials in order
N_SPLIT = lambda rows: -(-(-(-rows // 32)) // 4) + 2 + 32  # noqa: E731


def _split_case(x, d_x, n, tag):
    rows, cols = x.shape
    rng = np.random.default_rng(rows * 3 + cols)
    x64 = x.astype(np.float64)
    ref, terms = x64.sum(0), np.abs(x64).sum(0)
    ws = torch.full((32 * cols,), float("nan"), device=DEV)
    for acc in (0, 1):
        out0 = rng.standard_normal(cols).astype(np.float32) if acc else np.full(cols, np.nan, np.float32)
        outs = []
        for _ in range(2):  # a repeated call gives the same bits
            out = torch.cat([dev(out0), torch.full((3,), FILL, device=DEV)])
            _colsum_split(d_x, out, acc, ws)
            assert (out[-3:] == FILL).all()
            outs.append(_np(out[:-3]))
        np.testing.assert_array_equal(outs[0], outs[1])
        old = out0.astype(np.float64) if acc else 0.0
        _sum_ok(outs[0], ref + old, terms + np.abs(old), n(rows) + acc, f"{tag} {rows}x{cols} acc={acc}")


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 511, 512, 513, 4096])
def test_colsum_split_wide_path(rows, wide_base):
    x, d_x = wide_base
    for cols in (4, 60, 64, 68, 2048):
        _split_case(x[:rows, :cols], d_x[:rows, :cols], N_WIDE, "wide")


@pytest.mark.parametrize("rows,cols", [(4097, 64), (5000, 64), (1, 37), (31, 37), (33, 37), (1500, 37), (1, 65), (31, 65),
                                       (33, 65), (1500, 65)])
def test_colsum_split_split_path(rows, cols, wide_base):
    x, d_x = wide_base
    _split_case(x[:rows, :cols], d_x[:rows, :cols], N_SPLIT, "split")


def test_colsum_split_unaligned_pointer(wide_base):
    """Four bytes past a 16-byte boundary: the float4 kernel is not eligible, the split pair runs."""
    x, d_x = wide_base
    rows, cols = 100, 64
    v = d_x.reshape(-1)[1:1 + rows * 2052].view(rows, 2052)[:, :cols]
    assert v.data_ptr() % 16 == 4
    _split_case(x.reshape(-1)[1:1 + rows * 2052].reshape(rows, 2052)[:, :cols], v, N_SPLIT, "offset")


def test_colsum_split_rejects_short_workspace(wide_base):
    _, d_x = wide_base
    cols = 64
    ws = torch.zeros(32 * cols, device=DEV)
    out = torch.full((cols,), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_colsum_split_f32"):
        _colsum_split(d_x[:5000, :cols], out, 0, ws, 32 * cols - 1)
    torch.cuda.synchronize()
    assert (out == 3.0).all()


@pytest.mark.parametrize("rows,route", [(2048, "wide"), (1000, "one_group")])  # the wrapper's two routes
def test_colsum_wrapper(rows, route):
    from gmr import kernels as K
    n = {"wide": N_WIDE, "one_group": N_COLSUM}[route]
    x = np.random.default_rng(rows).standard_normal((rows, 1000)).astype(np.float32)
    out = torch.full((1000,), float("nan"), device=DEV)
    K.colsum(dev(x), out)
    x64 = x.astype(np.float64)
    _sum_ok(_np(out), x64.sum(0), np.abs(x64).sum(0), n(rows), f"K.colsum {rows}")


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (33, 31), (100, 7), (1000, 37)])
def test_transpose(rows, cols):
    x = np.random.default_rng(rows + cols).standard_normal((rows, cols)).astype(np.float32)
    d_x, out = _strided(x, 3), _nan(cols, rows, 5)
    _call("gmr_transpose_f32", rows, cols, _ptr(d_x), d_x.stride(0), _ptr(out), out.stride(0))
    np.testing.assert_array_equal(_np(out), x.T)
    assert _pads_ok(out, d_x)


def test_transpose_rejects_short_rows():
    rows, cols = 8, 4
    x = torch.ones((rows, cols), device=DEV)
    out = torch.full((cols, rows), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_transpose_f32"):
        _call("gmr_transpose_f32", rows, cols, _ptr(x), cols, _ptr(out), rows - 1)
    torch.cuda.synchronize()
    assert (out == 3.0).all()


# ------------------------------------------------------------------------------------------------ sparse hidden
@pytest.mark.parametrize("H", [4, 1020, 1024, 1028, 2052])  # above 1024: the second column pass
def test_sparse_hidden_and_pre(H):
    rng = np.random.default_rng(H)
    nI = 320
    degs = (300, 0, 1, 12)
    uptr, uitems, X = _csr(nI, degs, rng)
    W = (0.1 * rng.standard_normal((nI, H))).astype(np.float32)
    eb = (0.5 * rng.standard_normal(H)).astype(np.float32)
    d_W, d_eb = _strided(W, 4), dev(eb)
    for B in (1, 7):
        users = np.array([0, 1, 2, 3, 0, 2, 3][:B], np.int32)
        d_users = dev(users)
        a, h, h2 = _nan(B, H, 8), _nan(B, H, 4), _nan(B, H, 12)
        _call("gmr_diff_sparse_pre", B, H, _ptr(d_users), _ptr(uptr), _ptr(uitems), _ptr(d_W), d_W.stride(0), _ptr(d_eb),
              _ptr(a), a.stride(0), _ptr(h), h.stride(0))
        _call("gmr_diff_sparse_hidden", B, H, _ptr(d_users), _ptr(uptr), _ptr(uitems), _ptr(d_W), d_W.stride(0),
              _ptr(d_eb), _ptr(h2), h2.stride(0))
        assert torch.equal(h, h2) and _pads_ok(a, h, h2, d_W)
        # a = the user's item rows added in order: n = the degree
        Xu = X[users]
        n = int(Xu.sum(1).max())
        _sum_ok(_np(a), Xu @ W.astype(np.float64), Xu @ np.abs(W).astype(np.float64), n, f"a H={H} B={B}")
        # h = tanh(a + eb) from the kernel's own a: the fp32 sum is one IEEE add on both sides
        pre = _np(a) + eb[None, :]
        assert pre.dtype == np.float32
        _transc_ok(_np(h), np.tanh(pre.astype(np.float64)), np.tanh(pre), f"tanh (sparse) H={H} B={B}")


def test_sparse_hidden_rejects_width():
    H, B = 6, 1
    uptr, uitems, users = dev(np.zeros(2, np.int32)), dev(np.zeros(4, np.int32)), dev(np.zeros(1, np.int32))
    W, eb = torch.zeros((4, 8), device=DEV), torch.zeros(8, device=DEV)
    a, h = torch.full((B, 8), 3.0, device=DEV), torch.full((B, 8), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="gmr_diff_sparse_pre"):
        _call("gmr_diff_sparse_pre", B, H, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(W), 8, _ptr(eb), _ptr(a), 8,
              _ptr(h), 8)
    with pytest.raises(RuntimeError, match="gmr_diff_sparse_hidden"):
        _call("gmr_diff_sparse_hidden", B, H, _ptr(users), _ptr(uptr), _ptr(uitems), _ptr(W), 8, _ptr(eb), _ptr(h), 8)
    torch.cuda.synchronize()
    assert (a == 3.0).all() and (h == 3.0).all()


# ------------------------------------------------------------------------------------------------ tanh + bias
@pytest.mark.parametrize("rows,cols", [(1, 4), (300, 1000)])
def test_tanh_bias(rows, cols):
    rng = np.random.default_rng(rows)
    a = (1.5 * rng.standard_normal((rows, cols))).astype(np.float32)
    bias = rng.standard_normal(cols).astype(np.float32)
    d_a, h, d_bias = _strided(a, 4), _nan(rows, cols, 8), dev(bias)
    _call("gmr_tanh_bias_f32", rows, cols, _ptr(d_a), d_a.stride(0), _ptr(d_bias), _ptr(h), h.stride(0))
    pre = a + bias[None, :]
    _transc_ok(_np(h), np.tanh(pre.astype(np.float64)), np.tanh(pre), f"tanh_bias {rows}x{cols}")
    assert _pads_ok(h, d_a)


def test_tanh_bias_no_rows():
    cols = 8
    a, bias = torch.ones((2, cols), device=DEV), torch.ones(cols, device=DEV)
    h = torch.full((2, cols), 3.0, device=DEV)
    _call("gmr_tanh_bias_f32", 0, cols, _ptr(a), cols, _ptr(bias), _ptr(h), cols)
    torch.cuda.synchronize()
    assert (h == 3.0).all()


def test_tanh_bias_past_the_block_cap():
    """4099 x 4100: rows cols / 4 exceeds 16384 blocks of 256, so every thread strides.  The fp64 reference of this
    case alone is evaluated by torch on the device."""
    rows, cols = 4099, 4100
    assert rows * cols // 4 > 16384 * 256
    g = torch.Generator(device=DEV).manual_seed(5)
    base = 1.5 * torch.randn((rows, cols + 4), device=DEV, generator=g)
    a = base[:, :cols]
    bias = torch.randn(cols, device=DEV, generator=g)
    hb = torch.full((rows, cols + 8), float("nan"), device=DEV)
    hb[:, cols:] = FILL
    h = hb[:, :cols]
    _call("gmr_tanh_bias_f32", rows, cols, _ptr(a), a.stride(0), _ptr(bias), _ptr(h), h.stride(0))
    pre = a + bias[None, :]  # one IEEE add, as in the kernel
    ref = torch.tanh(pre.double())
    assert bool(torch.isfinite(h).all()) and bool((hb[:, cols:] == FILL).all())
    err = float((h.double() - ref).abs().max())
    own = float((torch.from_numpy(np.tanh(_np(pre))).to(DEV).double() - ref).abs().max())
    print(f"tanh_bias {rows}x{cols}: kernel {err:.3e} (fp32 numpy {own:.3e})")
    assert err <= 2 * own
