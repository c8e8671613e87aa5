"""The LD4MRec row kernels (csrc/ld4m.hip) against fp64 torch built here: FiLM-modulated LayerNorm forward and
backward, exact GELU with inverted dropout, the smoothed-target MSE rows, the loss-history moving average and
the importance draw of t."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a):
    return torch.as_tensor(a).to(DEV)


def _call(name, *args):
    from gmr import _lib
    return _lib.call(name, *args)


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _stream():
    from gmr.kernels import stream
    return stream()


def _strided(a, pad):
    """A device copy of the 2-D array a inside a buffer whose rows are `pad` floats longer (pad % 4 == 0)."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device=DEV)
    v = buf[:, :a.shape[1]]
    v.copy_(torch.as_tensor(a))
    return v


def _grad_bar(got, want, name):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * np.abs(want).max(), err_msg=name)


# ----------------------------------------------------------------------------- FiLM
def _film_case(rows, H, seed=3):
    rng = np.random.default_rng(seed + rows + H)
    f = lambda *s, sc=1.0: (sc * rng.standard_normal(s)).astype(np.float32)  # noqa: E731
    return dict(h=f(rows, H) + 0.3, w=1 + f(H, sc=0.2), b=f(H, sc=0.2), s=f(rows, H, sc=0.5), sh=f(rows, H, sc=0.5),
                dz=f(rows, H), dh0=f(rows, H))


def _film_ref(c, H):
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in ("h", "w", "b", "s", "sh")) for k, v in c.items()}
    n = torch.nn.functional.layer_norm(t["h"], (H,), t["w"], t["b"], 1e-5)
    z = n * (1 + t["s"]) + t["sh"]
    g = torch.autograd.grad(z, [t["h"], t["w"], t["b"], t["s"], t["sh"]], t["dz"])
    return z.detach().numpy(), [x.numpy() for x in g]


def _film_fp32_error(c, H, z_ref):
    """Largest absolute error of the same forward in fp32 CPU torch against fp64: the reference's own error."""
    t = {k: torch.tensor(c[k], dtype=torch.float32) for k in ("h", "w", "b", "s", "sh")}
    z = torch.nn.functional.layer_norm(t["h"], (H,), t["w"], t["b"], 1e-5) * (1 + t["s"]) + t["sh"]
    return float(np.abs(z.double().numpy() - z_ref).max())


# H 576 fills a lane's third float4 for lanes 0..15 only, 1024 all four; 8 rows are one film_bwd workgroup, 9 one more
@pytest.mark.parametrize("H", [64, 256, 320, 576, 1024])
@pytest.mark.parametrize("rows", [1, 5, 8, 9, 67, 300])
def test_film_fwd_bwd(rows, H):
    from gmr import _lib
    c = _film_case(rows, H)
    z_ref, (dh_ref, dw_ref, db_ref, ds_ref, dsh_ref) = _film_ref(c, H)
    h, s, sh, dz = _strided(c["h"], 8), _strided(c["s"], 4), _strided(c["sh"], 12), _strided(c["dz"], 4)
    w, b = dev(c["w"]), dev(c["b"])
    z = _strided(np.zeros((rows, H), np.float32), 16)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    _call("gmr_ld4_film_fwd", rows, H, _ptr(h), h.stride(0), _ptr(w), _ptr(b), _ptr(s), s.stride(0), _ptr(sh),
          sh.stride(0), 1e-5, _ptr(z), z.stride(0), _ptr(mean), _ptr(rstd), _stream())
    # rtol 1e-5.  It cannot hold in fp32 where the terms of n (1 + s) + sh cancel (the error is relative to the
    # terms, not to z), so next to it an entry may be off by twice the largest error of the fp32 torch forward
    # against fp64 on the same inputs (the rule for a bar that does not hold, both figures there)
    own = _film_fp32_error(c, H, z_ref)
    got = z.cpu().numpy().astype(np.float64)
    rel = np.abs(got - z_ref) / np.maximum(np.abs(z_ref), 1e-300)
    print(f"film_fwd rows={rows} H={H}: max abs error {np.abs(got - z_ref).max():.3e} (fp32 torch {own:.3e}), "
          f"entries past rtol 1e-5: {(rel > 1e-5).sum()} of {rel.size}")
    np.testing.assert_allclose(got, z_ref, rtol=1e-5, atol=2 * own)
    h64 = c["h"].astype(np.float64)
    np.testing.assert_allclose(mean.cpu().numpy(), h64.mean(1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rstd.cpu().numpy(), 1 / np.sqrt(h64.var(1) + 1e-5), rtol=1e-5)
    # backward: dh accumulates onto a non-zero residual gradient; dsh written, then aliased
    nparts = int(_lib.load().gmr_ld4_film_parts_floats(rows, H))
    assert nparts == (rows + 7) // 8 * 2 * H
    parts = torch.empty(nparts, device=DEV)
    for alias in (False, True):
        dh = _strided(c["dh0"], 4)
        ds, dsh = _strided(np.zeros((rows, H), np.float32), 8), _strided(np.zeros((rows, H), np.float32), 4)
        dw, db = torch.full((H,), 3.0, device=DEV), torch.full((H,), 3.0, device=DEV)
        dsh_arg = dz if alias else dsh
        _call("gmr_ld4_film_bwd", rows, H, _ptr(h), h.stride(0), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b), _ptr(s),
              s.stride(0), _ptr(dz), dz.stride(0), _ptr(ds), ds.stride(0), _ptr(dsh_arg), dsh_arg.stride(0), _ptr(dh),
              dh.stride(0), 1, _ptr(parts), _ptr(dw), _ptr(db), 0, _stream())
        _grad_bar(dh.cpu().numpy(), dh_ref + c["dh0"].astype(np.float64), "dh")
        _grad_bar(ds.cpu().numpy(), ds_ref, "ds")
        _grad_bar(dw.cpu().numpy(), dw_ref, "dw")
        _grad_bar(db.cpu().numpy(), db_ref, "db")
        if alias:
            np.testing.assert_array_equal(dz.cpu().numpy(), c["dz"])
        else:
            np.testing.assert_array_equal(dsh.cpu().numpy(), c["dz"])
            assert float(dsh._base[:, H:].min()) == 7.0 and float(ds._base[:, H:].min()) == 7.0  # pads untouched
    # overwrite mode and parameter accumulation
    dh = _strided(c["dh0"], 4)
    _call("gmr_ld4_film_bwd", rows, H, _ptr(h), h.stride(0), _ptr(mean), _ptr(rstd), _ptr(w), _ptr(b), _ptr(s),
          s.stride(0), _ptr(dz), dz.stride(0), _ptr(ds), ds.stride(0), None, 0, _ptr(dh), dh.stride(0), 0,
          _ptr(parts), _ptr(dw), _ptr(db), 1, _stream())
    _grad_bar(dh.cpu().numpy(), dh_ref, "dh overwrite")
    _grad_bar(dw.cpu().numpy(), 2 * dw_ref, "dw accumulate")


def test_film_rejects_width():
    x = torch.zeros((4, 96), device=DEV)
    v = torch.zeros(96, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        _call("gmr_ld4_film_fwd", 4, 96, _ptr(x), 96, _ptr(v), _ptr(v), _ptr(x), 96, _ptr(x), 96, 1e-5, _ptr(x), 96,
              _ptr(v), _ptr(v), _stream())


# ----------------------------------------------------------------------------- add_bias
@pytest.mark.parametrize("H", [64, 1024])
def test_add_bias(H):
    """y = x + bias is one IEEE add per entry: bit-equal to fp32 numpy, out of place and with y == x."""
    rows = 37
    rng = np.random.default_rng(H)
    x = rng.standard_normal((rows, H)).astype(np.float32)
    bias = rng.standard_normal(H).astype(np.float32)
    want = x + bias[None, :]
    d_x, d_b = _strided(x, 8), dev(bias)
    y = _strided(np.full((rows, H), np.nan, np.float32), 4)
    _call("gmr_ld4_add_bias", rows, H, _ptr(d_x), d_x.stride(0), _ptr(d_b), _ptr(y), y.stride(0), _stream())
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    np.testing.assert_array_equal(d_x.cpu().numpy(), x)
    _call("gmr_ld4_add_bias", rows, H, _ptr(d_x), d_x.stride(0), _ptr(d_b), _ptr(d_x), d_x.stride(0), _stream())
    np.testing.assert_array_equal(d_x.cpu().numpy(), want)
    assert float(y._base[:, H:].min()) == 7.0 and float(d_x._base[:, H:].min()) == 7.0  # pads untouched
    assert float(y._base[:, H:].max()) == 7.0 and float(d_x._base[:, H:].max()) == 7.0


# ----------------------------------------------------------------------------- GELU + dropout
def _gelu_fwd(x, p_keep, mask_in, mask_out, key=(11, 4, 1000), y=None):
    rows, H = x.shape
    y = torch.empty_like(x) if y is None else y
    _call("gmr_ld4_gelu_drop_fwd", rows, H, _ptr(x), x.stride(0), p_keep, _ptr(mask_in), _ptr(mask_out), H, key[0],
          key[1], key[2], _ptr(y), y.stride(0), _stream())
    return y


def test_gelu_drop():
    _gelu_drop_case(300, 256, "cpu")


# 4099 x 1024 is 4099 blocks of 256 float4; the launch is capped at 16384 blocks, which 16387 x 1024 passes, so every
# thread there takes a second grid stride.  For these two shapes alone the fp64 reference is evaluated on the device.
@pytest.mark.parametrize("rows", [4099, 16387])
def test_gelu_drop_large(rows):
    assert 16387 * (1024 // 4) > 16384 * 256
    _gelu_drop_case(rows, 1024, DEV)


def _gelu_drop_case(rows, H, ref_dev):
    rng = np.random.default_rng(8)
    x = dev((1.5 * rng.standard_normal((rows, H))).astype(np.float32))
    x64 = x.double().to(ref_dev)
    gelu = torch.nn.functional.gelu(x64).cpu().numpy()
    # p_keep = 1: exact GELU, no mask touched
    # rtol 1e-5, and where (1 + erf) cancels for negative x (fp32 error eps32 |x| / 2, far above 1e-5 of a tiny
    # result) twice the largest error of fp32 torch's own exact GELU against fp64
    own = float(np.abs(torch.nn.functional.gelu(x.cpu()).double().numpy() - gelu).max())
    tol = dict(rtol=1e-5, atol=2 * own)
    y = _gelu_fwd(x, 1.0, None, None)
    print(f"gelu: max abs error {np.abs(y.cpu().numpy() - gelu).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(y.cpu().numpy(), gelu, **tol)
    # draw + record
    mask = torch.full((rows, H), 9, dtype=torch.uint8, device=DEV)
    y1 = _gelu_fwd(x, 0.9, None, mask)
    mk = mask.cpu().numpy()
    assert set(np.unique(mk)) == {0, 1}
    n = rows * H
    assert abs(int(mk.sum()) - 0.9 * n) <= 5 * np.sqrt(n * 0.9 * 0.1)
    np.testing.assert_allclose(y1.cpu().numpy(), gelu * mk / np.float64(np.float32(0.9)), **tol)
    # the bytes are gmr_keep_mask_u8's at the same key
    want = torch.empty(n, dtype=torch.uint8, device=DEV)
    _call("gmr_keep_mask_u8", n, 0.9, 11, 4, 1000, _ptr(want), _stream())
    np.testing.assert_array_equal(mk.reshape(-1), want.cpu().numpy())
    # replay: identical bits
    y2 = _gelu_fwd(x, 0.9, mask, None)
    assert torch.equal(y1, y2)
    # backward against autograd on the replayed mask (and at p_keep = 1)
    dy = dev(rng.standard_normal((rows, H)).astype(np.float32))
    for pk, m in ((0.9, mask), (1.0, None)):
        xr = x64.clone().requires_grad_(True)
        out = torch.nn.functional.gelu(xr)
        if m is not None:
            out = out * m.to(ref_dev).double() / float(np.float32(0.9))
        ref = torch.autograd.grad(out, xr, dy.double().to(ref_dev))[0].cpu().numpy()
        dx = torch.empty_like(x)
        _call("gmr_ld4_gelu_drop_bwd", rows, H, _ptr(x), x.stride(0), _ptr(m), H, pk, _ptr(dy), dy.stride(0), _ptr(dx),
              dx.stride(0), _stream())
        _grad_bar(dx.cpu().numpy(), ref, f"dx p_keep {pk}")


# ----------------------------------------------------------------------------- loss rows
@pytest.mark.parametrize("I", [41, 1103])
def test_loss_rows(I):
    rng = np.random.default_rng(I)
    U, B, gamma = 23, 19, 0.1
    deg = rng.integers(1, min(I, 30), U)
    deg[4] = 0                                   # a user with an empty history
    if I > 300:
        deg[7] = 300                             # past one 256-thread pass of the bitmap fill
    items = [np.sort(rng.choice(I, d, replace=False)) for d in deg]
    uptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    uitems = np.concatenate(items).astype(np.int32)
    users = rng.integers(0, U, B).astype(np.int32)
    users[0], users[1], users[2] = 4, 9, 9       # the empty user; a user repeated in the batch
    users[3] = 7
    pred = rng.standard_normal((B, I)).astype(np.float32)
    X = np.zeros((U, I))
    for u_, it in enumerate(items):
        X[u_, it] = 1
    x = X[users]
    target = x * (1 - np.float64(np.float32(gamma))) + (1 - x) * np.float64(np.float32(gamma))
    d = pred.astype(np.float64) - target
    norm_rows = 31.0
    d_users, d_uptr, d_uitems = dev(users), dev(uptr), dev(uitems)
    for write in (0, 1):
        p = _strided(pred, 4 - I % 4 + 8)
        loss = torch.empty(B, dtype=torch.float64, device=DEV)
        _call("gmr_ld4_loss_rows", B, I, _ptr(d_users), _ptr(d_uptr), _ptr(d_uitems), gamma, _ptr(p),
              p.stride(0), 1.0 / norm_rows, _ptr(loss), write, _stream())
        np.testing.assert_allclose(loss.cpu().numpy(), (d ** 2).mean(1), rtol=1e-5)
        if write:
            _grad_bar(p.cpu().numpy(), 2 * d / (I * norm_rows), "dpred")
        else:
            np.testing.assert_array_equal(p.cpu().numpy(), pred)
        assert float(p._base[:, I:].min()) == 7.0  # nothing written past the row


# ----------------------------------------------------------------------------- history EMA
def _ema_loop(hist, t, loss):
    h = hist.copy()
    for tb, lb in zip(t, loss):
        if tb >= 0:
            h[tb] = np.float32(np.float32(0.9) * h[tb]) + np.float32(0.1 * float(np.float32(lb)))
    return h


@pytest.mark.parametrize("T,B", [(100, 64), (1024, 2100)])   # the second: the largest T, a batch past one staged chunk
def test_history_ema(T, B):
    rng = np.random.default_rng(2)
    t = rng.integers(0, T, B).astype(np.int32)
    shared = [3, 17, 30, 44, B - 4]
    t[shared] = 42
    t[[5, 6]] = -1
    loss = rng.uniform(0.1, 0.4, B)
    loss[shared] = 0.2 * np.linspace(1, 10, 5)   # the five rows of t = 42 span 10x
    hist0 = rng.uniform(0.5, 1.5, T).astype(np.float32)
    want = _ema_loop(hist0, t, loss)
    rev = t.copy(), loss.copy()
    rev[1][shared] = loss[shared][::-1]
    assert abs(_ema_loop(hist0, *rev)[42] - want[42]) > 1e-3 * want[42]   # the order of the five rows matters
    hist, d_t, d_loss = dev(hist0.copy()), dev(t), dev(loss)
    _call("gmr_ld4_history_ema", B, T, _ptr(d_t), _ptr(d_loss), _ptr(hist), _stream())
    got = hist.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=0)
    untouched = np.setdiff1d(np.arange(T), t[t >= 0])
    np.testing.assert_array_equal(got[untouched], hist0[untouched])


# ----------------------------------------------------------------------------- sample_t
def _sample(hist, u=None, B=None, key=(5, 9), row0=0):
    B = len(u) if u is not None else B
    t = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    d_hist, d_u = dev(hist), dev(u) if u is not None else None
    _call("gmr_ld4_sample_t", B, len(hist), _ptr(d_hist), _ptr(d_u), key[0], key[1],
          row0, _ptr(t), _stream())
    return t.cpu().numpy()


def test_sample_t_injected():
    _sample_t_injected_case(100)


@pytest.mark.parametrize("T", [1, 1024])  # one bin; the largest table
def test_sample_t_injected_other_T(T):
    _sample_t_injected_case(T)


def _sample_t_injected_case(T):
    rng = np.random.default_rng(6)
    hist = rng.uniform(0.2, 3.0, T).astype(np.float32)
    hist[::7] *= -1                              # |hist| is what counts
    a = np.abs(hist.astype(np.float64))
    cdf = np.cumsum(a / a.sum())
    edges = np.concatenate([[0.0], cdf])
    us, want = [], []
    for k in range(T):
        for q in (0.25, 0.5, 0.75):
            us.append(edges[k] + q * (edges[k + 1] - edges[k]))
            want.append(k)
    us += [0.0, 1 - 2.0 ** -24]
    want += [0, T - 1]
    u32 = np.asarray(us, np.float32)
    assert np.array_equal(np.minimum(np.searchsorted(cdf, u32.astype(np.float64), side="right"), T - 1), want)
    np.testing.assert_array_equal(_sample(hist, u32), want)


def test_sample_t_philox():
    T, B = 100, 4096
    hist = np.ones(T, np.float32)
    t = _sample(hist, B=B)
    assert t.min() >= 0 and t.max() < T
    assert len(np.unique(t)) == T
    np.testing.assert_array_equal(_sample(hist, B=B), t)                 # same key, same draw
    assert not np.array_equal(_sample(hist, B=B, key=(5, 10)), t)
    halves = np.concatenate([_sample(hist, B=2048), _sample(hist, B=2048, row0=2048)])
    np.testing.assert_array_equal(halves, t)                             # keyed by the global row


def _sample_replica(hist, B, key, row0):
    """The kernel's Philox branch on the CPU: 24-bit u in [0, 1), the fp64 cdf summed in order, t = #{k: cdf_k <= u}
    clamped; and the smallest distance of any u from an edge."""
    import philox_ref
    T = len(hist)
    a = np.abs(hist.astype(np.float64))
    tot = np.cumsum(a)[-1]  # np.cumsum adds in order
    cdf = np.cumsum(a / tot)
    w = philox_ref.philox(key[0] ^ 0xA5A5A5A5, key[1], row0 + np.arange(B, dtype=np.uint64))
    u = (w[:, 0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    t = np.minimum(np.searchsorted(cdf, u, side="right"), T - 1).astype(np.int32)
    return t, float(np.abs(u[:, None] - cdf[None, :]).min())


@pytest.mark.parametrize("T", [1, 100, 1024])
def test_sample_t_philox_replica(T):
    B, key, row0 = 4096, (5, 9), 123
    hist = np.random.default_rng(T).uniform(0.2, 3.0, T).astype(np.float32)
    hist[::5] *= -1
    want, gap = _sample_replica(hist, B, key, row0)
    assert T == 1 or gap > 1e-12   # decided on the CPU: a last-bit difference of the device's cdf moves no draw
    np.testing.assert_array_equal(_sample(hist, B=B, key=key, row0=row0), want)
