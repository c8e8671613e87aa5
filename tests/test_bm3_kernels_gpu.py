"""The BM3 loss kernel of csrc/bm3.hip by name, against the fp64 row restatement of tests/bm3_fixture.py.

Bars: rtol 1e-5 against fp64, and next to it (the cosine gradients cancel: d_on is orthogonal to the online row) an
entry may be off by twice the largest error of the same computation done by fp32 torch on the CPU against fp64,
measured here (the rule of test_ddrm_kernels_gpu.py)."""
import numpy as np
import pytest
import torch

import bm3_fixture as F
import philox_ref as PR

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL, SITE = 2.0, 0xB30
MODS = {"both": (True, True), "T null": (False, True), "V null": (True, False)}


def _lib():
    from gmr.utils import get_model
    get_model("BM3")  # the feature under test: raises ValueError without it
    from gmr import _lib as lib
    return lib


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _stream():
    from gmr.kernels import stream
    return stream()


def TR():
    return int(_lib().load().gmr_bm3_tile_rows())


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


DATA = {}


def make_data(B):
    """An (U + I) x 192 work table [G | T | V] (T, V on the item rows), the predictor and a batch with repeats; the
    mid shape for B = 700."""
    if B not in DATA:
        U, I = (300, 1100) if B >= 700 else (23, 19)
        rng = np.random.default_rng(1000 + B)
        d = {"U": U, "I": I, "tab": (rng.standard_normal((U + I, 192)) * 0.3).astype(np.float32),
             "Wp": (rng.standard_normal((64, 64)) * 0.15).astype(np.float32),
             "bp": (rng.standard_normal(64) * 0.05).astype(np.float32),
             "users": rng.integers(0, U, B).astype(np.int32), "items": rng.integers(0, I, B).astype(np.int32)}
        if B > 2:
            d["users"][2] = d["users"][0]
            d["items"][1] = d["items"][0]
        DATA[B] = d
    return DATA[B]


def streams(d, hasT, hasV):
    U, tab, us, it = d["U"], d["tab"], d["users"], d["items"]
    return [tab[us, :64], tab[U + it, :64], tab[U + it, 64:128] if hasT else None,
            tab[U + it, 128:] if hasV else None]


def table_keep(d, p, seed):
    rng = np.random.default_rng(seed)
    U, I = d["U"], d["I"]
    return {k: (rng.random((n, 64)) >= p).astype(np.uint8) for k, n in (("u", U), ("i", I), ("t", I), ("v", I))}


def run(d, hasT=True, hasV=True, p=0.0, keep=None, mode=None, seed=5, step=0, ldc=192, want_keep=True, B=None,
        ldg=192, keep_out_all=False, inv=None):
    """gmr_bm3_loss_fwd_bwd on the case.  keep: [u, i, t, v] batch keep bytes (given mode).  Every output starts as
    NaN (keep_out as 9).  Returns the outputs on the device."""
    lib = _lib()
    B = d["users"].size if B is None else B
    U = d["U"]
    tab = dev(d["tab"])
    T = tab[U:, 64:128] if hasT else None
    V = tab[U:, 128:] if hasV else None
    Wp, bp, us, it = dev(d["Wp"]), dev(d["bp"]), dev(d["users"]), dev(d["items"])
    mode = (1 if keep is not None else 2) if mode is None else mode
    kin = [dev(k) if k is not None else None for k in (keep if keep is not None else [None] * 4)]
    has = [True, True, hasT, hasV]
    ko = [torch.full((max(B, 1), 64), 9, dtype=torch.uint8, device=DEV)
          if (mode == 2 and want_keep and (h or keep_out_all)) else None for h in has]
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
    n = max(B, 1)
    out = {"cos": nan(6, n), "contrib": nan(2 * n, ldc), "xg": nan(4 * n, 64), "don": nan(4 * n, 64), "keep": ko}
    lib.call("gmr_bm3_loss_fwd_bwd", B, U, _ptr(tab), ldg, _ptr(T), 192, _ptr(V), 192, _ptr(us), _ptr(it), _ptr(Wp),
             64, _ptr(bp), p, CL, 1.0 / n if inv is None else inv, mode, *[_ptr(k) for k in kin], 64, seed, step, SITE,
             *[_ptr(k) for k in ko], 64, _ptr(out["cos"]), _ptr(out["contrib"]), ldc, _ptr(out["xg"]), _ptr(out["don"]),
             _stream())
    torch.cuda.synchronize()
    return out


def _bar(got, ref64, ref32, what):
    own = float(np.abs(ref32.astype(np.float64) - ref64).max())
    got = got.cpu().numpy().astype(np.float64)
    print(f"{what}: max abs error {np.abs(got - ref64).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(got, ref64, rtol=1e-5, atol=2 * own, err_msg=what)


def _check(got, d, hasT, hasV, keep, p, what):
    B = d["users"].size
    x = streams(d, hasT, hasV)
    r64 = F.bm3_rows_ref(x, d["Wp"], d["bp"], keep, p, CL, 1.0 / B, torch.float64)
    r32 = F.bm3_rows_ref(x, d["Wp"], d["bp"], keep, p, CL, 1.0 / B, torch.float32)
    for k in ("cos", "contrib", "don"):
        _bar(got[k], r64[k], r32[k], f"{what} {k}")
    assert np.array_equal(got["xg"].cpu().numpy(), r32["xg"])  # the gathered rows, copied
    assert not np.any(got["contrib"][:B, 64:].cpu().numpy())   # exact zeros beside dx_u
    for s, h in ((2, hasT), (3, hasV)):
        if not h:
            assert not np.any(got["don"][s * B:(s + 1) * B].cpu().numpy())
            assert not np.any(got["contrib"][B:, 64 * (s - 1):64 * s].cpu().numpy())


@pytest.mark.parametrize("mods", list(MODS))
@pytest.mark.parametrize("brel", ["1", "TR-1", "TR+1", "3TR+5", "700"])
def test_rows_against_fp64(brel, mods):
    tr = TR()
    B = {"1": 1, "TR-1": tr - 1, "TR+1": tr + 1, "3TR+5": 3 * tr + 5, "700": 700}[brel]
    hasT, hasV = MODS[mods]
    d = make_data(B)
    for p in (0.0, 0.5):
        tk = table_keep(d, p, 7 * B + 1)
        keep = F.batch_keep(tk, d["users"], d["items"], mods=(["text"] if hasT else []) + (["image"] if hasV else []))
        got = run(d, hasT, hasV, p=p, keep=keep)
        _check(got, d, hasT, hasV, keep, p, f"B={B} {mods} p={p}")


def test_zero_mask_row_and_zero_input_row():
    tr = TR()
    B = tr + 1
    d = dict(make_data(B))
    d["tab"] = d["tab"].copy()
    d["tab"][d["users"][3], :64] = 0.0               # an all-zero user row: its online row is bp
    d["tab"][d["U"] + d["items"][4], 64:128] = 0.0   # an all-zero text row
    tk = table_keep(d, 0.5, 3)
    tk["i"][d["items"][0]] = 0                       # the item target of row 0 (and of its repeat, row 1): all dropped
    tk["t"][d["items"][5]] = 0
    keep = F.batch_keep(tk, d["users"], d["items"])
    got = run(d, p=0.5, keep=keep)
    for k in ("cos", "contrib", "don", "xg"):
        assert bool(torch.isfinite(got[k]).all()), k
    cos, don = got["cos"].cpu().numpy(), got["don"].cpu().numpy()
    for row in (0, 1):
        assert cos[0, row] == 0 and cos[2, row] == 0 and cos[3, row] == 0   # ui, t, v against the zero target
        assert not np.any(don[row])                                          # d_on of the user stream: ui only
    assert cos[4, 5] == 0                                                    # tv against the zero text target
    _check(got, d, True, True, keep, 0.5, "zero rows")


def _philox_keep(seed, step, stream, ids, p):
    off = (ids.astype(np.uint64)[:, None] * np.uint64(16) + np.arange(16, dtype=np.uint64)[None]).reshape(-1)
    w = PR.philox(PR.site_seed(seed, SITE + stream), step, off).reshape(ids.size, 64)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u < np.float32(1) - np.float32(p)).astype(np.uint8)


def test_draw_mode():
    B, p = 700, 0.3
    d = dict(make_data(B))
    rng = np.random.default_rng(4)
    d["items"] = rng.permutation(d["I"])[:B].astype(np.int32)  # distinct items, then one repeat
    d["items"][9] = d["items"][3]
    a = run(d, p=p, seed=11, step=4)
    b = run(d, p=p, seed=11, step=4)
    o = run(d, p=p, seed=11, step=5)
    for k in ("cos", "contrib", "don"):
        assert torch.equal(a[k], b[k]), k
    keep = [k.cpu().numpy() for k in a["keep"]]
    ids = [d["users"], d["items"], d["items"], d["items"]]
    for s in range(4):
        assert np.array_equal(keep[s], _philox_keep(11, 4, s, ids[s], p)), s   # the documented key, bit for bit
        assert not np.array_equal(keep[s], o["keep"][s].cpu().numpy())         # two steps differ
    assert np.array_equal(keep[1][9], keep[1][3]) and np.array_equal(keep[0][2], keep[0][0])  # a mask per table row
    assert not np.array_equal(keep[1], keep[2]) and not np.array_equal(keep[2], keep[3])      # the sites differ
    assert not np.array_equal(keep[1], keep[3])
    same = d["users"][:, None] == d["items"][None]
    r, c = np.nonzero(same)
    if r.size:  # a user id equal to an item id draws another mask
        assert not np.array_equal(keep[0][r[0]], keep[1][c[0]])
    uniq = np.unique(d["items"], return_index=True)[1]
    for s in (1, 2, 3):
        k = keep[s][uniq]
        n = k.size
        assert n >= 699 * 64 and abs(k.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (s, k.mean())
        assert abs(k.mean(0) - (1 - p)).max() < 0.08  # every column draws
    _check(a, d, True, True, keep, p, "drawn masks")
    # keep_out is optional, and p = 0 keeps everything
    n0 = run(d, p=p, seed=11, step=4, want_keep=False)
    assert torch.equal(n0["cos"], a["cos"]) and torch.equal(n0["contrib"], a["contrib"])
    z = run(d, p=0.0, seed=11, step=4)
    assert all(int(k.min()) == 1 for k in z["keep"])


def test_rows_do_not_depend_on_the_batch():
    """A row's outputs depend on its own inputs and ids: the same rows in a shorter batch, bit for bit."""
    tr = TR()
    B = 3 * tr + 5
    d = make_data(B)
    full = run(d, p=0.5, seed=21, step=2)
    n = tr + 3
    part = dict(d, users=d["users"][:n].copy(), items=d["items"][:n].copy())
    got = run(part, p=0.5, seed=21, step=2, inv=1.0 / B)
    assert torch.equal(got["cos"], full["cos"][:, :n])
    assert torch.equal(got["contrib"][:n], full["contrib"][:n])
    assert torch.equal(got["contrib"][n:], full["contrib"][B:B + n])
    for s in range(4):
        assert torch.equal(got["don"][s * n:(s + 1) * n], full["don"][s * B:s * B + n]), s
        assert torch.equal(got["keep"][s], full["keep"][s][:n])


def test_rejects_bad_arguments():
    d = make_data(TR() + 1)
    with pytest.raises(RuntimeError):
        run(d, B=0)
    with pytest.raises(RuntimeError):
        run(d, ldc=190)              # contribution rows off 16-byte alignment
    with pytest.raises(RuntimeError):
        run(d, ldg=194)              # table rows off 16-byte alignment
    with pytest.raises(RuntimeError):
        run(d, hasT=False, keep_out_all=True)   # keep bytes of the text stream requested without its table
    with pytest.raises(RuntimeError):
        keep = F.batch_keep(table_keep(d, 0.5, 1), d["users"], d["items"])
        keep[3] = None
        run(d, p=0.5, keep=keep)     # given mode without the image stream's bytes
    with pytest.raises(RuntimeError):
        run(d, p=1.0)


def test_loss_reduce():
    lib = _lib()
    B = 700
    rng = np.random.default_rng(8)
    cos = rng.uniform(-1, 1, (6, B)).astype(np.float32)
    sq = np.array([3.7, 11.2], np.float32)
    I, rw = 1100, 0.1
    dcos, dsq = dev(cos), dev(sq)
    for has_t, has_v in ((1, 1), (0, 1), (1, 0)):
        loss = torch.full((10,), float("nan"), device=DEV)
        lib.call("gmr_bm3_loss_reduce", B, _ptr(dcos), _ptr(dsq), has_t, has_v, rw, CL, 1.0 / B, I, _ptr(loss),
                 _stream())
        m = 1 - cos.astype(np.float64).mean(1)
        m[[2, 4]] *= has_t
        m[[3, 5]] *= has_v
        nu, ni = np.sqrt(sq.astype(np.float64))
        reg = (nu + ni) / I
        want = np.concatenate([[m[0] + m[1] + rw * reg + CL * m[2:].sum()], m, [reg, rw / (I * nu), rw / (I * ni)]])
        np.testing.assert_allclose(loss.cpu().numpy(), want, rtol=2e-6)


def test_reg_bwd():
    lib = _lib()
    N, U = 53, 23
    rng = np.random.default_rng(2)
    G = rng.standard_normal((N, 64)).astype(np.float32)
    dG = rng.standard_normal((N, 192)).astype(np.float32)
    coef = np.array([0.25, -1.5], np.float32)
    g, dg, dcoef = dev(G), dev(dG), dev(coef)
    lib.call("gmr_bm3_reg_bwd", N, U, _ptr(dcoef), _ptr(g), 64, _ptr(dg), 192, _stream())
    want = dG.copy()
    want[:U, :64] += coef[0] * G[:U]
    want[U:, :64] += coef[1] * G[U:]
    np.testing.assert_allclose(dg.cpu().numpy(), want, rtol=1e-6, atol=1e-7)
    assert np.array_equal(dg.cpu().numpy()[:, 64:], dG[:, 64:])
