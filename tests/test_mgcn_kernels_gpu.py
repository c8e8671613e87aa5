"""The MGCN kernels of csrc/mgcn.hip by name, against fp64 row restatements with autograd (tests/mgcn_fixture.py).

Bars (the rule of test_bm3_kernels_gpu.py): rtol 1e-5 against fp64, and next to it an entry may be off by twice the
largest error of the same computation done by fp32 torch on the CPU against fp64, measured here and printed."""
import numpy as np
import pytest
import torch

import mgcn_fixture as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from gmr.utils import get_model
    get_model("MGCN")  # the feature under test: raises ValueError without it
    from gmr import _lib as lib
    return lib


def _ptr(t):
    from gmr.kernels import ptr
    return ptr(t)


def _stream():
    from gmr.kernels import stream
    return stream()


def TR():
    return int(_lib().load().gmr_mgcn_tile_rows())


def rows_of(rel):
    tr, mb = TR(), int(_lib().load().gmr_mgcn_max_blocks())
    return {"1": 1, "TR-1": tr - 1, "TR+1": tr + 1, "3TR+5": 3 * tr + 5, "2nd trip": mb * tr + 7}[rel]


ROWS = ["1", "TR-1", "TR+1", "3TR+5", "2nd trip"]


def mat(x, ld=64):
    """x (n x 64 array) as the first 64 columns of a NaN-filled n x ld device tensor."""
    t = torch.full((x.shape[0], ld), float("nan"), device=DEV)
    t[:, :64] = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    return t[:, :64]


def vec(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def nan(n, cols=64, ld=None):
    return torch.full((n, ld or cols), float("nan"), device=DEV)[:, :cols]


def weights(seed, names, scale=0.3):
    rng = np.random.default_rng(seed)
    out = {}
    for k in names:
        shape = (64, 64) if k.startswith("W") else (1, 64) if k == "w2" else (64,)
        out[k] = (rng.standard_normal(shape) * (scale if k.startswith("W") or k == "w2" else 0.2)).astype(np.float32)
    return out


def _bar(got, ref64, ref32, what):
    own = float(np.abs(ref32.astype(np.float64) - ref64).max())
    got = got.cpu().numpy().astype(np.float64)
    print(f"{what}: max abs error {np.abs(got - ref64).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(got, ref64, rtol=1e-5, atol=2 * own, err_msg=what)


# ----------------------------------------------------------------------------------------------- purifier
PW = ("Wgv", "bgv", "Wgt", "bgt")


def pur_data(n, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    d = {k: (rng.standard_normal((n, 64)) * 0.7).astype(np.float32) for k in ("E", "V", "T", "dPv", "dPt", "dE0")}
    d.update(weights(7 + seed, PW))
    return d


def pur_ref(d, dtype, accumulate=False):
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=k in ("E", "V", "T")) for k, v in d.items()}
    yv, yt = t["V"] @ t["Wgv"].T + t["bgv"], t["T"] @ t["Wgt"].T + t["bgt"]
    yv.retain_grad(), yt.retain_grad()
    gv, gt = torch.sigmoid(yv), torch.sigmoid(yt)
    Pv, Pt = t["E"] * gv, t["E"] * gt
    ((Pv * t["dPv"]).sum() + (Pt * t["dPt"]).sum()).backward()
    o = {"Pv": Pv, "Pt": Pt, "gv": gv, "gt": gt, "dE": t["E"].grad + (t["dE0"] if accumulate else 0),
         "z": torch.cat([yv.grad, yt.grad], 1), "dV": t["V"].grad, "dT": t["T"].grad}
    return {k: v.detach().numpy() for k, v in o.items()}


def pur_run(d, n=None, ld=64, accumulate=False):
    """gmr_mgcn_purify_fwd, then gmr_mgcn_purify_bwd on the gates it wrote; every output starts as NaN."""
    lib = _lib()
    n = d["E"].shape[0] if n is None else n
    E, V, T, dPv, dPt = (mat(d[k], ld) for k in ("E", "V", "T", "dPv", "dPt"))
    W = {k: (mat(d[k], ld) if k.startswith("W") else vec(d[k])) for k in PW}
    m = d["E"].shape[0]
    o = {"Pv": nan(m), "Pt": nan(m), "gv": nan(m, ld=128), "gt": nan(m, ld=128), "z": nan(m, 128), "dV": nan(m),
         "dT": nan(m), "dE": mat(d["dE0"]) if accumulate else nan(m)}
    lib.call("gmr_mgcn_purify_fwd", n, _ptr(E), ld, _ptr(V), ld, _ptr(T), ld, _ptr(W["Wgv"]), _ptr(W["bgv"]),
             _ptr(W["Wgt"]), _ptr(W["bgt"]), ld, _ptr(o["Pv"]), _ptr(o["Pt"]), 64, _ptr(o["gv"]), _ptr(o["gt"]), 128,
             _stream())
    lib.call("gmr_mgcn_purify_bwd", n, _ptr(dPv), _ptr(dPt), ld, _ptr(o["gv"]), _ptr(o["gt"]), 128, _ptr(E), ld,
             _ptr(W["Wgv"]), _ptr(W["Wgt"]), ld, _ptr(o["dE"]), 64, int(accumulate), _ptr(o["z"]), 128, _ptr(o["dV"]),
             _ptr(o["dT"]), 64, _stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("ld", [64, 192])
@pytest.mark.parametrize("rel", ROWS)
def test_purifier_against_fp64(rel, ld):
    n = rows_of(rel)
    d = pur_data(n)
    acc = ld == 192
    got = pur_run(d, ld=ld, accumulate=acc)
    r64, r32 = pur_ref(d, torch.float64, acc), pur_ref(d, torch.float32, acc)
    for k in r64:
        _bar(got[k], r64[k], r32[k], f"purifier n={n} ld={ld} {k}")


def test_purifier_rows_do_not_depend_on_the_call():
    tr = TR()
    d = pur_data(3 * tr + 5)
    full, again, short = pur_run(d), pur_run(d), pur_run(d, n=tr + 1)
    for k in full:
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k][:tr + 1], short[k][:tr + 1]), k
        assert bool(torch.isnan(short[k][tr + 1:]).all()), k   # rows past n are not written


@pytest.mark.parametrize("big", [45.0, 100.0])
def test_purifier_saturated_gates_and_zero_row(big):
    d = pur_data(37)
    for k in ("bgv", "bgt"):
        d[k] = np.where(np.arange(64) % 2 == 0, big, -big).astype(np.float32)
    d["Wgv"] *= 0.01
    d["Wgt"] *= 0.01
    for k in ("E", "V", "T"):
        d[k][5] = 0
    got = {k: v.cpu().numpy() for k, v in pur_run(d).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.all(got["gv"][:, 0::2] == 1) and np.all(got["gv"][:, 1::2] <= np.exp(-big + 1))
    bound = 0.0 if big >= 100 else 1e-17 * 16   # g (1 - g) <= e^-45 < 1e-19; |dP E| < 16
    assert np.abs(got["z"]).max() <= bound and np.abs(got["dV"]).max() <= bound * 64
    assert not np.any(got["z"][5]) and not np.any(got["Pv"][5]) and not np.any(got["Pt"][5])


# ----------------------------------------------------------------------------------------------- fuser
FW = ("W1", "b1", "w2", "Wi", "bi", "Wt", "bt")
F_OUT = ("side", "all", "wa", "wb", "da", "db", "dc", "z1a", "z1b", "zi", "zt", "r")


def fuse_data(n, seed=0):
    rng = np.random.default_rng(200 + n + seed)
    d = {k: (rng.standard_normal((n, 64)) * 0.7).astype(np.float32) for k in ("a", "b", "c", "dall", "dside", "dcin")}
    d.update(weights(11 + seed, FW))
    return d


def fuse_ref(d, dtype):
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=k in ("a", "b", "c")) for k, v in d.items()}
    y1a, y1b = t["a"] @ t["W1"].T + t["b1"], t["b"] @ t["W1"].T + t["b1"]
    yi, yt = t["c"] @ t["Wi"].T + t["bi"], t["c"] @ t["Wt"].T + t["bt"]
    ha, hb = torch.tanh(y1a), torch.tanh(y1b)
    q = torch.cat([ha @ t["w2"].T, hb @ t["w2"].T], dim=-1)
    for x in (y1a, y1b, yi, yt, q):
        x.retain_grad()
    w = torch.softmax(q, dim=-1)
    m = w[:, :1] * t["a"] + w[:, 1:] * t["b"]
    side = (torch.sigmoid(yi) * (t["a"] - m) + torch.sigmoid(yt) * (t["b"] - m) + m) / 3
    al = t["c"] + side
    ((al * t["dall"]).sum() + (side * t["dside"]).sum() + (t["c"] * t["dcin"]).sum()).backward()
    o = {"side": side, "all": al, "wa": w[:, 0], "wb": w[:, 1], "da": t["a"].grad, "db": t["b"].grad,
         "dc": t["c"].grad, "z1a": y1a.grad, "z1b": y1b.grad, "zi": yi.grad, "zt": yt.grad,
         "r": q.grad[:, :1] * ha + q.grad[:, 1:] * hb}
    o = {k: v.detach().numpy() for k, v in o.items()}
    # the restatement of the fixture gives the same forward
    s2, a2, wa2, _ = F.fuse_rows_ref(*[t[k].detach() for k in ("a", "b", "c")], *[t[k] for k in FW])
    np.testing.assert_allclose(s2.numpy(), o["side"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(wa2.numpy(), o["wa"], rtol=1e-5, atol=1e-6)
    return o


def fuse_run(d, n=None, ld=64, grads=(True, True)):
    """gmr_mgcn_fuse_fwd, then gmr_mgcn_fuse_bwd on the rows it saved; every output starts as NaN."""
    lib = _lib()
    n = d["a"].shape[0] if n is None else n
    a, b, c, dall, dside, dcin = (mat(d[k], ld) for k in ("a", "b", "c", "dall", "dside", "dcin"))
    W = {k: (mat(d[k], ld) if k.startswith("W") else vec(d[k])) for k in FW}
    m = d["a"].shape[0]
    o = {k: nan(m) for k in ("side", "all", "da", "db", "dc", "r")}
    sv, zf, wab = nan(m, 256), nan(m, 256), torch.full((m, 2), float("nan"), device=DEV)
    lib.call("gmr_mgcn_fuse_fwd", n, _ptr(a), _ptr(b), ld, _ptr(c), ld, _ptr(W["W1"]), _ptr(W["b1"]), _ptr(W["w2"]),
             _ptr(W["Wi"]), _ptr(W["bi"]), _ptr(W["Wt"]), _ptr(W["bt"]), ld, _ptr(o["side"]), _ptr(o["all"]), 64,
             _ptr(sv), _ptr(sv[:, 64:]), _ptr(sv[:, 128:]), _ptr(sv[:, 192:]), 256, _ptr(wab), _stream())
    lib.call("gmr_mgcn_fuse_bwd", n, _ptr(dall), ld, _ptr(dside if grads[0] else None),
             _ptr(dcin if grads[1] else None), ld, _ptr(a), _ptr(b), ld, _ptr(sv), _ptr(sv[:, 64:]), _ptr(sv[:, 128:]),
             _ptr(sv[:, 192:]), 256, _ptr(wab), _ptr(W["w2"]), _ptr(W["W1"]), _ptr(W["Wi"]), _ptr(W["Wt"]), ld,
             _ptr(o["da"]), _ptr(o["db"]), 64, _ptr(o["dc"]), 64, _ptr(zf), _ptr(zf[:, 64:]), _ptr(zf[:, 128:]),
             _ptr(zf[:, 192:]), 256, _ptr(o["r"]), 64, _stream())
    torch.cuda.synchronize()
    o.update(wa=wab[:, 0], wb=wab[:, 1], z1a=zf[:, :64], z1b=zf[:, 64:128], zi=zf[:, 128:192], zt=zf[:, 192:],
             saved=sv)
    return o


@pytest.mark.parametrize("ld", [64, 192])
@pytest.mark.parametrize("rel", ROWS)
def test_fuser_against_fp64(rel, ld):
    n = rows_of(rel)
    d = fuse_data(n)
    got = fuse_run(d, ld=ld)
    r64, r32 = fuse_ref(d, torch.float64), fuse_ref(d, torch.float32)
    for k in F_OUT:
        _bar(got[k], r64[k], r32[k], f"fuser n={n} ld={ld} {k}")


def test_fuser_null_direct_gradients_are_zero():
    d = fuse_data(TR() + 1)
    got = fuse_run(d, grads=(False, False))
    d0 = dict(d, dside=np.zeros_like(d["dside"]), dcin=np.zeros_like(d["dcin"]))
    want = fuse_run(d0)
    for k in F_OUT:
        assert torch.equal(got[k], want[k]), k


def test_fuser_rows_do_not_depend_on_the_call():
    tr = TR()
    d = fuse_data(3 * tr + 5)
    full, again, short = fuse_run(d), fuse_run(d), fuse_run(d, n=tr + 1)
    for k in F_OUT + ("saved",):
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k][:tr + 1], short[k][:tr + 1]), k
        assert bool(torch.isnan(short[k][tr + 1:]).all()), k


def test_fuser_saturation_zero_row_and_equal_logits():
    d = fuse_data(41)
    for k in ("b1", "bi", "bt"):
        d[k] = np.where(np.arange(64) % 2 == 0, 100.0, -100.0).astype(np.float32)
    for k in ("a", "b", "c"):
        d[k][5] = 0
    d["b"][7:11] = d["a"][7:11]     # q(a) == q(b)
    got = {k: v.cpu().numpy() for k, v in fuse_run(d).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    for k in ("z1a", "z1b", "zi", "zt"):     # 1 - tanh^2 and g (1 - g) are exactly 0
        assert not np.any(got[k]), k
    assert np.all(got["wa"][7:11] == 0.5) and np.all(got["wb"][7:11] == 0.5)
    assert np.all(got["wa"][5] == 0.5) and not np.any(got["side"][5]) and not np.any(got["all"][5])
    # unsaturated weights, equal logits: the attention passes no gradient to W1 (dq_a = wa wb <dm, a - b> = 0) and
    # a, b get the same share of dm
    d = fuse_data(41)
    d["b"][7:11] = d["a"][7:11]
    got = {k: v.cpu().numpy() for k, v in fuse_run(d).items()}
    r64 = fuse_ref(d, torch.float64)
    ha, hb = got["saved"][7:11, :64], got["saved"][7:11, 64:128]
    print("equal rows: tanh entries that differ", int((ha != hb).sum()), "largest", float(np.abs(ha - hb).max()),
          "wa", got["wa"][7:11], "wb", got["wb"][7:11])
    assert np.array_equal(ha, hb)   # the same row through the same product: the same bits
    assert np.all(got["wa"][7:11] == 0.5) and np.all(got["wb"][7:11] == 0.5)
    for k in ("z1a", "z1b", "r"):
        assert not np.any(got[k][7:11]), k
    np.testing.assert_allclose(got["da"][7:11], r64["da"][7:11], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["db"][7:11], r64["db"][7:11], rtol=1e-5, atol=1e-6)


def test_fuser_equal_logits_give_half_exactly():
    """w2 = 0: q(a) = q(b) = 0 for every row, so wa = wb = 0.5 exactly and the attention passes no gradient."""
    d = fuse_data(3 * TR() + 5)
    d["w2"][:] = 0
    got = {k: v.cpu().numpy() for k, v in fuse_run(d).items()}
    assert np.all(got["wa"] == 0.5) and np.all(got["wb"] == 0.5)
    for k in ("z1a", "z1b"):
        assert not np.any(got[k]), k
    r64, r32 = fuse_ref(d, torch.float64), fuse_ref(d, torch.float32)
    for k in ("side", "all", "da", "db", "dc", "zi", "zt", "r"):
        _bar(torch.as_tensor(got[k]), r64[k], r32[k], f"fuser w2=0 {k}")


# ----------------------------------------------------------------------------------------------- loss rows
def bpr_data(B):
    U, I = (300, 1100) if B > 100 else (23, 19)
    rng = np.random.default_rng(300 + B)
    d = {"U": U, "I": I, "all": (rng.standard_normal((U + I, 64)) * 0.4).astype(np.float32),
         "users": rng.integers(0, U, B).astype(np.int32), "pos": rng.integers(0, I, B).astype(np.int32),
         "neg": rng.integers(0, I, B).astype(np.int32)}
    if B > 2:
        d["users"][2], d["pos"][1], d["neg"][0] = d["users"][0], d["pos"][0], d["pos"][0]
    return d


def bpr_ref(d, inv_norm, reg_weight, div, dtype):
    al = torch.tensor(d["all"], dtype=dtype)
    U = d["U"]
    u, p, n = (al[torch.as_tensor(i.astype(np.int64)) + o].clone().requires_grad_()
               for i, o in ((d["users"], 0), (d["pos"], U), (d["neg"], U)))
    bpr = -torch.nn.functional.logsigmoid((u * p).sum(-1) - (u * n).sum(-1))
    sq = 0.5 * ((u ** 2).sum(-1) + (p ** 2).sum(-1) + (n ** 2).sum(-1))
    (bpr.sum() * inv_norm + sq.sum() * reg_weight / div).backward()
    return {"terms": torch.cat([bpr, sq]).detach().numpy(), "contrib": torch.cat([u.grad, p.grad, n.grad]).numpy()}


@pytest.mark.parametrize("ld", [64, 192])
@pytest.mark.parametrize("B", [1, 15, 17, 53, 5000])
def test_bpr_reg_rows_against_fp64(B, ld):
    lib = _lib()
    d = bpr_data(B)
    inv, rw, div = 1.0 / B, 0.37, 16.0
    terms, contrib = torch.full((2 * B,), float("nan"), device=DEV), nan(3 * B, ld=ld)
    al, us, po, ne = mat(d["all"], ld), vec(d["users"]), vec(d["pos"]), vec(d["neg"])
    lib.call("gmr_mgcn_bpr_reg_fwd_bwd", B, d["U"], _ptr(al), ld, _ptr(us), _ptr(po), _ptr(ne), inv, rw, div,
             _ptr(terms), _ptr(contrib), ld, _stream())
    torch.cuda.synchronize()
    r64, r32 = bpr_ref(d, inv, rw, div, torch.float64), bpr_ref(d, inv, rw, div, torch.float32)
    _bar(terms, r64["terms"], r32["terms"], f"bpr B={B} terms")
    _bar(contrib, r64["contrib"], r32["contrib"], f"bpr B={B} contrib")


def test_loss_reduce():
    lib = _lib()
    B = 2500
    rng = np.random.default_rng(5)
    t = rng.random((4, B)).astype(np.float32)
    loss = torch.full((5,), float("nan"), device=DEV)
    td = vec(t)
    lib.call("gmr_mgcn_loss_reduce", B, _ptr(td), 1.0 / B, 0.3, 2048.0, 0.1, _ptr(loss), _stream())
    s = t.astype(np.float64).sum(1)
    want = [s[0] / B, 0.3 * s[1] / 2048.0, s[2] / B, s[3] / B]
    want = [want[0] + want[1] + 0.1 * (want[2] + want[3])] + want
    np.testing.assert_allclose(loss.cpu().numpy(), want, rtol=3e-7)


# ----------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_raise():
    lib = _lib()
    d = pur_data(8)
    x = mat(d["E"])
    w, bias, o = mat(d["Wgv"]), vec(d["bgv"]), nan(8, 256)
    good = [8, _ptr(x), 64, _ptr(x), 64, _ptr(x), 64, _ptr(w), _ptr(bias), _ptr(w), _ptr(bias), 64, _ptr(o),
            _ptr(o[:, 64:]), 256, _ptr(o[:, 128:]), _ptr(o[:, 192:]), 256, _stream()]
    lib.call("gmr_mgcn_purify_fwd", *good)
    for i, v in ((0, 0), (1, None), (2, 66), (2, 60), (8, None), (12, None), (14, 62), (1, _ptr(x.view(-1)[1:]))):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError):
            lib.call("gmr_mgcn_purify_fwd", *bad)
    sv, zf, wab = nan(8, 256), nan(8, 256), torch.zeros((8, 2), device=DEV)
    w2 = vec(np.zeros((1, 64), np.float32))
    good = [8, _ptr(x), _ptr(x), 64, _ptr(x), 64, _ptr(w), _ptr(bias), _ptr(w2), _ptr(w), _ptr(bias), _ptr(w),
            _ptr(bias), 64, _ptr(o), _ptr(o[:, 64:]), 256, _ptr(sv), _ptr(sv[:, 64:]), _ptr(sv[:, 128:]),
            _ptr(sv[:, 192:]), 256, _ptr(wab), _stream()]
    lib.call("gmr_mgcn_fuse_fwd", *good)
    for i, v in ((0, 0), (1, None), (3, 66), (8, None), (13, 32), (16, 130), (22, None)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError):
            lib.call("gmr_mgcn_fuse_fwd", *bad)
    good = [8, _ptr(x), 64, None, None, 64, _ptr(x), _ptr(x), 64, _ptr(sv), _ptr(sv[:, 64:]), _ptr(sv[:, 128:]),
            _ptr(sv[:, 192:]), 256, _ptr(wab), _ptr(w2), _ptr(w), _ptr(w), _ptr(w), 64, _ptr(o), _ptr(o[:, 64:]), 256,
            _ptr(o[:, 128:]), 256, _ptr(zf), _ptr(zf[:, 64:]), _ptr(zf[:, 128:]), _ptr(zf[:, 192:]), 256,
            _ptr(o[:, 192:]), 256, _stream()]
    wab.fill_(0.5)
    sv.fill_(0.25)
    lib.call("gmr_mgcn_fuse_bwd", *good)
    for i, v in ((0, 0), (1, None), (2, 65), (14, None), (20, None), (29, 60), (31, 2)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError):
            lib.call("gmr_mgcn_fuse_bwd", *bad)
    good = [8, _ptr(x), _ptr(x), 64, _ptr(x), _ptr(x), 64, _ptr(x), 64, _ptr(w), _ptr(w), 64, _ptr(o), 256, 0,
            _ptr(sv), 256, _ptr(o[:, 64:]), _ptr(o[:, 128:]), 256, _stream()]
    lib.call("gmr_mgcn_purify_bwd", *good)
    for i, v in ((0, 0), (1, None), (3, 63), (12, None), (16, 64), (19, 66)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError):
            lib.call("gmr_mgcn_purify_bwd", *bad)
    idx = vec(np.zeros(8, np.int32))
    terms, cb = torch.zeros(16, device=DEV), nan(24)
    good = [8, 4, _ptr(x), 64, _ptr(idx), _ptr(idx), _ptr(idx), 0.125, 0.1, 16.0, _ptr(terms), _ptr(cb), 64, _stream()]
    lib.call("gmr_mgcn_bpr_reg_fwd_bwd", *good)
    for i, v in ((0, 0), (2, None), (3, 66), (4, None), (9, 0.0), (10, None), (12, 60)):
        bad = list(good)
        bad[i] = v
        with pytest.raises(RuntimeError):
            lib.call("gmr_mgcn_bpr_reg_fwd_bwd", *bad)
    torch.cuda.synchronize()
