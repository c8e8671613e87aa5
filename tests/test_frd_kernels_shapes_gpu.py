"""The FREEDOM kernels (csrc/freedom.hip) and gmr.freedom past the tiny golden shape:

  kNN union         n = 1024, 1025, 2500 rows: the carry loop of frd_rowptr_kernel (more than 1,024 rows)
  fused loss        T = NULL, V = NULL, both NULL: the single-modality model of the ABI
  knn_topk          the row-chunked similarity GEMM (KNN_SIM_FLOATS patched so that 300 rows split into chunks of 7)
  FREEDOM.rec_step  U = 300, I = 1,100, 6,000 train edges, feature widths 37 and 50 (rows padded to 16 bytes),
                    knn_k = 10, B = 700 (3B = 2,100 pads to 4,096 in the sort plan), against the fp64 restatement of
                    tests/freedom_fixture.py on the model's own kNN lists and keep bytes

Bars: those of test_freedom_gpu.py (loss rtol 1e-5; gradients rtol 1e-4 + 1e-6 x the parameter's largest gradient;
the analytically zero projection biases 1e-4 x the weight gradient's max).

Seen on the MI355X at the mid shape, largest error / largest gradient:
  case A  loss 0.69447827 (fp64 0.69447829); user 1.8e-11 / 1.5e-4, item 1.7e-11 / 1.4e-4, image table 4.4e-14 / 1.8e-7,
          image W 1.2e-12 / 2.7e-6, image b 3.2e-13 (bar 2.7e-10), text table 4.8e-14 / 1.5e-7, text W 1.4e-12 / 4.2e-6,
          text b 2.8e-13 (bar 4.2e-10)
  case B  loss 0.69450951 (fp64 0.69450950); user 5.3e-12 / 4.3e-5, item 5.9e-12 / 3.8e-5, image table 2.3e-14 / 9.0e-8,
          image W 6.1e-13 / 1.5e-6, image b 2.3e-13 (bar 1.5e-10), text table 2.7e-14 / 8.0e-8, text W 7.6e-13 / 2.0e-6,
          text b 1.6e-13 (bar 2.0e-10)
"""
import numpy as np
import pytest
import torch

from freedom_fixture import CASES, PARAMS, build_freedom_mid, check_grads, freedom_step_ref, knn_lists
from test_freedom_kernels_gpu import _loss_case, _loss_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.as_tensor(a).to(DEV)


# ----------------------------------------------------------------------------- kNN union
@pytest.fixture(scope="module", params=[1024, 1025, 2500])
def union_lists(request):
    n = request.param
    rng = np.random.default_rng(n)
    return n, {(kind, k): knn_lists(kind, n, k, rng) for kind in ("identical", "disjoint", "overlap") for k in (1, 10)}


def _union_ref(n, k, lists, weights):
    import scipy.sparse as sp
    r = np.power(np.float32(k) + np.float32(1e-7), np.float32(-0.5), dtype=np.float32)
    v = np.float64(r * r)
    rows = np.repeat(np.arange(n), k)
    want = sum(sp.coo_matrix((np.full(n * k, w * v), (rows, l.reshape(-1))), shape=(n, n)).tocsr()
               for l, w in zip(lists, weights)).tocsr()
    want.sort_indices()
    return want


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("kind", ["identical", "disjoint", "overlap"])
def test_knn_union_many_rows(union_lists, kind, k):
    from gmr.freedom import knn_union_csr
    n, lists = union_lists
    a, b = lists[(kind, k)]
    wa, wb = 0.1, 1.0 - 0.1
    da, db = dev(a.astype(np.int32)), dev(b.astype(np.int32))
    for got, want in ((knn_union_csr(da, wa, db, wb), _union_ref(n, k, (a, b), (wa, wb))),
                      (knn_union_csr(da, 1.0), _union_ref(n, k, (a,), (1.0,)))):
        assert np.array_equal(got.rowptr.cpu().numpy(), want.indptr)
        assert got.nnz == want.nnz and np.array_equal(got.col.cpu().numpy(), want.indices)
        np.testing.assert_allclose(got.val.cpu().numpy(), want.data, rtol=1e-6)


# ----------------------------------------------------------------------------- fused loss, absent modalities
def _run_loss(U, G, T, V, users, pos, neg, reg, inv_norm):
    from gmr import _lib
    from gmr.kernels import ptr, stream
    B = len(users)
    tab = torch.zeros((G.shape[0], 192), device=DEV)
    tab[:, :64] = dev(G)
    tt = tv = None
    if T is not None:
        tab[U:, 64:128] = dev(T)
        tt = tab[U:, 64:128]
    if V is not None:
        tab[U:, 128:] = dev(V)
        tv = tab[U:, 128:]
    parts = torch.full((3 * B,), float("nan"), dtype=torch.float64, device=DEV)
    loss = torch.full((4,), float("nan"), device=DEV)
    contrib = torch.full((3 * B, 192), float("nan"), device=DEV)
    du, dp, dn = dev(users), dev(pos), dev(neg)
    _lib.call("gmr_frd_loss_fwd_bwd", B, U, ptr(tab), 192, ptr(tt), 192 if tt is not None else 0, ptr(tv),
              192 if tv is not None else 0, ptr(du), ptr(dp), ptr(dn), reg, inv_norm, ptr(parts), ptr(loss),
              ptr(contrib), 192, stream())
    return loss.cpu().numpy(), contrib.cpu().numpy()


@pytest.mark.parametrize("absent", ["T", "V", "TV"])
@pytest.mark.parametrize("B", [1, 17])
def test_loss_absent_modality(B, absent):
    U, I, G, T, V, users, pos, neg = _loss_case(B)
    reg, inv_norm = 0.05, 1.0 / B
    zero = np.zeros_like(T)
    # _loss_ref with the absent table zero, then that term removed: its loss, its column blocks
    want_loss, want = _loss_ref(U, G, zero if "T" in absent else T, zero if "V" in absent else V, users, pos, neg,
                                reg, inv_norm)
    gone = [blk for blk, name in ((1, "T"), (2, "V")) if name in absent]
    for blk in gone:
        want_loss[1 + blk] = 0.0
        want[:, 64 * blk:64 * blk + 64] = 0.0
    want_loss[0] = want_loss[1] + reg * (want_loss[2] + want_loss[3])
    loss, contrib = _run_loss(U, G, None if "T" in absent else T, None if "V" in absent else V, users, pos, neg, reg,
                              inv_norm)
    np.testing.assert_allclose(loss, want_loss, rtol=1e-5)
    np.testing.assert_allclose(contrib, want, rtol=1e-4, atol=1e-6 * np.abs(want).max())
    assert np.all(contrib[:B, 64:] == 0)
    for blk in gone:
        assert loss[1 + blk] == 0.0
        assert np.all(contrib[:, 64 * blk:64 * blk + 64] == 0), blk
    loss2, contrib2 = _run_loss(U, G, None if "T" in absent else T, None if "V" in absent else V, users, pos, neg,
                                reg, inv_norm)
    assert np.array_equal(loss, loss2) and np.array_equal(contrib, contrib2)


# ----------------------------------------------------------------------------- knn_topk in row chunks
def _separated_features(n, d, k, gap):
    """Features (the first seed from 0) whose fp64 cosine similarities at ranks k and k + 1 differ by more than
    gap in every row, and the fp64 top-k sets."""
    for seed in range(64):
        f = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
        x = f.astype(np.float64)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        sim = x @ x.T
        s = -np.sort(-sim, axis=1)
        if (s[:, k - 1] - s[:, k]).min() > gap:
            return f, sim
    raise AssertionError("no seed with the kNN gap")


def test_knn_topk_chunked(monkeypatch):
    import gmr.freedom as F
    n, d, k = 300, 37, 10
    feat, sim = _separated_features(n, d, k, 1e-5)
    s = -np.sort(-sim, axis=1)
    assert ((s[:, k - 1] - s[:, k]) > 1e-5).all()  # the precondition, on the fp64 reference alone, every row
    whole = F.knn_topk(dev(feat), k).cpu().numpy()
    calls = []
    gemm = F.K.gemm
    monkeypatch.setattr(F.K, "gemm", lambda a, *r, **kw: (calls.append(a.shape[0]), gemm(a, *r, **kw))[1])
    monkeypatch.setattr(F, "KNN_SIM_FLOATS", 7 * 300 + 5)
    chunked = F.knn_topk(dev(feat), k).cpu().numpy()
    assert calls == [7] * 42 + [6]
    assert np.array_equal(chunked, whole)
    want = np.sort(np.argsort(-sim, axis=1, kind="stable")[:, :k], axis=1)
    assert np.array_equal(np.sort(chunked, axis=1), want)
    assert (chunked == np.arange(n)[:, None]).any(axis=1).all()  # the row itself is among its neighbours


# ----------------------------------------------------------------------------- the step at a mid shape
@pytest.mark.parametrize("case", ["A", "B"])
def test_rec_step_mid_shape(case):
    U, I, B = 300, 1100, 700
    m, rows, cols = build_freedom_mid(case, U=U, I=I, batch=B)
    assert rows.size == 6000 and m.N == U + I
    assert m.slab.view("image_embedding").stride(0) == 40 and m.slab.view("text_embedding").stride(0) == 52
    if case == "A":
        keep = m.prune_edges().cpu().numpy().astype(bool)
        assert keep.sum() == int(6000 * (1.0 - 0.8))
    else:
        m.pre_epoch_processing()
        assert m.masked_adj is m.norm_adj
        keep = np.ones(rows.size, bool)
    rng = np.random.default_rng(8)
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    neg[0] = pos[0]
    users[1:4] = users[0]
    assert 1 << (3 * B - 1).bit_length() == 4096
    loss = m.rec_step(*(dev(x.astype(np.int32)) for x in (users, pos, neg))).item()
    terms = m.loss_terms().cpu().numpy()
    P = {k: p.detach().cpu().numpy() for k, p in zip(PARAMS, m._params())}
    c = CASES[case]
    r = freedom_step_ref(P, U, I, rows[keep], cols[keep], m.knn_ind["image"].cpu().numpy(),
                         m.knn_ind["text"].cpu().numpy(), users, pos, neg, c["n_mm_layers"], c["n_ui_layers"],
                         mm_image_weight=m.mm_image_weight, reg_weight=m.reg_weight, dtype=torch.float64)
    print(f"mid shape {case}: loss {loss:.8f} (fp64 {r['loss']:.8f}), terms {terms[1:]} (fp64 {r['terms']})")
    np.testing.assert_allclose(loss, r["loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[0], r["loss"], rtol=1e-5)
    np.testing.assert_allclose(terms[1:], r["terms"], rtol=1e-5)
    check_grads([v.cpu().numpy() for v in m.grad_views()], r["grads"], show=f"mid shape {case}")
