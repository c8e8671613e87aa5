"""The FREEDOM kernels (csrc/freedom.hip) against numpy / scipy fp64 built here: the fused three-term BPR
loss with its contribution rows, the weighted draw without replacement (keys + radix select), and the
weighted kNN union."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a):
    return torch.as_tensor(a).to(DEV)


# ----------------------------------------------------------------------------- fused loss
def _loss_case(B, seed=5):
    rng = np.random.default_rng(seed)
    U, I = 500, 300
    G = (0.3 * rng.standard_normal((U + I, 64))).astype(np.float32)
    T = (0.3 * rng.standard_normal((I, 64))).astype(np.float32)
    V = (0.3 * rng.standard_normal((I, 64))).astype(np.float32)
    users = rng.integers(0, U, B).astype(np.int32)
    pos = rng.integers(0, I, B).astype(np.int32)
    neg = rng.integers(0, I, B).astype(np.int32)
    # logsigmoid saturation: user 7 = e_0, item 11 = 40 e_0, item 12 = 0 in all three tables
    G[7] = 0
    G[7, 0] = 1
    for tab, off in ((G, U), (T, 0), (V, 0)):
        tab[off + 11] = 0
        tab[off + 11, 0] = 40
        tab[off + 12] = 0
    users[0], pos[0], neg[0] = 7, 11, 12        # score difference +40
    if B > 1:
        users[1], pos[1], neg[1] = 7, 12, 11    # -40, and user 7 twice
    if B > 2:
        neg[2] = pos[2]                         # pos == neg
        users[3] = users[2]                     # a duplicate user
    return U, I, G, T, V, users, pos, neg


def _loss_ref(U, G, T, V, users, pos, neg, reg, inv_norm):
    G, T, V = (x.astype(np.float64) for x in (G, T, V))
    u = G[users]
    B = len(users)
    contrib = np.zeros((3 * B, 192))
    terms = []
    for blk, (tab, off, sc) in enumerate(((G, U, 1.0), (T, 0, reg), (V, 0, reg))):
        p, n = tab[off + pos], tab[off + neg]
        x = (u * p).sum(1) - (u * n).sum(1)
        terms.append(np.logaddexp(0.0, -x).sum() * inv_norm)       # -logsigmoid(x) = log(1 + exp(-x))
        c = -sc * inv_norm / (1.0 + np.exp(x))
        contrib[:B, :64] += c[:, None] * (p - n)
        contrib[B:2 * B, 64 * blk:64 * blk + 64] = c[:, None] * u
        contrib[2 * B:, 64 * blk:64 * blk + 64] = -c[:, None] * u
    return np.array([terms[0] + reg * (terms[1] + terms[2])] + terms), contrib


def _run_loss(U, G, T, V, users, pos, neg, reg, inv_norm):
    from gmr import _lib
    from gmr.kernels import ptr, stream
    B = len(users)
    tab = torch.zeros((G.shape[0], 192), device=DEV)       # the model's [G | T | V] work table
    tab[:, :64] = dev(G)
    tab[U:, 64:128] = dev(T)
    tab[U:, 128:] = dev(V)
    parts = torch.empty(3 * B, dtype=torch.float64, device=DEV)
    loss = torch.empty(4, device=DEV)
    contrib = torch.full((3 * B, 192), float("nan"), device=DEV)
    tt, tv = tab[U:, 64:128], tab[U:, 128:]
    du, dp, dn = dev(users), dev(pos), dev(neg)   # named: the pointers must outlive the launch
    _lib.call("gmr_frd_loss_fwd_bwd", B, U, ptr(tab), 192, ptr(tt), 192, ptr(tv), 192, ptr(du), ptr(dp), ptr(dn), reg,
              inv_norm, ptr(parts), ptr(loss), ptr(contrib), 192, stream())
    return loss.cpu().numpy(), contrib.cpu().numpy()


@pytest.mark.parametrize("B", [1, 16, 2050])
def test_frd_loss_kernel(B):
    U, I, G, T, V, users, pos, neg = _loss_case(B)
    reg, inv_norm = 0.05, 1.0 / B
    loss, contrib = _run_loss(U, G, T, V, users, pos, neg, reg, inv_norm)
    want_loss, want = _loss_ref(U, G, T, V, users, pos, neg, reg, inv_norm)
    np.testing.assert_allclose(loss, want_loss, rtol=1e-5)
    np.testing.assert_allclose(contrib, want, rtol=1e-4, atol=1e-6 * np.abs(want).max())
    assert np.all(contrib[:B, 64:] == 0)
    loss2, contrib2 = _run_loss(U, G, T, V, users, pos, neg, reg, inv_norm)
    assert np.array_equal(loss, loss2) and np.array_equal(contrib, contrib2)


# ----------------------------------------------------------------------------- weighted draw
def _select(w, m, u=None, seed=0, step=0):
    from gmr.freedom import prune_select
    keep = prune_select(dev(w), m, u=dev(u) if u is not None else None, seed=seed, step=step)
    return keep.cpu().numpy()


@pytest.mark.parametrize("E", [1, 255, 5003])
def test_frd_select_injected_uniforms(E):
    rng = np.random.default_rng(100 + E)
    w = rng.uniform(0.05, 1.0, E).astype(np.float32)
    u = rng.uniform(0.01, 0.99, E).astype(np.float32)
    key = w.astype(np.float64) / -np.log(u.astype(np.float64))
    order = np.argsort(-key, kind="stable")
    for m in sorted({0, 1, E // 5, E}):
        if 0 < m < E:  # precondition: the fp64 keys at ranks m and m + 1 are well apart
            a, b = key[order[m - 1]], key[order[m]]
            assert (a - b) > 1e-6 * a, (E, m)
        keep = _select(w, m, u)
        assert keep.sum() == m and set(np.unique(keep)) <= {0, 1}
        assert np.array_equal(np.flatnonzero(keep), np.sort(order[:m])), (E, m)


@pytest.mark.parametrize("E", [1, 255, 5003])
def test_frd_select_ties_keep_lowest_indices(E):
    w = np.full(E, 0.25, np.float32)
    u = np.full(E, 0.5, np.float32)
    for m in sorted({0, 1, E // 5, E}):
        keep = _select(w, m, u)
        assert np.array_equal(np.flatnonzero(keep), np.arange(m)), (E, m)


def test_frd_select_philox():
    E, m = 4096, 1024
    w = np.where(np.arange(E) % 2 == 0, 1.0, 4.0).astype(np.float32)
    a = _select(w, m, seed=9, step=0)
    assert a.sum() == m
    assert np.array_equal(a, _select(w, m, seed=9, step=0))
    b = _select(w, m, seed=9, step=1)
    assert b.sum() == m and not np.array_equal(a, b)
    assert a[w == 4.0].mean() > a[w == 1.0].mean()


def test_frd_select_bad_m():
    w = np.ones(16, np.float32)
    for m in (17, -1):
        with pytest.raises(RuntimeError, match="gmr_frd_prune_select"):
            _select(w, m)


# ----------------------------------------------------------------------------- kNN union
from freedom_fixture import knn_lists as _lists  # noqa: E402  (shared with test_frd_kernels_shapes_gpu.py)


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("kind", ["identical", "disjoint", "overlap"])
def test_frd_knn_union(kind, k):
    import scipy.sparse as sp
    from gmr.freedom import knn_union_csr
    n, wa, wb = 70, 0.1, 1.0 - 0.1
    rng = np.random.default_rng(3)
    a, b = _lists(kind, n, k, rng)
    r = np.power(np.float32(k) + np.float32(1e-7), np.float32(-0.5), dtype=np.float32)
    v = np.float64(r * r)
    rows = np.repeat(np.arange(n), k)
    A = sp.coo_matrix((np.full(n * k, wa * v), (rows, a.reshape(-1))), shape=(n, n))
    Bm = sp.coo_matrix((np.full(n * k, wb * v), (rows, b.reshape(-1))), shape=(n, n))
    want = (A + Bm).tocsr()
    want.sort_indices()
    got = knn_union_csr(dev(a.astype(np.int32)), wa, dev(b.astype(np.int32)), wb)
    assert np.array_equal(got.rowptr.cpu().numpy(), want.indptr)
    assert np.array_equal(got.col.cpu().numpy(), want.indices)
    np.testing.assert_allclose(got.val.cpu().numpy(), want.data, rtol=1e-6)
    one = knn_union_csr(dev(a.astype(np.int32)), 1.0)       # one list, weight 1: the single-modality graph
    w1 = sp.coo_matrix((np.full(n * k, v), (rows, a.reshape(-1))), shape=(n, n)).tocsr()
    w1.sort_indices()
    assert np.array_equal(one.col.cpu().numpy(), w1.indices)
    np.testing.assert_allclose(one.val.cpu().numpy(), w1.data, rtol=1e-6)


# ----------------------------------------------------------------------------- layer mean
def test_frd_mean_fwd():
    from gmr import _lib
    from gmr.kernels import ptr, stream
    rng = np.random.default_rng(1)
    N, U = 77, 30
    tabs = [rng.standard_normal((N, 64)).astype(np.float32) for _ in range(3)]
    h = rng.standard_normal((N - U, 64)).astype(np.float32)
    want = (tabs[0].astype(np.float64) + tabs[1] + tabs[2]) / 3
    want[U:] += h
    dt = [dev(t) for t in tabs]
    out = torch.zeros((N, 192), device=DEV)
    dh = dev(h)
    _lib.call("gmr_frd_mean_fwd", N, U, 3, (ctypes.c_void_p * 3)(*[t.data_ptr() for t in dt]),
              (ctypes.c_int64 * 3)(64, 64, 64), ptr(dh), 64, ptr(out), 192, stream())
    np.testing.assert_allclose(out[:, :64].cpu().numpy(), want, rtol=1e-6, atol=1e-6)
    assert float(out[:, 64:].abs().max()) == 0.0


def test_freedom_rejects_other_embedding_sizes(golden):
    from freedom_fixture import build_freedom
    with pytest.raises(NotImplementedError):
        build_freedom(golden("freedom_tiny"), embedding_size=32)
