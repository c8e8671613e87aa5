"""tests/diffmm_kernels_ref.py against itself, on the CPU: a wrong reference must not be able to pass a wrong kernel.

  * the hand-written closed forms (what the kernels implement) against torch.autograd in double, at 1e-12 of the
    magnitude of the terms, zero and clamped rows included
  * the strict fp32 slot-order scatter against fp64 index_add under (n + 2) 2^-24 sum|terms|, n = the longest run + 1
  * the plan builder against Python's sorted()
  * the fp32 restatements (kernel order) against their fp64 forms, loosely: they are yardsticks, not references
"""
import numpy as np

import diffmm_kernels_ref as R

U24 = 2.0 ** -24


def _rows(rng, n, cols=64):
    """n rows with the edge norms: exact zeros (one last), one of norm ~1e-20, one of ~1e18."""
    x = rng.standard_normal((n, cols)).astype(np.float32)
    if n >= 15:
        x[n - 1] = 0
        x[n // 2] = 0
        x[1] *= np.float32(1e-21)
        x[2] *= np.float32(1e17)
    return x


def _close(a, b, scale, what):
    assert np.isfinite(a).all() and np.isfinite(b).all(), what
    assert (np.abs(a - b) <= 1e-12 * scale + 1e-300).all(), (what, float(np.abs(a - b).max()))


def test_normalize_bwd_closed_form_is_autograd():
    rng = np.random.default_rng(0)
    for n in (1, 17, 333):
        for slope in (1.0, 0.2):
            z = _rows(rng, n)
            g = rng.standard_normal((n, 64))
            y, nv = R.normalize_rows(R.leaky(z, slope) if slope != 1.0 else z)
            got = R.normalize_bwd_closed(y, nv, g, slope)
            scale = (np.abs(g) + np.abs(y) * (np.abs(y * g)).sum(1, keepdims=True)) / nv[:, None]
            _close(got, R.normalize_bwd(z, g, slope), scale, (n, slope))
            if n >= 15:  # a clamped row is g / 1e-12 (times the slope everywhere: leaky_relu'(0) = slope)
                np.testing.assert_array_equal(got[n - 1], g[n - 1] / 1e-12 * slope)


def test_final_bwd_and_mw_grad_closed_forms_are_autograd():
    rng = np.random.default_rng(1)
    for n in (1, 17, 333):
        for mw in ((0.0, 0.0), (3.0, -2.0), (80.0, -80.0)):
            M, E = _rows(rng, n), rng.standard_normal((n, 128))
            dEmb, T1 = rng.standard_normal((n, 64)), rng.standard_normal((n, 64))
            ris = 0.7
            a = R.final_bwd(dEmb, T1, M, ris, E, mw)
            c = R.final_bwd_closed(dEmb, T1, M, ris, E, mw)
            y, nv = R.normalize_rows(M)
            s_dm = np.abs(dEmb) + np.abs(T1) + ris * (np.abs(dEmb) + np.abs(y) * np.abs(y * dEmb).sum(1, keepdims=True)) \
                / nv[:, None]
            _close(c[0], a[0], s_dm, "dM")
            _close(c[1], a[1], np.concatenate([s_dm, s_dm], 1), "dE")
            s_dw = np.array([(np.abs(E[:, :64]) * s_dm).sum(), (np.abs(E[:, 64:]) * s_dm).sum()])
            _close(c[2], a[2], s_dw, "dw")
            _close(c[3], a[3], s_dw.sum(), "dmw")
            _close(R.mw_grad_closed(a[2], mw), R.mw_grad(a[2], mw), np.abs(a[2]).sum(), "mw_grad")


def test_assemble_is_the_sum_of_its_paths():
    """dE0 and dNF as d/d(E0), d/d(NF) of a scalar that pairs every source with the table it is the gradient of."""
    import torch
    rng = np.random.default_rng(2)
    n, U = 23, 9
    I = n - U
    T2, T3, Ri, Rt = (rng.standard_normal((n, 128)) for _ in range(4))
    E0 = rng.standard_normal((n, 64))
    reg2 = 0.03
    for flag in (False, True):
        dE0, dNF = R.assemble(T2, T3, Ri, Rt, E0, reg2, U, flag)
        e = torch.tensor(E0, requires_grad=True)
        nf = torch.zeros((I, 128), dtype=torch.float64, requires_grad=True)
        t = lambda v: torch.tensor(v)  # noqa: E731
        T3u = T2 if flag else T3
        f = 0.5 * reg2 * (e * e).sum()
        f = f + (e[:U] * t(T3u[:U, :64] + T3u[:U, 64:] + Ri[:U, :64] + Ri[:U, 64:] + Rt[:U, :64] + Rt[:U, 64:])).sum()
        f = f + (e[U:] * t(T2[U:, :64] + T2[U:, 64:] + Ri[U:, :64] + Rt[U:, :64])).sum()
        f = f + (nf[:, :64] * t(T3[U:, :64] + Ri[U:, 64:])).sum() + (nf[:, 64:] * t(T3[U:, 64:] + Rt[U:, 64:])).sum()
        f.backward()
        _close(dE0, e.grad.numpy(), 8.0 + np.abs(dE0), "dE0")
        _close(dNF, nf.grad.numpy(), 2.0 + np.abs(dNF), "dNF")
    Z = _rows(rng, I, 128)
    got = R.assemble_projection(dNF, Z, 0.2)
    for h in (slice(0, 64), slice(64, 128)):
        y, nv = R.normalize_rows(R.leaky(Z[:, h], 0.2))
        want = R.normalize_bwd_closed(y, nv, dNF[:, h], 0.2)
        _close(got[:, h], want, (np.abs(dNF[:, h]) + np.abs(y) * np.abs(y * dNF[:, h]).sum(1, keepdims=True))
               / nv[:, None], "projection")


def _runs_keys(rng, table):
    """One key 40 times, runs of exactly 8, 9, 16 and 17, key 0 and the last table row, singles; shuffled."""
    keys = [5] * 40 + [0] * 8 + [table - 1] * 9 + [7] * 16 + [11] * 17 + [3, 4, 6, 8, 9, 10]
    return rng.permutation(np.array(keys, np.int32))


def test_slot_order_scatter_against_index_add():
    rng = np.random.default_rng(3)
    table = 20
    keys = _runs_keys(rng, table)
    for pow2 in (None, 128):
        plan = R.plan_of(keys, pow2)
        for cols in (4, 64):
            x = rng.standard_normal((len(keys), cols)).astype(np.float32)
            dst = rng.standard_normal((table, cols)).astype(np.float32)
            got = R.scatter_sorted_f32(plan, x, dst)
            want, terms, longest = R.scatter_index_add(plan, x, dst)
            assert longest == 40
            # a run of r slots is r additions (the first onto 0 is exact) and one more onto dst: n = longest + 1
            assert (np.abs(got - want) <= (longest + 1 + 2) * U24 * terms).all()
            untouched = np.setdiff1d(np.arange(table), keys)
            assert len(untouched) and (got[untouched].view(np.uint32) == dst[untouched].view(np.uint32)).all()


def test_scatter_restatement_adds_in_slot_order():
    """1e8 + 1 - 1e8 in fp32: slot order gives 0, any order that adds the two large terms first gives 1."""
    x = np.array([[1e8], [1.0], [-1e8]], np.float32)
    plan = R.plan_of([2, 2, 2])
    assert R.scatter_sorted_f32(plan, x, np.zeros((3, 1), np.float32))[2, 0] == 0.0
    assert R.scatter_sorted_f32(plan, x[[0, 2, 1]], np.zeros((3, 1), np.float32))[2, 0] == 1.0


def test_plan_builder_against_sorted():
    rng = np.random.default_rng(4)
    offs = [0, 37, 37, 53]
    nk, stride, pow2, out_stride = 3, 53, 128, 136
    keys = rng.integers(0, 9, (nk, stride)).astype(np.int32)
    key_add = [0, 100, 100]
    got = R.sort_batch_keys(keys, offs, key_add, nk, pow2, out_stride, fill=np.uint64(7))
    for b in range(3):
        beg, end = offs[b], offs[b + 1]
        ln = end - beg
        pairs = sorted((int(keys[k, beg + j]) + key_add[k], k * ln + j) for k in range(nk) for j in range(ln))
        want = [(key << 32) | slot for key, slot in pairs] + [2 ** 64 - 1] * (pow2 - len(pairs)) + [7] * 8
        assert [int(v) for v in got[b]] == want
    assert (got[1, :pow2] == R.PAD).all()
    keys1 = np.array([[4, 2, 2, 0, 4]], np.int32)
    assert [int(v) for v in R.plan_of(keys1[0], 8)] == [3, (2 << 32) | 1, (2 << 32) | 2, 4 << 32, (4 << 32) | 4] \
        + [2 ** 64 - 1] * 3


def test_fp32_restatements_follow_their_fp64_forms():
    rng = np.random.default_rng(5)
    n = 40
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    G, H, Qi, Qt, K2 = f(n, 128), f(n, 128), f(n, 128), f(n, 128), f(n, 128)
    mw = (0.3, -0.2)
    for a, b in zip(R.combine_fwd(G, H, Qi, Qt, mw, 0.5, np.float32), R.combine_fwd(G, H, Qi, Qt, mw, 0.5)):
        assert a.dtype == np.float32 and np.abs(a - b).max() < 1e-5
    M, L = _rows(rng, n), f(n, 64)
    for a, b in zip(R.final_fwd(M, L, 0.7, np.float32), R.final_fwd(M, L, 0.7)):
        assert a.dtype == np.float32 and (np.abs(a - b) <= 1e-6 * np.abs(b) + 1e-6).all()
    for a, b in zip(R.cl_fwd(Qi, Qt, K2, np.float32), R.cl_fwd(Qi, Qt, K2)):
        assert a.dtype == np.float32 and np.abs(a - b).max() < 1e-5
    Emb = f(30, 64)
    idx = lambda hi: rng.integers(0, hi, 25).astype(np.int32)  # noqa: E731
    users, pos, neg = idx(10), idx(20), idx(20)
    for a, b in zip(R.bpr(Emb, 10, users, pos, neg, 0.04, np.float32), R.bpr(Emb, 10, users, pos, neg, 0.04)):
        assert a.dtype == np.float32 and (np.abs(a - b) <= 1e-5 * (1 + np.abs(b))).all()
    Lg = f(7, 300)
    for a, b in zip(R.row_softmax(Lg, 0.1, np.float32), R.row_softmax(Lg, 0.1)):
        assert a.dtype == np.float32 and np.abs(a - b).max() < 1e-5
    x = f(3001)
    assert abs(float(R.block_sum(x, np.float32)) - x.astype(np.float64).sum()) < 1e-2
    assert abs(R.block_sum(x) - x.astype(np.float64).sum()) < 1e-9
    assert abs(R.sqnorm_parts(x, 2).sum() - (x.astype(np.float64) ** 2).sum()) < 1e-8
    assert [R.sqnorm_nparts(v) for v in (0, 1, 2048, 2049, 2 * 1024 * 2048 + 77)] == [1, 1, 1, 2, 1024]
