"""gmr_frd_prune_select (csrc/freedom.hip) called directly on crafted keys at the sizes where it changes path, against
an exact reference: keep the first m of np.lexsort((arange(E), -bits)) with bits the uint32 view of the keys
(largest key first, ties to the lowest edge id).  No tolerance: array_equal.

  E = 262,144    nb = 1024 chunks of 256 (frd_scan1024_kernel at its full width)
  E = 262,145    chunk = 512: two rounds of frd_keep_kernel, `base` carried between them
  E = 600,000    chunk = 768: three rounds
  E = 2,100,000  the grid-stride loop of frd_hist_kernel (more than 1024 x 2048 keys)

Key sets: random; about 1,000 distinct values with a heavy tie at the threshold, m cutting the ties in the middle of
a chunk and of a wave; one top-8 / 16 / 24-bit prefix shared by half the keys with the threshold inside that group
(the prefix test of radix passes 1..3); 60 % zeros with m above the number of positive keys (threshold 0, bin 0
picked in every pass).

Also gmr_frd_prune_keys: the u = 1 clamp, w = 0, a tiny u, and its Philox path against tests/philox_ref.py."""
import numpy as np
import pytest
import torch

import philox_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [262144, 262145, 600000, 2100000]
KINDS = ["random", "ties", "prefix8", "prefix16", "prefix24", "zeros"]


def _chunk(E):
    """The tie-rank chunk of gmr_frd_prune_select: ceil(E / 1024) rounded up to 256."""
    return (-(-E // 1024) + 255) // 256 * 256


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _keys(kind, E, rng):
    """(keys as float32, the crafted m)."""
    if kind == "random":
        return rng.uniform(0.01, 100.0, E).astype(np.float32), E // 2 + 1
    if kind == "ties":
        vals = np.unique(rng.uniform(0.1, 10.0, 1000).astype(np.float32))
        heavy = vals.size // 2  # 30 % of the keys take this value, the threshold
        pick = rng.integers(0, vals.size, E)
        pick[rng.random(E) < 0.3] = heavy
        keys = vals[pick]
        ties = np.flatnonzero(keys == vals[heavy])
        chunk = _chunk(E)
        for r in range(ties.size // 2, ties.size - 1):  # the last kept tie: mid-wave, mid-chunk, a tie after it
            p = ties[r - 1]
            if 16 <= p % 64 < 48 and ties[r] // 64 == p // 64 and 64 <= p % chunk < chunk - 64 \
                    and (chunk == 256 or 256 <= p % chunk):
                break
        else:
            raise AssertionError("no cut of the ties in the middle of a wave")
        return keys, int((keys > vals[heavy]).sum()) + r
    if kind.startswith("prefix"):
        nbits = int(kind[6:])
        base = np.uint32(0x3F812300) & np.uint32((0xFFFFFFFF << (32 - nbits)) & 0xFFFFFFFF)
        low = rng.integers(0, 1 << (32 - nbits), E, dtype=np.uint64).astype(np.uint32)
        bits = _bits(rng.uniform(0.01, 100.0, E))  # the others: below and above the group (which is near 1.0)
        group = rng.random(E) < 0.55
        bits[group] = base | low[group]
        shared = (bits >> np.uint32(32 - nbits)) == (base >> np.uint32(32 - nbits))
        assert shared.sum() >= E // 2
        above = int((bits > (base | np.uint32((1 << (32 - nbits)) - 1))).sum())
        return bits.view(np.float32), above + int(shared.sum()) // 2 + 37
    if kind == "zeros":
        keys = rng.uniform(0.01, 100.0, E).astype(np.float32)
        zero = rng.random(E) < 0.62
        keys[zero] = 0.0
        assert zero.sum() >= 0.6 * E
        return keys, int((~zero).sum()) + int(zero.sum()) // 3 + 21
    raise KeyError(kind)


def _select(keys_dev, m, ws, keep):
    from gmr import _lib
    from gmr.kernels import ptr, stream
    _lib.call("gmr_frd_prune_select", keys_dev.numel(), int(m), ptr(keys_dev), ptr(ws), ptr(keep), stream())
    return keep.clone()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", SIZES)
def test_select_exact(E, kind):
    from gmr import _lib
    rng = np.random.default_rng(E % 1000 + 7 * KINDS.index(kind))
    keys, crafted = _keys(kind, E, rng)
    bits = _bits(keys)
    order = np.lexsort((np.arange(E), -bits.astype(np.int64)))
    rank = np.empty(E, np.int64)
    rank[order] = np.arange(E)
    rank_dev = torch.as_tensor(rank).to(DEV)
    kd = torch.as_tensor(keys).to(DEV)
    ws = torch.empty(int(_lib.load().gmr_frd_prune_workspace_ints()), dtype=torch.int32, device=DEV)
    keep = torch.empty(E, dtype=torch.uint8, device=DEV)
    ms = sorted({1, E // 5, E - 1, E, crafted})
    assert 1 < crafted < E - 1
    if kind in ("ties", "prefix24", "zeros"):  # the crafted m cuts a run of equal keys
        assert bits[order[crafted - 1]] == bits[order[crafted]]
    if kind == "zeros":
        assert bits[order[crafted - 1]] == 0 and bits[order[E - 2]] == 0
    for m in ms:
        got = _select(kd, m, ws, keep)
        want = (rank_dev < m).to(torch.uint8)
        assert int(got.sum()) == m, (E, kind, m)
        assert torch.equal(got, want), (E, kind, m, int((got != want).sum()))
        assert torch.equal(_select(kd, m, ws, keep), got), (E, kind, m)  # the same workspace, the same bytes


# ----------------------------------------------------------------------------- keys
def _prune_keys(w, u=None, seed=0, step=0):
    from gmr import _lib
    from gmr.kernels import ptr, stream
    wd = torch.as_tensor(w).to(DEV)
    ud = torch.as_tensor(u).to(DEV) if u is not None else None
    keys = torch.full((wd.numel(),), float("nan"), device=DEV)
    _lib.call("gmr_frd_prune_keys", wd.numel(), ptr(wd), ptr(ud), int(seed), int(step), ptr(keys), stream())
    return keys.cpu().numpy()


def test_keys_edges():
    w = np.array([0.25, 1.0, 3.0e-3, 0.0, 0.0, 0.0, 0.5, 1e-30, 0.7, 1.0], np.float32)
    u = np.array([1.0, 1.0, 1.0, 1.0, 0.5, 1e-38, 1e-38, 1e-38, 1e-45, 0.0], np.float32)
    keys = _prune_keys(w, u)
    assert np.isfinite(keys).all() and (keys >= 0).all() and not np.signbit(keys).any()
    # u = 1: -log u = 0 is clamped to 2^-25, the key is w 2^25 rounded once
    want = (w[:3].astype(np.float64) / 2.0 ** -25).astype(np.float32)
    assert np.array_equal(keys[:3], want)
    assert np.array_equal(keys[3:6], np.zeros(3, np.float32))  # w = 0, whatever u
    # a tiny u: w / -log u, near 0; u = 0 gives -log u = inf and key 0
    with np.errstate(divide="ignore"):
        ref = w.astype(np.float64) / np.maximum(-np.log(u.astype(np.float64)), 2.0 ** -25)
    np.testing.assert_allclose(keys[6:], ref[6:].astype(np.float32), rtol=1e-6, atol=0)
    assert keys[6] < 0.5 / 80 and 0 < keys[7] < 1e-31 and keys[9] == 0


@pytest.mark.parametrize("E", [1, 5, 1027])
def test_keys_philox_path_is_the_replica(E):
    """The in-kernel uniforms are u32_to_unit of word 0 of Philox(seed ^ mix, step, edge)."""
    rng = np.random.default_rng(E)
    w = rng.uniform(0.05, 1.0, E).astype(np.float32)
    for seed, step in ((0, 0), (999, 3), (2 ** 63 + 12345, 2 ** 40 + 1)):
        x = philox_ref.philox(seed ^ philox_ref.FRD_KEY_MIX, step, np.arange(E))[:, 0]
        u = philox_ref.u32_to_unit(x)
        assert u.dtype == np.float32 and 0 < u.min() and u.max() <= 1
        got, want = _prune_keys(w, None, seed, step), _prune_keys(w, u)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (E, seed, step)
