"""Plain restatements of the operations in csrc/diffmm.hip lines 1-936 (the DiffMM rec-step row kernels and the
batch plumbing every model's backward goes through), written from the formulas in the kernel comments and
models/diffmm.py:129-258.  fp64 numpy / torch unless a dtype is passed; nothing here imports the package.

Three kinds of function:
  *            the operation in fp64 (forward kernels directly; the backward kernels by torch.autograd in double
               through the corresponding forward: F.normalize, leaky_relu(., 0.2), softmax)
  *_closed     the hand-derived backward the kernels implement, in fp64; tests/test_diffmm_kernels_ref_cpu.py holds
               it to the autograd form at 1e-12
  dtype=np.float32   the same computation in fp32 numpy in the kernel's order of operations (lane sums of four, the
               16-lane and 64-lane butterflies, the four wave partials): the yardstick of DESIGN section 2's rule for
               the transcendentals
The sorted scatter has one strict fp32 restatement (the slot-order sum the determinism claim rests on) and the sort
is np.sort of the plan words.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-12
C8 = float(np.float32(1e-8))    # the kernels' 1e-8f
C10 = float(np.float32(1e-10))  # and 1e-10f
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _n(t):
    return t.detach().numpy()


# ------------------------------------------------------------------------------------------------ lane helpers
def lane_dot(a, b):
    """dot4 of every lane: rows of 64 as 16 lanes of 4 columns, ((x0 y0 + x1 y1) + x2 y2) + x3 y3 in a's dtype."""
    p = (a * b).reshape(a.shape[0], -1, 4)
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]


def butterfly(v, width):
    """The xor butterfly over groups of `width` lanes along the last axis (row16_sum: 16, wave_sum: 64); every lane
    of a group ends with the same value, which is returned per group."""
    lanes = v.shape[-1]
    idx = np.arange(lanes)
    m = width // 2
    while m >= 1:
        v = v + v[..., idx ^ m]
        m //= 2
    return v[..., ::width]


def row_sumsq(x):
    """Sum of squares of 64-wide rows in the kernel's order (x's dtype)."""
    return butterfly(lane_dot(x, x), 16)[:, 0]


def block_sum(x, dtype=np.float64):
    """The one-block sum of sum_kernel / mw_grad_block: thread t adds x[t], x[t + 256], ... in order, each wave runs
    the 64-lane butterfly, the four wave partials combine as (r0 + r1) + (r2 + r3)."""
    x = np.asarray(x, dtype)
    acc = np.zeros(256, dtype)
    for i0 in range(0, len(x), 256):
        c = x[i0:i0 + 256]
        acc[:len(c)] = acc[:len(c)] + c
    r = butterfly(acc, 64)
    return dtype((r[0] + r[1]) + (r[2] + r[3]))


# ------------------------------------------------------------------------------------------------ forward kernels
def softmax2(mw, dtype=np.float64):
    a, b = dtype(mw[0]), dtype(mw[1])
    mx = max(a, b)
    ea, eb = np.exp(a - mx), np.exp(b - mx)
    s = ea + eb
    return ea / s, eb / s


def combine_fwd(G, H, Qi, Qt, mw, lam, dtype=np.float64):
    """E = G + H + lam [Qi[:, :64] | Qt[:, :64]];  M = w0 E_img + w1 E_txt, w = softmax(mw)."""
    f = lambda v: np.asarray(v, dtype)  # noqa: E731
    A = np.concatenate([f(Qi)[:, :64], f(Qt)[:, :64]], 1)
    E = dtype(lam) * A + (f(G) + f(H))
    w0, w1 = softmax2(mw, dtype)
    return E, w1 * E[:, 64:] + w0 * E[:, :64]


def _norms(x, dtype):
    if dtype is np.float32:
        return np.maximum(np.sqrt(row_sumsq(x)), np.float32(EPS))
    return np.maximum(np.sqrt((x * x).sum(1)), EPS)


def final_fwd(M, L, ris, dtype=np.float64):
    """Emb = M + L + ris M / max(|M|, 1e-12);  nrm = max(|M|, 1e-12)."""
    M, L = np.asarray(M, dtype), np.asarray(L, dtype)
    nv = _norms(M, dtype)
    return (dtype(ris) / nv)[:, None] * M + (M + L), nv


def cl_fwd(Qi, Qt, K2, dtype=np.float64):
    """K = [Qi[:, 64:] | Qt[:, 64:]] + K2;  CLN = normalize(K + 1e-8) per 64-column half;  nrm = [img | txt]."""
    f = lambda v: np.asarray(v, dtype)  # noqa: E731
    K = (np.concatenate([f(Qi)[:, 64:], f(Qt)[:, 64:]], 1) + f(K2)) + dtype(C8)
    ni, nt = _norms(K[:, :64], dtype), _norms(K[:, 64:], dtype)
    one = dtype(1)
    return np.concatenate([(one / ni)[:, None] * K[:, :64], (one / nt)[:, None] * K[:, 64:]], 1), np.concatenate([ni, nt])


def normalize_rows(x):
    x = np.asarray(x, np.float64)
    nv = np.maximum(np.sqrt((x * x).sum(1)), EPS)
    return x / nv[:, None], nv


def leaky(z, slope):
    z = np.asarray(z, np.float64)
    return np.where(z > 0, z, slope * z)


# ------------------------------------------------------------------------------------------------ normalize backward
def normalize_bwd(z, g, slope=1.0):
    """d/dz of <g, F.normalize(leaky_relu(z, slope))> by autograd in double (slope 1: no activation)."""
    z = _t(z).requires_grad_(True)
    a = F.leaky_relu(z, slope) if slope != 1.0 else z
    (F.normalize(a, dim=1, eps=EPS) * _t(g)).sum().backward()
    return _n(z.grad)


def normalize_bwd_closed(y, nrm, g, slope=1.0):
    """(g - y <y, g>) / nrm, the projection dropped where the norm was clamped, then the leaky-ReLU backward on
    sign(y): what nbwd_leaky and normalize_bwd_kernel compute."""
    y, nrm, g = (np.asarray(v, np.float64) for v in (y, nrm, g))
    dp = np.where(nrm <= EPS, 0.0, (y * g).sum(1))
    out = (g - dp[:, None] * y) / nrm[:, None]
    return out * np.where(y > 0, 1.0, slope) if slope != 1.0 else out


# ------------------------------------------------------------------------------------------------ final backward
def final_bwd(dEmb, T1, M, ris, E, mw):
    """By autograd in double: dM through Emb = M + adj@M + ris normalize(M) (T1 = adj^T dEmb is given), dE through
    M = w0 E_img + w1 E_txt, dw = (<E_img, dM>, <E_txt, dM>) and dmw through w = softmax(mw)."""
    Ml = _t(M).requires_grad_(True)
    ((Ml + ris * F.normalize(Ml, dim=1, eps=EPS)) * _t(dEmb)).sum().add((Ml * _t(T1)).sum()).backward()
    dM = Ml.grad
    El, mwl = _t(E).requires_grad_(True), _t(mw).requires_grad_(True)
    w = torch.softmax(mwl, 0)
    w.retain_grad()
    ((w[0] * El[:, :64] + w[1] * El[:, 64:]) * dM).sum().backward()
    return _n(dM), _n(El.grad), _n(w.grad), _n(mwl.grad)


def final_bwd_closed(dEmb, T1, M, ris, E, mw):
    dEmb, T1, M, E = (np.asarray(v, np.float64) for v in (dEmb, T1, M, E))
    y, nv = normalize_rows(M)
    dM = dEmb + T1 + ris * normalize_bwd_closed(y, nv, dEmb)
    w0, w1 = softmax2(mw)
    dw = np.array([(E[:, :64] * dM).sum(), (E[:, 64:] * dM).sum()])
    return dM, np.concatenate([w0 * dM, w1 * dM], 1), dw, mw_grad_closed(dw, mw)


def mw_grad(dw, mw):
    """Softmax backward by autograd in double: d/dmw of <softmax(mw), dw>."""
    mwl = _t(mw).requires_grad_(True)
    (torch.softmax(mwl, 0) * _t(dw)).sum().backward()
    return _n(mwl.grad)


def mw_grad_closed(dw, mw, dtype=np.float64):
    w0, w1 = softmax2(mw, dtype)
    da, db = dtype(dw[0]), dtype(dw[1])
    s = w0 * da + w1 * db
    return np.array([w0 * (da - s), w1 * (db - s)], dtype)


# ------------------------------------------------------------------------------------------------ the linear rows
def dg(dE, T2, U):
    """dG = dE + [T2[:U]; 0], in the dtype of dE (one addition: fp32 gives the kernel's bits)."""
    out = np.array(dE, copy=True)
    out[:U] = out[:U] + np.asarray(T2)[:U]
    return out


def cl_bwd(dK, T, dE, lam):
    """Ri = [lam dE_img | dK_img + T_img], Rt likewise for text."""
    dK, T, dE = (np.asarray(v, np.float64) for v in (dK, T, dE))
    dC = dK + T
    return (np.concatenate([lam * dE[:, :64], dC[:, :64]], 1), np.concatenate([lam * dE[:, 64:], dC[:, 64:]], 1))


def assemble(T2, T3, Ri, Rt, E0, reg2, U, t3u_from_t2=False):
    """dE0 (N x 64) and the unprojected dNF (I x 128), from the comment above assemble_kernel."""
    T2, T3, Ri, Rt, E0 = (np.asarray(v, np.float64) for v in (T2, T3, Ri, Rt, E0))
    T3u = T2 if t3u_from_t2 else T3
    h = lambda v, r: v[r, :64] + v[r, 64:]  # noqa: E731
    u, i = slice(0, U), slice(U, None)
    dE0 = np.empty_like(E0)
    dE0[u] = h(T3u, u) + h(Ri, u) + h(Rt, u) + reg2 * E0[u]
    dE0[i] = h(T2, i) + Ri[i, :64] + Rt[i, :64] + reg2 * E0[i]
    dNF = np.concatenate([T3[i, :64] + Ri[i, 64:], T3[i, 64:] + Rt[i, 64:]], 1)
    return dE0, dNF


def assemble_projection(dNF, Z, slope):
    """dNF through the modality projections' normalize(leaky_relu(Z)) backward, per 64-column half (autograd)."""
    return np.concatenate([normalize_bwd(Z[:, :64], dNF[:, :64], slope), normalize_bwd(Z[:, 64:], dNF[:, 64:], slope)], 1)


# ------------------------------------------------------------------------------------------------ BPR rows
def bpr(Emb, U, users, pos, neg, inv_norm, dtype=np.float64):
    """x = <a, p> - <a, n>, loss = -log(1e-10 + sigmoid(x)), and the three contribution blocks [d a; d p; d n] scaled
    by inv_norm.  Returns loss (B), contrib (3B x 64), x (B)."""
    Emb = np.asarray(Emb, dtype)
    a, p, q = Emb[users], Emb[U + pos], Emb[U + neg]
    if dtype is np.float32:
        x = butterfly(lane_dot(a, p) - lane_dot(a, q), 16)[:, 0]
    else:
        x = (a * p - a * q).sum(1)
    one, c = dtype(1), dtype(C10)
    with np.errstate(over="ignore"):
        s = one / (one + np.exp(-x))
    gx = -(s * (one - s)) / (c + s) * dtype(inv_norm)
    loss = -np.log(c + s)
    return loss, np.concatenate([gx[:, None] * (p - q), gx[:, None] * a, -gx[:, None] * a]), x


def row_softmax(L, coef, dtype=np.float64):
    """P = coef exp(L) / S, lse = log S, S = the row sum of exp(L) (no max subtraction, as the reference)."""
    e = np.exp(np.asarray(L, dtype))
    if dtype is np.float32:
        S = np.array([block_sum(r, np.float32) for r in e], np.float32)
    else:
        S = e.sum(1)
    return (dtype(coef) / S)[:, None] * e, np.log(S)


def contrast_rows(CLN, nodes, node_off, lse, inv_temp, coef, contrib0):
    """loss_b = lse_b - <p1, p2> / temp; contrib = [contrib0 - coef / temp p2 | -coef / temp p1]."""
    CLN, lse, contrib0 = (np.asarray(v, np.float64) for v in (CLN, lse, contrib0))
    r = CLN[node_off + np.asarray(nodes)]
    p1, p2 = r[:, :64], r[:, 64:]
    k = -coef * inv_temp
    return lse - (p1 * p2).sum(1) * inv_temp, np.concatenate([contrib0 + k * p2, k * p1], 1)


# ------------------------------------------------------------------------------------------------ sort and scatter
def plan_words(keys, key_add, beg, end, nk):
    """The unsorted plan words of one batch: slot i = k len + j holds (keys[k, beg + j] + key_add[k]) << 32 | i."""
    ln = end - beg
    out = np.empty(ln * nk, np.uint64)
    for k in range(nk):
        key = (np.asarray(keys[k, beg:end], np.int64) + int(key_add[k])).astype(np.uint64)
        out[k * ln:(k + 1) * ln] = (key << np.uint64(32)) | np.arange(k * ln, (k + 1) * ln, dtype=np.uint64)
    return out


def sort_batch_keys(keys, offsets, key_add, nk, pow2, out_stride=None, fill=None):
    """gmr_sort_batch_keys: per batch the plan words sorted ascending and padded with ~0 to pow2, at rows of
    out_stride words; the gap past pow2 keeps `fill`."""
    nb = len(offsets) - 1
    out_stride = pow2 if out_stride is None else out_stride
    out = np.full((nb, out_stride), PAD if fill is None else fill, np.uint64)
    for b in range(nb):
        w = plan_words(keys, key_add, int(offsets[b]), int(offsets[b + 1]), nk)
        out[b, :pow2] = np.sort(np.concatenate([w, np.full(pow2 - len(w), PAD, np.uint64)]))
    return out


def plan_of(keys, pow2=None):
    """A sorted plan for one keyset: slot i carries keys[i]."""
    keys = np.asarray(keys, np.int32).reshape(1, -1)
    n = keys.shape[1]
    return sort_batch_keys(keys, [0, n], [0], 1, n if pow2 is None else pow2)[0]


def scatter_sorted_f32(plan, contrib, dst):
    """The strict fp32 restatement: for each run of equal keys, s = 0; for slot in run order: s += x[slot];
    dst[key] += s.  Padding words are skipped.  Returns the new dst (float32)."""
    contrib = np.asarray(contrib, np.float32)
    dst = np.array(dst, np.float32, copy=True)
    i, n = 0, len(plan)
    while i < n:
        key = int(plan[i] >> np.uint64(32))
        if key == 0xFFFFFFFF:
            i += 1
            continue
        s = np.zeros(contrib.shape[1], np.float32)
        while i < n and int(plan[i] >> np.uint64(32)) == key:
            s = s + contrib[int(plan[i] & np.uint64(0xFFFFFFFF))]
            i += 1
        dst[key] = dst[key] + s
    return dst


def scatter_index_add(plan, contrib, dst):
    """fp64 index_add of the same plan; also the per-destination sum of |terms| and the longest run."""
    live = (plan >> np.uint64(32)) != np.uint64(0xFFFFFFFF)
    key = torch.as_tensor((plan[live] >> np.uint64(32)).astype(np.int64))
    slot = (plan[live] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    x = _t(contrib)[torch.as_tensor(slot)]
    out = _t(dst).clone().index_add_(0, key, x)
    terms = _t(np.abs(np.asarray(dst, np.float64))).index_add_(0, key, x.abs())
    longest = int(np.bincount(key.numpy()).max()) if len(key) else 0
    return _n(out), _n(terms), longest


# ------------------------------------------------------------------------------------------------ reductions
def sqnorm_parts(x, g):
    """The g partials of sqnorm_part_kernel: block b owns i with (i // 256) % g == b.  Accumulated in extended
    precision (a sequential fp64 sum of thousands of terms is further from the truth than the kernel's tree)."""
    assert np.finfo(np.longdouble).eps < 1e-18
    x = np.asarray(x, np.float64)
    sq = np.zeros(-(-max(len(x), 1) // (256 * g)) * 256 * g, np.longdouble)
    sq[:len(x)] = x * x  # the square of an fp32 value is exact in fp64
    return sq.reshape(-1, g, 256).sum(axis=(0, 2)).astype(np.float64)


def sqnorm_nparts(n):
    return int(min(max((n + 2047) // 2048, 1), 1024))


def loss_total(bpr_rows, inv_nr, parts, reg, cu, ci, ssl):
    """loss = sum(bpr) / nr + reg |E0|^2 + ssl / nr (sum(cu) + sum(ci)) in fp64, and the magnitudes of the four
    addends (the fp32 value rounds each once and adds them in this order)."""
    t = [np.asarray(bpr_rows, np.float64).sum() * inv_nr, np.asarray(parts, np.float64).sum() * reg,
         np.asarray(cu, np.float64).sum() * ssl, np.asarray(ci, np.float64).sum() * ssl]
    return sum(t), t
