"""MGCN on MI355X — drop-in for models/mgcn.py of the reference (GeneralRecommender API).

Multi-view graph convolution: the item id embeddings, gated by each modality's projected features ("purified"), are
propagated over that modality's frozen item-item kNN graph and carried to the users over the interaction graph; a
LightGCN pass over the user-item graph gives the behaviour view; an attention over the two modal views and two
preference gates driven by the behaviour view fuse them.  What it computes:

Init (the constructor's RNG order, which is also named_parameters() order except that the feature tables draw nothing)
  nn.Embedding(U, 64), nn.Embedding(I, 64) draw their normal init, then xavier_uniform_ on the user table, then the item
  table; image_trs = nn.Linear(Dv, 64), text_trs = nn.Linear(Dt, 64); query_common = Linear(64, 64), Tanh,
  Linear(64, 1, no bias); gate_v, gate_t, gate_image_prefer, gate_text_prefer = Linear(64, 64) + Sigmoid each; every
  nn.Linear keeps its default init.  The feature tables are trainable.  Both modalities are required.

Graphs
  adj   D^-1/2 A D^-1/2 of the binary bipartite train graph: no epsilon on the degrees, no self loops, a node without
        edges has an empty row.  R = the U x I block of adj with its normalised values.
  Av, At   per modality, frozen: cosine similarity of the raw features, the knn_k largest per row (the row itself among
        them) kept with their values, w_ij / sqrt(rowsum_i rowsum_j) with row sums on both ends; not symmetric.  Built
        on the device at construction (the reference caches them in a file; nothing is written here).

forward, with E = [E_u; E_i]
  V = image_trs(image),  T = text_trs(text)
  Pv = E_i * sigmoid(gate_v(V)),  Pt = E_i * sigmoid(gate_t(T))                    the purifier
  Hv = Av^n Pv,  a = [R Hv; Hv]  (n = n_layers);  b the same from Pt
  c = mean(E_0 .. E_L),  E_k+1 = adj E_k  (L = n_ui_layers)
  q(x) = w2 . tanh(W1 x + b1);  (wa, wb) = softmax(q(a), q(b));  m = wa a + wb b   the fuser
  side = (sigmoid(Wi c + bi) * (a - m) + sigmoid(Wt c + bt) * (b - m) + m) / 3;  all = c + side

calculate_loss(users, pos, neg)   (B rows, duplicates kept)
  u, p, n = all[users], all[U + pos], all[U + neg]
  loss = -mean logsigmoid(<u,p> - <u,n>) + reg_weight * 0.5 (|u|^2 + |p|^2 + |n|^2) / train_batch_size
         + cl_loss * (nce(side_i[pos], c_i[pos]) + nce(side_u[users], c_u[users]))
  nce(x, y) = mean_i(log sum_j exp(<x_i, y_j> / 0.2) - <x_i, y_i> / 0.2) on F.normalize'd rows, in-batch; the divisor of
  the L2 term is the configured batch size, also in a short last batch.

full_sort_predict(users)   forward, scores = all_u[users] all_i^T

On the device
  One Slab holds every parameter.  A step:
    forward    V, T GEMMs (BIAS epilogue) into VT = [V | T]; gmr_mgcn_purify_fwd (both modalities, gates saved);
               n SpMMs per modality on its kNN CSR into the item rows of ab = [a | b], one two-block SpMM on R into the
               user rows; the LightGCN layers and gmr_frd_mean_fwd into c; gmr_mgcn_fuse_fwd (side, all, saved rows)
    loss       gmr_mgcn_bpr_reg_fwd_bwd (one launch: both row terms and [du; dp; dn] — chosen over
               gmr_bpr_logsigmoid_f32 + an added L2 kernel, which would be two); four gathers + normalisations, the two
               InfoNCE terms each as the logits GEMM, gmr_nce_rows_f32 (loss rows, L <- coef (softmax - I)) and two
               gradient GEMMs (GMR_MGCN_NCE_FUSED=1: gmr_nce_pairs_f32 / gmr_contrast_fused_f32 / gmr_nce_combine_f32
               with n = B, nodes = arange(B); see NCE_FUSED below for why it is not the default);
               gmr_mgcn_loss_reduce leaves [total, bpr, reg, nce_items, nce_users] on the device
    backward   sorted scatter of the BPR rows into dall (the loader's BPR plan) and of the normalise-backward rows
               [dside | dc] (the loader's two-key plan); gmr_mgcn_fuse_bwd; dW1 = z1a^T a + z1b^T b, dWi = zi^T c, ...
               as GEMMs / colsums on the z rows; dH = da_i + R^T da_u (one two-block SpMM, in place), dP = (A^T)^n dH;
               gmr_mgcn_purify_bwd; per modality dW = dV^T raw, db = colsum(dV), draw = dV W; dE = Horner chain of
               dc / (L + 1) over the symmetric adj, + the purifier's dE_i
  No host read inside a step.  MGCN draws no random numbers.
"""
import ctypes
import os

import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, copy64, r4, sort_plan
from .freedom import KNN_SIM_FLOATS, _Linear, _Table
from .kernels import ptr, stream
from .slab import Slab

D = 64
MAX_TABLES = 8  # GMR_FRD_MAX_LAYERS of include/gmr.h: the layer mean takes n_ui_layers + 1 tables
TEMP = 0.2
# GMR_MGCN_NCE_FUSED=1: the two in-batch InfoNCE terms through gmr_contrast_fused_f32 (no B x B block).  Off by
# default: its split-bf16 passes leave the gradient of the normalised rows 2.9e-6 of its largest entry from fp64 on the
# golden case B, where the logits GEMM + gmr_nce_rows_f32 + two gradient GEMMs leave 2.5e-7;
# MGCN's feature-path gradients come through these terms alone and are tested at 1e-6 of the largest entry
NCE_FUSED = os.environ.get("GMR_MGCN_NCE_FUSED", "0") == "1"
# (slab prefix, module name) of the 64 x 64 linears after the projections, in the constructor's order
GATES = (("gv", "gate_v"), ("gt", "gate_t"), ("pi", "gate_image_prefer"), ("pt", "gate_text_prefer"))


def check_config(config, n_items=None, has=(True, True)):
    """Raise NotImplementedError naming the key for settings outside the hot path; returns (n_ui_layers, n_layers,
    knn_k)."""
    c = config
    if int(c["embedding_size"] or D) != D:
        raise NotImplementedError(f"embedding_size = {c['embedding_size']}: {D} (the SpMM blocks and the row tiles are "
                                  f"64 columns)")
    L = int(c["n_ui_layers"])
    if L < 0 or L + 1 > MAX_TABLES:
        raise NotImplementedError(f"n_ui_layers = {L}: 0..{MAX_TABLES - 1}")
    n = int(c["n_layers"])
    if n < 0:
        raise NotImplementedError(f"n_layers = {n}: >= 0")
    k = int(c["knn_k"])
    if k < 1 or (n_items is not None and k > n_items):
        raise NotImplementedError(f"knn_k = {k}: 1..{n_items} (the number of items)")
    for name, h in zip(("image", "text"), has):
        if not h:
            raise NotImplementedError(f"{name} features (inter_file's {name} feature file) are missing: MGCN's forward "
                                      f"uses both modalities")
    if dist.world() > 1:
        raise NotImplementedError("world size > 1: the in-batch InfoNCE is over the global batch; MGCN runs on one "
                                  "device")
    return L, n, k


def knn_graph(feat, k):
    """The 'sym'-normalised top-k cosine graph of the raw features as an I x I CSR (K.knn_graph with the similarity in
    row chunks of at most KNN_SIM_FLOATS floats, as freedom.knn_topk)."""
    n, d = feat.shape
    dev = feat.device
    pad = torch.zeros((n, r4(d)), dtype=torch.float32, device=dev)  # rows padded to 16 bytes with zeros
    pad[:, :d].copy_(feat)
    fn = torch.empty_like(pad)
    K.normalize_rows(pad, fn)
    del pad
    ti = torch.empty((n, k), dtype=torch.int32, device=dev)
    tv = torch.empty((n, k), dtype=torch.float32, device=dev)
    ldn = r4(n)
    chunk = max(1, min(n, KNN_SIM_FLOATS // ldn))
    sim = torch.empty((chunk, ldn), dtype=torch.float32, device=dev)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        s = sim[:hi - lo, :n]
        K.gemm(fn[lo:hi], fn, s, trans_b=True)
        K.topk_rows(s, k, ti[lo:hi], tv[lo:hi])
    del sim
    rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(n * k, dtype=torch.int32, device=dev)
    val = torch.empty(n * k, dtype=torch.float32, device=dev)
    dis = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.call("gmr_knn_symnorm_csr", n, k, ptr(ti), k, ptr(tv), k, ptr(dis), ptr(rp), ptr(col), ptr(val), stream())
    return K.CSR(rp, col, val, n_cols=n, symmetric=False)


class _Seq(nn.Module):
    """Holder with nn.Sequential's child names: children {index: module}."""

    def __init__(self, children):
        super().__init__()
        for i, m in children.items():
            self.add_module(str(i), m)


class MGCN(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        self.n_ui_layers, self.n_layers, self.knn_k = check_config(
            c, self.n_items, (self.v_feat is not None, self.t_feat is not None))
        self.embedding_dim = D
        self.reg_weight, self.cl_loss = float(c["reg_weight"]), float(c["cl_loss"])
        self.batch_size = int(c["train_batch_size"])
        U, I, dev = self.n_users, self.n_items, self.device
        N = self.N = U + I
        # parameters in the reference's RNG order (mgcn.py:36-102)
        e_u, e_i = nn.Embedding(U, D), nn.Embedding(I, D)
        nn.init.xavier_uniform_(e_u.weight)
        nn.init.xavier_uniform_(e_i.weight)
        self.mods = (("image", self.v_feat, 0), ("text", self.t_feat, 1))  # (name, features, column block)
        trs = {name: nn.Linear(feat.shape[1], D) for name, feat, _ in self.mods}
        q1, q2 = nn.Linear(D, D), nn.Linear(D, 1, bias=False)
        gates = {p: nn.Linear(D, D) for p, _ in GATES}
        specs = [("E", (N, D), None)]
        for name, feat, _ in self.mods:
            specs.append((name + "_embedding", (I, feat.shape[1]), r4(feat.shape[1])))
        for name, feat, _ in self.mods:
            specs += [(name + "_W", (D, feat.shape[1]), r4(feat.shape[1])), (name + "_b", (D,), None)]
        specs += [("q_W1", (D, D), None), ("q_b1", (D,), None), ("q_w2", (1, D), None)]
        for p, _ in GATES:
            specs += [(p + "_W", (D, D), None), (p + "_b", (D,), None)]
        s = self.slab = Slab(specs, dev)
        with torch.no_grad():
            s.view("E")[:U].copy_(e_u.weight)
            s.view("E")[U:].copy_(e_i.weight)
            for name, feat, _ in self.mods:
                s.load(name + "_embedding", feat)
                s.load(name + "_W", trs[name].weight)
                s.load(name + "_b", trs[name].bias)
            s.load("q_W1", q1.weight)
            s.load("q_b1", q1.bias)
            s.load("q_w2", q2.weight)
            for p, _ in GATES:
                s.load(p + "_W", gates[p].weight)
                s.load(p + "_b", gates[p].bias)
        # module views under the reference's names, registered in its order
        e, ge = s.view("E"), s.gview("E")
        self.user_embedding = _Table(nn.Parameter(e[:U]))
        self.user_embedding.weight.grad = ge[:U]
        self.item_id_embedding = _Table(nn.Parameter(e[U:]))
        self.item_id_embedding.weight.grad = ge[U:]
        for name, _, _ in self.mods:
            setattr(self, name + "_embedding", _Table(s.parameter(name + "_embedding")))
        for name, _, _ in self.mods:
            setattr(self, name + "_trs", _Linear(s.parameter(name + "_W"), s.parameter(name + "_b")))
        self.query_common = _Seq({0: _Linear(s.parameter("q_W1"), s.parameter("q_b1")),
                                  2: _Table(s.parameter("q_w2"))})
        for p, mod in GATES:
            setattr(self, mod, _Seq({0: _Linear(s.parameter(p + "_W"), s.parameter(p + "_b"))}))
        # graphs
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        ne = int(self.user_items.numel())
        # deg_eps = 0: a node without edges has an empty row and is no column of any entry, so its d = inf is never
        # multiplied in
        self.norm_adj = K.bipartite_symnorm(U, I, self.user_ptr, self.user_items, self_loops=False, deg_eps=0.0)
        adj = self.norm_adj
        # R: the user rows of adj (they come first and hold the columns U + item) as a U x I CSR; R^T once
        self.R = K.CSR(adj.rowptr[:U + 1].clone(), (adj.col[:ne] - U).contiguous(), adj.val[:ne].clone(), n_cols=I,
                       symmetric=False)
        self.R_t = K.csr_transpose(self.R)
        self.mm_adj = {name: knn_graph(feat, self.knn_k) for name, feat, _ in self.mods}
        self.mm_adj_t = {name: K.csr_transpose(a) for name, a in self.mm_adj.items()}
        # work buffers
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.vt, self.pur, self.gates_i = f(I, 2 * D), f(I, 2 * D), f(I, 2 * D)   # [V | T], [Pv | Pt], [gv | gt]
        self.ab, self.c, self.side, self.all = f(N, 2 * D), f(N, D), f(N, D), f(N, D)
        self.saved, self.wab = f(N, 4 * D), f(N, 2)                                # [ha | hb | gi | gt], (wa, wb)
        self._h = [f(I, 2 * D) for _ in range(2)] if self.n_layers > 1 else []
        self._layers = [f(N, D) for _ in range(self.n_ui_layers)]
        self._t = [f(N, D) for _ in range(2)]
        self.dall, self.gtab = f(N, D), f(N, 2 * D)                                # d all; [dside | dc] of the InfoNCE
        self.dab, self.dc, self.zf, self.r = f(N, 2 * D), f(N, D), f(N, 4 * D), f(N, D)
        self.dpur, self.zp, self.dvt = f(I, 2 * D), f(I, 2 * D), f(I, 2 * D)
        self._loss = f(5)
        self._w = None
        self._i1 = (ctypes.c_int32 * 2)(0, 2)   # queries: side_i[pos], side_u[users]
        self._i2 = (ctypes.c_int32 * 2)(1, 3)   # keys:    c_i[pos],    c_u[users]

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def _names(self):
        out = [n + "_embedding" for n, _, _ in self.mods]
        for n, _, _ in self.mods:
            out += [n + "_W", n + "_b"]
        out += ["q_W1", "q_b1", "q_w2"]
        for p, _ in GATES:
            out += [p + "_W", p + "_b"]
        return out

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order."""
        s, U = self.slab, self.n_users
        return [s.gview("E")[:U], s.gview("E")[U:]] + [s.gview(n) for n in self._names()]

    # ------------------------------------------------------------------ forward
    def _chain(self, graphs, src, dst):
        """dst[:, blk] = graph_m^n src[:, blk] per modality over I x 128 tables (n = n_layers; n = 0 copies)."""
        for name, _, blk in self.mods:
            x = src[:, D * blk:D * blk + D]
            for i in range(self.n_layers):
                last = i == self.n_layers - 1
                y = (dst if last else self._h[i % 2])[:, D * blk:D * blk + D]
                graphs[name].spmm(y, [(x,)])
                x = y
            if self.n_layers == 0:
                copy64(x, dst[:, D * blk:D * blk + D])

    def _forward(self):
        """mgcn.py:146-201 into self.side / self.all (and the rows the backward reads)."""
        s, U, I, N = self.slab, self.n_users, self.n_items, self.N
        E = s.view("E")
        vt, pur, g, ab, c = self.vt, self.pur, self.gates_i, self.ab, self.c
        for name, _, blk in self.mods:
            K.gemm(s.view(name + "_embedding"), s.view(name + "_W"), vt[:, D * blk:D * blk + D], trans_b=True,
                   epi=K.EPI_BIAS, bias=s.view(name + "_b"))
        _lib.call("gmr_mgcn_purify_fwd", I, ptr(E[U:]), D, ptr(vt), 2 * D, ptr(vt[:, D:]), 2 * D, ptr(s.view("gv_W")),
                  ptr(s.view("gv_b")), ptr(s.view("gt_W")), ptr(s.view("gt_b")), D, ptr(pur), ptr(pur[:, D:]), 2 * D,
                  ptr(g), ptr(g[:, D:]), 2 * D, stream())
        self._chain(self.mm_adj, pur, ab[U:])
        self.R.spmm(ab[:U], [(ab[U:, :D],), (ab[U:, D:],)])
        tabs = [E]
        for i in range(self.n_ui_layers):
            self.norm_adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", N, N, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(c), D, stream())
        sv = self.saved
        _lib.call("gmr_mgcn_fuse_fwd", N, ptr(ab), ptr(ab[:, D:]), 2 * D, ptr(c), D, ptr(s.view("q_W1")),
                  ptr(s.view("q_b1")), ptr(s.view("q_w2")), ptr(s.view("pi_W")), ptr(s.view("pi_b")),
                  ptr(s.view("pt_W")), ptr(s.view("pt_b")), D, ptr(self.side), ptr(self.all), D, ptr(sv),
                  ptr(sv[:, D:]), ptr(sv[:, 2 * D:]), ptr(sv[:, 3 * D:]), 4 * D, ptr(self.wab), stream())

    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev = self.device
            f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
            self._w = {"B": B, "terms": f(4 * B), "contrib": f(3 * B, D), "raw": f(4, B, D), "nv": f(4, B, D),
                       "nrm": f(4, B), "g": f(4, B, D), "cln": f(2, B, 2 * D), "ctr": f(2, B, 2 * D), "dt": f(2, B, D),
                       "cs": f(2 * B, 2 * D), "nodes": torch.arange(B, dtype=torch.int32, device=dev)}
        return self._w

    def _plans(self, users, pos, neg):
        U = self.n_users
        return [sort_plan((users, pos, neg), (0, U, U)), sort_plan((users, pos), (0, U))]

    # ------------------------------------------------------------------ the step
    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0):
        """calculate_loss (mgcn.py:233-253) and all parameter gradients (into the slab's twin).  Returns the loss as a
        device scalar; loss_terms() reads [total, bpr, reg, nce_items, nce_users]."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: MGCN runs on one device")
        B = users.numel()
        if plan_bpr is None or plan_cl is None:
            plan_bpr, plan_cl = self._plans(users, pos, neg)
        w = self._work(B)
        self._forward()
        self.loss_fwd_bwd(users, pos, neg, 1.0 / (norm_rows or B), w)
        self.step_backward(plan_bpr, plan_cl, w, B)
        return self._loss[0]

    def loss_fwd_bwd(self, users, pos, neg, inv_norm, w):
        """The loss terms of the batch, the BPR contribution rows and the gradients of the four normalised InfoNCE
        row sets (w['g'])."""
        B, U, Bm = users.numel(), self.n_users, w["B"]
        terms = w["terms"][:4 * B]
        _lib.call("gmr_mgcn_bpr_reg_fwd_bwd", B, U, ptr(self.all), D, ptr(users), ptr(pos), ptr(neg), float(inv_norm),
                  self.reg_weight, float(self.batch_size), ptr(terms), ptr(w["contrib"]), D, stream())
        raw, nv, nrm = w["raw"], w["nv"], w["nrm"]
        for j, (src, idx, off) in enumerate(((self.side, pos, U), (self.c, pos, U), (self.side, users, 0),
                                             (self.c, users, 0))):
            K.gather_rows(src, idx, raw[j][:B], off=off)
            K.normalize_rows(raw[j][:B], nv[j][:B], nrm[j][:B])
        if NCE_FUSED:
            i1p, i2p = ctypes.cast(self._i1, ctypes.c_void_p), ctypes.cast(self._i2, ctypes.c_void_p)
            cln, ctr, dt = w["cln"], w["ctr"], w["dt"]
            _lib.call("gmr_nce_pairs_f32", 2, B, B, 0, i1p, i2p, ptr(nv), Bm, ptr(cln), Bm, stream())
            ws = K.contrast_workspace(B, B, self.device, "mgcn_nce")
            for k in range(2):
                K.contrast_fused(nv[self._i1[k]][:B], nv[self._i2[k]][:B], cln[k], w["nodes"][:B], 0, 1.0 / TEMP,
                                 self.cl_loss * inv_norm, terms[(2 + k) * B:(3 + k) * B], ctr[k][:B], dt[k][:B], ws)
            _lib.call("gmr_nce_combine_f32", 2, B, B, 0, i1p, i2p, ptr(ctr), Bm, ptr(dt), Bm, ptr(w["g"]), Bm,
                      stream())
        else:
            if "L" not in w:
                w["L"] = torch.empty((Bm, r4(Bm)), dtype=torch.float32, device=self.device)
            L, g = w["L"][:B, :B], w["g"]
            for k in range(2):
                v1, v2 = nv[self._i1[k]][:B], nv[self._i2[k]][:B]
                K.gemm(v1, v2, L, trans_b=True, alpha=1.0 / TEMP)
                _lib.call("gmr_nce_rows_f32", B, ptr(L), L.stride(0), self.cl_loss * inv_norm,
                          ptr(terms[(2 + k) * B:(3 + k) * B]), stream())       # L <- coef (softmax - I)
                K.gemm(L, v2, g[self._i1[k]][:B], alpha=1.0 / TEMP)
                K.gemm(L, v1, g[self._i2[k]][:B], trans_a=True, alpha=1.0 / TEMP)
        _lib.call("gmr_mgcn_loss_reduce", B, ptr(terms), float(inv_norm), self.reg_weight, float(self.batch_size),
                  self.cl_loss, ptr(self._loss), stream())

    def scatter_loss_rows(self, plan_bpr, plan_cl, w, B):
        """The outputs of loss_fwd_bwd scattered into dall (d loss / d all) and gtab = [dside | dc] (SMORE shares
        it)."""
        dall, gtab, cs = self.dall, self.gtab, w["cs"][:2 * B]
        K.zero_(dall)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), D, ptr(plan_bpr), ptr(w["contrib"]), D, ptr(dall), D,
                  stream())
        # rows [users | pos] of [dside | dc]: the normalise backward of the four gathered row sets
        nv, nrm, g = w["nv"], w["nrm"], w["g"]
        for j, dst in ((2, cs[:B, :D]), (3, cs[:B, D:]), (0, cs[B:, :D]), (1, cs[B:, D:])):
            K.normalize_rows_bwd(nv[j][:B], nrm[j][:B], g[j][:B], dst)
        K.zero_(gtab)
        _lib.call("gmr_scatter_sorted_f32", plan_cl.numel(), 2 * D, ptr(plan_cl), ptr(cs), 2 * D, ptr(gtab), 2 * D,
                  stream())

    def behaviour_bwd(self, dc):
        """dE = (1 / (L + 1)) sum_k adj^k dc into the slab's gradient: t <- dc; L times t <- adj t + dc, the last one
        scaled."""
        L, gE = self.n_ui_layers, self.slab.gview("E")
        copy64(dc, gE)
        src = dc
        for i in range(L):
            last = i == L - 1
            dst = gE if last else self._t[i % 2]
            if not last:
                copy64(dc, dst)
            sc = 1.0 / (L + 1) if last else 1.0
            self.norm_adj.spmm(dst, [(src,)], alpha=sc, beta=sc)
            src = dst

    def step_backward(self, plan_bpr, plan_cl, w, B):
        """All parameter gradients from the outputs of loss_fwd_bwd over B rows."""
        s, U, I, N = self.slab, self.n_users, self.n_items, self.N
        s.zero_grad()
        self.scatter_loss_rows(plan_bpr, plan_cl, w, B)
        dall, gtab = self.dall, self.gtab
        ab, c, sv, dab, dc, zf, r = self.ab, self.c, self.saved, self.dab, self.dc, self.zf, self.r
        _lib.call("gmr_mgcn_fuse_bwd", N, ptr(dall), D, ptr(gtab), ptr(gtab[:, D:]), 2 * D, ptr(ab), ptr(ab[:, D:]),
                  2 * D, ptr(sv), ptr(sv[:, D:]), ptr(sv[:, 2 * D:]), ptr(sv[:, 3 * D:]), 4 * D, ptr(self.wab),
                  ptr(s.view("q_w2")), ptr(s.view("q_W1")), ptr(s.view("pi_W")), ptr(s.view("pt_W")), D, ptr(dab),
                  ptr(dab[:, D:]), 2 * D, ptr(dc), D, ptr(zf), ptr(zf[:, D:]), ptr(zf[:, 2 * D:]), ptr(zf[:, 3 * D:]),
                  4 * D, ptr(r), D, stream())
        K.gemm(zf[:, :D], ab[:, :D], s.gview("q_W1"), trans_a=True)                 # dW1 = z1a^T a + z1b^T b
        K.gemm(zf[:, D:2 * D], ab[:, D:], s.gview("q_W1"), trans_a=True, beta=1.0)
        K.colsum(zf[:, :D], s.gview("q_b1"))
        K.colsum(zf[:, D:2 * D], s.gview("q_b1"), accumulate=True)
        K.colsum(r, s.gview("q_w2"))                                                # dw2 = colsum(dq_a ha + dq_b hb)
        for p, blk in (("pi", 2), ("pt", 3)):
            K.gemm(zf[:, D * blk:D * blk + D], c, s.gview(p + "_W"), trans_a=True)  # dWi = zi^T c
            K.colsum(zf[:, D * blk:D * blk + D], s.gview(p + "_b"))
        # dH = da_i + R^T da_u (in place on the item rows), dP = (A^T)^n dH
        self.R_t.spmm(dab[U:], [(dab[:U, :D],), (dab[:U, D:],)], beta=1.0)
        self._chain(self.mm_adj_t, dab[U:], self.dpur)
        self.behaviour_bwd(dc)
        gE = s.gview("E")
        dp, g, zp, dvt, vt = self.dpur, self.gates_i, self.zp, self.dvt, self.vt
        _lib.call("gmr_mgcn_purify_bwd", I, ptr(dp), ptr(dp[:, D:]), 2 * D, ptr(g), ptr(g[:, D:]), 2 * D,
                  ptr(s.view("E")[U:]), D, ptr(s.view("gv_W")), ptr(s.view("gt_W")), D, ptr(gE[U:]), D, 1, ptr(zp),
                  2 * D, ptr(dvt), ptr(dvt[:, D:]), 2 * D, stream())
        for (name, _, blk), p in zip(self.mods, ("gv", "gt")):
            z, dv = zp[:, D * blk:D * blk + D], dvt[:, D * blk:D * blk + D]
            K.gemm(z, vt[:, D * blk:D * blk + D], s.gview(p + "_W"), trans_a=True)    # dWg = z^T V
            K.colsum(z, s.gview(p + "_b"))
            self._proj_bwd(name, dv)

    def loss_terms(self):
        """[total, bpr, reg, nce_items, nce_users] of the last rec_step (device tensor)."""
        return self._loss

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward(self):
        """(all_u, all_i) of mgcn.py:146-208."""
        self._forward()
        return self.all[:self.n_users], self.all[self.n_users:]

    @torch.no_grad()
    def forward_embeddings(self):
        """full_sort_predict's tables (mgcn.py:255-263)."""
        return self.forward()
