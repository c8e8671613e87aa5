"""FREEDOM on MI355X — drop-in for models/freedom.py of the reference (GeneralRecommender API).

Two graphs: the frozen item-item graph mm_adj (weighted union of the image / text kNN graphs, built
once on the device) and the user-item graph, pruned once per epoch by degree-sensitive sampling
(pre_epoch_processing) and renormalised.

Layout in HBM: the parameter slab holds E ((U + I) x 64: user rows, then item rows), the trainable
feature tables (rows padded to 16 bytes) and the two projections.  One (U + I) x 192 work table
`tab` = [G | T | V] carries the propagated embeddings [ua; ia] in columns 0:64 and, on the item rows,
text_trs(text) in 64:128 and image_trs(image) in 128:192; its gradient twin `gtab` takes the single
sorted scatter of the BPR contributions.
  forward      T, V GEMMs (BIAS epilogue) into tab; h = mm_adj^n E_item; E_k+1 = adj E_k;
               G = mean(E_0..E_L) (+ h on item rows)                  (gmr_frd_mean_fwd)
  loss         three BPR terms + contributions in one call             (gmr_frd_loss_fwd_bwd)
  backward     one sorted scatter into gtab; dW = dT^T raw, db = colsum(dT), draw = dT W per modality;
               dE = sum_k adj^k g / (L + 1) as a Horner chain (adj is symmetric), and on the item rows
               + (mm_adj^T)^n g_item
  predict      forward on norm_adj (the unpruned graph), scores = ua[users] @ ia^T
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, config_seed, copy64, r4, sort_plan
from .kernels import ptr, stream
from .slab import Slab

# the similarity GEMM of the kNN construction is chunked over rows above this many floats (~1 GB)
KNN_SIM_FLOATS = 1 << 28


class _Linear(nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = weight
        self.bias = bias


class _Table(nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = weight


def knn_topk(feat, k):
    """Per-row top-k of the cosine similarity (freedom.py:79-82): normalised rows, the MFMA GEMM in row
    chunks, gmr_topk_rows_f32.  Returns the n x k int32 index lists (the row itself is among them)."""
    n, d = feat.shape
    dev = feat.device
    if k > n:
        raise ValueError(f"knn_k = {k} exceeds the {n} items")
    pad = torch.zeros((n, r4(d)), dtype=torch.float32, device=dev)  # rows padded to 16 bytes with zeros
    pad[:, :d].copy_(feat)
    fn = torch.empty_like(pad)
    K.normalize_rows(pad, fn)
    del pad
    ti = torch.empty((n, k), dtype=torch.int32, device=dev)
    ldn = r4(n)
    chunk = max(1, min(n, KNN_SIM_FLOATS // ldn))
    sim = torch.empty((chunk, ldn), dtype=torch.float32, device=dev)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        s = sim[:hi - lo, :n]
        K.gemm(fn[lo:hi], fn, s, trans_b=True)
        K.topk_rows(s, k, ti[lo:hi])
    return ti


def knn_union_csr(idx_a, w_a, idx_b=None, w_b=0.0):
    """CSR of w_a A + w_b B for the binary top-k adjacencies (gmr_frd_knn_union_csr); one host read of
    the entry count."""
    n, k = idx_a.shape
    dev = idx_a.device
    scol = torch.empty(n * 2 * k, dtype=torch.int32, device=dev)
    sval = torch.empty(n * 2 * k, dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(n * 2 * k, dtype=torch.int32, device=dev)
    val = torch.empty(n * 2 * k, dtype=torch.float32, device=dev)
    _lib.call("gmr_frd_knn_union_csr", n, k, ptr(idx_a), idx_a.stride(0), float(w_a), ptr(idx_b),
              idx_b.stride(0) if idx_b is not None else 0, float(w_b), ptr(scol), ptr(sval), ptr(cnt), ptr(rp),
              ptr(col), ptr(val), stream())
    nnz = int(rp[-1].item())
    return K.CSR(rp, col[:nnz], val[:nnz], n_cols=n, symmetric=False)


def prune_select(w, m, u=None, seed=0, step=0):
    """Keep bytes of a weighted draw of m of the edges without replacement, P(e) ~ w[e]
    (gmr_frd_prune_keys + gmr_frd_prune_select); u: injected uniforms in (0, 1) instead of Philox."""
    E = w.numel()
    dev = w.device
    keys = torch.empty(E, dtype=torch.float32, device=dev)
    keep = torch.empty(E, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(_lib.load().gmr_frd_prune_workspace_ints()), dtype=torch.int32, device=dev)
    _lib.call("gmr_frd_prune_keys", E, ptr(w), ptr(u), int(seed), int(step), ptr(keys), stream())
    _lib.call("gmr_frd_prune_select", E, int(m), ptr(keys), ptr(ws), ptr(keep), stream())
    return keep


class FREEDOM(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        d = int(config["embedding_size"])
        if d != 64 or int(config["feat_embed_dim"] or d) != 64:
            raise NotImplementedError("embedding_size = feat_embed_dim = 64 (FREEDOM.yaml): the SpMM blocks are "
                                      "64 columns")
        self.embedding_dim = self.feat_embed_dim = d
        self.knn_k = int(config["knn_k"])
        self.n_layers = int(config["n_mm_layers"])
        self.n_ui_layers = int(config["n_ui_layers"])
        if not 0 <= self.n_ui_layers < 8 or self.n_layers < 0:
            raise NotImplementedError("n_ui_layers in 0..7, n_mm_layers >= 0")
        self.reg_weight = float(config["reg_weight"])
        self.mm_image_weight = float(config["mm_image_weight"])
        self.dropout = float(config["dropout"])
        # lambda_coeff, cf_model, degree_ratio, weight_size: read by the reference and never used
        self.seed = config_seed(config)
        U, I, dev = self.n_users, self.n_items, self.device
        self.N = U + I
        # parameters in the reference's RNG order (freedom.py:49-62): both nn.Embedding constructors draw
        # their normal init before the xavier draws replace it; from_pretrained draws nothing
        e_u, e_i = nn.Embedding(U, d), nn.Embedding(I, d)
        nn.init.xavier_uniform_(e_u.weight)
        nn.init.xavier_uniform_(e_i.weight)
        specs = [("E", (U + I, d), None)]
        lins = {}
        self.mods = []  # (name, feature tensor, column block of the work table), image first as the reference
        for name, feat, blk in (("image", self.v_feat, 2), ("text", self.t_feat, 1)):
            if feat is None:
                continue
            D = feat.shape[1]
            lins[name] = nn.Linear(D, d)
            specs += [(name + "_embedding", (I, D), r4(D)), (name + "_W", (d, D), r4(D)), (name + "_b", (d,), None)]
            self.mods.append((name, feat, blk))
        self.slab = Slab(specs, dev)
        s = self.slab
        with torch.no_grad():
            s.view("E")[:U].copy_(e_u.weight)
            s.view("E")[U:].copy_(e_i.weight)
            for name, feat, _ in self.mods:
                s.load(name + "_embedding", feat)
                s.load(name + "_W", lins[name].weight)
                s.load(name + "_b", lins[name].bias)
        e, ge = s.view("E"), s.gview("E")
        self.user_embedding = _Table(nn.Parameter(e[:U]))
        self.user_embedding.weight.grad = ge[:U]
        self.item_id_embedding = _Table(nn.Parameter(e[U:]))
        self.item_id_embedding.weight.grad = ge[U:]
        for name, _, _ in self.mods:
            setattr(self, name + "_embedding", _Table(s.parameter(name + "_embedding")))
            setattr(self, name + "_trs", _Linear(s.parameter(name + "_W"), s.parameter(name + "_b")))
        # graphs
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        self.n_edges = int(self.user_items.numel())
        self.norm_adj = K.bipartite_symnorm(U, I, self.user_ptr, self.user_items, self_loops=False, deg_eps=1e-7)
        # edge_values (freedom.py:156-162) are norm_adj's values on the user rows, in user-CSR order
        self.edge_values = self.norm_adj.val[:self.n_edges]
        self.masked_adj = None
        self._epoch = 0
        self.knn_ind = {name: knn_topk(feat, self.knn_k) for name, feat, _ in self.mods}
        if len(self.mods) == 2:
            w = self.mm_image_weight
            self.mm_adj = knn_union_csr(self.knn_ind["image"], w, self.knn_ind["text"], 1.0 - w)
        else:
            self.mm_adj = knn_union_csr(self.knn_ind[self.mods[0][0]], 1.0)
        self.mm_adj_t = K.csr_transpose(self.mm_adj)  # mm_adj is not symmetric
        # work buffers
        N = self.N
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.tab, self.gtab = f(N, 192), f(N, 192)
        self._layers = [f(N, d) for _ in range(self.n_ui_layers)]
        self._h = [f(I, d) for _ in range(min(self.n_layers, 2))]
        self._t = [f(N, d) for _ in range(2)]
        self._eval = f(N, d)
        self._w = None

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order."""
        s, U = self.slab, self.n_users
        out = [s.gview("E")[:U], s.gview("E")[U:]]
        for name, _, _ in self.mods:
            out += [s.gview(name + "_embedding"), s.gview(name + "_W"), s.gview(name + "_b")]
        return out

    def extra_state(self):
        """The pruning epoch counter: a resumed run redraws the graphs the uninterrupted one would."""
        return {"epoch_ctr": int(self._epoch)}

    def load_extra_state(self, st):
        self._epoch = int(st["epoch_ctr"])

    # ------------------------------------------------------------------ pruning
    def pre_epoch_processing(self):
        if self.dropout <= 0.0:
            self.masked_adj = self.norm_adj
            return
        self.prune_edges()
        self._epoch += 1

    def prune_edges(self, keep_idx=None, u=None):
        """Degree-sensitive edge pruning (freedom.py:128-143): int(E (1 - dropout)) of the E train edges drawn
        without replacement with probability ~ edge_values, the kept graph renormalised by its own degrees.
        keep_idx: kept edge ids (positions in the user CSR) instead of a draw; u: injected uniforms."""
        E, dev = self.n_edges, self.device
        if keep_idx is not None:
            keep = torch.zeros(E, dtype=torch.uint8, device=dev)
            keep[keep_idx.to(dev).long()] = 1
            m = int(keep_idx.numel())
        else:
            m = int(E * (1. - self.dropout))
            keep = prune_select(self.edge_values, m, u=u, seed=self.seed, step=self._epoch)
        U = self.n_users
        orp = torch.empty(U + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(U, dtype=torch.int32, device=dev)
        ocol = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        oval = torch.empty(max(m, 1), dtype=torch.float32, device=dev)
        # compaction of the binary U x I CSR by the keep bytes (exactly m set); the values are not used
        _lib.call("gmr_csr_drop_count", U, ptr(self.user_ptr), ptr(self.user_items), 0, ptr(keep), 1.0, 0, 0, ptr(ws),
                  ptr(orp), stream())
        _lib.call("gmr_csr_drop_write", U, ptr(self.user_ptr), ptr(self.user_items), ptr(self.edge_values), 0,
                  ptr(keep), 1.0, 0, 0, ptr(orp), ptr(ocol), ptr(oval), stream())
        self.masked_adj = K.bipartite_symnorm(U, self.n_items, orp, ocol[:m], self_loops=False, deg_eps=1e-7)
        return keep

    # ------------------------------------------------------------------ forward
    def _project(self):
        """tab[U:, 64:128] = text_trs(text), tab[U:, 128:192] = image_trs(image) (freedom.py:205, 208)."""
        s, U = self.slab, self.n_users
        for name, _, blk in self.mods:
            K.gemm(s.view(name + "_embedding"), s.view(name + "_W"), self.tab[U:, 64 * blk:64 * blk + 64], trans_b=True,
                   epi=K.EPI_BIAS, bias=s.view(name + "_b"))

    def _forward(self, adj, out):
        """freedom.py:164-178 into out (N x 64 view): mean of E_0..E_L, + mm_adj^n E_item on the item rows."""
        U, N = self.n_users, self.N
        E = self.slab.view("E")
        h = None
        if self.n_layers > 0:
            src = E[U:]
            for i in range(self.n_layers):
                h = self._h[i % 2]
                self.mm_adj.spmm(h, [(src,)])
                src = h
        tabs = [E]
        for i in range(self.n_ui_layers):
            adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", N, U, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), ptr(h), h.stride(0) if h is not None else 0,
                  ptr(out), out.stride(0), stream())

    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev = self.device
            self._w = {"B": B, "parts": torch.empty(3 * B, dtype=torch.float64, device=dev),
                       "loss": torch.empty(4, device=dev), "contrib": torch.empty((3 * B, 192), device=dev)}
        return self._w

    def _plan(self, users, pos, neg):
        return sort_plan((users, pos, neg), (0, self.n_users, self.n_users))

    def loss_fwd_bwd(self, users, pos, neg, inv_norm, w):
        """The three BPR terms of the batch on the work table and their 3B x 192 contribution rows."""
        U, tab = self.n_users, self.tab
        has = {name for name, _, _ in self.mods}
        T = tab[U:, 64:128] if "text" in has else None
        V = tab[U:, 128:192] if "image" in has else None
        _lib.call("gmr_frd_loss_fwd_bwd", users.numel(), U, ptr(tab), tab.stride(0), ptr(T), tab.stride(0), ptr(V),
                  tab.stride(0), ptr(users), ptr(pos), ptr(neg), self.reg_weight, float(inv_norm), ptr(w["parts"]),
                  ptr(w["loss"]), ptr(w["contrib"]), 192, stream())

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0):
        """calculate_loss (freedom.py:189-210) on the pruned graph and all parameter gradients (into the slab
        gradient).  Returns the loss as a device scalar; loss_terms() reads [total, graph, text, image]."""
        if dist.is_dist():
            raise NotImplementedError("FREEDOM runs on one device")
        if self.masked_adj is None:
            self.pre_epoch_processing()
        B = users.numel()
        if plan_bpr is None:
            plan_bpr = self._plan(users, pos, neg)
        w = self._work(B)
        self.step_forward()
        self.loss_fwd_bwd(users, pos, neg, 1.0 / (norm_rows or B), w)
        self.step_backward(plan_bpr, w)
        return w["loss"][0]

    def step_forward(self):
        """The propagated table and the projected features of one step, into the work table."""
        self._project()
        self._forward(self.masked_adj, self.tab[:, :64])

    def step_backward(self, plan_bpr, w):
        """All parameter gradients from the contribution rows of loss_fwd_bwd."""
        U, L = self.n_users, self.n_ui_layers
        s, gtab, adj = self.slab, self.gtab, self.masked_adj
        s.zero_grad()
        K.zero_(gtab)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), 192, ptr(plan_bpr), ptr(w["contrib"]), 192, ptr(gtab),
                  192, stream())
        for name, _, blk in self.mods:
            self._proj_bwd(name, gtab[U:, 64 * blk:64 * blk + 64])
        # dE = (1 / (L + 1)) sum_k adj^k g: t <- g; L times t <- adj t + g; the last one scaled
        g, gE = gtab[:, :64], s.gview("E")
        copy64(g, gE)
        src = g
        for i in range(L):
            last = i == L - 1
            dst = gE if last else self._t[i % 2]
            if not last:
                copy64(g, dst)
            sc = 1.0 / (L + 1) if last else 1.0
            adj.spmm(dst, [(src,)], alpha=sc, beta=sc)
            src = dst
        # dh = g on the item rows (ia = mean + h); through (mm_adj^T)^n into the item embeddings
        if self.n_layers > 0:
            src = g[U:]
            for i in range(self.n_layers):
                last = i == self.n_layers - 1
                dst = gE[U:] if last else self._h[i % 2]
                self.mm_adj_t.spmm(dst, [(src,)], beta=1.0 if last else 0.0)
                src = dst

    def loss_terms(self):
        """[total, graph, text, image] of the last rec_step (device tensor)."""
        return self._w["loss"]

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward(self, adj=None):
        """(ua, ia) of freedom.py:164-178 on adj (default: the pruned graph of this epoch)."""
        if adj is None:
            if self.masked_adj is None:
                self.pre_epoch_processing()
            adj = self.masked_adj
        self._forward(adj, self._eval)
        return self._eval[:self.n_users], self._eval[self.n_users:]

    @torch.no_grad()
    def forward_embeddings(self):
        """full_sort_predict's tables (freedom.py:212-216): forward on norm_adj, the unpruned graph."""
        return self.forward(self.norm_adj)
