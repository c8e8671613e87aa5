"""LATTICE on MI355X — drop-in for models/lattice.py of the reference (GeneralRecommender API).

The item-item graph is learned: at the first step of every epoch it is rebuilt from the projected features and the
loss gradient flows through it into image_trs, text_trs, modal_weight and the trainable feature tables; in the other
steps of the epoch it is the one built at the epoch's first step and a constant.  What it computes:

Init (the constructor's order)
  nn.Embedding(U, 64), nn.Embedding(I, 64) draw their normal init, then xavier_uniform_ on the user table, then the
  item table; the feature tables draw nothing and are trainable; image_trs = nn.Linear(Dv, 64), text_trs =
  nn.Linear(Dt, 64); modal_weight = [0.5, 0.5].  named_parameters() lists modal_weight first (the module's own
  parameter), then the submodules in this order.

Graphs
  adj     D^-1 (A + I) over the U + I nodes: row-normalised, with self loops, not symmetric; adj^T beside it.
  O_m     per modality, frozen: cosine similarity of the raw features, the knn_k largest per row (the row itself among
          them) kept with their values, w_ij / sqrt(rowsum_i rowsum_j); kept as its I x k lists.  No cache file.
  learned F_m = trs_m(emb_m), n_m = rows of F_m over their norms, idx_m = the top-k of n_m n_m^T,
          v_m[i, slot] = <n_i, n_j>, a = w_0 v_img + w_1 v_txt with w = softmax(modal_weight), r = row sums of a,
          s = r^-1/2 (0 where r = 0), L_ij = s_i a_ij s_j.  One modality: no w.
  item_adj = (1 - lambda) L + lambda (w_0 O_img + w_1 O_txt), stored with R = 2 M k slots per row: the learned lists of
          each modality, then the original lists.  A column may sit in several slots of a row; the products are linear
          in the slots, so the duplicates add and no union is formed.

forward   h = item_adj^n E_item;  ia = mean_k(E_k)[items] + F.normalize(h);  ua = mean_k(E_k)[users], E_k+1 = adj E_k
          over n_ui_layers = len(weight_size) layers (cf_model mf: E_0 alone)
loss      mean(-logsigmoid(<u,p> - <u,n>)) + reg_weight 0.5 (|u|^2 + |p|^2 + |n|^2) / train_batch_size on the gathered
          propagated rows (the divisor is the configured batch size, also in a short last batch)

On the device
  Two slabs: E ((U + I) x 64), and the graph side (feature tables, projections, modal_weight).  The graph slab is
  marked has_grad = False on the frozen steps, where the reference leaves .grad = None and Adam skips the parameters.
  build      two GEMMs (BIAS epilogue), normalize_rows, the similarity GEMM in row chunks + gmr_topk_rows_f32 per
             modality; gmr_lat_edge_fwd (v, r, s), gmr_lat_adj_fwd (the I x R values).  The forward CSR is wrapped once
             (rowptr[i] = i R; its plan depends on the row pointer alone) and its columns and values are rewritten in
             place.  The transpose and the incoming lists come from a stable sort of the columns (K.csr_transpose
             ranks equal columns of a row into one place, so it cannot take the duplicates).
  step       n SpMMs on item_adj, normalize_rows, the LightGCN layers, gmr_frd_mean_fwd; gmr_mgcn_bpr_reg_fwd_bwd and
             gmr_mgcn_loss_reduce (MGCN's loss is these two terms plus the InfoNCE rows, which are zero here); one
             sorted scatter; normalize_rows_bwd -> dh; (item_adj^T)^n into dE_item; the Horner chain on adj^T
  build step also  dA = sum_l <g_l[i], h_(l-1)[col]> on the pattern (gmr_lat_sddmm), gmr_lat_bwd_ds / _da /
             _dw_reduce / _dn, normalize_rows_bwd and the projection backward per modality.  Nothing I x I is formed.
  A frozen step issues n SpMMs forward and n backward for the item graph, as FREEDOM's mm_adj path.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, copy64, r4, sort_plan
from .freedom import KNN_SIM_FLOATS, _Linear, _Table
from .kernels import ptr, stream
from .mgcn import knn_graph
from .slab import Slab

D = 64
MAX_TABLES = 8  # GMR_FRD_MAX_LAYERS of include/gmr.h: the layer mean takes n_ui_layers + 1 tables
MAX_K = 64      # gmr_topk_rows_f32


def topk_normalised(fn, k, out):
    """Per-row top-k indices of fn fn^T for row-normalised fn (n x 64), the similarity in row chunks of at most
    KNN_SIM_FLOATS floats (as freedom.knn_topk)."""
    n = fn.shape[0]
    ldn = r4(n)
    chunk = max(1, min(n, KNN_SIM_FLOATS // ldn))
    sim = torch.empty((chunk, ldn), dtype=torch.float32, device=fn.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        s = sim[:hi - lo, :n]
        K.gemm(fn[lo:hi], fn, s, trans_b=True)
        K.topk_rows(s, k, out[lo:hi])
    return out


def ui_rownorm(U, I, user_ptr, user_items):
    """D^-1 (A + I) over the U + I nodes (lattice.py:100-122) as a CSR with ascending columns, in torch on the
    device."""
    dev = user_ptr.device
    N = U + I
    deg = (user_ptr[1:] - user_ptr[:-1]).long()
    u = torch.repeat_interleave(torch.arange(U, device=dev), deg)
    it = user_items.long() + U
    loop = torch.arange(N, device=dev)
    rows, cols = torch.cat([u, it, loop]), torch.cat([it, u, loop])
    order = torch.argsort(rows * N + cols)
    rows, cols = rows[order], cols[order]
    cnt = torch.bincount(rows, minlength=N)
    rp = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    rp[1:] = torch.cumsum(cnt, 0).to(torch.int32)
    val = (1.0 / cnt.double())[rows].float()
    return K.CSR(rp, cols.to(torch.int32).contiguous(), val.contiguous(), symmetric=False)


def incoming_lists(col, M, k):
    """The incoming lists of the learned edges from their columns (I x M k, any row stride): in_edge, the edge ids
    i M k + q sorted stably by the key m I + col, and in_ptr (M I + 1), the row pointer over the keys.  Item i's edges of
    modality m are in_edge[in_ptr[m I + i]:in_ptr[m I + i + 1]], in ascending edge id."""
    I, dev = col.shape[0], col.device
    keys = (col.reshape(I, M, k).long() + (torch.arange(M, device=dev) * I)[None, :, None]).reshape(-1)
    sk, perm = torch.sort(keys, stable=True)
    in_ptr = torch.zeros(M * I + 1, dtype=torch.int32, device=dev)
    in_ptr[1:] = torch.cumsum(torch.bincount(sk, minlength=M * I), 0).to(torch.int32)
    return in_ptr, perm.to(torch.int32)


class ItemGraph:
    """One item_adj in its fixed-width slot form and what its backward reads."""

    def __init__(self, I, M, k, ocol, dev):
        Mk, R = M * k, 2 * M * k
        self.col = torch.zeros((I, R), dtype=torch.int32, device=dev)
        self.col[:, Mk:] = ocol                       # the original lists' columns, once
        self.val = torch.zeros((I, R), dtype=torch.float32, device=dev)
        self.v = torch.zeros((I, Mk), dtype=torch.float32, device=dev)
        self.r = torch.zeros(I, dtype=torch.float32, device=dev)
        self.s = torch.zeros(I, dtype=torch.float32, device=dev)
        rp = (torch.arange(I + 1, device=dev) * R).to(torch.int32)
        # the plan is built from the row pointer; col / val are read at every product
        self.csr = K.CSR(rp, self.col.view(-1), self.val.view(-1), n_cols=I, symmetric=False)
        self.csr_t = None
        self.in_ptr = self.in_edge = None

    def build_transpose(self, M, k):
        """item_adj^T as a CSR and the incoming lists of the learned edges, both from stable sorts of the columns:
        equal keys keep the order of their edge ids, so the lists are the same in every run."""
        I, R = self.col.shape
        Mk, dev = M * k, self.col.device
        flat = self.col.reshape(-1).long()
        sc, perm = torch.sort(flat, stable=True)
        trp = torch.zeros(I + 1, dtype=torch.int32, device=dev)
        trp[1:] = torch.cumsum(torch.bincount(sc, minlength=I), 0).to(torch.int32)
        self.csr_t = K.CSR(trp, (perm // R).to(torch.int32), self.val.reshape(-1)[perm], n_cols=I, symmetric=False)
        self.in_ptr, self.in_edge = incoming_lists(self.col[:, :Mk], M, k)


class LATTICE(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        if dist.world() > 1:
            raise NotImplementedError("world size > 1: LATTICE runs on one device")
        if int(c["embedding_size"] or D) != D or int(c["feat_embed_dim"] or D) != D:
            raise NotImplementedError("embedding_size = feat_embed_dim = 64 (LATTICE.yaml): the SpMM blocks and the "
                                      "row kernels are 64 columns")
        self.cf_model = str(c["cf_model"] or "lightgcn")
        if self.cf_model == "ngcf":
            raise NotImplementedError("cf_model = ngcf is not on the hot path: lightgcn or mf")
        if self.cf_model not in ("lightgcn", "mf"):
            raise ValueError(f"cf_model = {self.cf_model}: lightgcn or mf")
        self.embedding_dim = self.feat_embed_dim = D
        self.n_ui_layers = len(c["weight_size"] or [])
        if self.n_ui_layers + 1 > MAX_TABLES:
            raise NotImplementedError(f"weight_size of {self.n_ui_layers} layers: 0..{MAX_TABLES - 1}")
        self.n_layers = int(c["n_layers"])
        if self.n_layers < 1:
            raise NotImplementedError(f"n_layers = {self.n_layers}: >= 1 (without a product the item graph is unused)")
        self.knn_k = int(c["knn_k"])
        if not 1 <= self.knn_k <= min(MAX_K, self.n_items):
            raise NotImplementedError(f"knn_k = {self.knn_k}: 1..{min(MAX_K, self.n_items)} (gmr_topk_rows_f32 keeps "
                                      f"up to {MAX_K}; at most the number of items)")
        self.lambda_coeff = float(c["lambda_coeff"])
        self.reg_weight = float(c["reg_weight"])
        self.batch_size = int(c["train_batch_size"])
        U, I, dev, k = self.n_users, self.n_items, self.device, self.knn_k
        N = self.N = U + I
        # parameters in the reference's RNG order (lattice.py:48-94)
        e_u, e_i = nn.Embedding(U, D), nn.Embedding(I, D)
        nn.init.xavier_uniform_(e_u.weight)
        nn.init.xavier_uniform_(e_i.weight)
        self.mods = [(name, feat) for name, feat in (("image", self.v_feat), ("text", self.t_feat)) if feat is not None]
        M = self.M = len(self.mods)
        trs = {name: nn.Linear(feat.shape[1], D) for name, feat in self.mods}
        self.slab = Slab([("E", (N, D), None)], dev)
        gspecs = [(name + "_embedding", (I, feat.shape[1]), r4(feat.shape[1])) for name, feat in self.mods]
        for name, feat in self.mods:
            gspecs += [(name + "_W", (D, feat.shape[1]), r4(feat.shape[1])), (name + "_b", (D,), None)]
        gspecs.append(("modal_weight", (2,), None))
        s, gs = self.slab, Slab(gspecs, dev)
        self.gslab = gs
        with torch.no_grad():
            s.view("E")[:U].copy_(e_u.weight)
            s.view("E")[U:].copy_(e_i.weight)
            for name, feat in self.mods:
                gs.load(name + "_embedding", feat)
                gs.load(name + "_W", trs[name].weight)
                gs.load(name + "_b", trs[name].bias)
            gs.view("modal_weight").fill_(0.5)
        # registered as the reference registers them: the module's own parameter, then the submodules in order
        e, ge = s.view("E"), s.gview("E")
        self.user_embedding = _Table(nn.Parameter(e[:U]))
        self.user_embedding.weight.grad = ge[:U]
        self.item_id_embedding = _Table(nn.Parameter(e[U:]))
        self.item_id_embedding.weight.grad = ge[U:]
        for name, _ in self.mods:
            setattr(self, name + "_embedding", _Table(gs.parameter(name + "_embedding")))
        for name, _ in self.mods:
            setattr(self, name + "_trs", _Linear(gs.parameter(name + "_W"), gs.parameter(name + "_b")))
        self.modal_weight = gs.parameter("modal_weight")
        # graphs
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        self.norm_adj = ui_rownorm(U, I, self.user_ptr, self.user_items)
        self.norm_adj_t = K.csr_transpose(self.norm_adj)
        Mk = M * k
        self.ocol = torch.empty((I, Mk), dtype=torch.int32, device=dev)
        self.oval = torch.empty((I, Mk), dtype=torch.float32, device=dev)
        for m, (name, feat) in enumerate(self.mods):
            g = knn_graph(feat, k)  # rowptr[i] = i k: col / val are the I x k lists in top-k order
            self.ocol[:, m * k:(m + 1) * k] = g.col.view(I, k)
            self.oval[:, m * k:(m + 1) * k] = g.val.view(I, k)
        self.graph = ItemGraph(I, M, k, self.ocol, dev)       # the training graph of this epoch
        self.eval_graph = ItemGraph(I, M, k, self.ocol, dev)  # full_sort_predict builds its own
        self.build_item_graph = True
        # work buffers
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.feats, self.nfeat, self.fnrm = f(I, M * D), f(I, M * D), f(M, I)
        self.idx = torch.zeros((M, I, k), dtype=torch.int32, device=dev)
        self._h = [f(I, D) for _ in range(self.n_layers)]
        self._g = [f(I, D) for _ in range(self.n_layers)]          # g_n = dh, ..., g_1
        self.hn, self.hnrm = f(I, D), f(I)
        L = self.n_ui_layers if self.cf_model == "lightgcn" else 0
        self._L = L
        self._layers = [f(N, D) for _ in range(L)]
        self._t = [f(N, D) for _ in range(2)] if L > 1 else []
        self.tab, self.gtab, self._eval = f(N, D), f(N, D), f(N, D)
        self.dA, self.dr, self.dv, self.parts = f(I, 2 * Mk), f(I), f(I, Mk), f(I, 2)
        self.dn, self.dfeat = f(I, M * D), f(I, M * D)
        self._loss = f(5)
        self._w = None

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab, self.gslab]

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order (zero on the graph side in a frozen step, where
        the reference has .grad = None)."""
        s, gs, U = self.slab, self.gslab, self.n_users
        out = [gs.gview("modal_weight"), s.gview("E")[:U], s.gview("E")[U:]]
        out += [gs.gview(name + "_embedding") for name, _ in self.mods]
        for name, _ in self.mods:
            out += [gs.gview(name + "_W"), gs.gview(name + "_b")]
        return out

    def pre_epoch_processing(self):
        self.build_item_graph = True

    # ------------------------------------------------------------------ the item graph
    def _mw(self):
        return self.gslab.view("modal_weight") if self.M == 2 else None

    def _nf(self, m, buf=None):
        return (self.nfeat if buf is None else buf)[:, D * m:D * m + D]

    def _build(self, G):
        """lattice.py:133-157 into G: the projections, their normalised rows and top-k lists, then the edge values,
        the row scales and the I x R values of item_adj."""
        gs, I, k, M = self.gslab, self.n_items, self.knn_k, self.M
        for m, (name, _) in enumerate(self.mods):
            Fm = self._nf(m, self.feats)
            K.gemm(gs.view(name + "_embedding"), gs.view(name + "_W"), Fm, trans_b=True, epi=K.EPI_BIAS,
                   bias=gs.view(name + "_b"))
            K.normalize_rows(Fm, self._nf(m), self.fnrm[m])
            topk_normalised(self._nf(m), k, self.idx[m])
        n0, n1 = self._nf(0), self._nf(M - 1)
        _lib.call("gmr_lat_edge_fwd", I, k, M, ptr(n0), n0.stride(0), ptr(self.idx[0]), k, ptr(n1), n1.stride(0),
                  ptr(self.idx[M - 1]), k, ptr(self._mw()), ptr(G.v), ptr(G.col), G.col.stride(0), ptr(G.r), ptr(G.s),
                  stream())
        _lib.call("gmr_lat_adj_fwd", I, k, M, ptr(G.v), ptr(G.s), ptr(G.col), G.col.stride(0), ptr(self.oval),
                  ptr(self._mw()), self.lambda_coeff, ptr(G.val), stream())

    def _graph_backward(self, G):
        """The gradients of the graph slab from g_l (self._g) and h_(l-1) of this step's products."""
        gs, U, I, k, M, n = self.gslab, self.n_users, self.n_items, self.knn_k, self.M, self.n_layers
        R, lam, ldc = 2 * M * k, self.lambda_coeff, G.col.stride(0)
        hs = [self.slab.view("E")[U:]] + self._h[:n - 1]
        for l in range(n):  # g_(l+1) with h_l; self._g[0] is g_n
            g, h = self._g[n - 1 - l], hs[l]
            _lib.call("gmr_lat_sddmm", I, R, ptr(G.col), ldc, ptr(g), g.stride(0), ptr(h), h.stride(0), int(l > 0),
                      ptr(self.dA), stream())
        mw = self._mw()
        _lib.call("gmr_lat_bwd_ds", I, k, M, ptr(self.dA), ptr(G.v), ptr(G.r), ptr(G.s), ptr(G.col), ldc,
                  ptr(G.in_ptr), ptr(G.in_edge), ptr(mw), lam, ptr(self.dr), stream())
        _lib.call("gmr_lat_bwd_da", I, k, M, ptr(self.dA), ptr(G.v), ptr(G.s), ptr(self.dr), ptr(G.col), ldc,
                  ptr(self.oval), ptr(mw), lam, ptr(self.dv), ptr(self.parts), stream())
        if M == 2:
            _lib.call("gmr_lat_dw_reduce", I, ptr(self.parts), ptr(mw), ptr(gs.gview("modal_weight")), stream())
        n0, n1 = self._nf(0), self._nf(M - 1)
        d0, d1 = self._nf(0, self.dn), self._nf(M - 1, self.dn)
        _lib.call("gmr_lat_bwd_dn", I, k, M, ptr(self.dv), ptr(n0), n0.stride(0), ptr(n1), n1.stride(0), ptr(G.col), ldc,
                  ptr(G.in_ptr), ptr(G.in_edge), ptr(d0), d0.stride(0), ptr(d1), d1.stride(0), stream())
        for m, (name, _) in enumerate(self.mods):
            dF = self._nf(m, self.dfeat)
            K.normalize_rows_bwd(self._nf(m), self.fnrm[m], self._nf(m, self.dn), dF)
            K.gemm(dF, gs.view(name + "_embedding"), gs.gview(name + "_W"), trans_a=True)   # dW = dF^T raw
            K.colsum(dF, gs.gview(name + "_b"))                                              # db
            K.gemm(dF, gs.view(name + "_W"), gs.gview(name + "_embedding"))                  # draw = dF W

    # ------------------------------------------------------------------ forward
    def _forward(self, G, out):
        """lattice.py:161-197 into out (N x 64): mean of E_0..E_L, + F.normalize(item_adj^n E_item) on the item
        rows."""
        U, N = self.n_users, self.N
        E = self.slab.view("E")
        src = E[U:]
        for i in range(self.n_layers):
            G.csr.spmm(self._h[i], [(src,)])
            src = self._h[i]
        K.normalize_rows(src, self.hn, self.hnrm)
        tabs = [E]
        for i in range(self._L):
            self.norm_adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", N, U, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), ptr(self.hn), D, ptr(out), out.stride(0),
                  stream())

    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev = self.device
            self._w = {"B": B, "terms": torch.zeros(4 * B, dtype=torch.float32, device=dev),
                       "contrib": torch.empty((3 * B, D), dtype=torch.float32, device=dev)}
        return self._w

    def _plan(self, users, pos, neg):
        return sort_plan((users, pos, neg), (0, self.n_users, self.n_users))

    # ------------------------------------------------------------------ the step
    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0):
        """calculate_loss (lattice.py:213-227) and all parameter gradients (into the slabs' twins).  The first call
        after pre_epoch_processing() rebuilds the item graph and differentiates through it; the others leave the
        graph slab without a gradient (has_grad = False).  Returns the loss as a device scalar; loss_terms() reads
        [total, bpr, reg, 0, 0]."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: LATTICE runs on one device")
        B = users.numel()
        if plan_bpr is None:
            plan_bpr = self._plan(users, pos, neg)
        w = self._work(B)
        build, G = self.build_item_graph, self.graph
        if build:
            self._build(G)
            G.build_transpose(self.M, self.knn_k)
            self.build_item_graph = False
        elif self.gslab.has_grad:
            self.gslab.zero_grad()  # once, at the first frozen step after a build
        self.gslab.has_grad = build
        self._forward(G, self.tab)
        inv_norm = 1.0 / (norm_rows or B)
        terms = w["terms"][:4 * B]
        if w["B"] != B:
            K.zero_(terms)  # the two InfoNCE rows of gmr_mgcn_loss_reduce: none here
        _lib.call("gmr_mgcn_bpr_reg_fwd_bwd", B, self.n_users, ptr(self.tab), D, ptr(users), ptr(pos), ptr(neg),
                  float(inv_norm), self.reg_weight, float(self.batch_size), ptr(terms), ptr(w["contrib"]), D, stream())
        _lib.call("gmr_mgcn_loss_reduce", B, ptr(terms), float(inv_norm), self.reg_weight, float(self.batch_size), 0.0,
                  ptr(self._loss), stream())
        self._backward(G, plan_bpr, w, build)
        return self._loss[0]

    def _backward(self, G, plan_bpr, w, build):
        U, L, n = self.n_users, self._L, self.n_layers
        s, gtab, adj_t = self.slab, self.gtab, self.norm_adj_t
        s.zero_grad()
        K.zero_(gtab)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), D, ptr(plan_bpr), ptr(w["contrib"]), D, ptr(gtab), D,
                  stream())
        # dE = (1 / (L + 1)) sum_k (adj^T)^k g: t <- g; L times t <- adj^T t + g; the last one scaled
        g, gE = gtab, s.gview("E")
        copy64(g, gE)
        src = g
        for i in range(L):
            last = i == L - 1
            dst = gE if last else self._t[i % 2]
            if not last:
                copy64(g, dst)
            sc = 1.0 / (L + 1) if last else 1.0
            adj_t.spmm(dst, [(src,)], alpha=sc, beta=sc)
            src = dst
        # ia = mean + F.normalize(h): dh, then g_(l-1) = item_adj^T g_l, the last one onto the item embeddings
        K.normalize_rows_bwd(self.hn, self.hnrm, g[U:], self._g[0])
        for i in range(n):
            last = i == n - 1
            dst = gE[U:] if last else self._g[i + 1]
            G.csr_t.spmm(dst, [(self._g[i],)], beta=1.0 if last else 0.0)
        if build:
            self.gslab.zero_grad()
            self._graph_backward(G)

    def loss_terms(self):
        """[total, bpr, reg, 0, 0] of the last rec_step (device tensor)."""
        return self._loss

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward_embeddings(self):
        """full_sort_predict's tables (lattice.py:229-237): forward on a graph built from the current parameters; the
        training graph of the epoch is left as it is."""
        self._build(self.eval_graph)
        self._forward(self.eval_graph, self._eval)
        return self._eval[:self.n_users], self._eval[self.n_users:]
