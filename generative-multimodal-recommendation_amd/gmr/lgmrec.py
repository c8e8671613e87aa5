"""LGMRec on MI355X — drop-in for models/lgmrec.py of the reference (GeneralRecommender API).

Local and global graph learning: a LightGCN pass over the user-item graph (the collaborative view, cge), each modality's
projected features propagated over the same graph (the modal views, mge), and a global hypergraph embedding (ghe): every
item is assigned softly to H learned hyperedges per modality by a Gumbel-softmax, every user by the sum of its items'
logits, and the item embeddings travel through the hyperedges to items and users.  What it computes:

Init (the constructor's RNG order)
  nn.Embedding(U, 64), nn.Embedding(I, 64), then xavier_uniform_ on the user table, then the item table; per modality
  (image first) item_<m>_trs = xavier_uniform_(D_m x 64), then <m>_hyper = xavier_uniform_(D_m x H).  The four
  projections are the module's own parameters, so named_parameters() lists them first; the feature tables are frozen.
  Both modalities are required.

Graphs
  adj       the raw U x I 0/1 interaction matrix.
  norm_adj  D^-1/2 A D^-1/2 of the bipartite graph with D = degree + 1e-7, no self loops.
  inv_deg   1 / (user degree + 1e-7), fp32 of the double value.

forward, per modality m in {v, t} with features X_m (I x D_m), W_m (D_m x 64), Hy_m (D_m x H), tau = 0.2
  Li_m = X_m Hy_m,  Lu_m = adj Li_m                                              a sum, not a mean
  S = softmax((L + g) / tau) per row, g ~ Gumbel(0, 1) drawn independently for Li and Lu (also in evaluation)
  h = dropout(S, p = 1 - keep_rate)                                              training only; hi_m, hu_m
  cge = mean(E_0 .. E_n), E_k+1 = norm_adj E_k (n = n_ui_layers; cf_model 'mf': cge = E)
  F_m = X_m W_m;  mge_m = norm_adj^n_mm [inv_deg * (adj F_m); F_m]               only the last hop is kept
  E_i = cge's item rows, i_0 = E_i;  for l = 1..L (n_hyper_layer): lat_m = hi_m^T i_(l-1), i_l = hi_m lat_m
  i_m = i_L,  u_m = hu_m lat_m (the last lat);  ghe = [u_v + u_t; i_v + i_t]
  all = cge + n(mge_v) + n(mge_t) + alpha n(ghe),  n(x) = x / max(|x|_2, 1e-12) per row

calculate_loss(users, pos, neg)   (B rows, duplicates kept)
  u, p, n = all[users], all[U + pos], all[U + neg]
  loss = -mean logsigmoid(<u,p> - <u,n>) + cl_weight (T(u_v[users], u_t[users], u_t) + T(i_v[pos], i_t[pos], i_t))
         + reg_weight (|u|_F + |p|_F + |n|_F) / B
  T(a, b, all) = sum_i (log sum_j exp(<n(a_i), n(all_j)> / 0.2) - <n(a_i), n(b_i)> / 0.2): summed over the batch, the
  positive counted again inside the table sum.

full_sort_predict(users)   forward (fresh Gumbel draws, no dropout), scores = all_u[users] all_i^T

On the device
  One Slab holds E and, per modality, Wcat_m = [W_m | Hy_m] (D_m x (64 + H)): the four parameters are column-block
  views of the two, so each feature matrix is read once per direction.  A step:
    forward    one GEMM per modality into P_m = X_m Wcat_m = [F_m | Li_m]; gmr_lgm_hyper_fwd (all N rows, both
               modalities: the user rows' CSR sums, the draws from Philox keyed on (seed, site, step counter, row,
               column) unless injected, softmax, dropout; S and h kept); the LightGCN layers and gmr_frd_mean_fwd into
               cge; one SpMM into mge's user rows and n_mm 128-wide SpMMs; gmr_lgm_lat per hyper layer (layers l > 1
               loop: gmr_lgm_apply then gmr_lgm_lat again); gmr_lgm_combine_fwd (all, the [n(x_v) | n(x_t)] table)
    loss       gmr_bpr_logsigmoid_f32, gmr_lgm_reg, two gmr_contrast_fused_nbwd_f32 passes (coef = cl_weight) and
               gmr_scatter_sorted_nbwd_f32 into dK = [d x_v | d x_t]
    backward   sorted scatter of the BPR rows into dall; gmr_lgm_combine_bwd; d lat = h^T dK over all N rows
               (gmr_lgm_lat); the item rows' d hi terms of the layer loop (gmr_lgm_dh, gmr_lgm_apply, gmr_lgm_lat);
               gmr_lgm_dh over N rows through the dropout and softmax backward to d L; d E_i = hi d lat_1 added to d cge
               (gmr_lgm_apply); gmr_lgm_logit_bwd carries the users' d Lu to the items; the mge chain backwards; one
               GEMM X_m^T [d F_m | d Li_m] per modality; the LightGCN Horner chain
  No host read inside a step.  The Philox counters (training step, evaluation pass) travel in extra_state().
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, config_seed, copy64, r4
from .freedom import _Table
from .kernels import ptr, stream
from .mgcn import MAX_TABLES, MGCN
from .slab import Slab

D = 64
MAX_H = 64
TAU = 0.2
EVAL_STEP0 = 1 << 40  # evaluation passes draw on Philox steps of their own


def check_config(config, has=(True, True)):
    """Raise NotImplementedError naming the key for settings outside the hot path; returns (cf_model, n_ui_layers,
    n_mm_layers, n_hyper_layer, hyper_num, keep_rate)."""
    c = config
    for key in ("embedding_size", "feat_embed_dim"):
        if int(c[key] or D) != D:
            raise NotImplementedError(f"{key} = {c[key]}: {D} (the SpMM blocks and the row kernels are 64 columns)")
    cf = c["cf_model"] or "lightgcn"
    if cf not in ("lightgcn", "mf"):
        raise NotImplementedError(f"cf_model = {cf}: 'lightgcn' or 'mf'")
    L = int(c["n_ui_layers"])
    if L < 0 or L + 1 > MAX_TABLES:
        raise NotImplementedError(f"n_ui_layers = {L}: 0..{MAX_TABLES - 1}")
    n_mm = int(c["n_mm_layers"])
    if n_mm < 0:
        raise NotImplementedError(f"n_mm_layers = {n_mm}: >= 0")
    n_hyper = int(c["n_hyper_layer"])
    if n_hyper < 1:
        raise NotImplementedError(f"n_hyper_layer = {n_hyper}: >= 1")
    H = int(c["hyper_num"])
    if not 1 <= H <= MAX_H:
        raise NotImplementedError(f"hyper_num = {H}: 1..{MAX_H}")
    keep = float(c["keep_rate"] if c["keep_rate"] is not None else 1.0)
    if not 0.0 < keep <= 1.0:
        raise NotImplementedError(f"keep_rate = {keep}: 0 < keep_rate <= 1")
    for name, h in zip(("image", "text"), has):
        if not h:
            raise NotImplementedError(f"{name} features are missing: LGMRec's hypergraph and modal views use both "
                                      f"modalities")
    if dist.world() > 1:
        raise NotImplementedError("world size > 1: the contrastive terms are over the global batch; LGMRec runs on "
                                  "one device")
    return cf, L, n_mm, n_hyper, H, keep


def symnorm_graph(n_users, n_items, user_ptr, user_items):
    """norm_adj (lgmrec.py:70-86): the pattern from gmr_bipartite_symnorm_build, the values as the reference rounds
    them: d = (degree + 1e-7)^-1/2 in double, the product d_row d_col in double, one rounding to fp32.  Once, at
    construction (K.bipartite_symnorm with the values replaced before the plans pack them)."""
    lib = _lib.load()
    dev = user_ptr.device
    n_ui = user_items.numel()
    nnz = lib.gmr_bipartite_nnz(n_users, n_items, n_ui, 0)
    N = n_users + n_items
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.gmr_bipartite_workspace_ints(n_users, n_items), dtype=torch.int32, device=dev)
    _lib.call("gmr_bipartite_symnorm_build", n_users, n_items, ptr(user_ptr), ptr(user_items), n_ui, 0, 1e-7, ptr(ws),
              ptr(rowptr), ptr(col), ptr(val), stream())
    rp, cl = rowptr.cpu().numpy().astype(np.int64), col[:nnz].cpu().numpy().astype(np.int64)
    deg = np.diff(rp).astype(np.float64)
    d = np.power(deg + 1e-7, -0.5)
    rows = np.repeat(np.arange(N), np.diff(rp))
    val[:nnz].copy_(torch.as_tensor((d[rows] * d[cl]).astype(np.float32)))
    return K.CSR(rowptr, col[:nnz], val[:nnz], class_split=n_users, side=True)


class LGMRec(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        (self.cf_model, self.n_ui_layers, self.n_mm_layers, self.n_hyper_layer, self.hyper_num,
         self.keep_rate) = check_config(c, (self.v_feat is not None, self.t_feat is not None))
        self.embedding_dim = D
        self.alpha, self.cl_weight, self.reg_weight = float(c["alpha"]), float(c["cl_weight"]), float(c["reg_weight"])
        self.tau = TAU
        self.seed = config_seed(c)
        U, I, dev, H = self.n_users, self.n_items, self.device, self.hyper_num
        N = self.N = U + I
        PW = self.PW = r4(D + H)  # row stride of [F_m | Li_m] and of Wcat_m
        # parameters in the reference's RNG order (lgmrec.py:46-61)
        e_u, e_i = nn.Embedding(U, D), nn.Embedding(I, D)
        nn.init.xavier_uniform_(e_u.weight)
        nn.init.xavier_uniform_(e_i.weight)
        self.mods = (("v", "image", self.v_feat), ("t", "text", self.t_feat))
        init = {}
        for m, _, feat in self.mods:
            d = feat.shape[1]
            init[m] = (nn.init.xavier_uniform_(torch.zeros(d, D)), nn.init.xavier_uniform_(torch.zeros(d, H)))
        specs = [("E", (N, D), None)] + [("Wcat_" + m, (feat.shape[1], D + H), PW) for m, _, feat in self.mods]
        s = self.slab = Slab(specs, dev)
        with torch.no_grad():
            s.view("E")[:U].copy_(e_u.weight)
            s.view("E")[U:].copy_(e_i.weight)
            for m, _, _ in self.mods:
                s.view("Wcat_" + m)[:, :D].copy_(init[m][0])
                s.view("Wcat_" + m)[:, D:].copy_(init[m][1])

        def block(name, lo, hi):
            p = nn.Parameter(s.view(name)[:, lo:hi])
            p.grad = s.gview(name)[:, lo:hi]
            return p

        # the module's own parameters first, then the tables, under the reference's names in its order
        self.item_image_trs, self.v_hyper = block("Wcat_v", 0, D), block("Wcat_v", D, D + H)
        self.item_text_trs, self.t_hyper = block("Wcat_t", 0, D), block("Wcat_t", D, D + H)
        e, ge = s.view("E"), s.gview("E")
        self.user_embedding = _Table(nn.Parameter(e[:U]))
        self.user_embedding.weight.grad = ge[:U]
        self.item_id_embedding = _Table(nn.Parameter(e[U:]))
        self.item_id_embedding.weight.grad = ge[U:]
        self.feat = {}
        for m, name, feat in self.mods:  # frozen, rows padded to 16 bytes
            buf = torch.zeros((I, r4(feat.shape[1])), dtype=torch.float32, device=dev)
            buf[:, :feat.shape[1]].copy_(feat)
            self.feat[m] = buf[:, :feat.shape[1]]
            setattr(self, name + "_embedding", _Table(nn.Parameter(self.feat[m], requires_grad=False)))
        # graphs
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        self.norm_adj = symnorm_graph(U, I, self.user_ptr, self.user_items)
        self.adj = K.user_item_csr(U, I, self.user_ptr, self.user_items)
        self.adj_t = K.csr_transpose(self.adj)
        deg = np.diff(np.asarray(tl.uptr_np, np.int64)).astype(np.float64)
        self.inv_deg = torch.as_tensor((1.0 / (deg + 1e-7)).astype(np.float32)).to(dev)
        # the user mean of the modal views: adj with inv_deg on every entry of the user's row, and its transpose
        val = torch.repeat_interleave(self.inv_deg, torch.as_tensor(np.diff(np.asarray(tl.uptr_np, np.int64))).to(dev))
        self.adj_mean = K.CSR(self.user_ptr, self.user_items, val.contiguous(), n_cols=I, symmetric=False)
        self.adj_mean_t = K.csr_transpose(self.adj_mean)
        # work buffers
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.proj = {m: f(I, PW) for m, _, _ in self.mods}       # [F_m | Li_m]
        self.dproj = {m: f(I, PW) for m, _, _ in self.mods}      # [d F_m | d Li_m]
        self.S, self.h, self.dL, self.acc = f(N, 2 * H), f(N, 2 * H), f(N, 2 * H), f(N, 2 * H)
        self.cge = f(N, D) if self.cf_model == "lightgcn" else None
        self._layers = [f(N, D) for _ in range(self.n_ui_layers)] if self.cf_model == "lightgcn" else []
        self._t = [f(N, D) for _ in range(2)]
        self.mge_u = f(U, 2 * D)
        self._mm = [f(N, 2 * D) for _ in range(min(self.n_mm_layers, 2))]
        self.mge0 = f(N, 2 * D) if self.n_mm_layers == 0 else None
        self.lats = [f(2, H, D) for _ in range(self.n_hyper_layer)]
        self.dlat = [f(2, H, D) for _ in range(2)]
        self.ilay = [f(I, 2 * D) for _ in range(self.n_hyper_layer - 1)]
        self.di = f(I, 2 * D) if self.n_hyper_layer > 1 else None
        self.all, self.CLN, self.nrmCL, self.nrm3 = f(N, D), f(N, 2 * D), f(2, N), f(3, N)
        self.dall, self.dK, self.dmge = f(N, D), f(N, 2 * D), f(N, 2 * D)
        self._ws = f(int(_lib.load().gmr_lgm_lat_ws_floats(N, H)))
        self._loss = f(5)
        self._w = None
        self._step = 0
        self._eval_pass = 0
        self._p_used = 1.0   # the keep rate of the last forward (1 in evaluation)

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def _params(self):
        return [p for p in self.parameters() if p.requires_grad]

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order (the trainable ones)."""
        s, U, H = self.slab, self.n_users, self.hyper_num
        gv, gt, ge = s.gview("Wcat_v"), s.gview("Wcat_t"), s.gview("E")
        return [gv[:, :D], gv[:, D:D + H], gt[:, :D], gt[:, D:D + H], ge[:U], ge[U:]]

    def extra_state(self):
        """The Philox counters: a resumed run draws what the uninterrupted one would."""
        return {"counters": {"step": int(self._step), "eval_pass": int(self._eval_pass)}}

    def load_extra_state(self, st):
        self._step = int(st["counters"]["step"])
        self._eval_pass = int(st["counters"].get("eval_pass", 0))

    # ------------------------------------------------------------------ forward
    def _cge(self):
        E = self.slab.view("E")
        if self.cf_model == "mf":
            return E
        tabs = [E]
        for i in range(self.n_ui_layers):
            self.norm_adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", self.N, self.N, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(self.cge), D, stream())
        return self.cge

    def _lat(self, n, A, Xv, Xt, out):
        _lib.call("gmr_lgm_lat", n, ptr(A), A.stride(0), self.hyper_num, ptr(Xv), ptr(Xt), Xv.stride(0), ptr(self._ws),
                  self._ws.numel(), 0, ptr(out), stream())

    def _apply(self, A, M, Y, mode):
        _lib.call("gmr_lgm_apply", A.shape[0], ptr(A), A.stride(0), self.hyper_num, ptr(M), ptr(Y), Y.stride(0), mode,
                  0, stream())

    def _dh(self, Xv, Xt, M, out, acc=None, sbwd=False):
        S, h = (self.S, self.h) if sbwd else (None, None)
        _lib.call("gmr_lgm_dh", out.shape[0], ptr(Xv), ptr(Xt), Xv.stride(0), ptr(M), self.hyper_num, ptr(acc),
                  acc.stride(0) if acc is not None else 0, ptr(S), ptr(h), self.h.stride(0), self._p_used, self.tau,
                  ptr(out), out.stride(0), 0, stream())

    def _draws(self, x, dtype, what):
        """Injected draws as the row kernel reads them: a packed (2, N, H) device tensor of `dtype` (a bool mask is
        taken as bytes); anything else raises, nothing is read with another layout."""
        if x is None:
            return None
        x = torch.as_tensor(x)
        if x.dtype == torch.bool and dtype == torch.uint8:
            x = x.to(torch.uint8)
        if x.dtype != dtype:
            raise TypeError(f"{what} must be {dtype}, got {x.dtype}")
        if tuple(x.shape) != (2, self.N, self.hyper_num):
            raise ValueError(f"{what} must be 2 x {self.N} x {self.hyper_num}, got {tuple(x.shape)}")
        return x.to(self.device).contiguous()

    def _cge_for_hyper(self, cge):
        """The collaborative view the hypergraph block and the combine read, once cge and self.mge of this forward
        stand: cge itself.  A model that mixes rows into it (gmr/rflgmrec.py) returns a table of its own."""
        return cge

    def _forward(self, train=False, step=0, g=None, keep=None):
        """lgmrec.py:115-151 into self.all (and the rows the backward reads).  g: (2, N, H) float Gumbel draws
        [image; text] (user rows first) instead of Philox's; keep: (2, N, H) uint8 keep masks likewise."""
        U, I, N, H = self.n_users, self.n_items, self.N, self.hyper_num
        s = self.slab
        g, keep = self._draws(g, torch.float32, "g"), self._draws(keep, torch.uint8, "keep")
        for m, _, _ in self.mods:
            K.gemm(self.feat[m], s.view("Wcat_" + m), self.proj[m][:, :D + H])
        pv, pt = self.proj["v"], self.proj["t"]
        p_keep = self.keep_rate if train else 1.0
        mode = 0 if p_keep == 1.0 else 1 if keep is not None else 2
        self._p_used = p_keep
        _lib.call("gmr_lgm_hyper_fwd", U, I, H, ptr(pv[:, D:]), pv.stride(0), ptr(pt[:, D:]), pt.stride(0),
                  ptr(self.adj.rowptr), ptr(self.adj.col), ptr(g[0]) if g is not None else None,
                  ptr(g[1]) if g is not None else None, H, ptr(keep[0]) if mode == 1 else None,
                  ptr(keep[1]) if mode == 1 else None, H, self.tau, p_keep, mode, self.seed, step, ptr(self.S),
                  ptr(self.h), 2 * H, 0, stream())
        cge = self._cge()
        # the modal views: the users' mean of F_m, then n_mm hops with the item rows of the first read in place
        fv, ft = pv[:, :D], pt[:, :D]
        self.adj_mean.spmm(self.mge_u, [(fv,), (ft,)])
        if self.n_mm_layers == 0:
            mge = self.mge0
            K.zero_(mge)
            copy64(self.mge_u[:, :D], mge[:U, :D])
            copy64(self.mge_u[:, D:], mge[:U, D:])
            copy64(fv, mge[U:, :D])
            copy64(ft, mge[U:, D:])
        for i in range(self.n_mm_layers):
            # the last hop lands in _mm[0]
            dst = self._mm[(self.n_mm_layers - 1 - i) % 2]
            if i == 0:
                self.norm_adj.spmm(dst, [(self.mge_u[:, :D], fv), (self.mge_u[:, D:], ft)], split=U)
            else:
                self.norm_adj.spmm(dst, [(mge[:, :D],), (mge[:, D:],)])
            mge = dst
        self.mge = mge
        # the hyperedge layers and the combine read hc; the backward is handed cge
        hc = self._cge_for_hyper(cge)
        hi = self.h[U:]
        xv = xt = hc[U:]
        for l in range(self.n_hyper_layer):
            self._lat(I, hi, xv, xt, self.lats[l])
            if l < self.n_hyper_layer - 1:
                self._apply(hi, self.lats[l], self.ilay[l], 0)
                xv, xt = self.ilay[l][:, :D], self.ilay[l][:, D:]
        _lib.call("gmr_lgm_combine_fwd", N, ptr(hc), D, ptr(mge), 2 * D, ptr(self.h), 2 * H, H, ptr(self.lats[-1]),
                  self.alpha, ptr(self.all), D, ptr(self.CLN), ptr(self.nrmCL), ptr(self.nrm3), 0, stream())
        return cge

    # ------------------------------------------------------------------ the step
    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev = self.device
            f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
            self._w = {"B": B, "bpr": f(B), "contrib": f(3 * B, D), "cl": f(2, B), "contrib_cl": f(2 * B, 2 * D),
                       "P1": f(B, D)}
        return self._w

    _plans = MGCN._plans
    behaviour_bwd = MGCN.behaviour_bwd

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, g=None, keep=None):
        """calculate_loss (lgmrec.py:175-194) and all parameter gradients (into the slab's twin).  g, keep: injected
        Gumbel draws and keep masks (see _forward).  Returns the loss as a device scalar; loss_terms() reads
        [total, bpr, cl_users, cl_items, reg]."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: LGMRec runs on one device")
        B, U, I, N = users.numel(), self.n_users, self.n_items, self.N
        if plan_bpr is None or plan_cl is None:
            plan_bpr, plan_cl = self._plans(users, pos, neg)
        w = self._work(B)
        inv = 1.0 / (norm_rows or B)
        cge = self._forward(train=self.training, step=self._step, g=g, keep=keep)
        # ---- loss
        contrib, ccl, loss = w["contrib"][:3 * B], w["contrib_cl"][:2 * B], self._loss
        _lib.call("gmr_bpr_logsigmoid_f32", B, U, ptr(self.all), ptr(users), ptr(pos), ptr(neg), ptr(w["bpr"]),
                  ptr(contrib), inv, stream())
        _lib.call("gmr_lgm_reg", B, U, ptr(self.all), D, ptr(users), ptr(pos), ptr(neg), self.reg_weight / B,
                  ptr(contrib), D, ptr(loss[4:]), stream())
        CLN, dK = self.CLN, self.dK
        K.zero_(dK)
        for k, (nodes, off, n) in enumerate(((users, 0, U), (pos, U, I))):
            P1 = w["P1"][:B]
            K.gather_rows(CLN[:, :D], nodes, P1, off=off)
            ws = K.contrast_workspace(B, n, self.device, "lgm_cl")
            T = CLN[off:off + n, D:]
            _lib.call("gmr_contrast_fused_nbwd_f32", B, n, ptr(P1), D, ptr(T), 2 * D, ptr(CLN), ptr(nodes), off,
                      1.0 / self.tau, self.cl_weight, ptr(w["cl"][k]), ptr(ccl[k * B:(k + 1) * B]), 2 * D,
                      ptr(dK[off:off + n, D:]), 2 * D, ptr(T), 2 * D, ptr(self.nrmCL[1][off:off + n]), ptr(ws),
                      ws.numel(), stream())
        _lib.call("gmr_scatter_sorted_nbwd_f32", plan_cl.numel(), ptr(plan_cl), ptr(ccl), 2 * D, ptr(CLN),
                  ptr(self.nrmCL), N, ptr(dK), stream())
        _lib.call("gmr_sum_f32", B, ptr(w["bpr"]), inv, ptr(loss[1:]), 0, stream())
        for k in range(2):
            _lib.call("gmr_sum_f32", B, ptr(w["cl"][k]), self.cl_weight, ptr(loss[2 + k:]), 0, stream())
        _lib.call("gmr_sum_f32", 4, ptr(loss[1:]), 1.0, ptr(loss), 0, stream())
        # ---- backward
        self.slab.zero_grad()
        K.zero_(self.dall)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), D, ptr(plan_bpr), ptr(contrib), D, ptr(self.dall), D,
                  stream())
        self.step_backward(cge)
        self._step += 1
        return loss[0]

    def step_backward(self, cge):
        """All parameter gradients from dall (d loss / d all) and dK (the contrastive terms' [d x_v | d x_t])."""
        U, I, N, H, s = self.n_users, self.n_items, self.N, self.hyper_num, self.slab
        dall, dK, dmge, hi, nl = self.dall, self.dK, self.dmge, self.h[U:], self.n_hyper_layer
        _lib.call("gmr_lgm_combine_bwd", N, ptr(dall), D, ptr(self.mge), 2 * D, ptr(self.CLN), ptr(self.nrmCL),
                  ptr(self.nrm3), self.alpha, ptr(dmge), 2 * D, ptr(dK), 0, stream())
        # the hyperedge layers: d lat_L over all rows, then the item rows' terms of d hi, layer by layer
        dlat = self.dlat[0]
        self._lat(N, self.h, dK[:, :D], dK[:, D:], dlat)
        acc = self.acc
        K.zero_(acc[:U])

        def layer_in(l):  # i_l as (v, t) tables; i_0 = E_i for both
            return (cge[U:], cge[U:]) if l == 0 else (self.ilay[l - 1][:, :D], self.ilay[l - 1][:, D:])

        self._dh(*layer_in(nl - 1), dlat, acc[U:])                          # i_(L-1) d lat_L^T
        for l in range(nl, 1, -1):
            di, prev = self.di, self.dlat[(nl - l + 1) % 2]
            self._apply(hi, dlat, di, 0)                                    # d i_(l-1) = hi d lat_l
            self._lat(I, hi, di[:, :D], di[:, D:], prev)                    # d lat_(l-1) = hi^T d i_(l-1)
            self._dh(di[:, :D], di[:, D:], self.lats[l - 2], acc[U:], acc=acc[U:])   # + d i_(l-1) lat_(l-1)^T
            self._dh(*layer_in(l - 2), prev, acc[U:], acc=acc[U:])          # + i_(l-2) d lat_(l-1)^T
            dlat = prev
        self._dh(dK[:, :D], dK[:, D:], self.lats[-1], self.dL, acc=acc, sbwd=True)   # d L of all rows
        self._apply(hi, dlat, dall[U:], 1)                                  # d E_i += hi d lat_1
        dv, dt = self.dproj["v"], self.dproj["t"]
        _lib.call("gmr_lgm_logit_bwd", U, I, H, ptr(self.dL), 2 * H, ptr(self.adj_t.rowptr), ptr(self.adj_t.col),
                  ptr(dv[:, D:]), dv.stride(0), ptr(dt[:, D:]), dt.stride(0), 0, stream())
        # the modal views backwards: n_mm hops over the symmetric graph, then the users' mean to the items
        t = dmge
        for i in range(self.n_mm_layers):
            dst = self._mm[i % len(self._mm)]  # the forward's hops are no longer read
            self.norm_adj.spmm(dst, [(t[:, :D],), (t[:, D:],)])
            t = dst
        for blk, m in enumerate(("v", "t")):
            dp = self.dproj[m]
            copy64(t[U:, D * blk:D * blk + D], dp[:, :D])
            self.adj_mean_t.spmm(dp[:, :D], [(t[:U, D * blk:D * blk + D],)], beta=1.0)
            K.gemm(self.feat[m], dp[:, :D + H], s.gview("Wcat_" + m), trans_a=True)   # X^T [d F | d Li]
        # the collaborative view
        if self.cf_model == "mf" or self.n_ui_layers == 0:
            copy64(dall, s.gview("E"))
        else:
            self.behaviour_bwd(dall)

    def loss_terms(self):
        """[total, bpr, cl_users, cl_items, reg] of the last rec_step (device tensor)."""
        return self._loss

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward(self, noise=None):
        """(all_u, all_i) of lgmrec.py:115-151 in evaluation: Gumbel draws, no dropout."""
        return self.forward_embeddings(noise)

    @torch.no_grad()
    def forward_embeddings(self, noise=None):
        """full_sort_predict's tables.  noise: (2, N, H) Gumbel draws [image; text], user rows first; None draws them
        from Philox once per call (seed, evaluation-pass counter), which the trainer makes once per evaluation pass."""
        g = None
        if noise is not None:
            g = self._draws(torch.as_tensor(noise, dtype=torch.float32), torch.float32, "noise")
        self._forward(train=False, step=EVAL_STEP0 + self._eval_pass, g=g)
        if noise is None:
            self._eval_pass += 1
        return self.all[:self.n_users], self.all[self.n_users:]
