"""BM3 on MI355X — drop-in for models/bm3.py of the reference (GeneralRecommender API).

Bootstrap latent representations: self-supervised, no negatives.  A LightGCN encoder gives 64-wide user / item rows, a
shared 64 x 64 predictor maps the "online" rows, and the targets are dropped-out copies of the same rows without
gradient; every loss term is 1 - mean cosine.  What it computes:

Init (the constructor's RNG order)
  parameters  nn.Embedding(U, 64), nn.Embedding(I, 64) draw their normal init, then xavier_uniform_ on the user table,
              then the item table; predictor = nn.Linear(64, 64) draws its default init, then xavier_normal_ on its
              weight (the bias keeps the default); image before text: from_pretrained draws nothing, nn.Linear(Dm, 64)
              draws its init, then xavier_normal_ on the weight.  Feature tables are trainable.  Either modality may
              be absent.  named_parameters(): user_embedding.weight, item_id_embedding.weight, predictor.weight,
              predictor.bias, image_embedding.weight, image_trs.weight, image_trs.bias, text_embedding.weight,
              text_trs.weight, text_trs.bias.
  graph       D^-1/2 A D^-1/2 of the binary bipartite train graph, degrees + 1e-7, no self loops.

encoder      [ua; ia] = mean(E_0 .. E_n), E_{k+1} = adj E_k, n = n_layers;  ib = ia + E_item (the residual)

calculate_loss(users, items)   (B rows, duplicates kept; a negative in the batch is ignored)
  T = text_trs(text_embedding.weight),  V = image_trs(image_embedding.weight),  P(x) = x Wp^T + bp
  targets (no gradient): drop(ua), drop(ib), drop(T), drop(V); drop = F.dropout(p = dropout) on the whole table, always
  on: a keep mask times 1 / (1 - p), the four masks drawn in the order u, i, t, v.  A mask belongs to a table row: an
  item that occurs twice in the batch has the same mask both times.
  cos(a, b) = <a, b> / (max(|a|, 1e-8) max(|b|, 1e-8)), each norm clamped on its own
    ui = 1 - mean cos(P(ua[u]), drop(ib)[i])        iu = 1 - mean cos(P(ib[i]), drop(ua)[u])
    t  = 1 - mean cos(P(T[i]),  drop(ib)[i])        tv = 1 - mean cos(P(T[i]),  drop(T)[i])
    v  = 1 - mean cos(P(V[i]),  drop(ib)[i])        vt = 1 - mean cos(P(V[i]),  drop(V)[i])
    reg = (|ua|_F + |ib|_F) / I                     (the whole tables, norms not squared)
  loss = ui + iu + reg_weight reg + cl_weight (t + v + tv + vt); the terms of an absent modality are 0

full_sort_predict(users)   encoder on norm_adj, scores = P(ua)[users] P(ib)^T

On the device
  One Slab holds E = [E_user; E_item], Wp, bp and per modality the feature table (rows padded to 16 bytes) and its
  projection.  A step:
    forward    T, V GEMMs (BIAS epilogue) into the I x 128 table tv = [T | V]; E_k+1 = adj E_k; g = [ua; ib] =
               mean(E_0..E_n) + E_item on the item rows (gmr_frd_mean_fwd with the residual table), kept contiguous
               so that the two Frobenius norms are plain gmr_sqnorm_f32 calls
    loss       gmr_bm3_loss_fwd_bwd: gather of the four streams, the predictor on the fp32 MFMA, targets, six cosines,
               the gradient rows of the online rows and dx = d_on Wp, one launch; gmr_bm3_loss_reduce: the loss terms
               and the two reg coefficients reg_weight / (I |.|_F), left on the device (no host read in the step)
    backward   dWp = don^T xg, dbp = colsum(don); one sorted scatter of the 2B x 192 contribution rows through the
               loader's two-key plan (keys [users | items + U]) into gtab = [dg | dT | dV]; the dense reg gradient
               coef g added to dg (gmr_bm3_reg_bwd); per modality dW = dT^T raw, db = colsum(dT), draw = dT W;
               dE = sum_k adj^k dg / (n + 1) as a Horner chain (adj is symmetric), plus dg of the item rows once more
               for the residual
  Prediction: g on norm_adj, then P over all N rows as one GEMM with the BIAS epilogue; forward_embeddings returns
  (P(ua), P(ib)), so the trainer's fused score -> mask -> top-K evaluation serves BM3 unchanged.

Random draws: the keep masks come from Philox keyed on (seed, step counter, stream site, table row id, column group)
unless injected (csrc/bm3.hip states the offset formula); the step counter travels in extra_state().
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, config_seed, copy64, r4, sort_plan
from .freedom import _Linear, _Table
from .kernels import ptr, stream
from .slab import Slab

D = 64
MAX_TABLES = 8  # GMR_FRD_MAX_LAYERS of include/gmr.h: the layer mean takes n_layers + 1 tables
SITE_DROP = 0xB30  # streams u, i, t, v draw at sites SITE_DROP + 0..3


def check_config(config):
    """Raise NotImplementedError naming the key for settings outside the hot path; returns (n_layers, dropout)."""
    c = config
    if int(c["embedding_size"] or D) != D:
        raise NotImplementedError(f"embedding_size = {c['embedding_size']}: {D} (the SpMM blocks and the loss tiles "
                                  f"are 64 columns)")
    if int(c["feat_embed_dim"] or D) != D:
        raise NotImplementedError(f"feat_embed_dim = {c['feat_embed_dim']}: {D} (the predictor is shared by the id and "
                                  f"the modal rows)")
    L = int(c["n_layers"])
    if L < 0 or L + 1 > MAX_TABLES:
        raise NotImplementedError(f"n_layers = {L}: 0..{MAX_TABLES - 1}")
    p = float(c["dropout"] or 0.0)
    if not 0.0 <= p < 1.0:
        raise NotImplementedError(f"dropout = {p}: 0 <= dropout < 1")
    if dist.world() > 1:
        raise NotImplementedError("world size > 1: reg is a norm over the whole tables and the keep masks belong to "
                                  "table rows; BM3 runs on one device")
    return L, p


class BM3(EmbeddingRecommender):
    LOSS_ROWS = 2  # users, items: no negatives

    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        self.n_layers, self.dropout = check_config(c)
        self.embedding_dim = self.feat_embed_dim = D
        self.reg_weight, self.cl_weight = float(c["reg_weight"]), float(c["cl_weight"])
        self.seed = config_seed(c)
        U, I, dev = self.n_users, self.n_items, self.device
        N = self.N = U + I
        # parameters in the reference's RNG order (bm3.py:39-56)
        e_u, e_i = nn.Embedding(U, D), nn.Embedding(I, D)
        nn.init.xavier_uniform_(e_u.weight)
        nn.init.xavier_uniform_(e_i.weight)
        pred = nn.Linear(D, D)
        nn.init.xavier_normal_(pred.weight)
        specs = [("E", (N, D), None), ("Wp", (D, D), None), ("bp", (D,), None)]
        lins = {}
        self.mods = []  # (name, feature tensor, column block of tv / gtab's modal part), image first as the reference
        for name, feat, blk in (("image", self.v_feat, 1), ("text", self.t_feat, 0)):
            if feat is None:
                continue
            Dm = feat.shape[1]
            lins[name] = nn.Linear(Dm, D)
            nn.init.xavier_normal_(lins[name].weight)
            specs += [(name + "_embedding", (I, Dm), r4(Dm)), (name + "_W", (D, Dm), r4(Dm)),
                      (name + "_b", (D,), None)]
            self.mods.append((name, feat, blk))
        s = self.slab = Slab(specs, dev)
        with torch.no_grad():
            s.view("E")[:U].copy_(e_u.weight)
            s.view("E")[U:].copy_(e_i.weight)
            s.load("Wp", pred.weight)
            s.load("bp", pred.bias)
            for name, feat, _ in self.mods:
                s.load(name + "_embedding", feat)
                s.load(name + "_W", lins[name].weight)
                s.load(name + "_b", lins[name].bias)
        e, ge = s.view("E"), s.gview("E")
        self.user_embedding = _Table(nn.Parameter(e[:U]))
        self.user_embedding.weight.grad = ge[:U]
        self.item_id_embedding = _Table(nn.Parameter(e[U:]))
        self.item_id_embedding.weight.grad = ge[U:]
        self.predictor = _Linear(s.parameter("Wp"), s.parameter("bp"))
        for name, _, _ in self.mods:
            setattr(self, name + "_embedding", _Table(s.parameter(name + "_embedding")))
            setattr(self, name + "_trs", _Linear(s.parameter(name + "_W"), s.parameter(name + "_b")))
        # graph
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        self.norm_adj = K.bipartite_symnorm(U, I, self.user_ptr, self.user_items, self_loops=False, deg_eps=1e-7)
        # work buffers
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.g, self.tv, self.gtab = f(N, D), f(I, 2 * D), f(N, 3 * D)
        self._layers = [f(N, D) for _ in range(self.n_layers)]
        self._t = [f(N, D) for _ in range(2)]
        self._eval, self._pred = f(N, D), f(N, D)
        self._sq = f(2)
        self._sqws = torch.zeros(1024, dtype=torch.float64, device=dev)
        self._loss = f(10)
        self._w = None
        self._step = 0

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order."""
        s, U = self.slab, self.n_users
        out = [s.gview("E")[:U], s.gview("E")[U:], s.gview("Wp"), s.gview("bp")]
        for name, _, _ in self.mods:
            out += [s.gview(name + "_embedding"), s.gview(name + "_W"), s.gview(name + "_b")]
        return out

    def extra_state(self):
        """The Philox step counter: a resumed run draws the keep masks the uninterrupted one would."""
        return {"counters": {"step": int(self._step)}}

    def load_extra_state(self, st):
        self._step = int(st["counters"]["step"])

    # ------------------------------------------------------------------ forward
    def _project(self):
        """tv[:, 0:64] = text_trs(text), tv[:, 64:128] = image_trs(image) (bm3.py:101-104)."""
        s = self.slab
        for name, _, blk in self.mods:
            K.gemm(s.view(name + "_embedding"), s.view(name + "_W"), self.tv[:, D * blk:D * blk + D], trans_b=True,
                   epi=K.EPI_BIAS, bias=s.view(name + "_b"))

    def _forward(self, out):
        """bm3.py:84-95 into out (N x 64): mean of E_0..E_n, + E_item on the item rows."""
        U, N = self.n_users, self.N
        E = self.slab.view("E")
        tabs = [E]
        for i in range(self.n_layers):
            self.norm_adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        h = E[U:]
        _lib.call("gmr_frd_mean_fwd", N, U, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), ptr(h), h.stride(0), ptr(out), out.stride(0),
                  stream())

    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev = self.device
            f = lambda *sh, dt=torch.float32: torch.empty(sh, dtype=dt, device=dev)  # noqa: E731
            self._w = {"B": B, "terms": f(6 * B), "contrib": f(2 * B, 3 * D), "xg": f(4 * B, D), "don": f(4 * B, D),
                       "keep": f(4, B, D, dt=torch.uint8)}
        return self._w

    def _plan(self, users, items):
        return sort_plan((users, items), (0, self.n_users))

    def _tables(self):
        has = {name for name, _, _ in self.mods}
        return (self.tv[:, :D] if "text" in has else None), (self.tv[:, D:] if "image" in has else None)

    def loss_fwd_bwd(self, users, items, inv_norm, w, keep=None, keep_out=None):
        """The six cosines of the batch and their contribution rows (gmr_bm3_loss_fwd_bwd), then the loss terms
        (gmr_bm3_loss_reduce).  keep: four B x 64 uint8 arrays (u, i, t, v; None for an absent modality) instead
        of the Philox draw; keep_out: the same for the drawn bytes."""
        B, g, s = users.numel(), self.g, self.slab
        T, V = self._tables()
        Wp = s.view("Wp")
        kin = list(keep) if keep is not None else [None] * 4
        kout = list(keep_out) if keep_out is not None else [None] * 4
        ldk = next((k.stride(0) for k in kin if k is not None), 0)
        ldko = next((k.stride(0) for k in kout if k is not None), 0)
        terms = w["terms"][:6 * B]
        xg, don = w["xg"][:4 * B], w["don"][:4 * B]
        _lib.call("gmr_bm3_loss_fwd_bwd", B, self.n_users, ptr(g), g.stride(0), ptr(T), self.tv.stride(0), ptr(V),
                  self.tv.stride(0), ptr(users), ptr(items), ptr(Wp), Wp.stride(0), ptr(s.view("bp")), self.dropout,
                  self.cl_weight, float(inv_norm), 1 if keep is not None else 2, *[ptr(k) for k in kin], ldk,
                  self.seed, self._step, SITE_DROP, *[ptr(k) for k in kout], ldko, ptr(terms), ptr(w["contrib"]),
                  3 * D, ptr(xg), ptr(don), stream())
        _lib.call("gmr_bm3_loss_reduce", B, ptr(terms), ptr(self._sq), int(T is not None), int(V is not None),
                  self.reg_weight, self.cl_weight, float(inv_norm), self.n_items, ptr(self._loss), stream())

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, keep=None):
        """calculate_loss (bm3.py:97-147) and all parameter gradients (into the slab's twin).  neg is ignored.  keep:
        the four table keep masks' batch rows (B x 64 uint8: u, i, t, v) instead of the Philox draw.  Returns the loss
        as a device scalar; loss_terms() reads [total, ui, iu, t, v, tv, vt, reg]."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: BM3 runs on one device")
        B = users.numel()
        if plan_cl is None:
            plan_cl = self._plan(users, pos)
        w = self._work(B)
        self.step_forward()
        self.loss_fwd_bwd(users, pos, 1.0 / (norm_rows or B), w, keep=keep)
        self.step_backward(plan_cl, w, B)
        self._step += 1
        return self._loss[0]

    def step_forward(self):
        """The projected features, the propagated table [ua; ib] and its two squared norms of one step."""
        U, g = self.n_users, self.g
        self._project()
        self._forward(g)
        _lib.call("gmr_sqnorm_f32", U * D, ptr(g[:U]), 1.0, ptr(self._sq[0:1]), 0, ptr(self._sqws), stream())
        _lib.call("gmr_sqnorm_f32", self.n_items * D, ptr(g[U:]), 1.0, ptr(self._sq[1:2]), 0, ptr(self._sqws),
                  stream())

    def step_backward(self, plan_cl, w, B):
        """All parameter gradients from the outputs of loss_fwd_bwd over B rows."""
        s, U, N, L = self.slab, self.n_users, self.N, self.n_layers
        g, gtab = self.g, self.gtab
        s.zero_grad()
        xg, don = w["xg"][:4 * B], w["don"][:4 * B]
        K.gemm(don, xg, s.gview("Wp"), trans_a=True)  # dWp = don^T xg over the four streams
        K.colsum(don, s.gview("bp"))
        K.zero_(gtab)
        _lib.call("gmr_scatter_sorted_f32", plan_cl.numel(), 3 * D, ptr(plan_cl), ptr(w["contrib"]), 3 * D, ptr(gtab),
                  3 * D, stream())
        dg = gtab[:, :D]
        _lib.call("gmr_bm3_reg_bwd", N, U, ptr(self._loss[8:10]), ptr(g), g.stride(0), ptr(dg), dg.stride(0), stream())
        for name, _, blk in self.mods:
            self._proj_bwd(name, gtab[U:, D * (1 + blk):D * (2 + blk)])
        # dE = (1 / (L + 1)) sum_k adj^k dg: t <- dg; L times t <- adj t + dg, the last one scaled; then the
        # residual: + dg on the item rows
        src = dg
        for i in range(L):
            dst = self._t[i % 2]
            copy64(dg, dst)
            sc = 1.0 / (L + 1) if i == L - 1 else 1.0
            self.norm_adj.spmm(dst, [(src,)], alpha=sc, beta=sc)
            src = dst
        copy64(src, s.gview("E"), res=dg[U:])

    def loss_terms(self):
        """[total, ui, iu, t, v, tv, vt, reg] of the last rec_step (device tensor)."""
        return self._loss[:8]

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward(self):
        """(ua, ib) of bm3.py:84-95."""
        self._forward(self._eval)
        return self._eval[:self.n_users], self._eval[self.n_users:]

    @torch.no_grad()
    def forward_embeddings(self):
        """full_sort_predict's tables (bm3.py:149-154): (P(ua), P(ib)), the predictor over all rows as one GEMM."""
        s = self.slab
        self._forward(self._eval)
        K.gemm(self._eval, s.view("Wp"), self._pred, trans_b=True, epi=K.EPI_BIAS, bias=s.view("bp"))
        return self._pred[:self.n_users], self._pred[self.n_users:]
