"""SMORE on MI355X — drop-in for models/smore.py of the reference (GeneralRecommender API).

Spectrum modality fusion: MGCN with a third, "fusion" view.  The projected features of the two modalities are filtered
in the frequency domain (a learned complex weight per bin) and multiplied there into a fusion signal; each of the three
filtered signals gates the item id embeddings, which are propagated over that view's frozen item-item graph and carried
to the users; an attention driven by the fusion view weighs the two modal views feature by feature, and three
preference gates driven by the behaviour view (with dropout) fuse the three.  What it computes:

Init (the constructor's RNG order)
  nn.Embedding(U, 64), nn.Embedding(I, 64), then xavier_uniform_ on the user table, then the item table; image_trs =
  nn.Linear(Dv, 64), text_trs = nn.Linear(Dt, 64); query_v, query_t = Linear(64, 64), Tanh, Linear(64, 64, no bias)
  each; gate_v, gate_t, gate_f, gate_image_prefer, gate_text_prefer, gate_fusion_prefer = Linear(64, 64) + Sigmoid each;
  last, image_complex_weight, text_complex_weight, fusion_complex_weight = randn(1, 33, 2) each, read as 33 complex
  numbers.  The three complex weights are the module's own parameters, so named_parameters() lists them first.  The
  feature tables are trainable.  Both modalities are required.

Graphs
  adj, R   as MGCN.
  Av, At   mgcn.knn_graph with image_knn_k and text_knn_k neighbours.
  Af       the union of the two patterns: a shared entry takes the larger of the two values, an entry of one graph keeps
           its value; no renormalisation.  Built once at construction (torch ops on the device), and its transpose.

forward, with E = [E_u; E_i], theta = 2 pi / 64, c_k = 1 for k in {0, 32}, else 2
  V = image_trs(image),  T = text_trs(text)
  A_k = 1/8 sum_n V_n e^{-i theta k n},  B_k likewise from T,  k = 0..32               rfft, norm 'ortho'
  inv(Y)_n = 1/8 sum_k c_k Re(Y_k e^{+i theta k n})                                    irfft; Im Y_0, Im Y_32 ignored
  image_conv = inv(A Wi),  text_conv = inv(B Wt),  fusion_conv = inv(A B Wf)           the spectrum step
  Pv = E_i * sigmoid(gate_v(image_conv)),  Pt, Pf likewise from gate_t, gate_f
  a = [R Av^n Pv; Av^n Pv]  (n = n_layers);  b, f the same from (At, Pt), (Af, Pf)
  c = mean(E_0 .. E_L),  E_k+1 = adj E_k  (L = n_ui_layers)
  sv = softmax_64(Wv2 tanh(Wv1 f + bv1)),  st = softmax_64(Wt2 tanh(Wt1 f + bt1))      over a row's 64 features
  gi, gt, gf = dropout_p(sigmoid(W. c + b.))       three independent masks, training only, kept entries / (1 - p)
  side = (gi * sv * a + gt * st * b + gf * f) / 3;  all = c + side

calculate_loss, full_sort_predict   MGCN's, term for term (BPR + L2 over the configured batch size + cl_loss times two
  in-batch InfoNCE terms at temperature 0.2).  The config keys temperature and lambda_coeff are read by nothing.

On the device
  One Slab holds every parameter.  A step:
    forward    V, T GEMMs (BIAS epilogue) into vt = [V | T]; gmr_smore_spectrum_fwd (both transforms, the three
               spectral products in the 64-real layout, the three inverses and the three gates in one launch; the
               spectra, the conv rows and the gate rows saved); n SpMMs per view into the item rows of
               abf = [a | b | f], R into the user rows; the LightGCN layers and gmr_frd_mean_fwd into c;
               gmr_smore_fuse_fwd (seven products, the feature softmax, the dropout masks from Philox keyed on (seed,
               step counter, gate, row, column group) unless injected)
    loss       MGCN.loss_fwd_bwd, unchanged
    backward   MGCN.scatter_loss_rows; gmr_smore_fuse_bwd; the weight gradients as GEMMs / colsums on its z rows;
               dH = d_i + R^T d_u, dP = (A^T)^n dH per view; MGCN.behaviour_bwd; gmr_smore_spectrum_bwd (+ dE_i, the
               gate z rows, dV, dT and the three filter gradients through a fixed-order fp64 reduction); the gate and
               projection gradients as GEMMs
  No host read inside a step.  The step counter travels in extra_state(): a resumed run draws the next step's masks.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, config_seed, copy64, r4
from .freedom import _Linear, _Table
from .kernels import ptr, stream
from .mgcn import MAX_TABLES, MGCN, _Seq, knn_graph
from .slab import Slab

D = 64
NBIN = D // 2 + 1
FILTERS = ("image", "text", "fusion")
QUERIES = (("qv", "query_v"), ("qt", "query_t"))
# (slab prefix, module name) of the six 64 x 64 gates, in the constructor's order
GATES = (("gv", "gate_v"), ("gt", "gate_t"), ("gf", "gate_f"), ("pi", "gate_image_prefer"),
         ("pt", "gate_text_prefer"), ("pf", "gate_fusion_prefer"))


def check_config(config, n_items=None, has=(True, True)):
    """Raise NotImplementedError naming the key for settings outside the hot path; returns (n_ui_layers, n_layers,
    image_knn_k, text_knn_k, dropout_rate)."""
    c = config
    if int(c["embedding_size"] or D) != D:
        raise NotImplementedError(f"embedding_size = {c['embedding_size']}: {D} (the spectrum step is a 64-point "
                                  f"transform on 64-column row tiles)")
    if c["sparse"] is not None and not c["sparse"]:
        raise NotImplementedError("sparse = False: the dense item graphs are not built; the kNN graphs are CSR")
    L = int(c["n_ui_layers"])
    if L < 0 or L + 1 > MAX_TABLES:
        raise NotImplementedError(f"n_ui_layers = {L}: 0..{MAX_TABLES - 1}")
    n = int(c["n_layers"])
    if n < 0:
        raise NotImplementedError(f"n_layers = {n}: >= 0")
    ks = []
    for key in ("image_knn_k", "text_knn_k"):
        k = int(c[key])
        if k < 1 or (n_items is not None and k > n_items):
            raise NotImplementedError(f"{key} = {k}: 1..{n_items} (the number of items)")
        ks.append(k)
    p = float(c["dropout_rate"] or 0.0)
    if not 0.0 <= p < 1.0:
        raise NotImplementedError(f"dropout_rate = {p}: 0 <= p < 1")
    for name, h in zip(("image", "text"), has):
        if not h:
            raise NotImplementedError(f"{name} features (inter_file's {name} feature file) are missing: SMORE's "
                                      f"spectrum step multiplies both modalities")
    if dist.world() > 1:
        raise NotImplementedError("world size > 1: the in-batch InfoNCE is over the global batch; SMORE runs on one "
                                  "device")
    return L, n, ks[0], ks[1], p


def max_pool_fusion(a, b):
    """The union of two I x I CSR graphs: a shared entry takes the larger value, no renormalisation (smore.py:132-153).
    Torch ops on the device, once at construction."""
    n = a.n_cols
    keys, vals = [], []
    for g in (a, b):
        rows = torch.repeat_interleave(torch.arange(g.n_rows, device=g.col.device),
                                       (g.rowptr[1:] - g.rowptr[:-1]).long())
        keys.append(rows * n + g.col.long())
        vals.append(g.val)
    uk, inv = torch.unique(torch.cat(keys), sorted=True, return_inverse=True)
    val = torch.full((uk.numel(),), float("-inf"), dtype=torch.float32, device=uk.device)
    val.scatter_reduce_(0, inv, torch.cat(vals), reduce="amax")
    rows = torch.div(uk, n, rounding_mode="floor")
    rp = torch.zeros(a.n_rows + 1, dtype=torch.int64, device=uk.device)
    rp[1:] = torch.cumsum(torch.bincount(rows, minlength=a.n_rows), 0)
    return K.CSR(rp.to(torch.int32), (uk - rows * n).to(torch.int32).contiguous(), val, n_cols=n, symmetric=False)


class SMORE(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        self.n_ui_layers, self.n_layers, self.image_knn_k, self.text_knn_k, self.dropout_rate = check_config(
            c, self.n_items, (self.v_feat is not None, self.t_feat is not None))
        self.embedding_dim = D
        self.sparse = True
        self.reg_weight, self.cl_loss = float(c["reg_weight"]), float(c["cl_loss"])
        self.batch_size = int(c["train_batch_size"])
        self.seed = config_seed(c)
        U, I, dev = self.n_users, self.n_items, self.device
        N = self.N = U + I
        # parameters in the reference's RNG order (smore.py:40-126)
        e_u, e_i = nn.Embedding(U, D), nn.Embedding(I, D)
        nn.init.xavier_uniform_(e_u.weight)
        nn.init.xavier_uniform_(e_i.weight)
        self.mods = (("image", self.v_feat, 0), ("text", self.t_feat, 1))  # (name, features, column block)
        trs = {name: nn.Linear(feat.shape[1], D) for name, feat, _ in self.mods}
        qs = {p: (nn.Linear(D, D), nn.Linear(D, D, bias=False)) for p, _ in QUERIES}
        gates = {p: nn.Linear(D, D) for p, _ in GATES}
        cw = {f: torch.randn(1, NBIN, 2, dtype=torch.float32) for f in FILTERS}
        specs = [(f + "_cw", (1, NBIN, 2), None) for f in FILTERS] + [("E", (N, D), None)]
        for name, feat, _ in self.mods:
            specs.append((name + "_embedding", (I, feat.shape[1]), r4(feat.shape[1])))
        for name, feat, _ in self.mods:
            specs += [(name + "_W", (D, feat.shape[1]), r4(feat.shape[1])), (name + "_b", (D,), None)]
        for p, _ in QUERIES:
            specs += [(p + "_W1", (D, D), None), (p + "_b1", (D,), None), (p + "_W2", (D, D), None)]
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
            for p, _ in QUERIES:
                s.load(p + "_W1", qs[p][0].weight)
                s.load(p + "_b1", qs[p][0].bias)
                s.load(p + "_W2", qs[p][1].weight)
            for p, _ in GATES:
                s.load(p + "_W", gates[p].weight)
                s.load(p + "_b", gates[p].bias)
            for f in FILTERS:
                s.load(f + "_cw", cw[f])
        # the module's own parameters first, then the module views under the reference's names in its order
        for f in FILTERS:
            setattr(self, f + "_complex_weight", s.parameter(f + "_cw"))
        e, ge = s.view("E"), s.gview("E")
        self.user_embedding = _Table(nn.Parameter(e[:U]))
        self.user_embedding.weight.grad = ge[:U]
        self.item_id_embedding = _Table(nn.Parameter(e[U:]))
        self.item_id_embedding.weight.grad = ge[U:]
        for name, _, _ in self.mods:
            setattr(self, name + "_embedding", _Table(s.parameter(name + "_embedding")))
        for name, _, _ in self.mods:
            setattr(self, name + "_trs", _Linear(s.parameter(name + "_W"), s.parameter(name + "_b")))
        for p, mod in QUERIES:
            setattr(self, mod, _Seq({0: _Linear(s.parameter(p + "_W1"), s.parameter(p + "_b1")),
                                     2: _Table(s.parameter(p + "_W2"))}))
        for p, mod in GATES:
            setattr(self, mod, _Seq({0: _Linear(s.parameter(p + "_W"), s.parameter(p + "_b"))}))
        # graphs
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        ne = int(self.user_items.numel())
        self.norm_adj = K.bipartite_symnorm(U, I, self.user_ptr, self.user_items, self_loops=False, deg_eps=0.0)
        adj = self.norm_adj
        self.R = K.CSR(adj.rowptr[:U + 1].clone(), (adj.col[:ne] - U).contiguous(), adj.val[:ne].clone(), n_cols=I,
                       symmetric=False)
        self.R_t = K.csr_transpose(self.R)
        self.mm_adj = {"image": knn_graph(self.v_feat, self.image_knn_k),
                       "text": knn_graph(self.t_feat, self.text_knn_k)}
        self.mm_adj["fusion"] = max_pool_fusion(self.mm_adj["image"], self.mm_adj["text"])
        self.mm_adj_t = {name: K.csr_transpose(a) for name, a in self.mm_adj.items()}
        # work buffers
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.vt, self.spec, self.conv = f(I, 2 * D), f(I, 2 * D), f(I, 3 * D)   # [V | T], [A | B], the three conv rows
        self.gates_i, self.pur = f(I, 3 * D), f(I, 3 * D)                        # the gate rows, [Pv | Pt | Pf]
        self.abf, self.c, self.side, self.all = f(N, 3 * D), f(N, D), f(N, D), f(N, D)
        self.saved = f(N, 7 * D)                                                 # [hv | ht | sv | st | gi | gt | gf]
        self._h = [f(I, 3 * D) for _ in range(2)] if self.n_layers > 1 else []
        self._layers = [f(N, D) for _ in range(self.n_ui_layers)]
        self._t = [f(N, D) for _ in range(2)]
        self.dall, self.gtab = f(N, D), f(N, 2 * D)                              # d all; [dside | dc] of the InfoNCE
        self.dabf, self.dc, self.zf = f(N, 3 * D), f(N, D), f(N, 7 * D)
        self.dpur, self.zp, self.dvt = f(I, 3 * D), f(I, 3 * D), f(I, 2 * D)
        self._ws = f(int(_lib.load().gmr_smore_spectrum_ws_floats(I)))
        self._loss = f(5)
        self._w = None
        self._i1 = (ctypes.c_int32 * 2)(0, 2)   # queries: side_i[pos], side_u[users]
        self._i2 = (ctypes.c_int32 * 2)(1, 3)   # keys:    c_i[pos],    c_u[users]
        self._step = 0
        self._p_used = 0.0                      # the dropout rate of the last forward (0 in evaluation)

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def _names(self):
        out = [n + "_embedding" for n, _, _ in self.mods]
        for n, _, _ in self.mods:
            out += [n + "_W", n + "_b"]
        for p, _ in QUERIES:
            out += [p + "_W1", p + "_b1", p + "_W2"]
        for p, _ in GATES:
            out += [p + "_W", p + "_b"]
        return out

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order."""
        s, U = self.slab, self.n_users
        return ([s.gview(f + "_cw") for f in FILTERS] + [s.gview("E")[:U], s.gview("E")[U:]] +
                [s.gview(n) for n in self._names()])

    def extra_state(self):
        """The Philox step counter: a resumed run draws the keep masks the uninterrupted one would."""
        return {"counters": {"step": int(self._step)}}

    def load_extra_state(self, st):
        self._step = int(st["counters"]["step"])

    # ------------------------------------------------------------------ forward
    def _chain(self, graphs, src, dst):
        """dst[:, blk] = graph_v^n src[:, blk] per view over I x 192 tables (n = n_layers; n = 0 copies)."""
        for blk, name in enumerate(FILTERS):
            x = src[:, D * blk:D * blk + D]
            for i in range(self.n_layers):
                last = i == self.n_layers - 1
                y = (dst if last else self._h[i % 2])[:, D * blk:D * blk + D]
                graphs[name].spmm(y, [(x,)])
                x = y
            if self.n_layers == 0:
                copy64(x, dst[:, D * blk:D * blk + D])

    def _forward(self, train=False, keep=None):
        """smore.py:208-291 into self.side / self.all (and the rows the backward reads).  keep: N x 192 uint8, the
        three preference gates' keep masks [image | text | fusion] instead of the Philox draw."""
        s, U, I, N = self.slab, self.n_users, self.n_items, self.N
        E = s.view("E")
        vt, abf, c = self.vt, self.abf, self.c
        for name, _, blk in self.mods:
            K.gemm(s.view(name + "_embedding"), s.view(name + "_W"), vt[:, D * blk:D * blk + D], trans_b=True,
                   epi=K.EPI_BIAS, bias=s.view(name + "_b"))
        _lib.call("gmr_smore_spectrum_fwd", I, ptr(vt), 2 * D, ptr(vt[:, D:]), 2 * D, ptr(E[U:]), D,
                  *[ptr(s.view(f + "_cw")) for f in FILTERS], ptr(s.view("gv_W")), ptr(s.view("gv_b")),
                  ptr(s.view("gt_W")), ptr(s.view("gt_b")), ptr(s.view("gf_W")), ptr(s.view("gf_b")), D,
                  ptr(self.spec), 2 * D, ptr(self.conv), 3 * D, ptr(self.gates_i), 3 * D, ptr(self.pur), 3 * D,
                  stream())
        self._chain(self.mm_adj, self.pur, abf[U:])
        self.R.spmm(abf[:U, :2 * D], [(abf[U:, :D],), (abf[U:, D:2 * D],)])
        self.R.spmm(abf[:U, 2 * D:], [(abf[U:, 2 * D:],)])
        tabs = [E]
        for i in range(self.n_ui_layers):
            self.norm_adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", N, N, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(c), D, stream())
        p = self.dropout_rate if train else 0.0
        mode = 0 if p == 0.0 else 1 if keep is not None else 2
        self._p_used = p
        _lib.call("gmr_smore_fuse_fwd", N, ptr(abf), 3 * D, ptr(c), D, ptr(s.view("qv_W1")), ptr(s.view("qv_b1")),
                  ptr(s.view("qv_W2")), ptr(s.view("qt_W1")), ptr(s.view("qt_b1")), ptr(s.view("qt_W2")),
                  ptr(s.view("pi_W")), ptr(s.view("pi_b")), ptr(s.view("pt_W")), ptr(s.view("pt_b")),
                  ptr(s.view("pf_W")), ptr(s.view("pf_b")), D, p, mode, ptr(keep) if mode == 1 else None,
                  keep.stride(0) if mode == 1 else 0, self.seed, self._step, ptr(self.side), ptr(self.all), D,
                  ptr(self.saved), 7 * D, stream())

    # MGCN's loss, its work buffers and its plans, unchanged
    _work = MGCN._work
    _plans = MGCN._plans
    loss_fwd_bwd = MGCN.loss_fwd_bwd
    scatter_loss_rows = MGCN.scatter_loss_rows
    behaviour_bwd = MGCN.behaviour_bwd

    # ------------------------------------------------------------------ the step
    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, keep=None):
        """calculate_loss (smore.py:316-336) and all parameter gradients (into the slab's twin).  keep: the three
        preference gates' keep masks (N x 192 uint8) instead of the Philox draw.  Returns the loss as a device
        scalar; loss_terms() reads [total, bpr, reg, nce_items, nce_users]."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: SMORE runs on one device")
        B = users.numel()
        if plan_bpr is None or plan_cl is None:
            plan_bpr, plan_cl = self._plans(users, pos, neg)
        w = self._work(B)
        self._forward(train=True, keep=keep)
        self.loss_fwd_bwd(users, pos, neg, 1.0 / (norm_rows or B), w)
        self.step_backward(plan_bpr, plan_cl, w, B)
        self._step += 1
        return self._loss[0]

    def step_backward(self, plan_bpr, plan_cl, w, B):
        """All parameter gradients from the outputs of loss_fwd_bwd over B rows."""
        s, U, I, N = self.slab, self.n_users, self.n_items, self.N
        s.zero_grad()
        self.scatter_loss_rows(plan_bpr, plan_cl, w, B)
        abf, c, sv, dabf, dc, zf = self.abf, self.c, self.saved, self.dabf, self.dc, self.zf
        _lib.call("gmr_smore_fuse_bwd", N, ptr(self.dall), D, ptr(self.gtab), ptr(self.gtab[:, D:]), 2 * D, ptr(abf),
                  3 * D, ptr(sv), 7 * D, self._p_used, ptr(s.view("qv_W1")), ptr(s.view("qv_W2")),
                  ptr(s.view("qt_W1")), ptr(s.view("qt_W2")), ptr(s.view("pi_W")), ptr(s.view("pt_W")),
                  ptr(s.view("pf_W")), D, ptr(dabf), 3 * D, ptr(dc), D, ptr(zf), 7 * D, stream())
        fus = abf[:, 2 * D:]
        for q, (p, _) in enumerate(QUERIES):      # zf = [z1v | z2v | z1t | z2t | zi | zt | zf]
            z1, z2 = zf[:, 2 * D * q:2 * D * q + D], zf[:, 2 * D * q + D:2 * D * q + 2 * D]
            K.gemm(z1, fus, s.gview(p + "_W1"), trans_a=True)                       # dW1 = z1^T f
            K.colsum(z1, s.gview(p + "_b1"))
            K.gemm(z2, sv[:, D * q:D * q + D], s.gview(p + "_W2"), trans_a=True)    # dW2 = z2^T tanh(.)
        for blk, p in ((4, "pi"), (5, "pt"), (6, "pf")):
            z = zf[:, D * blk:D * blk + D]
            K.gemm(z, c, s.gview(p + "_W"), trans_a=True)                           # dWi = zi^T c
            K.colsum(z, s.gview(p + "_b"))
        # dH = d_i + R^T d_u (in place on the item rows), dP = (A^T)^n dH
        self.R_t.spmm(dabf[U:, :2 * D], [(dabf[:U, :D],), (dabf[:U, D:2 * D],)], beta=1.0)
        self.R_t.spmm(dabf[U:, 2 * D:], [(dabf[:U, 2 * D:],)], beta=1.0)
        self._chain(self.mm_adj_t, dabf[U:], self.dpur)
        self.behaviour_bwd(dc)
        gE = s.gview("E")
        zp, dvt, cv = self.zp, self.dvt, self.conv
        _lib.call("gmr_smore_spectrum_bwd", I, ptr(self.dpur), 3 * D, ptr(self.gates_i), 3 * D, ptr(s.view("E")[U:]),
                  D, ptr(self.spec), 2 * D, *[ptr(s.view(f + "_cw")) for f in FILTERS], ptr(s.view("gv_W")),
                  ptr(s.view("gt_W")), ptr(s.view("gf_W")), D, ptr(gE[U:]), D, 1, ptr(zp), 3 * D, ptr(dvt),
                  ptr(dvt[:, D:]), 2 * D, ptr(self._ws), self._ws.numel(), *[ptr(s.gview(f + "_cw")) for f in FILTERS],
                  stream())
        for blk, p in enumerate(("gv", "gt", "gf")):
            z = zp[:, D * blk:D * blk + D]
            K.gemm(z, cv[:, D * blk:D * blk + D], s.gview(p + "_W"), trans_a=True)  # dWg = z^T conv
            K.colsum(z, s.gview(p + "_b"))
        for name, _, blk in self.mods:
            self._proj_bwd(name, dvt[:, D * blk:D * blk + D])

    def loss_terms(self):
        """[total, bpr, reg, nce_items, nce_users] of the last rec_step (device tensor)."""
        return self._loss

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward(self):
        """(all_u, all_i) of smore.py:208-291 in evaluation: no dropout, nothing drawn."""
        self._forward(train=False)
        return self.all[:self.n_users], self.all[self.n_users:]

    @torch.no_grad()
    def forward_embeddings(self):
        """full_sort_predict's tables (smore.py:338-346)."""
        return self.forward()
