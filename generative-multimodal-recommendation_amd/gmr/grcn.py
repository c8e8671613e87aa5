"""GRCN on MI355X — drop-in for models/grcn.py of the reference (GeneralRecommender API).

Graph-Refined Convolutional Network (MM 2020): per modality, user preference rows are routed over the user's items by
an edge softmax; the final attention layer runs in both directions and its softmax values, gated by a learned per-node
confidence, reduced by a max over the modalities and pruned by a ReLU, weight a two-hop LightGCN-style propagation of
the id embedding.  What it computes (grcn.py line numbers):

Init (the constructor's RNG order, :196-214)
  id_gcn.id_embedding = xavier_normal_(rand(N, 64)) (:89); per modality (image first) preference =
  xavier_normal_(rand(U, 64)) (:122), MLP = nn.Linear(D_m, 64) with xavier_normal_ on its weight (:134-136);
  model_specific_conf = xavier_normal_(rand(N, M)) (:212); result = xavier_normal_(rand(N, 64)) (:214), the table
  full_sort_predict reads before any step.  named_parameters(): model_specific_conf, id_gcn.id_embedding, then per
  modality <m>_gcn.preference, <m>_gcn.MLP.weight, <m>_gcn.MLP.bias.
  Hard-coded as in the reference (:180-197): aggr 'add', weight_mode 'confid', fusion_mode 'concat', has_norm, no
  activation, edge dropout 0, pruning on, is_word False.  Image features are required (text alone crashes in the
  reference, :257; here a ValueError); embedding_size = latent_embedding = 64.

forward (:224-298), n(x) = x / max(|x|, 1e-12) per row, N(u) a user's items, N(i) an item's users
  per modality m (CGCN.forward, :139-166):
    f = n(leaky_relu(X_m W_m^T + b_m, 0.01)),  p^0 = n(preference_m)
    routing, r = 0 .. n_layers - 1 (:149-156):  p^(r+1)_u = n(p^r_u + m_u).  The reference routes over its E edges
      from the users to the items, so the messages land on the item rows, which it drops, and m_u = 0: a round only
      normalises the row again.  `routing: items` (not a reference setting; the paper's routing, whose edge list holds
      both directions) sends m_u = sum_{j in N(u)} alpha_uj f_j with alpha = softmax_j <p^r_u, f_j>.
    final layer over x = [p^R; f] in both directions (GATConv.message, :61-72):
      h_u = sum_j a_uj f_j, a_u. = softmax_j <p_u, f_j>;  h_i = sum_u b_iu p_u, b_i. = softmax_u <f_i, p_u>
    rep_m = x + h;  alpha_m = [b in edge order | a in edge order]
  The softmax subtracts the group's maximum and divides by sum + 1e-16; the sum is at least 1, so in fp32 the 1e-16 is
  below one ulp and is not reproduced.
  refining (:272-281): w_e = relu(max_m alpha_m,e conf[s(e), m]), s(e) the edge's source (the user for the E
    item-destination edges, the item for the E user-destination ones)
  id branch (EGCN.forward, :93-109): x = n(id_embedding), x1[d] = sum_{e -> d} w_e x[s(e)], x2 the same over x1,
    id_rep = x + x1 + x2
  result = [id_rep | rep_v | rep_t]  (N x 192, or N x 128 with image features only)

calculate_loss (:300-333), users = each batch user twice, items = positives and negatives interleaved
  -mean log sigmoid(<r_u, r_p> - <r_u, r_n>) + reg_weight (mean(id[users]^2 + id[items]^2) + mean(pref_v^2)
  + sum_m mean(pref_m[users]^2))

full_sort_predict (:335-341) scores from the table the last forward wrote; it is not recomputed in evaluation, and
  before any step it is the random init table above.

Backward of one attention row (destination x_d, sources x_k, incoming dh and dalpha; dalpha = 0 inside routing)
  t_k = dalpha_k + <dh, x_k>,  ds_k = alpha_k (t_k - sum_l alpha_l t_l),  dx_d += sum_k ds_k x_k,
  dx_k += alpha_k dh + ds_k x_d
  dw_e = <x[s(e)], dx1[d]> + <x1[s(e)], dx2[d]>; dconf[s, m] and dalpha_m,e from dw_e through the ReLU and the argmax.

On the device (csrc/grcn.hip, gmr_grcn_*)
  One Slab holds the eight parameters.  The graph is the users' CSR and the items' CSC with the position maps between
  the two list orders, built once; the weighted id propagation runs the CSR SpMM over the N x N pattern
  [CSR; CSC] with the step's weights W, its backward the same pattern with the transposed weights WT that
  gmr_grcn_refine_fwd writes alongside.
    forward    per modality one GEMM with the leaky-ReLU epilogue and two row normalisations; gmr_grcn_route_fwd (all
               rounds, both modalities, the preference row in registers); gmr_grcn_attn_fwd (rep into result's
               columns, alpha); gmr_grcn_refine_fwd; the id rows' normalisation and two SpMMs
    loss       gmr_grcn_loss_rows, one sorted scatter of [d result | reg d id | reg d preference], the reductions
    backward   two SpMMs with WT; gmr_grcn_dw; gmr_grcn_refine_bwd; gmr_grcn_attn_bwd_dst; gmr_grcn_bwd_src for the
               users; gmr_grcn_route_bwd_dst (the rounds in reverse, alpha recomputed from p^r); gmr_grcn_bwd_src for the
               items over the final layer and every round; the normalisation backwards and the weight GEMMs
  No host read inside a step, no float atomics.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, copy64, r4, sort_plan
from .freedom import _Linear
from .kernels import ptr, stream
from .slab import Slab

D = 64
SLOPE = 0.01
MAX_LAYERS = 7  # gmr_grcn_max_layers()


def check_config(config, has=(True, True)):
    """n_layers, after raising for what the port does not run: a ValueError that names the key."""
    c = config
    for key in ("embedding_size", "latent_embedding"):
        if int(c[key] or D) != D:
            raise ValueError(f"{key} = {c[key]}: {D} (the row kernels hold one 64-column row per quarter wave)")
    R = int(c["n_layers"])
    if not 0 <= R <= MAX_LAYERS:
        raise ValueError(f"n_layers = {R}: 0..{MAX_LAYERS}")
    if str(c["routing"] or "reference") not in ("reference", "items"):
        raise ValueError(f"routing = {c['routing']}: 'reference' (the users receive no routing message, as in "
                         f"grcn.py) or 'items' (routed over the user's items)")
    if not has[0]:
        raise ValueError("text features alone: GRCN's regulariser and its first modality are the image's; "
                         "image features, or image and text" if has[1] else "GRCN needs image features")
    if dist.world() > 1:
        raise NotImplementedError("world size > 1: GRCN runs on one device")
    return R


def draw_init(U, I, dims):
    """The reference constructor's draws in its RNG order (grcn.py:196-214) on the CPU: ({state_dict name: tensor} in
    named_parameters() order, the N x 64 table full_sort_predict reads before any step).  dims: the feature widths of
    the modalities present (image first)."""
    N = U + I
    init = {"id_gcn.id_embedding": nn.init.xavier_normal_(torch.rand((N, D)))}
    for m, d in zip("vt", dims):
        init[m + "_gcn.preference"] = nn.init.xavier_normal_(torch.rand((U, D)))
        lin = nn.Linear(d, D)
        nn.init.xavier_normal_(lin.weight)
        init[m + "_gcn.MLP.weight"], init[m + "_gcn.MLP.bias"] = lin.weight.detach(), lin.bias.detach()
    conf = nn.init.xavier_normal_(torch.rand((N, len(dims))))
    result0 = nn.init.xavier_normal_(torch.rand((N, D)))
    return dict([("model_specific_conf", conf)] + list(init.items())), result0


class _EGCN(nn.Module):
    def __init__(self, id_embedding):
        super().__init__()
        self.id_embedding = id_embedding


class _CGCN(nn.Module):
    def __init__(self, preference, weight, bias):
        super().__init__()
        self.preference = preference
        self.MLP = _Linear(weight, bias)


class UIGraph:
    """The train graph as the kernels read it: the users' CSR, the items' CSC, the position maps between the two list
    orders, and the N x N pattern [CSR (columns U + item); CSC (columns user)] of the weighted id propagation."""

    def __init__(self, U, I, uptr, uitems, dev):
        uptr, uitems = np.asarray(uptr, np.int64), np.asarray(uitems, np.int64)
        E = self.E = int(uitems.size)
        rows = np.repeat(np.arange(U), np.diff(uptr))
        order = np.lexsort((rows, uitems))            # CSC order: by item, then by user; order[t] = CSR position
        inv = np.empty(E, np.int64)
        inv[order] = np.arange(E)
        trp = np.zeros(I + 1, np.int64)
        np.cumsum(np.bincount(uitems, minlength=I), out=trp[1:])
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
        self.rowptr, self.col = i32(uptr), i32(uitems)
        self.trp, self.tcol = i32(trp), i32(rows[order])
        self.csc2csr, self.csr2csc = i32(order), i32(inv)
        self.rowptr_n = i32(np.concatenate([uptr, E + trp[1:]]))
        self.col_n = i32(np.concatenate([uitems + U, rows[order]]))
        self.args = (U, I, E, ptr(self.rowptr), ptr(self.col), ptr(self.trp), ptr(self.tcol))


class GRCN(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        R = self.n_layers = check_config(c, (self.v_feat is not None, self.t_feat is not None))
        self.reg_weight = float(c["reg_weight"])
        self.route_items = str(c["routing"] or "reference") == "items"
        self.embedding_dim = D
        U, I, dev = self.n_users, self.n_items, self.device
        N = self.N = U + I
        self.mods = [(m, feat) for m, feat in (("v", self.v_feat), ("t", self.t_feat)) if feat is not None]
        M = self.M = len(self.mods)
        Wd = self.width = D * (1 + M)
        CW = self.cw = Wd + D + D * M
        init, result0 = draw_init(U, I, [feat.shape[1] for _, feat in self.mods])
        specs = [("conf", (N, M), None), ("E", (N, D), None)]
        for m, feat in self.mods:
            specs += [("pref_" + m, (U, D), None), ("W_" + m, (D, feat.shape[1]), r4(feat.shape[1])), ("b_" + m, (D,), None)]
        s = self.slab = Slab(specs, dev)
        names = ["conf", "E"] + [k + m for m, _ in self.mods for k in ("pref_", "W_", "b_")]
        with torch.no_grad():
            for name, value in zip(names, init.values()):
                s.load(name, value)
        # registered under the reference's names in its order
        self.model_specific_conf = s.parameter("conf")
        self.id_gcn = _EGCN(s.parameter("E"))
        for m, _ in self.mods:
            setattr(self, m + "_gcn", _CGCN(s.parameter("pref_" + m), s.parameter("W_" + m), s.parameter("b_" + m)))
        self._names = names
        self.feat = {}
        for m, feat in self.mods:  # frozen, rows padded to 16 bytes
            buf = torch.zeros((I, r4(feat.shape[1])), dtype=torch.float32, device=dev)
            buf[:, :feat.shape[1]].copy_(feat)
            self.feat[m] = buf[:, :feat.shape[1]]
        g = self.graph = UIGraph(U, I, dataloader.uptr_np, dataloader.uitems_np, dev)
        E = self.E = g.E
        # the reference's edge order (the train interactions as listed) as positions of the CSR
        key = np.asarray(dataloader.u_np, np.int64) * I + np.asarray(dataloader.i_np, np.int64)
        rows = np.repeat(np.arange(U), np.diff(np.asarray(dataloader.uptr_np, np.int64)))
        ckey = rows * I + np.asarray(dataloader.uitems_np, np.int64)
        pos = np.empty(E, np.int64)
        pos[np.argsort(key, kind="stable")] = np.argsort(ckey, kind="stable")
        self._edge_pos = torch.as_tensor(pos).to(dev)
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        n1 = max(E, 1)
        self.Wv, self.WTv = f(2 * n1), f(2 * n1)
        self.adj = K.CSR(g.rowptr_n, g.col_n, self.Wv[:2 * E], symmetric=False)
        self.adj_t = K.CSR(g.rowptr_n, g.col_n, self.WTv[:2 * E], symmetric=False)
        self.arg = torch.zeros(2 * n1, dtype=torch.int32, device=dev)
        self.Z, self.F, self.nrmF = f(I, D * M), f(I, D * M), f(M, I)
        self.P, self.nrm0, self.nrmY = f(R + 1, U, D * M), f(M, U), f(max(R, 1), M, U)
        self.alpha, self.dalpha, self.ds, self.dw = f(M, 2 * n1), f(M, 2 * n1), f(M, 2 * n1), f(2 * n1)
        self.RA, self.RD, self.DY = f(max(R, 1), M, n1), f(max(R, 1), M, n1), f(max(R, 1), U, D * M)
        self.x, self.x1, self.nrmE = f(N, D), f(N, D), f(N)
        self.dx1, self.dx, self.dxd, self.dZ = f(N, D), f(N, D), f(N, D * M), f(I, D * M)
        self.result, self.G = f(N, Wd), f(N, CW)
        self._result0 = result0.to(dev)
        self._table = self._result0
        self._loss, self._sq = f(4), torch.zeros(1024, dtype=torch.float64, device=dev)
        self._w = None
        self._src = None

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order."""
        return [self.slab.gview(n) for n in self._names]

    def _pref(self, m, grad=False):
        s = self.slab
        name = "pref_" + self.mods[min(m, self.M - 1)][0]
        return s.gview(name) if grad else s.view(name)

    # ------------------------------------------------------------------ forward
    def _forward(self):
        """grcn.py:224-298 into self.result (and the rows the backward reads)."""
        s, g, U, I, M, R = self.slab, self.graph, self.n_users, self.n_items, self.M, self.n_layers
        for k, (m, _) in enumerate(self.mods):
            Zm, Fm = self.Z[:, D * k:D * k + D], self.F[:, D * k:D * k + D]
            K.gemm(self.feat[m], s.view("W_" + m), Zm, trans_b=True, epi=K.EPI_LEAKY, bias=s.view("b_" + m), slope=SLOPE)
            K.normalize_rows(Zm, Fm, self.nrmF[k])
            K.normalize_rows(s.view("pref_" + m), self.P[0][:, D * k:D * k + D], self.nrm0[k])
        self.block_forward()
        self._table = self.result

    def block_forward(self):
        """The graph block from f, p^0 and the id embedding: routing, the final attention, refining and the weighted id
        propagation into self.result."""
        s, g, U, M, R = self.slab, self.graph, self.n_users, self.M, self.n_layers
        P, F = self.P, self.F
        _lib.call("gmr_grcn_route_fwd", U, R, M, int(self.route_items), ptr(g.rowptr), ptr(g.col), ptr(F), F.stride(0), ptr(P), P.stride(1),
                  P.stride(0), ptr(self.nrmY), 0, stream())
        rep = self.result[:, D:]
        _lib.call("gmr_grcn_attn_fwd", *g.args[:3], M, *g.args[3:], ptr(P[R]), P.stride(1), ptr(F), F.stride(0), ptr(rep),
                  self.result.stride(0), ptr(self.alpha), 0, stream())
        conf = s.view("conf")
        _lib.call("gmr_grcn_refine_fwd", *g.args[:3], M, *g.args[3:], ptr(g.csr2csc), ptr(g.csc2csr), ptr(self.alpha),
                  ptr(conf), conf.stride(0), ptr(self.Wv), ptr(self.WTv), ptr(self.arg), 0, stream())
        K.normalize_rows(s.view("E"), self.x, self.nrmE)
        idr = self.result[:, :D]
        self.adj.spmm(self.x1, [(self.x,)])
        copy64(self.x1, idr, res=self.x)
        self.adj.spmm(idr, [(self.x1,)], beta=1.0)

    def alpha_ref_order(self):
        """alpha of the last forward as the reference lays it out: 2E x M, the item-destination values in the order of
        the train interactions, then the user-destination ones."""
        E, pos = self.E, self._edge_pos
        a, b = self.alpha[:, :E], self.alpha[:, E:2 * E]
        return torch.cat([b[:, self.graph.csr2csc.long()][:, pos], a[:, pos]], dim=1).t().contiguous()

    # ------------------------------------------------------------------ the step
    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev = self.device
            self._w = {"B": B, "terms": torch.zeros(2 * B, dtype=torch.float32, device=dev),
                       "contrib": torch.zeros((3 * B, self.cw), dtype=torch.float32, device=dev)}
        return self._w

    def _plan(self, users, pos, neg):
        return sort_plan((users, pos, neg), (0, self.n_users, self.n_users))

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0):
        """calculate_loss (grcn.py:300-333) and all parameter gradients (into the slab's twin).  Returns the loss as a
        device scalar; loss_terms() reads [total, bpr, reg, 0]."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: GRCN runs on one device")
        B, U, M, s = users.numel(), self.n_users, self.M, self.slab
        if plan_bpr is None:
            plan_bpr = self._plan(users, pos, neg)
        w = self._work(B)
        self._forward()
        terms, contrib, loss, G = w["terms"][:2 * B], w["contrib"][:3 * B], self._loss, self.G
        pv = s.view("pref_v")
        _lib.call("gmr_grcn_loss_rows", B, U, M, ptr(self.result), self.result.stride(0), ptr(s.view("E")), D, ptr(pv),
                  ptr(self._pref(1)), D, ptr(users), ptr(pos), ptr(neg), 1.0 / (norm_rows or B), self.reg_weight,
                  ptr(terms), ptr(contrib), contrib.stride(0), 0, stream())
        K.zero_(G)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), self.cw, ptr(plan_bpr), ptr(contrib), contrib.stride(0),
                  ptr(G), G.stride(0), stream())
        _lib.call("gmr_sum_f32", B, ptr(terms), 1.0 / (norm_rows or B), ptr(loss[1:]), 0, stream())
        _lib.call("gmr_sum_f32", B, ptr(terms[B:]), self.reg_weight, ptr(loss[2:]), 0, stream())
        _lib.call("gmr_sqnorm_f32", pv.numel(), ptr(pv), self.reg_weight / pv.numel(), ptr(loss[2:]), 1, ptr(self._sq),
                  stream())
        _lib.call("gmr_sum_f32", 2, ptr(loss[1:]), 1.0, ptr(loss), 0, stream())
        self.step_backward()
        return loss[0]

    def _src_terms(self):
        """The (alpha, ds) terms of the two source passes as the host arrays gmr_grcn_bwd_src takes; the buffers are
        the model's own, so they are built once."""
        if self._src is not None:
            return self._src
        E, R, U, M, G, P = self.E, self.n_layers, self.n_users, self.M, self.G, self.P
        n2 = self.alpha.stride(0)

        def pack(terms):
            T = len(terms)
            PA, LA = ctypes.c_void_p * T, ctypes.c_int64 * T
            cols = list(zip(*terms))
            return (T, PA(*cols[0]), PA(*cols[1]), LA(*cols[2]), PA(*cols[3]), LA(*cols[4]), PA(*cols[5]), LA(*cols[6]))

        drep = G[:, D:]
        fl = 4  # bytes per float
        users = pack([(self.alpha.data_ptr() + fl * E, self.ds.data_ptr() + fl * E, n2, drep[U:].data_ptr(),
                       G.stride(0), self.F.data_ptr(), self.F.stride(0))])
        items = [(self.alpha.data_ptr(), self.ds.data_ptr(), n2, drep.data_ptr(), G.stride(0), P[R].data_ptr(),
                  P.stride(1))]
        for r in range(R if self.route_items else 0):
            items.append((self.RA[r].data_ptr(), self.RD[r].data_ptr(), self.RA.stride(1), self.DY[r].data_ptr(),
                          self.DY.stride(1), P[r].data_ptr(), P.stride(1)))
        self._src = (users, pack(items))
        return self._src

    def step_backward(self):
        """All parameter gradients from G = [d result | reg d id | reg d preference] (N x cw)."""
        s, U = self.slab, self.n_users
        s.zero_grad()
        self.block_backward()
        for k, (m, _) in enumerate(self.mods):
            dZ = self.dZ[:, D * k:D * k + D]
            K.normalize_rows_bwd(self.F[:, D * k:D * k + D], self.nrmF[k], self.dxd[U:, D * k:D * k + D], dZ, slope=SLOPE)
            K.gemm(dZ, self.feat[m], s.gview("W_" + m), trans_a=True)
            K.colsum(dZ, s.gview("b_" + m))

    def block_backward(self):
        """The graph block backwards: the gradients of the id embedding, the confidences and the preferences, and
        d loss / d f in self.dxd's item rows."""
        s, g, U, I, M, R, E = self.slab, self.graph, self.n_users, self.n_items, self.M, self.n_layers, self.E
        G, Wd = self.G, self.width
        gid, drep = G[:, :D], G[:, D:]
        # the id branch: dx1 = g + A^T g, dx = g + A^T dx1, dw the sampled products
        copy64(gid, self.dx1)
        self.adj_t.spmm(self.dx1, [(gid,)], beta=1.0)
        copy64(gid, self.dx)
        self.adj_t.spmm(self.dx, [(self.dx1,)], beta=1.0)
        _lib.call("gmr_grcn_dw", *g.args, ptr(self.x), D, ptr(self.x1), D, ptr(self.dx1), D, ptr(gid), G.stride(0),
                  ptr(self.dw), 0, stream())
        gE = s.gview("E")
        copy64(G[:, Wd:Wd + D], gE)
        K.normalize_rows_bwd(self.x, self.nrmE, self.dx, gE, accumulate=True)
        conf, dconf = s.view("conf"), s.gview("conf")
        _lib.call("gmr_grcn_refine_bwd", *g.args[:3], M, *g.args[3:], ptr(g.csr2csc), ptr(g.csc2csr), ptr(self.alpha),
                  ptr(conf), conf.stride(0), ptr(self.arg), ptr(self.dw), ptr(self.dalpha), ptr(dconf), dconf.stride(0),
                  0, stream())
        # the final layer, then the routing rounds in reverse
        P, F, dxd = self.P, self.F, self.dxd
        _lib.call("gmr_grcn_attn_bwd_dst", *g.args[:3], M, *g.args[3:], ptr(P[R]), P.stride(1), ptr(F), F.stride(0),
                  ptr(self.alpha), ptr(self.dalpha), ptr(drep), G.stride(0), ptr(self.ds), ptr(dxd), dxd.stride(0), 0,
                  stream())
        su, si = self._src_terms()
        if E:
            _lib.call("gmr_grcn_bwd_src", U, M, su[0], ptr(g.rowptr), ptr(g.col), ptr(g.csr2csc), *su[1:], ptr(dxd),
                      dxd.stride(0), 0, stream())
        pv = s.view("pref_v")
        reg = G[:U, Wd + D:]
        _lib.call("gmr_grcn_route_bwd_dst", U, E, R, M, int(self.route_items), ptr(g.rowptr), ptr(g.col), ptr(F), F.stride(0), ptr(P),
                  P.stride(1), P.stride(0), ptr(self.nrmY), ptr(dxd), dxd.stride(0), ptr(self.RA), ptr(self.RD),
                  ptr(self.DY), ptr(pv), ptr(self._pref(1)), D, ptr(self.nrm0), ptr(reg), G.stride(0),
                  2.0 * self.reg_weight / pv.numel(), 0.0, ptr(self._pref(0, True)), ptr(self._pref(1, True)), D, 0,
                  stream())
        if E:
            _lib.call("gmr_grcn_bwd_src", I, M, si[0], ptr(g.trp), ptr(g.tcol), ptr(g.csc2csr), *si[1:], ptr(dxd[U:]),
                      dxd.stride(0), 0, stream())

    def loss_terms(self):
        """[total, bpr, reg, 0] of the last rec_step (device tensor)."""
        return self._loss

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward(self):
        self._forward()
        return self.result

    @torch.no_grad()
    def forward_embeddings(self):
        """full_sort_predict's tables (grcn.py:335-341): the rows of the table the last forward wrote (the random init
        table before any step); nothing is recomputed in evaluation, as in the reference."""
        return self._table[:self.n_users], self._table[self.n_users:]
