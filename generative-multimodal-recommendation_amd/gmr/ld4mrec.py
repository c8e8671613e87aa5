"""LD4MRec on MI355X — drop-in for models/ld4mrec.py of the reference (GeneralRecommender API).

A diffusion recommender over per-user interaction rows whose denoiser (C-Net) is conditioned on the user, with
one-step inference.  What it computes, in this package's words:

Init
  user_svd_emb  U_k sqrt(S_k) of the rank-svd_k truncated SVD of the train matrix R (largest singular values
                first, fp32).  Not a parameter.  The Lanczos start vector is random, so two constructions agree
                only up to column signs and low bits: the table may be injected (constructor argument or
                set_user_svd_emb) and travels in extra_state, so a resumed run scores with the table it trained with.
  user_mm_emb   D_u^-1/2 R D_i^-1/2 [v_feat | t_feat]  (U x (Dv + Dt), fp32; D^-1/2 of a zero degree is 0), one
                SpMM per block of feature columns, computed once and kept on the device.  Not a parameter.
  schedule      1 - ab_t = a + (t - 1)/(T - 1) (1 - a) for t = 1..T (a = min_noise_level);  alpha_t = ab_t / ab_{t-1}
                (ab_0 = 1);  beta = clamp(1 - alpha, 1e-4, 0.9999);  alpha_bar = cumprod(1 - beta).  fp32, in this
                order (evaluated with CPU torch so that alpha_bar equals the reference's bit for bit, then moved).
  parameters    t_in (1); mm_project (64 x (Dv + Dt)); cnet.item_proj (H x I); cnet.cond_proj (H x (svd_k + 64));
                cnet.time_proj (H x H); per layer norm1, linear1, linear2, cond_scale, cond_shift; cnet.output_proj
                (I x H).  nn.Linear default init, the RNG consumed in that order (mm_project first).
  loss_history  buffer of T ones (in state_dict): the importance weights of the timesteps.

calculate_loss(users)   (duplicates kept)
  x_in   = the users' binary train rows;  target = x_in (1 - gamma) + (1 - x_in) gamma   (gamma = smoothing_gamma)
  t      ~ p, p = |loss_history| / sum;  eps ~ N(0, 1);  x_t = sqrt(ab[t]) x_in + sqrt(1 - ab[t]) eps
  cond   = [user_svd_emb[u] | mm_project(user_mm_emb[u])]
  temb(t)= [sin(t f) | cos(t f)],  f_k = exp(-k ln(1e4) / (H/2 - 1))
  C-Net:   h = item_proj(x_t);  g = cond_proj(cond) + time_proj(temb(t));
           per layer, n = LN(h):  h <- h + linear2(dropout(GELU(linear1(n (1 + cond_scale(g)) + cond_shift(g)))))
           (exact erf GELU; dropout in train mode only);  pred = output_proj(h)
  loss_b = mean_I (pred_b - target_b)^2;  loss = mean_b loss_b
  loss_history[t_b] <- 0.9 loss_history[t_b] + 0.1 loss_b, row by row in batch order (fp32; rows sharing a t compound)
  t_in takes no gradient (prediction only) and so stays 0.

full_sort_predict(users): scores = C-Net(x_in, temb(|t_in|), cond) in eval mode - one forward pass on the clean
  history, raw scores.

On the device
  One Slab holds every parameter.  The cond_scale / cond_shift weights of all L layers lie contiguously as
  Wss = [scale_0; shift_0; scale_1; ...] (2LH x H), so the modulation of every layer is ONE product
  S = g Wss^T + bss (B x 2LH), its dg one product and its weight gradient one product.  g itself is one product:
  time_proj(temb(t)) takes T values, so TP = time_proj(temb table) + cond_proj.bias is a T x H table (recomputed
  per step) added by the GEMM's bias_row epilogue.  x_t is built from the user CSR (gmr_diff_qsample), the
  residual add rides the linear2 GEMM epilogue, and the rows between the products are csrc/ld4m.hip:
  gmr_ld4_film_fwd/bwd, gmr_ld4_gelu_drop_fwd/bwd, gmr_ld4_loss_rows, gmr_ld4_history_ema, gmr_ld4_sample_t.
  Backward (hand-derived, gradients written straight into the slab's twin), from dpred = 2 (pred - target)/(I B):
    dWo = dpred^T h_L, dbo = colsum(dpred), dh = dpred Wo
    layer l = L-1..0:  dW2 = dh^T y_l, db2 = colsum(dh), da = (dh W2) * keep/p * gelu'(a_l)
                       dW1 = da^T z_l, db1 = colsum(da), dz = da W1   (written into the shift slot of dS)
                       film_bwd: dS[scale_l] = dz n, dS[shift_l] = dz, dh += LN-backward(dz (1 + s)), dnorm1
    dWi = dh^T x_t, dbi = colsum(dh)
    dWss = dS^T g, dbss = colsum(dS), dg = dS Wss
    dWc = dg^T cond, dbc = colsum(dg), dTP[t] = sum of the dg rows with that t, dWt = dTP^T temb, dbt = colsum(dTP)
    dmm = (dg Wc[:, svd_k:]) -> dmm_W = dmm^T mm_rows, dmm_b = colsum(dmm)
  Prediction needs no densified rows: item_proj(x_in) is the sum of the item_proj columns of the user's items
  (gmr_diff_sparse_pre over a transposed copy of the weight, then gmr_ld4_add_bias).
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import GeneralRecommender, config_seed, r4
from .denoise import _Linear
from .kernels import ptr, stream
from .slab import Slab

MM_DIM = 64          # mm_project output width = embedding_size of the reference yaml
DROP_SEED = 0x4C44344D  # xor-ed into the seed for the dropout draws (their key space is (seed, step, counter))


def check_config(config, n_users, n_items):
    """Raise NotImplementedError naming the key for settings outside the hot path; returns (H, L, T, k)."""
    H, L = int(config["cnet_hidden_size"]), int(config["cnet_n_layers"])
    T, k = int(config["steps"]), int(config["svd_k"])
    if H % 64 or not 64 <= H <= 1024:
        raise NotImplementedError(f"cnet_hidden_size = {H}: a multiple of 64 in 64..1024 (the row kernels' widths)")
    if not 1 <= L <= 8:
        raise NotImplementedError(f"cnet_n_layers = {L}: 1..8")
    if not 2 <= T <= 1024:
        raise NotImplementedError(f"steps = {T}: 2..1024")
    if not 1 <= k < min(n_users, n_items):
        raise NotImplementedError(f"svd_k = {k}: must be below min(n_users, n_items) = {min(n_users, n_items)}")
    if int(config["embedding_size"] or MM_DIM) != MM_DIM:
        raise NotImplementedError(f"embedding_size = {config['embedding_size']}: {MM_DIM} (LD4MRec.yaml)")
    return H, L, T, k


def ld4_schedule(steps, min_noise_level):
    """alpha_bar (T, fp32, CPU) in the reference's order of operations."""
    t = torch.arange(1, steps + 1, dtype=torch.float32)
    one_minus = 1.0 * (min_noise_level + (t - 1) / (steps - 1) * (1 - min_noise_level))
    ab = 1 - one_minus
    prev = torch.cat([torch.tensor([1.0]), ab[:-1]])
    betas = torch.clamp(1 - ab / prev, min=0.0001, max=0.9999)
    return torch.cumprod(1 - betas, dim=0)


def time_embedding(timesteps, H):
    """[sin(t f) | cos(t f)], f_k = exp(-k ln(1e4) / (H/2 - 1)); timesteps: 1-D tensor (any dtype)."""
    half = H // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32, device=timesteps.device) * -np.log(10000.0) / (half - 1))
    e = timesteps[:, None].float() * f[None, :]
    return torch.cat([torch.sin(e), torch.cos(e)], dim=1)


def svd_user_table(rows, cols, n_users, n_items, k):
    """U_k sqrt(S_k) of the train matrix, largest singular values first (fp32, host)."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import svds
    R = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items)).astype(np.float32)
    u, s, _ = svds(R, k=k)
    return torch.from_numpy(np.ascontiguousarray(u[:, ::-1] * np.sqrt(s[::-1]))).float()


class _LD4Loss(torch.autograd.Function):
    """calculate_loss as an autograd node: the fused step fills the slab's gradient; backward hands it to the
    parameters scaled by the incoming gradient."""

    @staticmethod
    def forward(ctx, model, users, *params):
        loss = model.rec_step(users)
        ctx.model = model
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        return (None, None, *[gv * g for gv in ctx.model._grad_views])


class _Block(nn.Module):
    def __init__(self, norm1, linear1, linear2, cond_scale, cond_shift):
        super().__init__()
        self.norm1, self.linear1, self.linear2 = norm1, linear1, linear2
        self.cond_scale, self.cond_shift = cond_scale, cond_shift


class _CNet(nn.Module):
    def __init__(self, item_proj, cond_proj, time_proj, layers, output_proj):
        super().__init__()
        self.item_proj, self.cond_proj, self.time_proj = item_proj, cond_proj, time_proj
        self.layers = nn.ModuleList(layers)
        self.output_proj = output_proj


class LD4MRec(GeneralRecommender):
    rec_step_takes_row0 = True

    def __init__(self, config, dataloader, user_svd_emb=None):
        super().__init__(config, dataloader)
        c = config
        self.config = config
        U, I = self.n_users, self.n_items
        H, L, T, k = check_config(c, U, I)
        if self.v_feat is None and self.t_feat is None:
            raise NotImplementedError("is_multimodal_model = False: LD4MRec conditions on the modal features")
        self.H, self.L, self.steps, self.svd_k = H, L, T, k
        self.gamma = float(c["smoothing_gamma"])
        self.keep_prob = 1.0 - float(c["dropout"] or 0.0)
        self.seed = config_seed(c)
        dev = self.device
        feats = torch.cat([f for f in (self.v_feat, self.t_feat) if f is not None], dim=1)
        D = self.mm_dim = feats.shape[1]
        C = self.cond_dim = k + MM_DIM
        self.user_ptr = torch.as_tensor(dataloader.uptr_np).to(dev)
        self.user_items = torch.as_tensor(dataloader.uitems_np).to(dev)

        # ---- parameters (one slab); RNG consumed as the reference's constructor does
        specs = [("t_in", (1,), None), ("mm_W", (MM_DIM, D), r4(D)), ("mm_b", (MM_DIM,), None),
                 ("Wi", (H, I), r4(I)), ("bi", (H,), None), ("Wc", (H, C), r4(C)), ("bc", (H,), None),
                 ("Wt", (H, H), None), ("bt", (H,), None)]
        for l in range(L):
            specs += [(f"n1w{l}", (H,), None), (f"n1b{l}", (H,), None), (f"W1_{l}", (H, H), None),
                      (f"b1_{l}", (H,), None), (f"W2_{l}", (H, H), None), (f"b2_{l}", (H,), None)]
        specs += [("Wss", (2 * L * H, H), None), ("bss", (2 * L * H,), None), ("Wo", (I, H), None), ("bo", (I,), None)]
        s = self.slab = Slab(specs, dev)
        self._grad_views, self._param_list = [], []

        def lin(wn, bn, rows=None):
            wv, bv, gw, gb = s.view(wn), s.view(bn), s.gview(wn), s.gview(bn)
            if rows is not None:
                wv, bv, gw, gb = wv[rows], bv[rows], gw[rows], gb[rows]
            w, b = nn.Parameter(wv), nn.Parameter(bv)
            w.grad, b.grad = gw, gb
            self._param_list += [w, b]
            self._grad_views += [gw, gb]
            return _Linear(w, b)

        self.t_in = s.parameter("t_in")
        self._param_list.append(self.t_in)
        self._grad_views.append(s.gview("t_in"))
        self.mm_project = lin("mm_W", "mm_b")
        item_proj, cond_proj, time_proj = lin("Wi", "bi"), lin("Wc", "bc"), lin("Wt", "bt")
        blocks = []
        for l in range(L):
            blocks.append(_Block(lin(f"n1w{l}", f"n1b{l}"), lin(f"W1_{l}", f"b1_{l}"), lin(f"W2_{l}", f"b2_{l}"),
                                 lin("Wss", "bss", slice(2 * l * H, (2 * l + 1) * H)),
                                 lin("Wss", "bss", slice((2 * l + 1) * H, (2 * l + 2) * H))))
        self.cnet = _CNet(item_proj, cond_proj, time_proj, blocks, lin("Wo", "bo"))
        self._init_like_reference()
        self.register_buffer("loss_history", torch.ones(T, dtype=torch.float32, device=dev))

        # ---- fixed tables
        if user_svd_emb is None:
            rows = np.repeat(np.arange(U), np.diff(dataloader.uptr_np))
            user_svd_emb = svd_user_table(rows, np.asarray(dataloader.uitems_np), U, I, k)
        self.set_user_svd_emb(user_svd_emb)
        self.user_mm_emb = self._build_user_mm_emb(feats)
        self.alpha_bar = ld4_schedule(T, float(c["min_noise_level"]))
        self._sqrt_ab = torch.sqrt(self.alpha_bar).to(dev)
        self._sqrt_1mab = torch.sqrt(1 - self.alpha_bar).to(dev)
        self.alpha_bar = self.alpha_bar.to(dev)
        self._temb = time_embedding(torch.arange(T, device=dev), H).contiguous()
        self._w = None
        self._step = 0
        self._loss32 = torch.zeros(1, dtype=torch.float32, device=dev)
        self._loss64 = torch.zeros(1, dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ construction
    @torch.no_grad()
    def _init_like_reference(self):
        H, L, I, s = self.H, self.L, self.n_items, self.slab

        def put(layer, wn, bn, rows=None):
            wv, bv = s.view(wn), s.view(bn)
            if rows is not None:
                wv, bv = wv[rows], bv[rows]
            wv.copy_(layer.weight)
            bv.copy_(layer.bias)

        put(nn.Linear(self.mm_dim, MM_DIM), "mm_W", "mm_b")
        put(nn.Linear(I, H), "Wi", "bi")
        put(nn.Linear(self.cond_dim, H), "Wc", "bc")
        put(nn.Linear(H, H), "Wt", "bt")
        for l in range(L):
            s.view(f"n1w{l}").fill_(1.0)
            put(nn.Linear(H, H), f"W1_{l}", f"b1_{l}")
            put(nn.Linear(H, H), f"W2_{l}", f"b2_{l}")
            put(nn.Linear(H, H), "Wss", "bss", slice(2 * l * H, (2 * l + 1) * H))
            put(nn.Linear(H, H), "Wss", "bss", slice((2 * l + 1) * H, (2 * l + 2) * H))
        put(nn.Linear(H, I), "Wo", "bo")

    def set_user_svd_emb(self, table):
        table = torch.as_tensor(table, dtype=torch.float32)
        if tuple(table.shape) != (self.n_users, self.svd_k):
            raise ValueError(f"user_svd_emb must be {self.n_users} x {self.svd_k}")
        pad = torch.zeros((self.n_users, r4(self.svd_k)), dtype=torch.float32, device=self.device)
        pad[:, :self.svd_k] = table.to(self.device)
        self._svd_pad = pad  # rows padded to a multiple of 4 floats for the float4 gather
        self.user_svd_emb = pad[:, :self.svd_k]

    @torch.no_grad()
    def _build_user_mm_emb(self, feats):
        """D_u^-1/2 R D_i^-1/2 feats on the device: the entry values from the degrees, then one SpMM per block of
        up to 256 feature columns (the SpMM plans take 64-column blocks; the pad columns are zero)."""
        U, I, dev = self.n_users, self.n_items, self.device
        D = feats.shape[1]
        Dp = (D + 63) // 64 * 64
        X = torch.zeros((I, Dp), dtype=torch.float32, device=dev)
        X[:, :D] = feats
        cnt = (self.user_ptr[1:] - self.user_ptr[:-1]).long()
        items = self.user_items.long()
        # the U + I inverse square roots on the host in fp32 (np.power, as the reference takes them): a device
        # pow differs in the last bit for some degrees, which shows at 1e-4 relative where a row's terms cancel

        def inv_sqrt(deg):
            with np.errstate(divide="ignore"):
                r = np.power(deg.cpu().numpy().astype(np.float32), -0.5)
            r[np.isinf(r)] = 0.0
            return torch.from_numpy(r).to(dev)

        du, di = inv_sqrt(cnt), inv_sqrt(torch.bincount(items, minlength=I))
        val = (du.repeat_interleave(cnt) * di[items]).contiguous()
        A = K.CSR(self.user_ptr, self.user_items, val, n_cols=I, symmetric=False)
        out = torch.empty((U, Dp), dtype=torch.float32, device=dev)
        c = 0
        while c < Dp:
            nb = 4 if Dp - c >= 256 else 2 if Dp - c >= 128 else 1
            A.spmm(out[:, c:c + 64 * nb], [(X[:, c + 64 * j:c + 64 * (j + 1)],) for j in range(nb)])
            c += 64 * nb
        self._mm_pad = out  # U x Dp, pad columns zero
        return out[:, :D]

    def optim_slabs(self):
        return [self.slab]

    # ------------------------------------------------------------------ buffers
    def _work(self, B):
        if self._w is not None and self._w["B"] >= B:
            return self._w
        I, H, L, T, dev = self.n_items, self.H, self.L, self.steps, self.device
        Ip, Cp, Dp = r4(I), r4(self.cond_dim), r4(self.mm_dim)
        f = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)  # noqa: E731
        parts = int(_lib.load().gmr_ld4_film_parts_floats(B, H))
        self._w = {"B": B, "x": f(B, Ip), "pred": f(B, Ip), "cond": torch.zeros((B, Cp), device=dev), "mm": f(B, Dp),
                   "g": f(B, H), "S": f(B, 2 * L * H), "dS": f(B, 2 * L * H), "h": f(L + 1, B, H), "z": f(L, B, H),
                   "a": f(L, B, H), "y": f(L, B, H), "mask": f(L, B, H, dt=torch.uint8), "mean": f(L, B),
                   "rstd": f(L, B), "dh": f(B, H), "da": f(B, H), "dg": f(B, H), "dcm": f(B, MM_DIM), "TP": f(T, H),
                   "dTP": f(T, H), "bsum": f(H), "parts": f(max(parts, 1)), "rowloss": f(B, dt=torch.float64),
                   "t": f(B, dt=torch.int32), "TP1": f(1, H), "WiT": f(I, H)}
        return self._w

    # ------------------------------------------------------------------ forward pieces
    def _condition(self, users, w, B):
        """cond = [user_svd_emb[u] | mm_project(user_mm_emb[u])] (B x (svd_k + 64))."""
        s, k = self.slab, self.svd_k
        cond = w["cond"][:B]
        mm = w["mm"][:B, :self.mm_dim]
        # float4 gathers over the zero-padded tables; the mm_project product then overwrites cond[:, k:]
        K.gather_rows(self._svd_pad, users, cond[:, :r4(k)])
        K.gather_rows(self._mm_pad, users, w["mm"][:B])
        K.gemm(mm, s.view("mm_W"), cond[:, k:k + MM_DIM], trans_b=True, epi=K.EPI_BIAS, bias=s.view("mm_b"))
        return cond[:, :self.cond_dim], mm

    def _time_table(self, temb, out, w):
        """out = time_proj(temb) + cond_proj.bias (rows of temb)."""
        s = self.slab
        torch.add(s.view("bt"), s.view("bc"), out=w["bsum"])
        return K.gemm(temb, s.view("Wt"), out, trans_b=True, epi=K.EPI_BIAS, bias=w["bsum"])

    def _blocks_fwd(self, w, B, g, train, masks, row0):
        """The L conditional blocks on w['h'][0]; saves z, a, y, mean, rstd (and the masks) per layer."""
        s, H, L = self.slab, self.H, self.L
        S = w["S"][:B]
        K.gemm(g, s.view("Wss"), S, trans_b=True, epi=K.EPI_BIAS, bias=s.view("bss"))
        pk = self.keep_prob if train else 1.0
        for l in range(L):
            h, hn = w["h"][l, :B], w["h"][l + 1, :B]
            z, a, y, mk = w["z"][l, :B], w["a"][l, :B], w["y"][l, :B], w["mask"][l, :B]
            sc, sh = S[:, 2 * l * H:(2 * l + 1) * H], S[:, (2 * l + 1) * H:(2 * l + 2) * H]
            _lib.call("gmr_ld4_film_fwd", B, H, ptr(h), h.stride(0), ptr(s.view(f"n1w{l}")), ptr(s.view(f"n1b{l}")),
                      ptr(sc), sc.stride(0), ptr(sh), sh.stride(0), 1e-5, ptr(z), z.stride(0), ptr(w["mean"][l]),
                      ptr(w["rstd"][l]), stream())
            K.gemm(z, s.view(f"W1_{l}"), a, trans_b=True, epi=K.EPI_BIAS, bias=s.view(f"b1_{l}"))
            if masks is not None and pk < 1.0:
                mk.copy_(masks[l])
            _lib.call("gmr_ld4_gelu_drop_fwd", B, H, ptr(a), a.stride(0), pk,
                      ptr(mk) if masks is not None else None, ptr(mk), mk.stride(0), self.seed ^ DROP_SEED, self._step,
                      (l << 40) + row0 * H, ptr(y), y.stride(0), stream())
            # h' = 1 (y W2^T + b2) + 1 h: the residual add in the epilogue
            K.gemm(y, s.view(f"W2_{l}"), hn, trans_b=True, epi=K.EPI_POSTERIOR, bias=s.view(f"b2_{l}"), aux=h,
                   slope=1.0, beta=1.0)
        return w["h"][L, :B]

    # ------------------------------------------------------------------ training
    _marks = None  # scripts/ld4mrec_step.py sets a list: (phase, HIP event) is appended at every phase boundary

    def _mark(self, name):
        if self._marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._marks.append((name, e))

    def rec_step(self, users, pos=None, neg=None, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0,
                 t=None, noise=None, masks=None, row0=0, u=None):
        """Forward + hand-derived backward for the users of one batch (duplicates kept).  Returns the batch loss
        (a device fp32 scalar); gradients land in the slab's twin.  t (int B), noise (B x I fp32), masks (L
        tensors of B x H keep bytes) and u (B uniforms for the draw of t) may be injected (parity tests);
        otherwise they come from the device Philox.  The per-row losses stay in self.row_loss (fp64)."""
        if dist.is_dist():
            raise NotImplementedError("LD4MRec runs on one device")
        s, H, L, I, T, k = self.slab, self.H, self.L, self.n_items, self.steps, self.svd_k
        B = users.numel()
        nr = float(norm_rows or B)
        w = self._work(B)
        x, pred, tt = w["x"][:B], w["pred"][:B], w["t"][:B]
        sid = self._step
        self._mark("start")
        if t is None:
            _lib.call("gmr_ld4_sample_t", B, T, ptr(self.loss_history), ptr(u), self.seed, sid, row0, ptr(tt), stream())
        else:
            tt.copy_(t)
        _lib.call("gmr_diff_qsample", B, I, ptr(users), ptr(self.user_ptr), ptr(self.user_items), ptr(tt),
                  ptr(self._sqrt_ab), ptr(self._sqrt_1mab), ptr(noise), noise.stride(0) if noise is not None else 0,
                  None, 0, 1.0, 0, self.seed, sid, row0, ptr(x), x.stride(0), stream())
        self._mark("draw_xt")
        xi, po = x[:, :I], pred[:, :I]
        cond, mm = self._condition(users, w, B)
        TP = self._time_table(self._temb, w["TP"], w)
        g = w["g"][:B]
        K.gemm(cond, s.view("Wc"), g, trans_b=True, epi=K.EPI_BIAS, bias=TP, bias_row=tt, ld_bias=H)
        self._mark("cond_g")
        K.gemm(xi, s.view("Wi"), w["h"][0, :B], trans_b=True, epi=K.EPI_BIAS, bias=s.view("bi"))
        self._mark("item_proj")
        hL = self._blocks_fwd(w, B, g, True, masks, row0)
        self._mark("blocks_fwd")
        K.gemm(hL, s.view("Wo"), po, trans_b=True, epi=K.EPI_BIAS, bias=s.view("bo"))
        self._mark("output_proj")
        _lib.call("gmr_ld4_loss_rows", B, I, ptr(users), ptr(self.user_ptr), ptr(self.user_items), self.gamma, ptr(po),
                  po.stride(0), 1.0 / nr, ptr(w["rowloss"]), 1, stream())
        self.row_loss = w["rowloss"][:B]
        self._mark("loss_rows")
        # ---- backward
        dh, da, dS, dg = w["dh"][:B], w["da"][:B], w["dS"][:B], w["dg"][:B]
        K.gemm(po, hL, s.gview("Wo"), trans_a=True)
        K.colsum(po, s.gview("bo"))
        K.gemm(po, s.view("Wo"), dh)
        self._mark("output_proj_bwd")
        S = w["S"][:B]
        for l in reversed(range(L)):
            h, z, a, y, mk = w["h"][l, :B], w["z"][l, :B], w["a"][l, :B], w["y"][l, :B], w["mask"][l, :B]
            K.gemm(dh, y, s.gview(f"W2_{l}"), trans_a=True)
            K.colsum(dh, s.gview(f"b2_{l}"))
            K.gemm(dh, s.view(f"W2_{l}"), da)
            _lib.call("gmr_ld4_gelu_drop_bwd", B, H, ptr(a), a.stride(0), ptr(mk), mk.stride(0), self.keep_prob, ptr(da),
                      da.stride(0), ptr(da), da.stride(0), stream())
            K.gemm(da, z, s.gview(f"W1_{l}"), trans_a=True)
            K.colsum(da, s.gview(f"b1_{l}"))
            sc = S[:, 2 * l * H:(2 * l + 1) * H]
            dsc, dsh = dS[:, 2 * l * H:(2 * l + 1) * H], dS[:, (2 * l + 1) * H:(2 * l + 2) * H]
            K.gemm(da, s.view(f"W1_{l}"), dsh)  # dz, in place as d shift
            _lib.call("gmr_ld4_film_bwd", B, H, ptr(h), h.stride(0), ptr(w["mean"][l]), ptr(w["rstd"][l]),
                      ptr(s.view(f"n1w{l}")), ptr(s.view(f"n1b{l}")), ptr(sc), sc.stride(0), ptr(dsh), dsh.stride(0),
                      ptr(dsc), dsc.stride(0), ptr(dsh), dsh.stride(0), ptr(dh), dh.stride(0), 1, ptr(w["parts"]),
                      ptr(s.gview(f"n1w{l}")), ptr(s.gview(f"n1b{l}")), 0, stream())
        self._mark("blocks_bwd")
        K.gemm(dh, xi, s.gview("Wi"), trans_a=True)
        K.colsum(dh, s.gview("bi"))
        self._mark("item_proj_bwd")
        K.gemm(dS, g, s.gview("Wss"), trans_a=True)
        K.colsum(dS, s.gview("bss"))
        K.gemm(dS, s.view("Wss"), dg)
        K.gemm(dg, cond, s.gview("Wc"), trans_a=True)
        K.colsum(dg, s.gview("bc"))
        K.colsum(dg, w["dTP"], group=tt, n_groups=T)
        K.gemm(w["dTP"], self._temb, s.gview("Wt"), trans_a=True)
        K.colsum(w["dTP"], s.gview("bt"))
        dcm = w["dcm"][:B]
        K.gemm(dg, s.view("Wc")[:, k:k + MM_DIM], dcm)
        K.gemm(dcm, mm, s.gview("mm_W"), trans_a=True)
        K.colsum(dcm, s.gview("mm_b"))
        self._mark("cond_bwd")
        # ---- loss and history
        _lib.call("gmr_sum_f64", B, ptr(w["rowloss"]), 1.0 / nr, ptr(self._loss64), 0, stream())
        self._loss32.copy_(self._loss64)
        _lib.call("gmr_ld4_history_ema", B, T, ptr(tt), ptr(w["rowloss"]), ptr(self.loss_history), stream())
        self._mark("loss_history")
        self._step += 1
        return self._loss32[0]

    def calculate_loss(self, interaction):
        users = interaction[0].to(torch.int32).contiguous()
        for p in self._param_list:
            p.grad = None
        return _LD4Loss.apply(self, users, *self._param_list)

    def extra_state(self):
        """What a resumed run needs beside state_dict: the SVD table it trained with (not reproducible bit for
        bit) and the Philox step counter."""
        return {"user_svd_emb": self.user_svd_emb.cpu(), "counters": {"step": self._step}}

    def load_extra_state(self, st):
        self.set_user_svd_emb(st["user_svd_emb"])
        self._step = int(st["counters"]["step"])

    # ------------------------------------------------------------------ prediction
    def _transpose_wi(self, WiT):
        Wi = self.slab.view("Wi")
        _lib.call("gmr_transpose_f32", self.H, self.n_items, ptr(Wi), Wi.stride(0), ptr(WiT), WiT.stride(0), stream())

    @torch.no_grad()
    def full_sort_predict(self, interaction):
        """scores = C-Net(x_in, temb(|t_in|), cond), no dropout; x_in is read as item lists (no B x I input).
        The result is a view of the model's work buffer (as DiffRec's): the next call overwrites it."""
        s, H, I = self.slab, self.H, self.n_items
        users = interaction[0].to(torch.int32).contiguous()
        B = users.numel()
        w = self._work(B)
        cond, _ = self._condition(users, w, B)
        temb = time_embedding(torch.abs(s.view("t_in")), H)
        TP1 = self._time_table(temb, w["TP1"], w)
        g = w["g"][:B]
        K.gemm(cond, s.view("Wc"), g, trans_b=True, epi=K.EPI_BIAS, bias=TP1[0])
        WiT, h0, scratch = w["WiT"], w["h"][0, :B], w["da"][:B]
        # the I x H copy of item_proj.weight is rebuilt per call: Adam writes the slab through the C-ABI, past
        # torch's version counter, so there is no version to key a cache on (10 us of a 0.41 ms 4,096-user call)
        self._transpose_wi(WiT)
        _lib.call("gmr_diff_sparse_pre", B, H, ptr(users), ptr(self.user_ptr), ptr(self.user_items), ptr(WiT),
                  WiT.stride(0), ptr(s.view("bi")), ptr(h0), h0.stride(0), ptr(scratch), scratch.stride(0), stream())
        _lib.call("gmr_ld4_add_bias", B, H, ptr(h0), h0.stride(0), ptr(s.view("bi")), ptr(h0), h0.stride(0), stream())
        hL = self._blocks_fwd(w, B, g, False, None, 0)
        po = w["pred"][:B, :I]
        K.gemm(hL, s.view("Wo"), po, trans_b=True, epi=K.EPI_BIAS, bias=s.view("bo"))
        return po
