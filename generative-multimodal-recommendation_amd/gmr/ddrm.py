"""DDRM on MI355X — drop-in for models/ddrm.py of the reference (GeneralRecommender API).

Diffusion in embedding space: a LightGCN encoder gives 64-wide user / item rows, two conditional denoisers (one per
side) learn to rebuild a row from its noised copy given the partner's row, and prediction generates an "ideal item"
row per user from the noised mean of the user's history and scores it against all items.  What it computes:

Init
  parameters  rec_model.embedding_user / embedding_item (N(0, 0.1^2)); per denoiser emb_layer (64 x 64), in_layers.0
              (H x 192, columns [x | time | cond]), out_layers.0 (64 x H), H = dims[0]; every denoiser tensor
              N(0, 2 / (fan_in + fan_out)), biases N(0, 1e-6), drawn after nn.Linear's own init consumed its draws.
  graph       D^-1/2 A D^-1/2 of the binary bipartite train graph, no self loops, D^-1/2 of a zero degree 0.
  schedule    fp64: variance v = linspace(noise_scale noise_min, noise_scale noise_max, T), alpha_bar' = 1 - v,
              beta_0 = v_0, beta_i = min(1 - alpha_bar'_i / alpha_bar'_{i-1}, 0.999) ('linear-var'; 'linear': beta = v);
              then beta_0 = 1e-5; alpha_bar = cumprod(1 - beta); posterior c1 = beta sqrt(ab_prev) / (1 - ab),
              c2 = (1 - ab_prev) sqrt(1 - beta) / (1 - ab), log variance with entry 1 repeated at entry 0.  Tables
              are cast to fp32 where they are read.

encoder      [ua; ia] = mean(E_0 .. E_n), E_{k+1} = adj E_k  (n = lightGCN_n_layers)
denoiser     net(x, cond, t) = W2 tanh(W1 [drop(x) | emb_layer(temb(t)) | cond] + b1) + b2,
             temb(t) = [cos(t f) | sin(t f)], f_k = exp(-k ln(1e4) / 32); drop = nn.Dropout(0.5) in train mode only

calculate_loss(users, pos, neg)   (B rows, duplicates kept)
  u, p, n = ua[users], ia[pos], ia[neg];  t ~ U{0..T-1} per row, shared by both models;  two noises
  out_u = net_user(q_sample(u, t), cond = p, t);  out_i = net_item(q_sample(p, t), cond = u, t)
  rec_b = (mean_64 (u - out_u)^2 + mean_64 (p - out_i)^2) / 2
  reg   = (|E0_u[users]|^2 + |E0_i[pos]|^2 + |E0_i[neg]|^2) / (2 B)      (a scalar over the gathered rows)
  w_b   = sigmoid(<u, p>)^beta, no gradient
  loss  = mean_b w_b ((1 - alpha) (softplus(<u, n> - <u, p>) + reg_weight reg) + alpha rec_b)

full_sort_predict(users)
  x_start = mean of ia over the user's train items (count clamped to 1);  x = q_sample(x_start, T - 1, noise)
  for i = sampling_steps-1 .. 0:  x <- c1[i] net_item(x, cond = ua[user], i) + c2[i] x
                                  (+ exp(logvar[i] / 2) noise_i where i != 0, with sampling_noise)
  scores = x ia^T

On the device
  One Slab holds E = [E0_u; E0_i] and both denoisers.  The encoder is FREEDOM's: SpMM per layer, gmr_frd_mean_fwd,
  the backward a Horner chain over the symmetric adjacency.  A denoiser's training forward is ONE launch
  (gmr_ddrm_denoise_fwd: gather, q_sample, dropout, both layers, the row MSE), with the time columns folded: only T
  timesteps exist, so TB = emb_layer(temb(0..T-1)) W1[:, 64:128]^T + b1 is a T x H table rebuilt per step by two
  small GEMMs and read by row t.  gmr_ddrm_loss_fwd_bwd gives the loss, the contribution rows of [users | pos | neg]
  and d out of both models.  Backward of a denoiser (GEMMs of this package and two grouped column sums):
    dW2 = dout^T h, db2 = colsum(dout), da = (dout W2) (1 - h^2)
    dW1[:, x] = da^T xd, dW1[:, cond] = da^T cond, dTB[t] = sum of the da rows with that t (deterministic grouped sum)
    db1 = colsum(dTB), dW1[:, time] = dTB^T E, dE = dTB W1[:, time], dWe = dE^T temb, dbe = colsum(dE)
    dxd = da W1[:, x], dcond = da W1[:, cond] -> gmr_ddrm_input_bwd adds sqrt_ac[t] 2 keep dxd to the row's own
    contribution and dcond to the partner's
  then one sorted scatter through the loader's BPR plan, the Horner chain, and the reg term: the gathered E0 rows
  scattered through the same plan (row counts included) times the device scalar (1 - alpha) reg_weight mean(w) / B.
  Prediction: the history mean is one SpMM over the user CSR with values 1 / max(deg, 1); q_sample at T - 1 and the
  whole reverse chain are one launch (gmr_ddrm_chain).  forward_embeddings returns (generated U x 64, ia), so the
  trainer's fused score -> mask -> top-K kernel serves DDRM unchanged.

Random draws: t, both noises and both keep masks come from Philox (seed, step counter, site, row) unless injected; the
eval noise from Philox (seed, eval-pass counter, user id), so scores do not depend on the eval batching.  Both
counters travel in extra_state().
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import dist
from . import kernels as K
from .abstract_recommender import EmbeddingRecommender, config_seed, copy64, sort_plan
from .freedom import _Linear, _Table
from .kernels import ptr, stream
from .slab import Slab

D = 64
MAX_TABLES = 8  # GMR_FRD_MAX_LAYERS of include/gmr.h: the layer mean takes n_layers + 1 tables
SITE_T, SITE_U, SITE_I, SITE_EVAL, SITE_CHAIN = 0x7444, 0x10, 0x20, 0x30, 0x40


def check_config(config):
    """Raise NotImplementedError naming the key for settings outside the hot path; returns (H, n_layers, T)."""
    c = config
    if int(c["embedding_size"] or D) != D:
        raise NotImplementedError(f"embedding_size = {c['embedding_size']}: {D} (the SpMM blocks and the denoiser "
                                  f"tiles are 64 columns)")
    if c["dropout"]:
        raise NotImplementedError("dropout = True: the encoder's independent edge drop needs a transposed CSR per step")
    if c["A_split"]:
        raise NotImplementedError("A_split = True: the graph is one CSR here")
    if (c["act"] or "tanh") != "tanh":
        raise NotImplementedError(f"act = {c['act']}: tanh (DDRM.yaml)")
    if c["norm"]:
        raise NotImplementedError("norm = True: the denoiser input is not normalised (DDRM.yaml)")
    dims = c["dims"] if isinstance(c["dims"], (list, tuple)) else [c["dims"]]
    if len(dims) != 1:
        raise NotImplementedError(f"dims = {list(dims)}: one hidden layer")
    H = int(dims[0])
    if H % 4 or not 4 <= H <= 1024:
        raise NotImplementedError(f"dims = [{H}]: a multiple of 4 in 4..1024")
    if not c["noise_scale"]:
        raise NotImplementedError("noise_scale = 0: no diffusion schedule")
    L = int(c["lightGCN_n_layers"])
    if L < 0 or L + 1 > MAX_TABLES:
        raise NotImplementedError(f"lightGCN_n_layers = {L}: 0..{MAX_TABLES - 1}")
    T = int(c["steps"])
    if not 2 <= T <= 4096:
        raise NotImplementedError(f"steps = {T}: 2..4096")
    S = int(c["sampling_steps"] or 0)
    if not 0 <= S <= T:
        raise NotImplementedError(f"sampling_steps = {S}: 0..steps")
    if dist.world() > 1:
        raise NotImplementedError("world size > 1: the loss multiplies two batch sums (mean(w) and reg), which the "
                                  "norm_rows / reg_share split does not cover")
    return H, L, T


def ddrm_schedule(T, noise_scale, noise_min, noise_max, noise_schedule="linear-var"):
    """The fp64 tables of the reference's GaussianDiffusion (numpy), beta_0 pinned to 1e-5."""
    v = np.linspace(noise_scale * noise_min, noise_scale * noise_max, T, dtype=np.float64)
    if noise_schedule == "linear-var":
        ab = 1 - v
        betas = np.array([1 - ab[0]] + [min(1 - ab[i] / ab[i - 1], 0.999) for i in range(1, T)])
    else:
        betas = v.copy()
    betas[0] = 0.00001
    alphas = 1.0 - betas
    ac = np.cumprod(alphas)
    prev = np.concatenate([[1.0], ac[:-1]])
    pv = betas * (1.0 - prev) / (1.0 - ac)
    return {"betas": betas, "alphas_cumprod": ac, "sqrt_alphas_cumprod": np.sqrt(ac),
            "sqrt_one_minus_alphas_cumprod": np.sqrt(1.0 - ac), "posterior_variance": pv,
            "posterior_log_variance_clipped": np.log(np.concatenate([pv[1:2], pv[1:]])),
            "posterior_mean_coef1": betas * np.sqrt(prev) / (1.0 - ac),
            "posterior_mean_coef2": (1.0 - prev) * np.sqrt(alphas) / (1.0 - ac)}


def time_embedding(timesteps, dim=D, max_period=10000):
    """[cos(t f) | sin(t f)], f_k = exp(-k ln(max_period) / half), in fp32 as the reference takes it."""
    half = dim // 2
    f = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    a = timesteps[:, None].float() * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=-1)


@torch.no_grad()
def init_parameters(n_users, n_items, H):
    """The fourteen parameter tensors in named_parameters() order, drawn on the host generator as the reference's
    constructor draws them (ddrm.py:27-31, :88-126): both nn.Embedding and every nn.Linear consume their own init
    first, each denoiser re-draws in_layers, out_layers, emb_layer in that order."""
    eu, ei = nn.Embedding(n_users, D), nn.Embedding(n_items, D)
    nn.init.normal_(eu.weight, std=0.1)
    nn.init.normal_(ei.weight, std=0.1)
    out = [eu.weight.detach(), ei.weight.detach()]
    for _ in range(2):
        emb, inl, outl = nn.Linear(D, D), nn.Linear(3 * D, H), nn.Linear(H, D)
        for layer in (inl, outl, emb):
            fan_out, fan_in = layer.weight.size()
            layer.weight.data.normal_(0.0, np.sqrt(2.0 / (fan_in + fan_out)))
            layer.bias.data.normal_(0.0, 0.001)
        for layer in (emb, inl, outl):
            out += [layer.weight.detach(), layer.bias.detach()]
    return out


class _Encoder(nn.Module):
    def __init__(self, eu, ei):
        super().__init__()
        self.embedding_user = _Table(eu)
        self.embedding_item = _Table(ei)


class _DNN(nn.Module):
    def __init__(self, emb, inl, outl):
        super().__init__()
        self.emb_layer = emb
        self.in_layers = nn.ModuleList([inl])
        self.out_layers = nn.ModuleList([outl])


class DDRM(EmbeddingRecommender):
    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        c = config
        self.config = config
        H, L, T = check_config(c)
        self.H, self.n_layers, self.steps = H, L, T
        self.reg_weight, self.alpha, self.beta = float(c["reg_weight"]), float(c["alpha"]), float(c["beta"])
        self.sampling_steps = int(c["sampling_steps"] or 0)
        self.sampling_noise = bool(c["sampling_noise"])
        self.seed = config_seed(c)
        U, I, dev = self.n_users, self.n_items, self.device
        N = self.N = U + I

        # ---- parameters (one slab), the generator consumed as the reference's constructor consumes it
        specs = [("E", (N, D), None)]
        for m in ("u", "i"):
            specs += [(m + "We", (D, D), None), (m + "be", (D,), None), (m + "W1", (H, 3 * D), None),
                      (m + "b1", (H,), None), (m + "W2", (D, H), None), (m + "b2", (D,), None)]
        s = self.slab = Slab(specs, dev)
        self._init_like_reference()
        e, ge = s.view("E"), s.gview("E")
        eu, ei = nn.Parameter(e[:U]), nn.Parameter(e[U:])
        eu.grad, ei.grad = ge[:U], ge[U:]
        self.rec_model = _Encoder(eu, ei)

        def dnn(m):
            return _DNN(_Linear(s.parameter(m + "We"), s.parameter(m + "be")),
                        _Linear(s.parameter(m + "W1"), s.parameter(m + "b1")),
                        _Linear(s.parameter(m + "W2"), s.parameter(m + "b2")))

        self.user_reverse_model = dnn("u")
        self.item_reverse_model = dnn("i")

        # ---- graphs
        tl = dataloader
        self.user_ptr = torch.as_tensor(tl.uptr_np).to(dev)
        self.user_items = torch.as_tensor(tl.uitems_np).to(dev)
        self.norm_adj = K.bipartite_symnorm(U, I, self.user_ptr, self.user_items, self_loops=False, deg_eps=0.0)
        deg = (self.user_ptr[1:] - self.user_ptr[:-1]).long()
        hv = (1.0 / deg.clamp(min=1).float()).repeat_interleave(deg).contiguous()
        self.hist = K.CSR(self.user_ptr, self.user_items, hv, n_cols=I, symmetric=False)

        # ---- schedule (fp64 on the host, fp32 where the kernels read it)
        self.schedule = ddrm_schedule(T, float(c["noise_scale"]), float(c["noise_min"]), float(c["noise_max"]),
                                      c["noise_schedule"] or "linear-var")
        f32 = lambda k: torch.from_numpy(self.schedule[k]).float().to(dev)  # noqa: E731
        self._sqrt_ac, self._sqrt_1mac = f32("sqrt_alphas_cumprod"), f32("sqrt_one_minus_alphas_cumprod")
        self._c1, self._c2 = f32("posterior_mean_coef1"), f32("posterior_mean_coef2")
        self._sigma = torch.exp(0.5 * torch.from_numpy(self.schedule["posterior_log_variance_clipped"]).float()).to(dev)
        self._qa = float(self._sqrt_ac[T - 1].item())
        self._qb = float(self._sqrt_1mac[T - 1].item())
        self._temb = time_embedding(torch.arange(T)).to(dev).contiguous()

        # ---- work buffers
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self.tab, self.gtab, self._greg, self._eval = f(N, D), f(N, D), f(N, D), f(N, D)
        self._layers = [f(N, D) for _ in range(L)]
        self._t = [f(N, D) for _ in range(2)]
        self._tE = {m: f(T, D) for m in "ui"}
        self._tB = {m: f(T, H) for m in "ui"}
        self._dTB, self._dE = f(T, H), f(T, D)
        self._xs, self._gen, self._n0 = f(U, D), f(U, D), f(U, D)
        self._sqws = torch.zeros(1024, dtype=torch.float64, device=dev)
        self._loss = f(4)
        self._reg = f(1)
        self._w = None
        self._step = 0
        self._eval_pass = 0

    # ------------------------------------------------------------------ construction
    @torch.no_grad()
    def _init_like_reference(self):
        U, s = self.n_users, self.slab
        p = init_parameters(U, self.n_items, self.H)
        s.view("E")[:U].copy_(p[0])
        s.view("E")[U:].copy_(p[1])
        names = [m + n for m in ("u", "i") for n in ("We", "be", "W1", "b1", "W2", "b2")]
        for n, v in zip(names, p[2:]):
            s.load(n, v)

    # ------------------------------------------------------------------ parameters
    def optim_slabs(self):
        return [self.slab]

    def grad_views(self):
        """Gradient views in the reference's named_parameters() order."""
        s, U = self.slab, self.n_users
        out = [s.gview("E")[:U], s.gview("E")[U:]]
        for m in ("u", "i"):
            out += [s.gview(m + n) for n in ("We", "be", "W1", "b1", "W2", "b2")]
        return out

    def extra_state(self):
        """The Philox counters: a resumed run draws (and scores with) what the uninterrupted one would."""
        return {"counters": {"step": int(self._step), "eval_pass": int(self._eval_pass)}}

    def load_extra_state(self, st):
        self._step = int(st["counters"]["step"])
        self._eval_pass = int(st["counters"]["eval_pass"])

    # ------------------------------------------------------------------ encoder
    def _forward(self, out):
        """[ua; ia] = mean(E_0 .. E_n) into out (N x 64)."""
        tabs = [self.slab.view("E")]
        for i in range(self.n_layers):
            self.norm_adj.spmm(self._layers[i], [(tabs[-1],)])
            tabs.append(self._layers[i])
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", self.N, self.n_users, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(out), out.stride(0), stream())

    def _time_table(self, m):
        """E = emb_layer(temb(0..T-1)) (T x 64) and TB = E W1[:, 64:128]^T + b1 (T x H) of denoiser m."""
        s = self.slab
        K.gemm(self._temb, s.view(m + "We"), self._tE[m], trans_b=True, epi=K.EPI_BIAS, bias=s.view(m + "be"))
        K.gemm(self._tE[m], s.view(m + "W1")[:, D:2 * D], self._tB[m], trans_b=True, epi=K.EPI_BIAS,
               bias=s.view(m + "b1"))
        return self._tB[m]

    def _work(self, B):
        if self._w is None or self._w["B"] < B:
            dev, H = self.device, self.H
            f = lambda *sh, dt=torch.float32: torch.empty(sh, dtype=dt, device=dev)  # noqa: E731
            w = {"B": B, "t": f(B, dt=torch.int32), "terms": f(4, B), "contrib": f(3 * B, D), "e0": f(3 * B, D),
                 "da": f(B, H), "cu": f(B, D), "ci": f(B, D)}
            for m in "ui":
                w.update({m + "out": f(B, D), m + "xd": f(B, D), m + "h": f(B, H), m + "mse": f(B),
                          m + "keep": f(B, D, dt=torch.uint8), m + "dout": f(B, D), m + "dxd": f(B, D),
                          m + "dcond": f(B, D)})
            self._w = w
        return self._w

    def _plan(self, users, pos, neg):
        return sort_plan((users, pos, neg), (0, self.n_users, self.n_users))

    # ------------------------------------------------------------------ training
    def denoise_fwd(self, m, X, idx_x, C, idx_c, t, TB, out, noise=None, keep=None, drop=None, xd=None, keep_out=None,
                    h=None, rowmse=None, row_off=0, site=0):
        """gmr_ddrm_denoise_fwd of denoiser m ('u' / 'i') over idx_x.numel() rows.  drop: None = no dropout,
        "given" = the keep bytes, "draw" = Philox."""
        s = self.slab
        n = t.numel()
        mode = {None: 0, "given": 1, "draw": 2}[drop]
        _lib.call("gmr_ddrm_denoise_fwd", n, self.H, self.steps, row_off, ptr(X), X.stride(0), ptr(idx_x), ptr(C),
                  C.stride(0), ptr(idx_c), ptr(t), ptr(self._sqrt_ac), ptr(self._sqrt_1mac), ptr(noise),
                  noise.stride(0) if noise is not None else 0, mode, ptr(keep), keep.stride(0) if keep is not None else 0,
                  self.seed, self._step, site, ptr(s.view(m + "W1")), ptr(TB), ptr(s.view(m + "W2")),
                  ptr(s.view(m + "b2")), ptr(out), out.stride(0), ptr(xd), xd.stride(0) if xd is not None else 0,
                  ptr(keep_out), keep_out.stride(0) if keep_out is not None else 0, ptr(h),
                  h.stride(0) if h is not None else 0, ptr(rowmse), stream())

    def _denoise_bwd(self, m, w, B, tt, cond):
        """All gradients of denoiser m from w[m + 'dout']; leaves dxd and dcond in the work buffers."""
        s, T = self.slab, self.steps
        dout, h, xd, da = w[m + "dout"][:B], w[m + "h"][:B], w[m + "xd"][:B], w["da"][:B]
        W1, gW1 = s.view(m + "W1"), s.gview(m + "W1")
        K.gemm(dout, h, s.gview(m + "W2"), trans_a=True)
        K.colsum(dout, s.gview(m + "b2"))
        K.gemm(dout, s.view(m + "W2"), da, epi=K.EPI_DTANH, aux=h)
        K.gemm(da, xd, gW1[:, :D], trans_a=True)
        K.gemm(da, cond, gW1[:, 2 * D:], trans_a=True)
        K.colsum(da, self._dTB, group=tt, n_groups=T)
        K.colsum(self._dTB, s.gview(m + "b1"))
        K.gemm(self._dTB, self._tE[m], gW1[:, D:2 * D], trans_a=True)
        K.gemm(self._dTB, W1[:, D:2 * D], self._dE)
        K.gemm(self._dE, self._temb, s.gview(m + "We"), trans_a=True)
        K.colsum(self._dE, s.gview(m + "be"))
        K.gemm(da, W1[:, :D], w[m + "dxd"][:B])
        K.gemm(da, W1[:, 2 * D:], w[m + "dcond"][:B])

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, t=None,
                 noise_u=None, noise_i=None, keep_u=None, keep_i=None):
        """calculate_loss (ddrm.py:384-433) and all parameter gradients (into the slab's twin).  Returns the loss as a
        device scalar.  t (int B), the noises (B x 64) and the keep bytes (B x 64 uint8) may be injected; otherwise
        they come from Philox (seed, step counter).  loss_terms() reads [w | softplus | recon | loss_b] (4 x B)."""
        if dist.is_dist():
            raise NotImplementedError("world size > 1: DDRM runs on one device")
        s, U, T, N = self.slab, self.n_users, self.steps, self.N
        B = users.numel()
        if plan_bpr is None:
            plan_bpr = self._plan(users, pos, neg)
        w = self._work(B)
        tt = w["t"][:B]
        tab = self.tab
        ua, ia = tab[:U], tab[U:]
        s.zero_grad()
        self._forward(tab)
        if t is None:
            _lib.call("gmr_diff_sample_t", B, T, self.seed ^ SITE_T, self._step, 0, ptr(tt), stream())
        else:
            tt.copy_(t)
        drop = None if not self.training else "draw"
        keeps = {}
        for m, X, ix, C, ic, nz, kp, site in (("u", ua, users, ia, pos, noise_u, keep_u, SITE_U),
                                              ("i", ia, pos, ua, users, noise_i, keep_i, SITE_I)):
            dm = drop
            if kp is not None:
                w[m + "keep"][:B].copy_(kp)
                dm = "given"
            keeps[m] = w[m + "keep"][:B] if dm else None
            self.denoise_fwd(m, X, ix, C, ic, tt, self._time_table(m), w[m + "out"][:B], noise=nz,
                             keep=keeps[m] if dm == "given" else None, drop=dm, xd=w[m + "xd"][:B],
                             keep_out=keeps[m] if dm == "draw" else None, h=w[m + "h"][:B], rowmse=w[m + "mse"][:B],
                             site=site)
        # reg over the gathered raw rows (duplicates count), a device scalar
        E, e0 = s.view("E"), w["e0"]
        K.gather_rows(E, users, e0[:B])
        K.gather_rows(E, pos, e0[B:2 * B], off=U)
        K.gather_rows(E, neg, e0[2 * B:3 * B], off=U)
        _lib.call("gmr_sqnorm_f32", 3 * B * D, ptr(e0), 0.5 / B, ptr(self._reg), 0, ptr(self._sqws), stream())
        contrib = w["contrib"][:3 * B]
        _lib.call("gmr_ddrm_loss_fwd_bwd", B, U, ptr(tab), tab.stride(0), ptr(users), ptr(pos), ptr(neg),
                  ptr(w["uout"]), D, ptr(w["iout"]), D, ptr(w["umse"]), ptr(w["imse"]), ptr(self._reg), self.alpha,
                  self.beta, self.reg_weight, 1.0 / B, ptr(w["terms"]), ptr(self._loss), ptr(contrib), D,
                  ptr(w["udout"]), ptr(w["idout"]), stream())
        self._terms = w["terms"].view(-1)[:4 * B].view(4, B)
        # ---- backward: the denoisers, then the rows, then the encoder
        cu, ci = w["cu"][:B], w["ci"][:B]
        K.gather_rows(tab, pos, cu, off=U)
        K.gather_rows(tab, users, ci)
        self._denoise_bwd("u", w, B, tt, cu)
        self._denoise_bwd("i", w, B, tt, ci)
        # users rows: own q_sample input (user model) + cond of the item model; pos rows the other way round
        for dst, own, other in ((contrib[:B], "u", "i"), (contrib[B:2 * B], "i", "u")):
            kp = keeps[own]
            _lib.call("gmr_ddrm_input_bwd", B, ptr(w[own + "dxd"]), ptr(kp), kp.stride(0) if kp is not None else 0,
                      ptr(tt), ptr(self._sqrt_ac), ptr(w[other + "dcond"]), ptr(dst), dst.stride(0), stream())
        gtab, greg, gE, adj, L = self.gtab, self._greg, s.gview("E"), self.norm_adj, self.n_layers
        K.zero_(gtab)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), D, ptr(plan_bpr), ptr(contrib), D, ptr(gtab), D, stream())
        # dE = (1 / (L + 1)) sum_k adj^k g as a Horner chain (adj is symmetric)
        copy64(gtab, gE)
        src = gtab
        for i in range(L):
            last = i == L - 1
            dst = gE if last else self._t[i % 2]
            if not last:
                copy64(gtab, dst)
            sc = 1.0 / (L + 1) if last else 1.0
            adj.spmm(dst, [(src,)], alpha=sc, beta=sc)
            src = dst
        # reg: d/dE0[r] = coef count(r) E0[r] / B, coef = loss[1] on the device (loss[2] = coef / B)
        K.zero_(greg)
        _lib.call("gmr_scatter_sorted_f32", plan_bpr.numel(), D, ptr(plan_bpr), ptr(e0), D, ptr(greg), D, stream())
        _lib.call("gmr_axpy_dev_f32", N * D, ptr(self._loss[2:3]), ptr(greg), ptr(gE), stream())
        self._step += 1
        return self._loss[0]

    def loss_terms(self):
        """[w | softplus | recon | loss_b] (4 x B) of the last rec_step (device tensor)."""
        return self._terms

    # ------------------------------------------------------------------ prediction
    @torch.no_grad()
    def forward_embeddings(self, noise=None, step_noise=None):
        """(generated U x 64, ia): the tables whose product is full_sort_predict's score matrix.  noise (U x 64):
        the q_sample draw; step_noise (sampling_steps x U x 64, indexed by timestep): the chain's draws with
        sampling_noise.  Not injected, they come from Philox (seed, eval-pass counter, user id)."""
        U, T, S, dev = self.n_users, self.steps, self.sampling_steps, self.device
        self._forward(self._eval)
        ua, ia = self._eval[:U], self._eval[U:]
        self.hist.spmm(self._xs, [(ia,)])
        if noise is None:
            _lib.call("gmr_rf_randn", U * D, self.seed, self._eval_pass, SITE_EVAL, ptr(self._n0), stream())
            n0 = self._n0
        else:
            n0 = torch.as_tensor(noise, dtype=torch.float32).to(dev).contiguous()
        sn = None
        if step_noise is not None:
            sn = torch.as_tensor(step_noise, dtype=torch.float32).to(dev).contiguous()
            if tuple(sn.shape) != (S, U, D):
                raise ValueError(f"step_noise must be {S} x {U} x {D}")
        s = self.slab
        TB = self._time_table("i") if S > 0 else None
        _lib.call("gmr_ddrm_chain", U, self.H, T, S, 0, ptr(self._xs), D, ptr(n0), n0.stride(0), self._qa, self._qb,
                  ptr(ua), ua.stride(0), None, ptr(s.view("iW1")), ptr(TB), ptr(s.view("iW2")), ptr(s.view("ib2")),
                  ptr(self._c1), ptr(self._c2), ptr(self._sigma) if self.sampling_noise else None, ptr(sn), self.seed,
                  self._eval_pass, SITE_CHAIN, ptr(self._gen), D, stream())
        if noise is None or (self.sampling_noise and sn is None):
            self._eval_pass += 1
        return self._gen, ia
