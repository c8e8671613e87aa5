"""Rectified-flow embedding generator on MI355X — models/rf_modules.py of the reference (RFEmbeddingGenerator with
SimpleVelocityNet), backbone-agnostic: a backbone hands it the detached target table X1 ((U + I) x D) and the
condition table ((U + I) x C) and mixes generate()'s output into its evaluation embeddings.

Supported: rf_hidden_dim 128, rf_n_layers 1..4, 1-RF (use_2rf False), and (embedding_dim D, condition_dim C) = (64,
64 | 128 | 192), or D = C = 128 or 192 for the concat-fusion backbones, whose generated rows are as wide as their
conditions.  At D != 64 the same steps run on the width-taking entry points (gmr_rf_*_w); "64" below reads D there.

  train_step   X0 ~ N(0, 1), t ~ U[0, 1), X_t; the velocity net forward with saved pre-activations (the Linear
               layers on the GEMM with the BIAS epilogue, gmr_rf_act_fwd rows between them); the guidance / MSE head
               (gmr_rf_head_fwd, or gmr_rf_head_prior_fwd when the backbone passes a user_prior table);
               the two sampled InfoNCE terms on the predicted end points; the backward through the same layers (dW =
               dY^T X, db = colsum(dY), dX = dY W; gmr_rf_act_bwd); one AdamW step on the velocity slab
  generate     the Euler integration in one launch (gmr_rf_sample), or composed per layer from the same kernels
               (fused=False: the comparison path of scripts/rffreedom_step.py); with base=, the evaluation's mix
               base + ratio * rows as that launch's epilogue (gmr_rf_sample_mix)

Random draws come from Philox streams keyed on (seed, step counter, site); each has an injected alternative.

RFBackbone is the mixin of the RF-on-X models (class RFX(RFBackbone, X)): the generator built from the rf_* config
keys, the warm-up / resume protocol and the "backbone step, then RF step" of rec_step.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from .abstract_recommender import config_seed, copy64, sort_plan
from .kernels import ptr, stream
from .slab import Slab

H, D = 128, 64
SITE_X0, SITE_T, SITE_NEG_ITEMS, SITE_NEG_USERS, SITE_Z0, SITE_DROP = 0, 1, 2, 3, 4, 16
GUIDANCE_SCALE = 0.1  # cosine_guidance_scale; cosine_decay_power 2 is in the kernel
PRIOR_SCALE = 0.2  # user_guidance_scale (guidance_decay_power 2 likewise): the constructor defaults, no backbone sets them


def param_specs(C, n_layers, D=D):
    """(name, shape) of velocity_net.named_parameters() in the reference's order; D: embedding_dim."""
    out = [("time_embed.1.weight", (H, 64)), ("time_embed.1.bias", (H,))]
    for m, k in (("condition_encoder", C), ("input_proj", D)):
        out += [(f"{m}.0.weight", (H, k)), (f"{m}.0.bias", (H,)), (f"{m}.1.weight", (H,)), (f"{m}.1.bias", (H,))]
    for l in range(n_layers):
        b = f"res_blocks.{l}.net."
        out += [(b + "0.weight", (H, H)), (b + "0.bias", (H,)), (b + "1.weight", (H,)), (b + "1.bias", (H,)),
                (b + "4.weight", (H, H)), (b + "4.bias", (H,)), (b + "5.weight", (H,)), (b + "5.bias", (H,))]
    out += [("output_proj.0.weight", (H, H)), ("output_proj.0.bias", (H,)), ("output_proj.1.weight", (H,)),
            ("output_proj.1.bias", (H,)), ("output_proj.4.weight", (D, H)), ("output_proj.4.bias", (D,))]
    return out


# RFGenerator keyword: (config key, default), the constructor defaults of the reference's RF models
RF_CONFIG = {"n_layers": ("rf_n_layers", 2), "dropout": ("rf_dropout", 0.1), "learning_rate": ("rf_learning_rate", 1e-4),
             "sampling_steps": ("rf_sampling_steps", 10), "warmup_epochs": ("rf_warmup_epochs", 5),
             "inference_mix_ratio": ("rf_inference_mix_ratio", 0.2), "contrast_temp": ("rf_contrast_temp", 0.2),
             "contrast_weight": ("rf_loss_weight", 1.0), "n_negatives": ("rf_infonce_negatives", 1024)}


def _get(config, key, default):
    return config[key] if key in config and config[key] is not None else default


def check_config(config):
    """The RF settings this package runs; anything else raises with the key's name."""
    if bool(_get(config, "use_denoise", False)):
        raise NotImplementedError("use_denoise: True needs interaction ratings, which the loaders do not carry")
    if bool(_get(config, "use_2rf", True)):
        raise NotImplementedError("use_2rf: True (reflow) is not built; set use_2rf: False")
    if int(_get(config, "rf_hidden_dim", 128)) != H:
        raise NotImplementedError("rf_hidden_dim must be 128 (the kernels' hidden width)")
    if not 1 <= int(_get(config, "rf_n_layers", 2)) <= 4:
        raise NotImplementedError("rf_n_layers must be in 1..4")


class RFGenerator(nn.Module):
    def __init__(self, n_users, n_items, condition_dim, device, n_layers=2, dropout=0.1, learning_rate=1e-4,
                 sampling_steps=10, warmup_epochs=5, inference_mix_ratio=0.2, contrast_temp=0.2, contrast_weight=1.0,
                 n_negatives=1024, weight_decay=0.01, seed=0, fused=True, embedding_dim=D):
        super().__init__()
        C, L, Dw = int(condition_dim), int(n_layers), int(embedding_dim)
        if int(_lib.load().gmr_rf_param_floats_w(Dw, C, L)) < 0:
            raise NotImplementedError(f"embedding_dim {Dw} / condition_dim {C} / rf_n_layers {L}: the kernels take "
                                      f"condition_dim 64, 128 or 192 at embedding_dim 64, or both 128 or both 192, "
                                      f"and 1..4 layers")
        self.U, self.I, self.N, self.C, self.L, self.D = int(n_users), int(n_items), int(n_users + n_items), C, L, Dw
        self.dev = device
        self.dropout, self.lr, self.wd = float(dropout), float(learning_rate), float(weight_decay)
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.sampling_steps, self.warmup_epochs = int(sampling_steps), int(warmup_epochs)
        self.inference_mix_ratio = float(inference_mix_ratio)
        self.temp, self.weight, self.n_neg = float(contrast_temp), float(contrast_weight), int(n_negatives)
        self.seed, self.fused = int(seed), bool(fused)
        self.step_ctr, self.epoch = 0, 0
        self.specs = param_specs(C, L, Dw)
        self.slab = Slab([(n, sh, None) for n, sh in self.specs], device)
        assert self.slab.numel == int(_lib.load().gmr_rf_param_floats_w(Dw, C, L)), "the slab is the kernel's packed layout"
        # nn.Linear / nn.LayerNorm default initialisation
        with torch.no_grad():
            for name, sh in self.specs:
                if name.endswith(".weight") and len(sh) == 2:
                    lin = nn.Linear(sh[1], sh[0])
                    self.slab.load(name, lin.weight)
                    self.slab.load(name[:-6] + "bias", lin.bias)
                elif name.endswith(".weight"):
                    self.slab.view(name).fill_(1.0)
        # state_dict carries the parameters and the AdamW moments
        self.register_buffer("velocity_params", self.slab.data)
        self.register_buffer("exp_avg", torch.zeros_like(self.slab.data))
        self.register_buffer("exp_avg_sq", torch.zeros_like(self.slab.data))
        self._w = None
        self._ratio = torch.tensor([self.inference_mix_ratio], dtype=torch.float32, device=device)

    # ------------------------------------------------------------------ state
    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def warmed_up(self):
        return self.epoch >= self.warmup_epochs

    def load_reference_state(self, sd):
        """Parameters from the reference's names (velocity_net.<name>, with or without the prefix)."""
        with torch.no_grad():
            for name, _ in self.specs:
                v = sd["velocity_net." + name] if "velocity_net." + name in sd else sd[name]
                self.slab.load(name, torch.as_tensor(v).to(self.dev))

    def grad_views(self):
        return [self.slab.gview(n) for n, _ in self.specs]

    def param_views(self):
        return [self.slab.view(n) for n, _ in self.specs]

    def _rf(self, name, *args, at=1):
        """An RF entry point at this generator's width: `name` itself at 64, else `name`_w with the width as the
        argument at position `at`."""
        if self.D == D:
            return _lib.call(name, *args)
        return _lib.call(name + "_w", *args[:at], self.D, *args[at:])

    # ------------------------------------------------------------------ buffers
    def _work(self, B):
        w = self._w
        if w is None or w["B"] < B:
            N, dev, D = self.N, self.dev, self.D
            f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
            w = {"B": B, "X0": f(N, D), "t": f(N), "Xt": f(N, D), "S": f(N, 64), "V": f(N, D), "pred": f(N, D),
                 "dpred": f(N, D), "dV": f(N, D), "G1": f(N, H), "G2": f(N, H), "GH": f(N, H), "GR": f(N, H),
                 "rowparts": torch.zeros(N, dtype=torch.float64, device=dev),
                 "clparts": torch.zeros(2 * B, dtype=torch.float64, device=dev), "contrib": f(2 * B, D),
                 "loss": f(3), "parts": f(int(_lib.load().gmr_rf_act_parts_floats(N))),
                 "ka": torch.tensor([0, self.U], dtype=torch.int32, device=dev), "Y": {}, "A": {}, "M": {}}
            for site in self._sites():
                w["Y"][site], w["A"][site] = f(N, H), f(N, H)
            self._w = w
        return w

    def _sites(self):
        return ["time", "cond", "input"] + [f"block{l}{h}" for l in range(self.L) for h in "ab"] + ["out"]

    def _mask(self, w, site, masks, idx):
        """Keep bytes of one dropout site: injected, drawn by Philox, or None at dropout 0."""
        if masks is not None:
            m = masks.get(site)
            return None if m is None else m.to(self.dev).to(torch.uint8).contiguous()
        if self.dropout <= 0.0:
            return None
        m = w["M"].get(site)
        if m is None:
            m = w["M"][site] = torch.empty((self.N, H), dtype=torch.uint8, device=self.dev)
        _lib.call("gmr_keep_mask_u8", self.N * H, 1.0 - self.dropout, self.seed, self.step_ctr,
                  (SITE_DROP + idx) << 40, ptr(m), stream())
        return m

    # ------------------------------------------------------------------ layers
    def _lin(self, x, name, out):
        s = self.slab
        K.gemm(x, s.view(name + ".weight"), out, trans_b=True, epi=K.EPI_BIAS, bias=s.view(name + ".bias"))

    def _lin_bwd(self, dy, x, name, dx=None, beta=0.0):
        s = self.slab
        K.gemm(dy, x, s.gview(name + ".weight"), trans_a=True)
        K.colsum(dy, s.gview(name + ".bias"))
        if dx is not None:
            K.gemm(dy, s.view(name + ".weight"), dx, beta=beta)

    def _act(self, y, ln, out, res=None, mask=None, add1=None, add2=None):
        s = self.slab
        _lib.call("gmr_rf_act_fwd", y.shape[0], ptr(y), ptr(s.view(ln + ".weight")) if ln else None,
                  ptr(s.view(ln + ".bias")) if ln else None, ptr(res), ptr(mask), self._scale(), ptr(add1), ptr(add2),
                  ptr(out), stream())

    def _act_bwd(self, w, y, ln, dout, dy, res=None, mask=None, dres=None):
        s = self.slab
        _lib.call("gmr_rf_act_bwd", y.shape[0], ptr(y), ptr(s.view(ln + ".weight")) if ln else None,
                  ptr(s.view(ln + ".bias")) if ln else None, ptr(res), ptr(mask), self._scale(), ptr(dout), ptr(dy),
                  ptr(dres), ptr(w["parts"]), ptr(s.gview(ln + ".weight")) if ln else None,
                  ptr(s.gview(ln + ".bias")) if ln else None, stream())

    def _scale(self):
        return 1.0 / (1.0 - self.dropout) if self.dropout > 0.0 else 1.0

    def _net_fwd(self, w, x, S, cond, masks):
        """The velocity net on x (N x D) with the time features S (N x 64); pre-activations in w["Y"], layer
        outputs in w["A"] (the block outputs h_l are A["input"], A["block{l}b"]); returns V (N x D)."""
        Y, A = w["Y"], w["A"]
        mk = {site: self._mask(w, site, masks, i) for i, site in enumerate(self._sites()) if not site.endswith("b")}
        w["mk"] = mk
        self._lin(S, "time_embed.1", Y["time"])
        self._act(Y["time"], None, A["time"], mask=mk["time"])
        self._lin(cond, "condition_encoder.0", Y["cond"])
        self._act(Y["cond"], "condition_encoder.1", A["cond"], mask=mk["cond"])
        self._lin(x, "input_proj.0", Y["input"])
        self._act(Y["input"], "input_proj.1", A["input"], mask=mk["input"], add1=A["time"], add2=A["cond"])
        h = A["input"]
        for l in range(self.L):
            b, a_, b_ = f"res_blocks.{l}.net.", f"block{l}a", f"block{l}b"
            self._lin(h, b + "0", Y[a_])
            self._act(Y[a_], b + "1", A[a_], mask=mk[a_])
            self._lin(A[a_], b + "4", Y[b_])
            self._act(Y[b_], b + "5", A[b_], res=h)
            h = A[b_]
        self._lin(h, "output_proj.0", Y["out"])
        self._act(Y["out"], "output_proj.1", A["out"], mask=mk["out"])
        self._lin(A["out"], "output_proj.4", w["V"])
        return w["V"]

    def _net_bwd(self, w, x, S, cond):
        Y, A, mk = w["Y"], w["A"], w["mk"]
        G1, G2, GH, GR = w["G1"], w["G2"], w["GH"], w["GR"]
        hs = [A["input"]] + [A[f"block{l}b"] for l in range(self.L)]
        self._lin_bwd(w["dV"], A["out"], "output_proj.4", dx=G1)
        self._act_bwd(w, Y["out"], "output_proj.1", G1, G2, mask=mk["out"])
        self._lin_bwd(G2, hs[-1], "output_proj.0", dx=GH)
        for l in reversed(range(self.L)):
            b, a_, b_ = f"res_blocks.{l}.net.", f"block{l}a", f"block{l}b"
            self._act_bwd(w, Y[b_], b + "5", GH, G2, res=hs[l], dres=GR)
            self._lin_bwd(G2, A[a_], b + "4", dx=G1)
            self._act_bwd(w, Y[a_], b + "1", G1, G2, mask=mk[a_])
            self._lin_bwd(G2, hs[l], b + "0", dx=GR, beta=1.0)  # dh_l = dY1 W1 + the residual's share
            GH, GR = GR, GH
        self._act_bwd(w, Y["input"], "input_proj.1", GH, G2, mask=mk["input"])
        self._lin_bwd(G2, x, "input_proj.0")
        self._act_bwd(w, Y["cond"], "condition_encoder.1", GH, G2, mask=mk["cond"])
        self._lin_bwd(G2, cond, "condition_encoder.0")
        self._act_bwd(w, Y["time"], None, GH, G2, mask=mk["time"])
        self._lin_bwd(G2, S, "time_embed.1")

    # ------------------------------------------------------------------ training
    def infonce(self, pred, target, row_off, n, idx, parts, contrib, neg=None, site=0, coef=1.0):
        """Sampled InfoNCE of B anchors of one side (gmr_rf_infonce_sampled_fwd_bwd)."""
        self._rf("gmr_rf_infonce_sampled_fwd_bwd", idx.numel(), n, ptr(pred), pred.stride(0), ptr(target),
                 target.stride(0), row_off, ptr(idx), neg.shape[1] if neg is not None else self.n_neg, ptr(neg),
                 self.seed, self.step_ctr, site, 1.0 / self.temp, float(coef), ptr(parts), ptr(contrib),
                 contrib.stride(0), stream(), at=2)

    def train_step(self, X1, cond, users, pos, X0=None, t=None, neg_items=None, neg_users=None, masks=None,
                   apply=True, prior=None):
        """compute_loss_and_step (rf_modules.py:779-894).  X1: N x 64 (any row stride), cond: N x C, users / pos:
        int32 batch indices.  Returns the device tensor [rf_loss, cl_loss, total]; the velocity gradients stay in
        the slab gradient.  X0 / t / neg_* / masks: injected draws; apply=False skips the AdamW step.  prior: the
        backbone's user_prior, N x 64 fp32 of any row stride >= 64 (a constant of the step: v += (1 - t)^2 0.2 prior
        before the cosine term, rf_modules.py:460-465); None: no such term."""
        N, U, B, D = self.N, self.U, users.numel(), self.D
        w = self._work(B)
        i32 = lambda a: None if a is None else a.to(self.dev).to(torch.int32).contiguous()  # noqa: E731
        neg_items, neg_users = i32(neg_items), i32(neg_users)
        if X0 is None:
            _lib.call("gmr_rf_randn", N * D, self.seed, self.step_ctr, SITE_X0, ptr(w["X0"]), stream())
        else:
            w["X0"].copy_(X0.reshape(N, D))
        if t is None:
            _lib.call("gmr_rf_rand", N, self.seed, self.step_ctr, SITE_T, ptr(w["t"]), stream())
        else:
            w["t"].copy_(t.reshape(N))
        self._rf("gmr_rf_interp", N, ptr(X1), X1.stride(0), ptr(w["X0"]), ptr(w["t"]), ptr(w["Xt"]), stream())
        _lib.call("gmr_rf_time_embed", N, ptr(w["t"]), ptr(w["S"]), stream())
        V = self._net_fwd(w, w["Xt"], w["S"], cond, masks)
        if prior is None:
            self._rf("gmr_rf_head_fwd", N, ptr(V), ptr(w["Xt"]), ptr(X1), X1.stride(0), ptr(w["X0"]), ptr(w["t"]),
                     GUIDANCE_SCALE, ptr(w["pred"]), ptr(w["rowparts"]), stream())
        else:
            if prior.dtype != torch.float32 or tuple(prior.shape) != (N, D) or prior.stride(1) != 1:
                raise ValueError(f"prior must be a {N} x {D} fp32 table with unit column stride")
            self._rf("gmr_rf_head_prior_fwd", N, ptr(V), ptr(w["Xt"]), ptr(X1), X1.stride(0), ptr(w["X0"]),
                     ptr(w["t"]), ptr(prior), prior.stride(0), PRIOR_SCALE, GUIDANCE_SCALE, ptr(w["pred"]),
                     ptr(w["rowparts"]), stream())
        # contrib rows [users | positive items] -> one sorted scatter into dpred (anchors repeat)
        coef = self.weight / B
        cp, cb = w["clparts"], w["contrib"]
        self.infonce(w["pred"], X1, 0, U, users, cp[:B], cb[:B], neg_users, SITE_NEG_USERS, coef)
        self.infonce(w["pred"], X1, U, self.I, pos, cp[B:2 * B], cb[B:2 * B], neg_items, SITE_NEG_ITEMS, coef)
        self._rf("gmr_rf_losses", N, ptr(w["rowparts"]), B, ptr(cp), self.weight, ptr(w["loss"]), stream())
        plan = sort_plan((users, pos), w["ka"])
        K.zero_(w["dpred"])
        _lib.call("gmr_scatter_sorted_f32", plan.numel(), D, ptr(plan), ptr(cb), D, ptr(w["dpred"]), D, stream())
        self._rf("gmr_rf_head_bwd", N, ptr(V), ptr(X1), X1.stride(0), ptr(w["X0"]), ptr(w["t"]), ptr(w["dpred"]),
                 ptr(w["dV"]), stream())
        self.slab.zero_grad()
        self._net_bwd(w, w["Xt"], w["S"], cond)
        self.step_ctr += 1
        if apply:
            self.adamw_step()
        return w["loss"]

    def adamw_step(self):
        """torch.optim.AdamW on the velocity slab; the step count is the generator's step counter."""
        b1, b2 = self.betas
        k = self.step_ctr
        bc1, bc2 = 1.0 - b1 ** k, 1.0 - b2 ** k
        _lib.call("gmr_adamw_f32", self.slab.numel, ptr(self.slab.data), ptr(self.slab.grad), ptr(self.exp_avg),
                  ptr(self.exp_avg_sq), b1, b2, self.eps, 1.0 - self.lr * self.wd, self.lr / bc1, bc2 ** 0.5, stream())

    # ------------------------------------------------------------------ sampling
    @torch.no_grad()
    def generate(self, cond, z0=None, n_steps=None, out=None, fused=None, base=None):
        """generate() (:896-975): n_steps Euler steps of the net from z0 ~ N(0, 1); dropout and guidance off.  base
        (N x 64 fp32, any row stride that is a multiple of 4, not out's table): out = base + inference_mix_ratio *
        rows instead of the rows, the mix as the sampler's epilogue (gmr_rf_sample_mix, the ratio read from the
        device scalar _ratio) or, fused=False, composed from the same entry points as the other RF models' mix."""
        N, D = cond.shape[0], self.D
        n_steps = int(n_steps or self.sampling_steps)
        if z0 is None:
            z0 = torch.empty((N, D), dtype=torch.float32, device=self.dev)
            _lib.call("gmr_rf_randn", N * D, self.seed, self.step_ctr, SITE_Z0, ptr(z0), stream())
        else:
            z0 = z0.to(self.dev).contiguous()
        if out is None:
            out = torch.empty((N, D), dtype=torch.float32, device=self.dev)
        fused = self.fused if fused is None else fused
        if base is not None:
            if base.dtype != torch.float32 or tuple(base.shape) != (N, D) or base.stride(1) != 1:
                raise ValueError(f"base must be a {N} x {D} fp32 table with unit column stride")
            if fused:
                self._rf("gmr_rf_sample_mix", N, H, self.C, self.L, n_steps, ptr(z0), z0.stride(0), ptr(cond),
                         cond.stride(0), ptr(self.slab.data), ptr(base), base.stride(0), ptr(self._ratio), ptr(out),
                         out.stride(0), stream(), at=2)
                return out
            if not out.is_contiguous():
                raise ValueError(f"the composed mix writes a contiguous N x {D} table")
            gen = self._generate_composed(cond, z0, n_steps, torch.empty_like(out))
            for c0 in range(0, D, 64):
                copy64(base[:, c0:c0 + 64], out[:, c0:c0 + 64])
            _lib.call("gmr_axpy_dev_f32", N * D, ptr(self._ratio), ptr(gen), ptr(out), stream())
            return out
        if fused:
            self._rf("gmr_rf_sample", N, H, self.C, self.L, n_steps, ptr(z0), z0.stride(0), ptr(cond),
                     cond.stride(0), ptr(self.slab.data), ptr(out), out.stride(0), stream(), at=2)
            return out
        return self._generate_composed(cond, z0, n_steps, out)

    def _generate_composed(self, cond, z0, n_steps, out):
        """The same integration, one launch per layer (the training kernels with no masks); N must be self.N."""
        if cond.shape[0] != self.N:
            raise ValueError("the composed sampler runs on the generator's own N rows")
        w, D = self._work(1), self.D
        save, self.dropout = self.dropout, 0.0
        try:
            z = w["Xt"]
            z.copy_(z0)
            dt = 1.0 / n_steps
            dtd = torch.tensor([dt], dtype=torch.float32, device=self.dev)
            for i in range(n_steps):
                w["t"].fill_(i * dt)
                _lib.call("gmr_rf_time_embed", self.N, ptr(w["t"]), ptr(w["S"]), stream())
                V = self._net_fwd(w, z, w["S"], cond, None)
                _lib.call("gmr_axpy_dev_f32", self.N * D, ptr(dtd), ptr(V), ptr(z), stream())
        finally:
            self.dropout = save
        if out.is_contiguous():
            out.copy_(z)
        else:
            out[:] = z
        return out


class RFBackbone:
    """What the RF-on-X models share, mixed in before the backbone: class RFX(RFBackbone, X).  use_rf: False is X and
    allocates no generator.  The model adds its buffers in __init__ (when use_rf), rf_step_inputs() -> (X1, cond,
    prior or None), the tables of the last backbone step the RF step trains on, and forward_embeddings(z0=None), its
    rule for mixing generate()'s rows into the evaluation tables once rf_warm().  rf_condition_dim() is the width of
    cond: 64 per modality unless the model says otherwise; rf_embedding_dim() the width of X1 and of the generated
    rows: 64 unless the model says otherwise."""

    def __init__(self, config, dataloader):
        super().__init__(config, dataloader)
        self.use_rf = bool(_get(config, "use_rf", True))
        self.rf_generator = None
        if not self.use_rf:
            return
        check_config(config)
        self.rf_generator = RFGenerator(self.n_users, self.n_items, self.rf_condition_dim(), self.device,
                                        seed=config_seed(config), embedding_dim=self.rf_embedding_dim(),
                                        **{kw: _get(config, key, d) for kw, (key, d) in RF_CONFIG.items()})
        self._training_epoch = -1  # incremented to 0 by the first pre_epoch_processing

    def rf_condition_dim(self):
        """Columns of the condition table: one 64-wide block per modality."""
        return 64 * len(self.mods)

    def rf_embedding_dim(self):
        """Columns of the target table and of the generated rows."""
        return D

    # ------------------------------------------------------------------ state
    def extra_state(self):
        """The backbone's state (none: {}) and the RF counters: a resumed run warms up and draws as the uninterrupted
        one would."""
        st = getattr(super(), "extra_state", dict)()
        if self.use_rf:
            st.update({"rf_epoch": int(self._training_epoch), "rf_step": int(self.rf_generator.step_ctr)})
        return st

    def load_extra_state(self, st):
        getattr(super(), "load_extra_state", lambda st: None)(st)
        if self.use_rf:
            self._training_epoch = int(st["rf_epoch"])
            self.rf_generator.step_ctr = int(st["rf_step"])
            self.rf_generator.set_epoch(self._training_epoch)

    def pre_epoch_processing(self):
        super().pre_epoch_processing()
        if self.use_rf:
            self._training_epoch += 1
            self.rf_generator.set_epoch(self._training_epoch)

    def rf_warm(self):
        return self.use_rf and self.rf_generator.warmed_up()

    # ------------------------------------------------------------------ training
    def rf_layer_mean(self, n_layers):
        """X1 of a LightGCN backbone: mean(E_0..E_n) of the last _forward, without the backbone's item term
        (all_embeddings_ori), into _x1."""
        tabs = [self.slab.view("E")] + self._layers[:n_layers]
        n = len(tabs)
        _lib.call("gmr_frd_mean_fwd", self.N, self.n_users, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs]),
                  (ctypes.c_int64 * n)(*[t.stride(0) for t in tabs]), None, 0, ptr(self._x1), self._x1.stride(0),
                  stream())
        return self._x1

    def rec_step(self, users, pos, neg, plan_bpr=None, plan_cl=None, norm_rows=None, reg_share=1.0, rf_draws=None,
                 **backbone_kw):
        """The backbone's step (backbone_kw: its own injected draws), then the RF step on the tables of that step.  The
        reference detaches them all, so nothing flows back and the backbone's gradients are the backbone's.  rf_draws:
        injected draws for RFGenerator.train_step.  rf_loss_terms() reads the RF losses."""
        loss = super().rec_step(users, pos, neg, plan_bpr, plan_cl, norm_rows, reg_share, **backbone_kw)
        if self.use_rf:
            X1, cond, prior = self.rf_step_inputs()
            self.rf_generator.train_step(X1, cond, users, pos, prior=prior, **(rf_draws or {}))
        return loss

    def rf_loss_terms(self):
        """[rf_loss, cl_loss, total] of the last RF step (device tensor)."""
        return self.rf_generator._w["loss"]
