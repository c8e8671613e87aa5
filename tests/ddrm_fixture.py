"""Shared pieces of the DDRM tests: the golden tiny data (ddrm_tiny.npz), model builders on it and on a synthetic mid
shape, and a plain torch restatement of the schedule, the training step and the prediction, written from the module
docstring of gmr/ddrm.py (tests/test_ddrm_restatement_cpu.py pins it to the golden values in fp32; the GPU tests use
it in fp64 at shapes the reference recorded nothing for)."""
import math
import os

import numpy as np
import torch

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddrm_tiny.npz")
TABLES = ("betas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_variance",
          "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def load_golden():
    """ddrm_tiny.npz and the recorded gradients (ddrm_tiny_grad.npz, a file of their own for its size)."""
    g = dict(np.load(GOLDEN, allow_pickle=False))
    g.update(np.load(GOLDEN.replace(".npz", "_grad.npz"), allow_pickle=False))
    return g


def key(name):
    return name.replace(".", "_")


def param_names():
    n = ["rec_model.embedding_user.weight", "rec_model.embedding_item.weight"]
    for m in ("user_reverse_model", "item_reverse_model"):
        for layer in ("emb_layer", "in_layers.0", "out_layers.0"):
            n += [f"{m}.{layer}.weight", f"{m}.{layer}.bias"]
    return n


def ddrm_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "is_multimodal_model": False}
    d.update(over)
    return Config("DDRM", "baby", d)


def build_model(rows, cols, U, I, seed=3, batch=16, **over):
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.ddrm import DDRM
    cfg = ddrm_config(train_batch_size=batch, **over)
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I)
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(seed)
    return DDRM(cfg, tl)


def build_ddrm(g, **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference
    model was."""
    return build_model(g["train_rows"], g["train_cols"], int(g["U"]), int(g["I"]), **over)


def mid_data(U=301, I=203, per_user=9, seed=23):
    """Synthetic interactions in (user, item) order; the last user has no train edge, some items none."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(U - 1), per_user)
    cols = np.concatenate([np.sort(rng.choice(I - 5, per_user, replace=False)) for _ in range(U - 1)])
    return rows, cols


# ----------------------------------------------------------------------------- restatement
def schedule_ref(T, noise_scale, noise_min, noise_max):
    """The fp64 tables of the 'linear-var' schedule with beta_0 pinned to 1e-5."""
    v = np.linspace(noise_scale * noise_min, noise_scale * noise_max, T, dtype=np.float64)
    ab = 1 - v
    betas = np.array([1 - ab[0]] + [min(1 - ab[i] / ab[i - 1], 0.999) for i in range(1, T)])
    betas[0] = 1e-5
    ac = np.cumprod(1 - betas)
    prev = np.concatenate([[1.0], ac[:-1]])
    pv = betas * (1 - prev) / (1 - ac)
    return {"betas": betas, "alphas_cumprod": ac, "sqrt_alphas_cumprod": np.sqrt(ac),
            "sqrt_one_minus_alphas_cumprod": np.sqrt(1 - ac), "posterior_variance": pv,
            "posterior_log_variance_clipped": np.log(np.concatenate([pv[1:2], pv[1:]])),
            "posterior_mean_coef1": betas * np.sqrt(prev) / (1 - ac),
            "posterior_mean_coef2": (1 - prev) * np.sqrt(1 - betas) / (1 - ac)}


def f32_table(a, dtype):
    """A schedule table as the model reads it: cast to fp32, then to the working type."""
    return torch.as_tensor(np.asarray(a, np.float64)).float().to(dtype)


def adj_ref(U, I, rows, cols, dtype):
    """D^-1/2 A D^-1/2 of the bipartite graph (dense, (U + I)^2); the entries are rounded to fp32 as the reference
    stores them."""
    N = U + I
    A = np.zeros((N, N), np.float64)
    A[np.asarray(rows), U + np.asarray(cols)] = 1
    A[U + np.asarray(cols), np.asarray(rows)] = 1
    deg = A.sum(1)
    with np.errstate(divide="ignore"):
        d = np.power(deg, -0.5)
    d[np.isinf(d)] = 0
    return torch.as_tensor((d[:, None] * A * d[None, :]).astype(np.float32)).to(dtype)


def encoder_ref(E, adj, n_layers):
    tabs = [E]
    for _ in range(n_layers):
        tabs.append(adj @ tabs[-1])
    return torch.stack(tabs, 1).mean(1)


def temb_ref(t, dtype):
    f = torch.exp(-math.log(10000.0) * torch.arange(32, dtype=torch.float32) / 32).to(dtype)
    a = t.to(dtype)[:, None] * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], -1)


def dnn_ref(P, m, x, cond, t, keep=None):
    """The denoiser m ('user_reverse_model' / 'item_reverse_model'); keep: 0/1 tensor (nn.Dropout(0.5)) or None.
    Returns (out, h, dropped input)."""
    dtype = x.dtype
    emb = temb_ref(t, dtype) @ P[m + ".emb_layer.weight"].T + P[m + ".emb_layer.bias"]
    if keep is not None:
        x = x * keep.to(dtype) * 2.0
    h = torch.tanh(torch.cat([x, emb, cond], -1) @ P[m + ".in_layers.0.weight"].T + P[m + ".in_layers.0.bias"])
    return h @ P[m + ".out_layers.0.weight"].T + P[m + ".out_layers.0.bias"], h, x


def tensors(P, dtype, grad=False):
    return {n: torch.tensor(np.asarray(P[key(n)]), dtype=dtype, requires_grad=grad) for n in param_names()}


def _lt(a):
    return torch.as_tensor(np.asarray(a).astype(np.int64))


def row_loss_ref(u, p, n, out_u, out_i, reg, alpha, beta, reg_weight):
    """The weighted row loss from the gathered rows and the denoiser outputs.  Returns (loss, w, softplus, recon)."""
    rec = (((u - out_u) ** 2).mean(1) + ((p - out_i) ** 2).mean(1)) / 2
    ps, ns = (u * p).sum(1), (u * n).sum(1)
    sp = torch.nn.functional.softplus(ns - ps)
    w = torch.sigmoid(ps).detach() ** beta
    return (w * ((1 - alpha) * (sp + reg_weight * reg) + alpha * rec)).mean(), w, sp, rec


def step_ref(P, U, I, rows, cols, users, pos, neg, t, noise_u, noise_i, keep_u, keep_i, sched, n_layers=3, alpha=0.1,
             beta=0.1, reg_weight=1e-4, dtype=torch.float64):
    """One training step at `dtype`.  Returns dict(loss, w, sp, rec, grads in param_names order)."""
    P = tensors(P, dtype, True)
    users, pos, neg, t = _lt(users), _lt(pos), _lt(neg), _lt(t)
    E = torch.cat([P["rec_model.embedding_user.weight"], P["rec_model.embedding_item.weight"]])
    G = encoder_ref(E, adj_ref(U, I, rows, cols, dtype), n_layers)
    u, p, n = G[users], G[U + pos], G[U + neg]
    sa = f32_table(sched["sqrt_alphas_cumprod"], dtype)[t][:, None]
    s1 = f32_table(sched["sqrt_one_minus_alphas_cumprod"], dtype)[t][:, None]
    tn = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    out_u, _, _ = dnn_ref(P, "user_reverse_model", sa * u + s1 * tn(noise_u), p, t, tn(keep_u))
    out_i, _, _ = dnn_ref(P, "item_reverse_model", sa * p + s1 * tn(noise_i), u, t, tn(keep_i))
    B = len(users)
    reg = 0.5 * ((E[users] ** 2).sum() + (E[U + pos] ** 2).sum() + (E[U + neg] ** 2).sum()) / B
    loss, w, sp, rec = row_loss_ref(u, p, n, out_u, out_i, reg, alpha, beta, reg_weight)
    names = param_names()
    gr = torch.autograd.grad(loss, [P[k] for k in names])
    return {"loss": loss.item(), "w": w.detach().numpy(), "sp": sp.detach().numpy(), "rec": rec.detach().numpy(),
            "grads": [x.numpy() for x in gr]}


def chain_ref(P, x, cond, S, sched, step_noise=None, dtype=torch.float64):
    """x <- c1[i] net_item(x, cond, i) + c2[i] x (+ exp(logvar[i] / 2) step_noise[i] where i != 0) for i = S-1..0;
    step_noise is indexed by timestep."""
    c1, c2 = f32_table(sched["posterior_mean_coef1"], dtype), f32_table(sched["posterior_mean_coef2"], dtype)
    sg = torch.exp(0.5 * torch.as_tensor(sched["posterior_log_variance_clipped"]).float()).to(dtype)
    for i in range(S - 1, -1, -1):
        t = torch.full((x.shape[0],), i, dtype=torch.int64)
        out, _, _ = dnn_ref(P, "item_reverse_model", x, cond, t)
        x = c1[i] * out + c2[i] * x
        if step_noise is not None and i != 0:
            x = x + sg[i] * torch.as_tensor(np.asarray(step_noise[i])).to(dtype)
    return x


def predict_ref(P, U, I, rows, cols, noise, S, sched, step_noise=None, n_layers=3, dtype=torch.float64):
    """(scores U x I, generated U x 64, items I x 64) for all users."""
    P = tensors(P, dtype)
    with torch.no_grad():
        E = torch.cat([P["rec_model.embedding_user.weight"], P["rec_model.embedding_item.weight"]])
        G = encoder_ref(E, adj_ref(U, I, rows, cols, dtype), n_layers)
        ua, ia = G[:U], G[U:]
        R = torch.zeros((U, I), dtype=dtype)
        R[_lt(rows), _lt(cols)] = 1
        xs = (R @ ia) / R.sum(1, keepdim=True).clamp(min=1)
        T = len(sched["betas"])
        sa = f32_table(sched["sqrt_alphas_cumprod"], dtype)[T - 1]
        s1 = f32_table(sched["sqrt_one_minus_alphas_cumprod"], dtype)[T - 1]
        x = sa * xs + s1 * torch.as_tensor(np.asarray(noise)).to(dtype)
        x = chain_ref(P, x, ua, S, sched, step_noise, dtype)
        return (x @ ia.T).numpy(), x.numpy(), ia.numpy()


def check_grads(got, want, names, show=None):
    """Gradient bars of DESIGN section 2: rtol 1e-4 with atol 1e-6 max|g| per parameter."""
    for v, w, n in zip(got, want, names):
        v, w = np.asarray(v), np.asarray(w)
        if show:
            print(f"{show} {n}: max error {np.abs(v - w).max():.3e}, largest gradient {np.abs(w).max():.3e}")
        np.testing.assert_allclose(v, w, rtol=1e-4, atol=1e-6 * np.abs(w).max(), err_msg=n)


def model_grads(m):
    sd = dict(m.named_parameters())
    return [sd[n].grad.detach().cpu().numpy() for n in param_names()]


def model_params(m):
    sd = dict(m.named_parameters())
    return {key(n): sd[n].detach().cpu().numpy() for n in param_names()}
