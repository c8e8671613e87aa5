"""Shared pieces of the LD4MRec tests: the golden tiny data (ld4mrec_tiny.npz), model builders on it and on a
synthetic mid shape, and a plain torch restatement of the training step and the prediction, written from the
module docstring of gmr/ld4mrec.py (tests/test_ld4mrec_restatement_cpu.py pins it to the golden values in fp32;
the GPU tests use it in fp64 at shapes the reference recorded nothing for)."""
import math
import os

import numpy as np
import torch

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ld4mrec_tiny.npz")


def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def key(name):
    return name.replace(".", "_")


def param_names(L):
    n = ["t_in", "mm_project.weight", "mm_project.bias"]
    for m in ("item_proj", "cond_proj", "time_proj"):
        n += [f"cnet.{m}.weight", f"cnet.{m}.bias"]
    for l in range(L):
        for m in ("norm1", "linear1", "linear2", "cond_scale", "cond_shift"):
            n += [f"cnet.layers.{l}.{m}.weight", f"cnet.layers.{l}.{m}.bias"]
    return n + ["cnet.output_proj.weight", "cnet.output_proj.bias"]


def ld4_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "svd_k": 8, "cnet_hidden_size": 64, "cnet_n_layers": 2,
         "steps": 100, "dropout": 0.0}
    d.update(over)
    return Config("LD4MRec", "baby", d)


def build_ld4(g, svd=True, **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference
    model was; svd=True injects the fixture's user_svd_emb."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.ld4mrec import LD4MRec
    cfg = ld4_config(**over)
    U, I = int(g["U"]), int(g["I"])
    ds = RecDataset.from_arrays(cfg, g["train_rows"], g["train_cols"], np.zeros(len(g["train_rows"])), U, I,
                                g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    return LD4MRec(cfg, tl, user_svd_emb=g["user_svd_emb"] if svd else None)


def mid_data(U=300, I=1103, per_user=20, widths=(37, 50), seed=21):
    """Synthetic interactions (per_user distinct items for every user, so some items have no edge) and random
    features; edges in (user, item) order."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(U), per_user)
    cols = np.concatenate([np.sort(rng.choice(I, per_user, replace=False)) for _ in range(U)])
    v = np.abs(rng.standard_normal((I, widths[0]))).astype(np.float32)
    t = rng.standard_normal((I, widths[1])).astype(np.float32)
    return rows, cols, v, t


def build_ld4_mid(L, U=300, I=1103, batch=700, svd_k=16, H=256, dropout=0.1):
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.ld4mrec import LD4MRec
    rows, cols, v, t = mid_data(U, I)
    cfg = ld4_config(train_batch_size=batch, svd_k=svd_k, cnet_hidden_size=H, cnet_n_layers=L, dropout=dropout)
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(rows.size), U, I, v, t)
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    np.random.seed(5)
    return LD4MRec(cfg, tl), rows, cols, v, t


# ----------------------------------------------------------------------------- restatement
def schedule_ref(T, a):
    """alpha_bar in fp32, the docstring's order of operations."""
    t = torch.arange(1, T + 1, dtype=torch.float32)
    ab = 1 - (a + (t - 1) / (T - 1) * (1 - a))
    alpha = ab / torch.cat([torch.ones(1), ab[:-1]])
    beta = torch.clamp(1 - alpha, 1e-4, 0.9999)
    return torch.cumprod(1 - beta, 0)


def user_mm_ref(U, I, rows, cols, feats, dtype=torch.float64):
    """D_u^-1/2 R D_i^-1/2 feats; D^-1/2 of a zero degree is 0."""
    R = torch.zeros((U, I), dtype=dtype)
    R[torch.as_tensor(rows).long(), torch.as_tensor(cols).long()] = 1
    du, di = R.sum(1), R.sum(0)
    iu = torch.where(du > 0, du.pow(-0.5), torch.zeros_like(du))
    ii = torch.where(di > 0, di.pow(-0.5), torch.zeros_like(di))
    return (iu[:, None] * R * ii[None, :]) @ torch.as_tensor(feats).to(dtype)


def temb_ref(t, H, dtype):
    half = H // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32) * -math.log(10000.0) / (half - 1)).to(dtype)
    e = t.to(dtype)[:, None] * f[None, :]
    return torch.cat([torch.sin(e), torch.cos(e)], 1)


def _lin(P, n, x):
    return x @ P[n + ".weight"].T + P[n + ".bias"]


def cnet_ref(P, L, x, temb, cond, masks=None, p_keep=1.0):
    """C-Net forward.  masks: L keep tensors (B x H) applied as inverted dropout, or None."""
    H = P["cnet.time_proj.weight"].shape[0]
    h = _lin(P, "cnet.item_proj", x)
    g = _lin(P, "cnet.cond_proj", cond) + _lin(P, "cnet.time_proj", temb)
    for l in range(L):
        b = f"cnet.layers.{l}."
        n = torch.nn.functional.layer_norm(h, (H,), P[b + "norm1.weight"], P[b + "norm1.bias"], 1e-5)
        z = n * (1 + _lin(P, b + "cond_scale", g)) + _lin(P, b + "cond_shift", g)
        a = torch.nn.functional.gelu(_lin(P, b + "linear1", z))
        if masks is not None:
            a = a * masks[l].to(a.dtype) * (1.0 / p_keep)
        h = h + _lin(P, b + "linear2", a)
    return _lin(P, "cnet.output_proj", h)


def _tensors(P, L, dtype, grad):
    return {n: torch.tensor(np.asarray(P[key(n)]), dtype=dtype, requires_grad=grad and n != "t_in")
            for n in param_names(L)}


def _cond(P, users, svd, mm):
    return torch.cat([svd[users], _lin(P, "mm_project", mm[users])], 1)


def ld4_step_ref(P, L, U, I, rows, cols, users, t, noise, alpha_bar, svd, mm, gamma=0.1, masks=None, p_keep=1.0,
                 hist=None, dtype=torch.float64):
    """One training step at `dtype`.  P: {name with dots -> underscores: array}.  Returns dict(loss, rows, grads in
    param_names order (t_in: zeros), hist = loss_history after the step (fp32 loop), when hist is given)."""
    P = _tensors(P, L, dtype, True)
    lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    users, t = lt(users), lt(t)
    X = torch.zeros((U, I), dtype=dtype)
    X[lt(rows), lt(cols)] = 1
    x_in = X[users]
    target = x_in * (1 - gamma) + (1 - x_in) * gamma
    ab = torch.as_tensor(np.asarray(alpha_bar))  # fp32 table; its square roots are taken in fp32
    sa, s1 = torch.sqrt(ab)[t].to(dtype)[:, None], torch.sqrt(1 - ab)[t].to(dtype)[:, None]
    x_t = sa * x_in + s1 * torch.as_tensor(np.asarray(noise)).to(dtype)
    H = P["cnet.time_proj.weight"].shape[0]
    svd, mm = torch.as_tensor(np.asarray(svd)).to(dtype), torch.as_tensor(np.asarray(mm)).to(dtype)
    mk = None if masks is None else [torch.as_tensor(np.asarray(m)) for m in masks]
    pred = cnet_ref(P, L, x_t, temb_ref(t, H, dtype), _cond(P, users, svd, mm), mk, p_keep)
    row = ((pred - target) ** 2).mean(1)
    loss = row.mean()
    names = param_names(L)
    gr = torch.autograd.grad(loss, [P[n] for n in names if n != "t_in"])
    grads = [np.zeros(1, np.float32)] + [x.numpy() for x in gr]
    res = {"loss": loss.item(), "rows": row.detach().numpy(), "grads": grads}
    if hist is not None:
        res["hist"] = history_ref(hist, t.numpy(), row.detach().numpy())
    return res


def history_ref(hist, t, row_loss):
    """loss_history[t_b] <- 0.9 loss_history[t_b] + 0.1 loss_b in batch order, in the fp32 arithmetic of a torch
    fp32 element updated with python floats; t_b < 0 skips the row."""
    h = np.asarray(hist, np.float32).copy()
    for tb, lb in zip(t, row_loss):
        if tb < 0:
            continue
        h[tb] = np.float32(np.float32(0.9) * h[tb]) + np.float32(0.1 * float(np.float32(lb)))
    return h


def ld4_predict_ref(P, L, U, I, rows, cols, users, svd, mm, t_in=None, dtype=torch.float64):
    """Scores of `users`: C-Net(x_in, temb(|t_in|), cond), no dropout."""
    P = _tensors(P, L, dtype, False)
    lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    users = lt(users)
    X = torch.zeros((U, I), dtype=dtype)
    X[lt(rows), lt(cols)] = 1
    H = P["cnet.time_proj.weight"].shape[0]
    tv = torch.abs(P["t_in"] if t_in is None else torch.tensor([t_in], dtype=dtype)).expand(len(users))
    svd, mm = torch.as_tensor(np.asarray(svd)).to(dtype), torch.as_tensor(np.asarray(mm)).to(dtype)
    with torch.no_grad():
        return cnet_ref(P, L, X[users], temb_ref(tv, H, dtype), _cond(P, users, svd, mm)).numpy()


def check_grads(got, want, names, show=None):
    """Gradient bars of DESIGN section 2: rtol 1e-4 with atol 1e-6 max|g| per parameter."""
    for v, w, n in zip(got, want, names):
        v, w = np.asarray(v), np.asarray(w)
        if show:
            print(f"{show} {n}: max error {np.abs(v - w).max():.3e}, largest gradient {np.abs(w).max():.3e}")
        np.testing.assert_allclose(v, w, rtol=1e-4, atol=1e-6 * np.abs(w).max(), err_msg=n)


def model_grads(m, L):
    """The model's gradients in param_names order (host arrays)."""
    sd = dict(m.named_parameters())
    return [sd[n].grad.detach().cpu().numpy() for n in param_names(L)]


def model_params(m, L):
    sd = dict(m.named_parameters())
    return {key(n): sd[n].detach().cpu().numpy() for n in param_names(L)}
