"""A plain functional torch restatement of the rectified-flow generator (velocity net, training losses, sampler),
taking the weights, the draws and optional dropout masks.  tests/test_rf_cpu.py pins it to the golden values of
the reference at dropout 0 (tests/golden/rffreedom_tiny.npz); the GPU tests use its autograd as the expected
gradient with injected masks, and its fp64 run gives the fp32 spread behind the sampler / LayerNorm-gradient bars."""
import numpy as np
import torch
import torch.nn.functional as F

H = 128


def drop_sites(n_layers):
    """The dropout sites, by the names gmr.rf.RFGenerator gives them."""
    return ["time", "cond", "input"] + [f"block{l}a" for l in range(n_layers)] + ["out"]


def load_golden(golden):
    """The fixture of make_golden_rffreedom.py: four files (size limit), one dict."""
    g = {}
    for name in ("rffreedom_tiny", "rffreedom_tiny_param", "rffreedom_tiny_grad", "rffreedom_tiny_step"):
        g.update(golden(name))
    return g


def param_names(n_layers):
    """velocity_net.named_parameters() of the reference, in order."""
    out = ["time_embed.1.weight", "time_embed.1.bias"]
    for m in ("condition_encoder", "input_proj"):
        out += [f"{m}.0.weight", f"{m}.0.bias", f"{m}.1.weight", f"{m}.1.bias"]
    for l in range(n_layers):
        out += [f"res_blocks.{l}.net.{i}.{w}" for i in (0, 1, 4, 5) for w in ("weight", "bias")]
    out += [f"output_proj.{i}.{w}" for i in (0, 1, 4) for w in ("weight", "bias")]
    return out


def key(name):
    return name.replace(".", "_")


def params_from(g, tag, n_layers, prefix="p0_", dtype=torch.float32):
    return {n: torch.tensor(g[tag + prefix + key(n)], dtype=dtype) for n in param_names(n_layers)}


def sinusoidal(t):
    half = 32
    e = torch.log(torch.tensor(10000.0)) / (half - 1)
    f = torch.exp(torch.arange(half) * -e).to(t.dtype)
    a = t * f[None, :]
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


def _ln(x, P, name):
    return F.layer_norm(x, (H,), P[name + ".weight"], P[name + ".bias"], 1e-5)


def velocity(P, x, t, cond, n_layers, masks=None, p=0.0):
    """SimpleVelocityNet.forward without the guidance; t: (N, 1); masks: {site: N x 128 keep mask}."""
    def drop(a, site):
        if not masks or site not in masks:
            return a
        return a * (masks[site].to(a.dtype) * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(a.dtype))

    te = drop(F.silu(F.linear(sinusoidal(t), P["time_embed.1.weight"], P["time_embed.1.bias"])), "time")
    ce = drop(F.silu(_ln(F.linear(cond, P["condition_encoder.0.weight"], P["condition_encoder.0.bias"]), P,
                         "condition_encoder.1")), "cond")
    h = drop(F.silu(_ln(F.linear(x, P["input_proj.0.weight"], P["input_proj.0.bias"]), P, "input_proj.1")), "input")
    h = h + te + ce
    for l in range(n_layers):
        b = f"res_blocks.{l}.net."
        a = drop(F.silu(_ln(F.linear(h, P[b + "0.weight"], P[b + "0.bias"]), P, b + "1")), f"block{l}a")
        h = F.silu(_ln(F.linear(a, P[b + "4.weight"], P[b + "4.bias"]), P, b + "5") + h)
    a = drop(F.silu(_ln(F.linear(h, P["output_proj.0.weight"], P["output_proj.0.bias"]), P, "output_proj.1")), "out")
    return F.linear(a, P["output_proj.4.weight"], P["output_proj.4.bias"])


def cos_grad(x_t, x_1):
    cs = F.cosine_similarity(x_t, x_1, dim=-1).unsqueeze(-1)
    nt = x_t.norm(dim=-1, keepdim=True).clamp(min=1e-8)
    return F.normalize(x_1, dim=-1) / nt - F.normalize(x_t, dim=-1) * cs / nt


def infonce(pred, target, idx, neg, temp):
    """pred / target: one side's rows; idx (B) positives; neg (B, n_neg) after the collision rule."""
    a = F.normalize(pred[idx], dim=1)
    pos = torch.exp((a * F.normalize(target[idx], dim=1)).sum(-1) / temp)
    tn = F.normalize(target[neg], dim=1)  # as the reference (:762): over the n_neg axis of (B, n_neg, 64), per column
    ns = torch.exp(torch.bmm(a.unsqueeze(1), tn.transpose(1, 2)).squeeze(1) / temp)
    return torch.mean(-torch.log(pos / (pos + ns.sum(1))))


def collide(neg, pos, n):
    """The reference's rule on raw draws: a negative equal to the positive becomes (neg + 1) % n."""
    neg = np.asarray(neg).copy()
    hit = neg == np.asarray(pos)[:, None]
    neg[hit] = (neg[hit] + 1) % n
    return neg


def train_losses(P, X1, X0, t, cond, users, pos, neg_items, neg_users, n_users, n_layers, temp=0.2, weight=1.0,
                 masks=None, p=0.0):
    """compute_loss_and_step up to the total loss.  Returns dict(v, pred, rf_loss, cl_loss, total)."""
    X_t = t * X1 + (1 - t) * X0
    v = velocity(P, X_t, t, cond, n_layers, masks, p) + (1 - t) ** 2 * 0.1 * cos_grad(X_t, X1)
    rf = F.mse_loss(v, X1 - X0)
    pred = X_t + (1 - t) * v
    U = n_users
    cl = infonce(pred[U:], X1[U:], pos, neg_items, temp) + infonce(pred[:U], X1[:U], users, neg_users, temp)
    return {"v": v, "pred": pred, "rf_loss": rf, "cl_loss": cl, "total": rf + weight * cl}


def generate(P, cond, z0, n_steps, n_layers):
    z, dt = z0, 1.0 / n_steps
    for i in range(n_steps):
        t = torch.full((z.shape[0], 1), i * dt).to(z.dtype)
        z = z + velocity(P, z, t, cond, n_layers) * dt
    return z


def grads_of(P, loss):
    names = list(P)
    gs = torch.autograd.grad(loss, [P[n] for n in names])
    return dict(zip(names, gs))


def record_inputs(g, tag, dtype=torch.float32):
    """(X1, X0, t, cond, users, pos, neg_items, neg_users) of a golden record as tensors."""
    f = lambda k: torch.tensor(g[tag + k], dtype=dtype)  # noqa: E731
    i = lambda k: torch.tensor(g[tag + k].astype(np.int64))  # noqa: E731
    return f("X1"), f("X0"), f("t"), f("cond"), i("users"), i("pos"), i("neg_items"), i("neg_users")


def rel_to_max(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ---------------------------------------------------------------------------------------------- GPU builders
RF_TINY = dict(use_rf=True, use_denoise=False, use_2rf=False, rf_hidden_dim=128, rf_n_layers=2, rf_dropout=0.0,
               rf_learning_rate=0.001, rf_sampling_steps=3, rf_warmup_epochs=0, rf_inference_mix_ratio=0.2,
               rf_contrast_temp=0.2, rf_loss_weight=1.0, rf_infonce_negatives=7)


def build_rffreedom(f, rows=None, cols=None, labels=None, **over):
    """RFFREEDOM on the data of freedom_tiny.npz (case A), constructed under torch.manual_seed(3) as the
    fixture's reference model was."""
    from freedom_fixture import CASES
    from gmr.configurator import Config
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rffreedom import RFFREEDOM
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "knn_k": 5, "mm_image_weight": 0.1, "reg_weight": 0.001}
    d.update(CASES["A"])
    d.update(RF_TINY)
    d.update(over)
    cfg = Config("RFFREEDOM", "baby", d)
    U, I = int(f["U"]), int(f["I"])
    rows = f["train_rows"] if rows is None else rows
    cols = f["train_cols"] if cols is None else cols
    labels = np.zeros(len(rows)) if labels is None else labels
    ds = RecDataset.from_arrays(cfg, rows, cols, labels, U, I, f["v_feat"], f["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    return RFFREEDOM(cfg, tl), cfg, ds, tl


def build_generator(g, tag, n_layers, prefix="p0_", dropout=0.0, **kw):
    """gmr.rf.RFGenerator with a golden record's parameters."""
    from gmr.rf import RFGenerator
    U, I = 37, 41
    C = g[tag + "cond"].shape[1]
    gen = RFGenerator(U, I, C, "cuda", n_layers=n_layers, dropout=dropout, learning_rate=float(g["lr"]),
                      sampling_steps=int(g["steps"]), warmup_epochs=0, contrast_temp=0.2, contrast_weight=1.0,
                      n_negatives=int(g["n_neg"]), **kw)
    gen.load_reference_state({n: g[tag + prefix + key(n)] for n in param_names(n_layers)})
    return gen


def draws(g, tag, dev="cuda"):
    t = lambda k: torch.as_tensor(g[tag + k]).to(dev)  # noqa: E731
    return dict(X0=t("X0"), t=t("t"), neg_items=t("neg_items"), neg_users=t("neg_users"))


def grad_bar(g, tag):
    """Relative-to-max bound of a velocity gradient: 4x the reference's own fp32-vs-fp64 error on this record."""
    return 4.0 * float(g[tag + "err_grad"])
