"""Shared builders of the RFBM3 tests: a plain torch restatement of RFBM3's RF inputs and of the generator's training
losses with the user-prior term, put together from tests/rf_fixture.py (the velocity net, InfoNCE) and
tests/bm3_fixture.py (the BM3 step); tests/test_rfbm3_cpu.py pins it to the reference's golden values
(tests/golden/make_golden_rfbm3.py), the GPU tests use its fp64 run where the reference recorded nothing."""
import numpy as np
import torch
import torch.nn.functional as F

import bm3_fixture as B
import rf_fixture as R

PRIOR_SCALE, COS_SCALE = 0.2, 0.1
FILES = ("rfbm3_tiny", "rfbm3_tiny_param", "rfbm3_tiny_grad", "rfbm3_tiny_step")
RF_TINY = dict(R.RF_TINY)


def load_golden(golden):
    """The fixture of make_golden_rfbm3.py: four files (size limit), one dict."""
    g = {}
    for name in FILES:
        g.update(golden(name))
    return g


def encoder_mean(P, U, I, rows, cols, n_layers, dtype=torch.float64):
    """X1 = mean(E_0..E_n) of BM3's encoder without the item residual (all_embeddings_ori)."""
    lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    rows, cols = lt(rows), lt(cols)
    N = U + I
    du = torch.bincount(rows, minlength=U).to(dtype) + 1e-7
    di = torch.bincount(cols, minlength=I).to(dtype) + 1e-7
    val = du.pow(-0.5)[rows] * di.pow(-0.5)[cols]
    adj = torch.zeros((N, N), dtype=dtype)
    adj[rows, U + cols] = val
    adj[U + cols, rows] = val
    ego = torch.cat([torch.tensor(np.asarray(P["user_embedding_weight"]), dtype=dtype),
                     torch.tensor(np.asarray(P["item_id_embedding_weight"]), dtype=dtype)])
    layers = [ego]
    for _ in range(n_layers):
        ego = adj @ ego
        layers.append(ego)
    return torch.stack(layers, dim=1).mean(dim=1)


def projected(P, mods=("image", "text"), dtype=torch.float64):
    """{modality: <name>_trs(<name>_embedding.weight)} at `dtype`."""
    f = lambda k: torch.tensor(np.asarray(P[k]), dtype=dtype)  # noqa: E731
    return {m: f(m + "_embedding_weight") @ f(m + "_trs_weight").T + f(m + "_trs_bias") for m in mods}


def rf_inputs_ref(T, V, U):
    """(cond, prior) of rfbm3.py:107-175 from the projected item tables (torch, either may be None): image then
    text on the item rows, zero user rows; prior = [0; Z - mean_items(Z)], Z = (0 + V) + T."""
    tabs = [x for x in (V, T) if x is not None]
    I, dt = tabs[0].shape[0], tabs[0].dtype
    cond = torch.cat([torch.cat([torch.zeros((U, 64), dtype=dt), x]) for x in tabs], dim=1)
    Z = torch.zeros((I, 64), dtype=dt)
    for x in tabs:
        Z = Z + x
    prior = torch.cat([torch.zeros((U, 64), dtype=dt), Z - Z.mean(dim=0, keepdim=True)])
    return cond, prior


def head_ref(V, Xt, X1, X0, t, prior):
    """The head's rows: v = (V + lam 0.2 prior) + lam 0.1 cos_grad, lam = (1 - t)^2; pred; squared-error row sums."""
    lam = (1 - t) ** 2
    v = V
    if prior is not None:
        v = v + lam * PRIOR_SCALE * prior
    v = v + lam * COS_SCALE * R.cos_grad(Xt, X1)
    return v, Xt + (1 - t) * v, ((v - (X1 - X0)) ** 2).sum(-1)


def train_losses(P, X1, X0, t, cond, prior, users, pos, neg_items, neg_users, n_users, n_layers, temp=0.2, weight=1.0,
                 masks=None, p=0.0):
    """compute_loss_and_step with user_prior up to the total loss: rf_fixture.train_losses with the prior term added
    before the cosine term.  Returns dict(v, pred, rf_loss, cl_loss, total)."""
    X_t = t * X1 + (1 - t) * X0
    v, pred, _ = head_ref(R.velocity(P, X_t, t, cond, n_layers, masks, p), X_t, X1, X0, t, prior)
    rf = F.mse_loss(v, X1 - X0)
    U = n_users
    cl = R.infonce(pred[U:], X1[U:], pos, neg_items, temp) + R.infonce(pred[:U], X1[:U], users, neg_users, temp)
    return {"v": v, "pred": pred, "rf_loss": rf, "cl_loss": cl, "total": rf + weight * cl}


def record_inputs(g, tag, dtype=torch.float32):
    """rf_fixture.record_inputs and the prior of a golden record."""
    return (*R.record_inputs(g, tag, dtype), torch.tensor(g[tag + "prior"], dtype=dtype))


def record_losses(g, tag, n_layers, dtype=torch.float32, prefix="p0_"):
    """train_losses on a golden record; returns (result dict, {name: gradient})."""
    P = {n: torch.tensor(g[tag + prefix + R.key(n)], dtype=dtype, requires_grad=True) for n in R.param_names(n_layers)}
    X1, X0, t, cond, users, pos, ni, nu, prior = record_inputs(g, tag, dtype)
    r = train_losses(P, X1, X0, t, cond, prior, users, pos, ni, nu, int(g["U"]), n_layers)
    return r, R.grads_of(P, r["total"])


def p1_bound(g, tag, name, bar, lr):
    """Bound on a stepped parameter given gradients within `bar` (as tests/test_rf_kernels_gpu.py): the
    first AdamW step moves p by lr g / (|g| + eps), whose slope in g is at most 1 / (|g| + eps) and whose range is
    2 lr; so an element's error is at most lr min(2, dg / (|g| + eps)) with dg the gradient bound, next to the 1e-5
    value bar."""
    gw = g[tag + "g_" + R.key(name)].astype(np.float64)
    dg = 1e-4 * np.abs(gw) + bar * np.abs(gw).max()
    return 1e-5 * np.abs(g[tag + "p1_" + R.key(name)]) + lr * np.minimum(2.0, dg / (np.abs(gw) + 1e-8))


# ---------------------------------------------------------------------------------------------- GPU builders
def rfbm3_config(case="A", **over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": B.REG_WEIGHT, "cl_weight": B.CL_WEIGHT}
    d.update(B.CASES[case])
    d.update(RF_TINY)
    d.update(over)
    return Config("RFBM3", "baby", d)


def build_rfbm3(g, case="A", mods=("image", "text"), rows=None, cols=None, labels=None, **over):
    """RFBM3 on the data of bm3_tiny.npz, constructed under torch.manual_seed(3) as the fixture's reference model
    was.  Returns (model, cfg, dataset, loader)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rfbm3 import RFBM3
    cfg = rfbm3_config(case, **over)
    U, I = int(g["U"]), int(g["I"])
    rows = g["train_rows"] if rows is None else rows
    cols = g["train_cols"] if cols is None else cols
    labels = np.zeros(len(rows)) if labels is None else labels
    ds = RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"] if "image" in mods else None,
                                g["t_feat"] if "text" in mods else None)
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    return RFBM3(cfg, tl), cfg, ds, tl


def build_rfbm3_mid(case="A", **over):
    """RFBM3 on bm3_fixture.mid_data (U = 300, I = 1,100, widths 37 / 50, B = 700).  Returns (model, data)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rfbm3 import RFBM3
    d = B.mid_data()
    batch = d["users"].size
    cfg = rfbm3_config(case, train_batch_size=batch, **over)
    ds = RecDataset.from_arrays(cfg, d["rows"], d["cols"], np.zeros(d["rows"].size), d["U"], d["I"], d["v_feat"],
                                d["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    return RFBM3(cfg, tl), d


def draws(g, tag, dev="cuda"):
    return R.draws(g, tag, dev)


def random_draws(rng, N, U, I, users, pos, n_neg=7):
    """Injected draws for a shape the reference recorded nothing at (numpy Generator): X0, t, collided negatives."""
    X0 = rng.standard_normal((N, 64)).astype(np.float32)
    t = rng.random((N, 1)).astype(np.float32)
    ni = R.collide(rng.integers(0, I, (len(pos), n_neg)), pos, I).astype(np.int32)
    nu = R.collide(rng.integers(0, U, (len(users), n_neg)), users, U).astype(np.int32)
    return {"X0": X0, "t": t, "neg_items": ni, "neg_users": nu}
