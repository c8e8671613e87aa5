"""Shared builders of the BM3 tests: the model on the golden tiny data (bm3_tiny.npz) or on a synthetic mid shape, a
plain torch restatement of the BM3 step from the formulas in the module docstring of gmr/bm3.py
(tests/test_bm3_restatement_cpu.py pins it to the golden values; the GPU tests use its fp64 autograd where the
reference recorded nothing), and a row-level restatement of the fused loss kernel (csrc/bm3.hip)."""
import numpy as np
import torch

DEV = "cuda"
PARAMS = ["user_embedding_weight", "item_id_embedding_weight", "predictor_weight", "predictor_bias",
          "image_embedding_weight", "image_trs_weight", "image_trs_bias", "text_embedding_weight", "text_trs_weight",
          "text_trs_bias"]
CASES = {"A": dict(n_layers=1, dropout=0.3), "B": dict(n_layers=2, dropout=0.5)}
REG_WEIGHT, CL_WEIGHT = 0.1, 2.0
TERMS = ("ui", "iu", "t", "v", "tv", "vt")


def params_of(mods=("image", "text")):
    """PARAMS without the tensors of an absent modality."""
    return [k for k in PARAMS if not any(k.startswith(m) for m in ("image", "text") if m not in mods)]


def bm3_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": REG_WEIGHT, "cl_weight": CL_WEIGHT,
         "n_layers": 1, "dropout": 0.3}
    d.update(over)
    return Config("BM3", "baby", d)


def build_bm3(g, case="A", mods=("image", "text"), **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference
    model was.  mods: the modalities given to it."""
    from gmr.bm3 import BM3
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    cfg = bm3_config(**dict(CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I,
                                g["v_feat"] if "image" in mods else None, g["t_feat"] if "text" in mods else None)
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    return BM3(cfg, tl), cfg, ds, tl


def mid_data(U=300, I=1100, per_user=20, widths=(37, 50), batch=700, seed=21):
    """Synthetic interactions (per_user distinct items for every user, so some items have no edge), random
    features of the given (image, text) widths and a batch that repeats users and items."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(U), per_user)
    cols = np.concatenate([np.sort(rng.choice(I, per_user, replace=False)) for _ in range(U)])
    v = np.abs(rng.standard_normal((I, widths[0]))).astype(np.float32)
    t = rng.standard_normal((I, widths[1])).astype(np.float32)
    users = rng.integers(0, U, batch).astype(np.int32)
    items = rng.integers(0, I, batch).astype(np.int32)
    return {"U": U, "I": I, "rows": rows, "cols": cols, "v_feat": v, "t_feat": t, "users": users, "items": items}


def build_bm3_mid(case="A", **kw):
    """The model on mid_data.  Returns (model, data)."""
    from gmr.bm3 import BM3
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    d = mid_data(**kw)
    batch = d["users"].size
    cfg = bm3_config(**dict(CASES[case], train_batch_size=batch))
    ds = RecDataset.from_arrays(cfg, d["rows"], d["cols"], np.zeros(d["rows"].size), d["U"], d["I"], d["v_feat"],
                                d["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    return BM3(cfg, tl), d


# ----------------------------------------------------------------------------- restatement
def cos_ref(a, b, eps=1e-8):
    """<a, b> / (max(|a|, eps) max(|b|, eps)) over rows, each norm clamped on its own."""
    return (a * b).sum(-1) / (a.norm(dim=-1).clamp_min(eps) * b.norm(dim=-1).clamp_min(eps))


def bm3_step_ref(P, U, I, rows, cols, users, items, keep, n_layers, dropout, reg_weight=REG_WEIGHT,
                 cl_weight=CL_WEIGHT, dtype=torch.float64, mods=("image", "text"), drop_terms=()):
    """One BM3 step in plain torch at `dtype`.  P: {name of PARAMS: array}; keep: {"u": U x 64, "i" / "t" / "v":
    I x 64} table keep masks; mods: the modalities present; drop_terms: modal terms left out of the loss by hand.
    Returns dict(loss, terms [ui, iu, t, v, tv, vt], reg, grads in params_of(mods) order, ua, ib) as numpy."""
    N = U + I
    names = params_of(mods)
    lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    P = {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=True) for k in names}
    K = {k: torch.tensor(np.asarray(v) != 0).to(dtype) for k, v in keep.items()}
    rows, cols, users, items = lt(rows), lt(cols), lt(users), lt(items)
    du = torch.bincount(rows, minlength=U).to(dtype) + 1e-7
    di = torch.bincount(cols, minlength=I).to(dtype) + 1e-7
    val = du.pow(-0.5)[rows] * di.pow(-0.5)[cols]
    adj = torch.zeros((N, N), dtype=dtype)
    adj[rows, U + cols] = val
    adj[U + cols, rows] = val
    ego = torch.cat([P["user_embedding_weight"], P["item_id_embedding_weight"]])
    layers = [ego]
    for _ in range(n_layers):
        ego = adj @ ego
        layers.append(ego)
    mean = torch.stack(layers, dim=1).mean(dim=1)
    ua, ib = mean[:U], mean[U:] + P["item_id_embedding_weight"]
    sc = 1.0 / (1.0 - dropout)
    pred = lambda x: x @ P["predictor_weight"].T + P["predictor_bias"]  # noqa: E731
    drop = lambda x, k: (x.detach() * K[k] * sc)  # noqa: E731
    ti, tu = drop(ib, "i")[items], drop(ua, "u")[users]
    zero = torch.zeros((), dtype=dtype)
    terms = {k: zero for k in TERMS}
    terms["ui"] = 1 - cos_ref(pred(ua)[users], ti).mean()
    terms["iu"] = 1 - cos_ref(pred(ib)[items], tu).mean()
    if "text" in mods:
        tf = P["text_embedding_weight"] @ P["text_trs_weight"].T + P["text_trs_bias"]
        on = pred(tf)[items]
        terms["t"] = 1 - cos_ref(on, ti).mean()
        terms["tv"] = 1 - cos_ref(on, drop(tf, "t")[items]).mean()
    if "image" in mods:
        vf = P["image_embedding_weight"] @ P["image_trs_weight"].T + P["image_trs_bias"]
        on = pred(vf)[items]
        terms["v"] = 1 - cos_ref(on, ti).mean()
        terms["vt"] = 1 - cos_ref(on, drop(vf, "v")[items]).mean()
    reg = (ua.norm() + ib.norm()) / I
    loss = terms["ui"] + terms["iu"] + reg_weight * reg
    loss = loss + cl_weight * sum(terms[k] for k in ("t", "v", "tv", "vt") if k not in drop_terms)
    grads = torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)
    grads = [np.zeros(P[k].shape) if x is None else x.numpy() for k, x in zip(names, grads)]
    return {"loss": loss.item(), "terms": np.array([terms[k].item() for k in TERMS]), "reg": reg.item(),
            "grads": grads, "ua": ua.detach().numpy(), "ib": ib.detach().numpy()}


def bm3_rows_ref(x, Wp, bp, keep, p, cl_weight, inv_norm, dtype=torch.float64):
    """The fused loss kernel's rows in plain torch at `dtype`.  x: the four gathered streams [u, i, t, v] (B x 64
    each; None for an absent modality); keep: their keep masks (B x 64; None = no dropout for that stream).
    Returns dict(cos 6 x B [ui, iu, t, v, tv, vt], contrib 2B x 192, don 4B x 64, xg 4B x 64) as numpy, the outputs
    of an absent stream zero."""
    B = x[0].shape[0]
    W = torch.tensor(np.asarray(Wp), dtype=dtype)
    b = torch.tensor(np.asarray(bp), dtype=dtype)
    has = [v is not None for v in x]
    xs = [torch.tensor(np.asarray(v) if h else np.zeros((B, 64)), dtype=dtype, requires_grad=True)
          for v, h in zip(x, has)]
    sc = torch.tensor(1.0, dtype=dtype) / (torch.tensor(1.0, dtype=dtype) - torch.tensor(p, dtype=dtype))
    tg = [xs[s].detach() * (torch.tensor(np.asarray(keep[s]) != 0).to(dtype) * sc if keep[s] is not None else 1.0)
          for s in range(4)]
    on = [v @ W.T + b for v in xs]
    for o in on:
        o.retain_grad()
    pairs = [(0, 1), (1, 0), (2, 1), (3, 1), (2, 2), (3, 3)]  # (online stream, target stream) of ui, iu, t, v, tv, vt
    cos = [cos_ref(on[a], tg[t]) if has[a] else torch.zeros(B, dtype=dtype) for a, t in pairs]
    wt = [1.0, 1.0, cl_weight, cl_weight, cl_weight, cl_weight]
    loss = sum(w * (1 - c.sum() * inv_norm) for w, c in zip(wt, cos))
    loss.backward()
    z = torch.zeros((B, 64), dtype=dtype)
    don = [o.grad if h else z for o, h in zip(on, has)]
    dx = [v.grad if h else z for v, h in zip(xs, has)]
    contrib = torch.cat([torch.cat([dx[0], z, z], 1), torch.cat([dx[1], dx[2], dx[3]], 1)])
    return {"cos": torch.stack(cos).detach().numpy(), "contrib": contrib.numpy(), "don": torch.cat(don).numpy(),
            "xg": torch.cat([v.detach() for v in xs]).numpy()}


def check_grads(got, want, names=PARAMS, show=None):
    """The bars of freedom_fixture.check_grads on gradient lists in `names` order (BM3's parameter names): a bias
    is bounded against its layer's weight gradient, everything else at rtol 1e-4 / atol 1e-6 of the largest entry."""
    want = dict(zip(names, want))
    for v, k in zip(got, names):
        w = want[k]
        if show:
            print(f"{show} {k}: max error {np.abs(v - w).max():.3e}, largest gradient {np.abs(w).max():.3e}")
        if k.endswith("_bias"):
            gw = want[k.replace("_bias", "_weight")]
            np.testing.assert_allclose(v, w, rtol=0, atol=1e-4 * np.abs(gw).max(), err_msg=k)
        else:
            np.testing.assert_allclose(v, w, rtol=1e-4, atol=1e-6 * np.abs(w).max(), err_msg=k)


def golden_keep(g, case):
    """The reference's four table keep masks of a case."""
    return {k: g[f"{case}_keep_{k}"] for k in "uitv"}


def batch_keep(keep, users, items, mods=("image", "text")):
    """The batch rows of the table masks in stream order [u, i, t, v]; None for an absent modality."""
    out = [keep["u"][users], keep["i"][items], keep["t"][items] if "text" in mods else None,
           keep["v"][items] if "image" in mods else None]
    return [None if k is None else np.ascontiguousarray(k) for k in out]
