"""Shared builders of the MGCN tests: the model on the golden tiny data (mgcn_tiny.npz) or on a synthetic mid shape, a
plain torch restatement of the MGCN step from the formulas in the module docstring of gmr/mgcn.py
(tests/test_mgcn_restatement_cpu.py pins it to the golden values; the GPU tests use its fp64 autograd where the
reference recorded nothing), and row-level restatements of the purifier and the fuser (csrc/mgcn.hip)."""
import numpy as np
import torch
import torch.nn.functional as Fn

DEV = "cuda"
PARAMS = ["user_embedding_weight", "item_id_embedding_weight", "image_embedding_weight", "text_embedding_weight",
          "image_trs_weight", "image_trs_bias", "text_trs_weight", "text_trs_bias", "query_common_0_weight",
          "query_common_0_bias", "query_common_2_weight", "gate_v_0_weight", "gate_v_0_bias", "gate_t_0_weight",
          "gate_t_0_bias", "gate_image_prefer_0_weight", "gate_image_prefer_0_bias", "gate_text_prefer_0_weight",
          "gate_text_prefer_0_bias"]
STATE_KEYS = ["user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
              "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias", "query_common.0.weight",
              "query_common.0.bias", "query_common.2.weight", "gate_v.0.weight", "gate_v.0.bias", "gate_t.0.weight",
              "gate_t.0.bias", "gate_image_prefer.0.weight", "gate_image_prefer.0.bias", "gate_text_prefer.0.weight",
              "gate_text_prefer.0.bias"]
WIDE = ["query_common_0_weight", "query_common_2_weight", "gate_v_0_weight", "gate_t_0_weight",
        "gate_image_prefer_0_weight", "gate_text_prefer_0_weight"]
CASES = {"A": dict(n_layers=1, cl_loss=0.001), "B": dict(n_layers=2, cl_loss=0.1)}
KNN_K, N_UI_LAYERS, REG_WEIGHT, TEMP = 5, 2, 1e-4, 0.2


def case_params(g, case):
    """{name of PARAMS: fp32 array} of a golden case: case A is the stored init, case B the init with the two embedding
    tables times 8 and the six 64-input weights times fp32(sqrt(8)) (the maker asserts both against the reference)."""
    s8 = np.float32(np.sqrt(8.0))
    out = {}
    for k in PARAMS:
        p = g["init_" + k]
        if case == "B" and k in ("user_embedding_weight", "item_id_embedding_weight"):
            p = p * np.float32(8.0)
        elif case == "B" and k in WIDE:
            p = p * s8
        out[k] = p
    return out


def mgcn_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": REG_WEIGHT, "knn_k": KNN_K,
         "n_ui_layers": N_UI_LAYERS, "n_layers": 1, "cl_loss": 0.001}
    d.update(over)
    return Config("MGCN", "baby", d)


def set_params(m, P):
    """Load {name of PARAMS: array} into the model's slab through its parameter views."""
    with torch.no_grad():
        for p, k in zip(m._params(), PARAMS):
            p.copy_(torch.as_tensor(np.asarray(P[k], np.float32)).to(p.device))


def build_mgcn(g, case="A", **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference
    model was (its graphs come from the raw features), then given the case's parameters."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.mgcn import MGCN
    cfg = mgcn_config(**dict(CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = MGCN(cfg, tl)
    if case != "A":
        set_params(m, case_params(g, case))
    return m, cfg, ds, tl


def mid_data(U=300, I=1100, per_user=20, widths=(37, 50), batch=700, seed=21):
    """Synthetic interactions (per_user distinct items for every user, so some items have no edge), random
    features of the given (image, text) widths and a batch that repeats users and items."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(U), per_user)
    cols = np.concatenate([np.sort(rng.choice(I, per_user, replace=False)) for _ in range(U)])
    v = np.abs(rng.standard_normal((I, widths[0]))).astype(np.float32)
    t = rng.standard_normal((I, widths[1])).astype(np.float32)
    users = rng.integers(0, U, batch).astype(np.int32)
    pos = rng.integers(0, I, batch).astype(np.int32)
    neg = rng.integers(0, I, batch).astype(np.int32)
    return {"U": U, "I": I, "rows": rows, "cols": cols, "v_feat": v, "t_feat": t, "users": users, "pos": pos,
            "neg": neg}


def build_mgcn_mid(case="B", scale=True, **kw):
    """The model on mid_data, with case B's scaling of the drawn parameters (so that every gradient is large enough to
    test).  Returns (model, data)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.mgcn import MGCN
    d = mid_data(**kw)
    batch = d["users"].size
    cfg = mgcn_config(**dict(CASES[case], train_batch_size=batch, knn_k=10))
    ds = RecDataset.from_arrays(cfg, d["rows"], d["cols"], np.zeros(d["rows"].size), d["U"], d["I"], d["v_feat"],
                                d["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    m = MGCN(cfg, tl)
    if scale:
        g = {"init_" + k: p.detach().cpu().numpy() for k, p in zip(PARAMS, m._params())}
        set_params(m, case_params(g, "B"))
    return m, d


# ----------------------------------------------------------------------------- restatement
def knn_ref(feat, k, dtype=torch.float64):
    """The frozen item graph as a dense I x I matrix at `dtype`: cosine similarity, the k largest per row kept with
    their values, w_ij / sqrt(rowsum_i rowsum_j) with the row sums of the kept values on both ends."""
    f = torch.as_tensor(np.asarray(feat)).to(dtype)
    f = f / f.norm(dim=-1, keepdim=True)
    val, ind = torch.topk(f @ f.T, k, dim=-1)
    w = torch.zeros((f.shape[0], f.shape[0]), dtype=dtype).scatter_(-1, ind, val)
    d = w.sum(-1).pow(-0.5)
    d[torch.isinf(d)] = 0
    return d[:, None] * w * d[None, :]


def adj_ref(U, I, rows, cols, dtype=torch.float64):
    """D^-1/2 A D^-1/2 of the bipartite graph, dense (U + I)^2; a node without edges has d = 0."""
    rows, cols = torch.as_tensor(np.asarray(rows, np.int64)), torch.as_tensor(np.asarray(cols, np.int64))
    d = torch.cat([torch.bincount(rows, minlength=U), torch.bincount(cols, minlength=I)]).to(dtype).pow(-0.5)
    d[torch.isinf(d)] = 0
    adj = torch.zeros((U + I, U + I), dtype=dtype)
    adj[rows, U + cols] = d[rows] * d[U + cols]
    adj[U + cols, rows] = d[rows] * d[U + cols]
    return adj


def purify_rows_ref(E, V, T, Wgv, bgv, Wgt, bgt):
    """(Pv, Pt, gv, gt) of the purifier on torch tensors of one dtype."""
    gv, gt = torch.sigmoid(V @ Wgv.T + bgv), torch.sigmoid(T @ Wgt.T + bgt)
    return E * gv, E * gt, gv, gt


def fuse_rows_ref(a, b, c, W1, b1, w2, Wi, bi, Wt, bt):
    """(side, all, wa, wb) of the fuser on torch tensors of one dtype; w2 is the 1 x 64 weight."""
    q = torch.cat([torch.tanh(a @ W1.T + b1) @ w2.T, torch.tanh(b @ W1.T + b1) @ w2.T], dim=-1)
    w = torch.softmax(q, dim=-1)
    m = w[:, :1] * a + w[:, 1:] * b
    side = (torch.sigmoid(c @ Wi.T + bi) * (a - m) + torch.sigmoid(c @ Wt.T + bt) * (b - m) + m) / 3
    return side, c + side, w[:, 0], w[:, 1]


def nce_ref(x, y, temp=TEMP):
    x, y = Fn.normalize(x, dim=1), Fn.normalize(y, dim=1)
    return (torch.logsumexp(x @ y.T / temp, dim=1) - (x * y).sum(-1) / temp).mean()


def mgcn_step_ref(P, U, I, rows, cols, users, pos, neg, n_layers, cl_loss, feats=None, knn_k=KNN_K,
                  n_ui_layers=N_UI_LAYERS, reg_weight=REG_WEIGHT, batch_size=None, dtype=torch.float64):
    """One MGCN step in plain torch at `dtype`.  P: {name of PARAMS: array}; feats: the (image, text) features the
    frozen kNN graphs are built from (default: P's feature tables); batch_size: the divisor of the L2 term (default
    the number of rows).  Returns dict(loss, terms [bpr, reg, nce_items, nce_users], grads in PARAMS order, a, b, c,
    side, all, scores, adj, image_adj, text_adj) as numpy."""
    lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    feats = feats if feats is not None else (P["image_embedding_weight"], P["text_embedding_weight"])
    P = {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=True) for k in PARAMS}
    users, pos, neg = lt(users), lt(pos), lt(neg)
    adj = adj_ref(U, I, rows, cols, dtype)
    R = adj[:U, U:]
    graphs = [knn_ref(f, knn_k, dtype) for f in feats]
    Ei = P["item_id_embedding_weight"]
    V = P["image_embedding_weight"] @ P["image_trs_weight"].T + P["image_trs_bias"]
    T = P["text_embedding_weight"] @ P["text_trs_weight"].T + P["text_trs_bias"]
    Pv, Pt, _, _ = purify_rows_ref(Ei, V, T, P["gate_v_0_weight"], P["gate_v_0_bias"], P["gate_t_0_weight"],
                                   P["gate_t_0_bias"])
    views = []
    for h, A in zip((Pv, Pt), graphs):
        for _ in range(n_layers):
            h = A @ h
        views.append(torch.cat([R @ h, h]))
    a, b = views
    ego = torch.cat([P["user_embedding_weight"], Ei])
    layers = [ego]
    for _ in range(n_ui_layers):
        ego = adj @ ego
        layers.append(ego)
    c = torch.stack(layers, dim=1).mean(dim=1)
    side, al, _, _ = fuse_rows_ref(a, b, c, P["query_common_0_weight"], P["query_common_0_bias"],
                                   P["query_common_2_weight"], P["gate_image_prefer_0_weight"],
                                   P["gate_image_prefer_0_bias"], P["gate_text_prefer_0_weight"],
                                   P["gate_text_prefer_0_bias"])
    u, p, n = al[users], al[U + pos], al[U + neg]
    bpr = -Fn.logsigmoid((u * p).sum(-1) - (u * n).sum(-1)).mean()
    reg = reg_weight * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / (batch_size or users.numel())
    nce_i = nce_ref(side[U + pos], c[U + pos])
    nce_u = nce_ref(side[users], c[users])
    loss = bpr + reg + cl_loss * (nce_i + nce_u)
    grads = torch.autograd.grad(loss, [P[k] for k in PARAMS])
    det = lambda x: x.detach().numpy()  # noqa: E731
    return {"loss": loss.item(), "terms": np.array([bpr.item(), reg.item(), nce_i.item(), nce_u.item()]),
            "grads": [x.numpy() for x in grads], "a": det(a), "b": det(b), "c": det(c), "side": det(side),
            "all": det(al), "scores": det(al[:U] @ al[U:].T), "adj": det(adj), "image_adj": det(graphs[0]),
            "text_adj": det(graphs[1])}


def check_grads(got, want, show=None):
    """bm3_fixture.check_grads on MGCN's parameter names."""
    from bm3_fixture import check_grads as cg
    cg(got, want, names=PARAMS, show=show)


def dense_of(idx, val, shape):
    out = np.zeros(shape, np.float64)
    out[idx[0], idx[1]] = val
    return out
