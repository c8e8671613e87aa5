"""Shared builders of the FREEDOM tests: the model on the golden tiny data (freedom_tiny.npz) or on a synthetic
mid shape, the kNN list kinds of the union tests, and a plain torch restatement of the FREEDOM step from the
formulas in the module docstring of gmr/freedom.py (tests/test_freedom_restatement_cpu.py pins it to the golden
values; the GPU tests use its fp64 autograd at shapes the reference recorded nothing for)."""
import numpy as np
import torch

DEV = "cuda"
PARAMS = ["user_embedding_weight", "item_id_embedding_weight", "image_embedding_weight", "image_trs_weight",
          "image_trs_bias", "text_embedding_weight", "text_trs_weight", "text_trs_bias"]
CASES = {"A": dict(n_mm_layers=1, n_ui_layers=2, dropout=0.8), "B": dict(n_mm_layers=2, n_ui_layers=3, dropout=0.0)}


def freedom_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "knn_k": 5, "mm_image_weight": 0.1, "reg_weight": 0.001,
         "n_mm_layers": 1, "n_ui_layers": 2, "dropout": 0.8}
    d.update(over)
    return Config("FREEDOM", "baby", d)


def build_freedom(g, case="A", rows=None, cols=None, labels=None, **over):
    """The model on the fixture's train edges (or the given interactions), constructed under
    torch.manual_seed(3) as the fixture's reference model was."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.freedom import FREEDOM
    cfg = freedom_config(**dict(CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows = g["train_rows"] if rows is None else rows
    cols = g["train_cols"] if cols is None else cols
    labels = np.zeros(len(rows)) if labels is None else labels
    ds = RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    return FREEDOM(cfg, tl), cfg, ds, tl


def csr_keys(a):
    """(row * n_cols + col keys in CSR order, values) of a gmr CSR, on the host."""
    rp = a.rowptr.cpu().numpy().astype(np.int64)
    col = a.col.cpu().numpy().astype(np.int64)
    row = np.repeat(np.arange(a.n_rows), np.diff(rp))
    assert rp[-1] == col.size == a.nnz
    return row * a.n_cols + col, a.val.cpu().numpy()


def coo_keys(idx, val, n_cols):
    """The same of a coalesced COO (row-major order)."""
    key = idx[0].astype(np.int64) * n_cols + idx[1]
    o = np.argsort(key, kind="stable")
    return key[o], val[o]


def knn_lists(kind, n, k, rng):
    """Two n x k index lists without repeats in a row: identical, disjoint, or overlapping in alternate rows."""
    a = np.stack([rng.choice(n, k, replace=False) for _ in range(n)])
    if kind == "identical":
        return a, a.copy()
    rest = [np.setdiff1d(np.arange(n), r) for r in a]
    b = np.stack([rng.choice(r, k, replace=False) for r in rest])
    if kind == "overlap":   # rows alternate: shares ceil(k / 2) entries with a / disjoint from a
        h = (k + 1) // 2
        b[::2, :h] = a[::2, k - h:]
    return a, b


def build_freedom_mid(case, U=300, I=1100, per_user=20, widths=(37, 50), knn_k=10, batch=700, seed=21):
    """The model on synthetic interactions (per_user distinct items for every user, so some items have no edge)
    and random features of the given (image, text) widths.  Returns (model, rows, cols) with the edges in
    (user, item) order, the order of the model's user CSR."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.freedom import FREEDOM
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(U), per_user)
    cols = np.concatenate([np.sort(rng.choice(I, per_user, replace=False)) for _ in range(U)])
    v = np.abs(rng.standard_normal((I, widths[0]))).astype(np.float32)
    t = rng.standard_normal((I, widths[1])).astype(np.float32)
    cfg = freedom_config(**dict(CASES[case], knn_k=knn_k, train_batch_size=batch))
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(rows.size), U, I, v, t)
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    return FREEDOM(cfg, tl), rows, cols


# ----------------------------------------------------------------------------- restatement
def freedom_step_ref(P, U, I, rows, cols, knn_image, knn_text, users, pos, neg, n_mm_layers, n_ui_layers,
                     mm_image_weight=0.1, reg_weight=0.001, dtype=torch.float64):
    """One FREEDOM step in plain torch at `dtype`.  P: {name of PARAMS: array}; rows / cols: the kept user-item
    edges; knn_*: the I x k neighbour lists.  Returns dict(loss, terms [graph, text, image], grads in PARAMS
    order) as numpy."""
    N = U + I
    lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
    P = {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=True) for k in PARAMS}
    rows, cols, users, pos, neg = lt(rows), lt(cols), lt(users), lt(pos), lt(neg)
    # D^-1/2 A D^-1/2 of the kept bipartite edges, degrees + 1e-7
    du = torch.bincount(rows, minlength=U).to(dtype) + 1e-7
    di = torch.bincount(cols, minlength=I).to(dtype) + 1e-7
    val = du.pow(-0.5)[rows] * di.pow(-0.5)[cols]
    adj = torch.zeros((N, N), dtype=dtype)
    adj[rows, U + cols] = val
    adj[U + cols, rows] = val
    # w A_image + (1 - w) A_text, every entry of a k-list valued 1 / (k + 1e-7)
    mm = torch.zeros((I, I), dtype=dtype)
    for ind, wt in ((knn_image, mm_image_weight), (knn_text, 1.0 - mm_image_weight)):
        ind = lt(ind)
        k = ind.shape[1]
        r = torch.tensor(k + 1e-7, dtype=dtype).pow(-0.5)
        mm.index_put_((torch.arange(I).repeat_interleave(k), ind.reshape(-1)),
                      (wt * r * r).to(dtype).expand(I * k), accumulate=True)
    h = P["item_id_embedding_weight"]
    for _ in range(n_mm_layers):
        h = mm @ h
    ego = torch.cat([P["user_embedding_weight"], P["item_id_embedding_weight"]])
    layers = [ego]
    for _ in range(n_ui_layers):
        ego = adj @ ego
        layers.append(ego)
    mean = torch.stack(layers, dim=1).mean(dim=1)
    ua, ia = mean[:U], mean[U:] + h
    tf = P["text_embedding_weight"] @ P["text_trs_weight"].T + P["text_trs_bias"]
    vf = P["image_embedding_weight"] @ P["image_trs_weight"].T + P["image_trs_bias"]
    u = ua[users]

    def bpr(tab):
        x = (u * tab[pos]).sum(1) - (u * tab[neg]).sum(1)
        return -torch.nn.functional.logsigmoid(x).mean()

    terms = [bpr(ia), bpr(tf), bpr(vf)]
    loss = terms[0] + reg_weight * (terms[1] + terms[2])
    grads = torch.autograd.grad(loss, [P[k] for k in PARAMS])
    return {"loss": loss.item(), "terms": np.array([x.item() for x in terms]),
            "grads": [x.numpy() for x in grads]}


def check_grads(got, want, show=None):
    """The bars of test_freedom_gpu.py::_check_grads on gradient lists in PARAMS order."""
    want = dict(zip(PARAMS, want))
    for v, k in zip(got, PARAMS):
        w = want[k]
        if show:
            print(f"{show} {k}: max error {np.abs(v - w).max():.3e}, largest gradient {np.abs(w).max():.3e}")
        if k.endswith("_bias"):
            # analytically zero (the pos and neg terms cancel); bounded against the layer's weight gradient
            gw = want[k.replace("_bias", "_weight")]
            np.testing.assert_allclose(v, w, rtol=0, atol=1e-4 * np.abs(gw).max(), err_msg=k)
        else:
            np.testing.assert_allclose(v, w, rtol=1e-4, atol=1e-6 * np.abs(w).max(), err_msg=k)
