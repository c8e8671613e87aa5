"""Shared builders of the LATTICE tests: the model on the golden tiny data (tests/golden/lattice_tiny*.npz) and a plain
torch restatement of the LATTICE step in the sparse slot form of gmr/lattice.py (the formulas of its module
docstring), with autograd at any dtype.  tests/test_lattice_restatement_cpu.py pins the restatement to the golden
values of the reference's dense formulation; the GPU tests use it where the reference recorded nothing."""
import numpy as np
import torch
import torch.nn.functional as Fn

DEV = "cuda"
ALL_PARAMS = ["modal_weight", "user_embedding_weight", "item_id_embedding_weight", "image_embedding_weight",
              "text_embedding_weight", "image_trs_weight", "image_trs_bias", "text_trs_weight", "text_trs_bias"]
GRAPH_SIDE = ("modal_weight", "image_embedding_weight", "text_embedding_weight", "image_trs_weight", "image_trs_bias",
              "text_trs_weight", "text_trs_bias")
CASES = {"A": dict(mods=("image", "text"), cf_model="lightgcn", n_layers=1, lambda_coeff=0.9),
         "B": dict(mods=("image", "text"), cf_model="lightgcn", n_layers=2, lambda_coeff=0.5),
         "C": dict(mods=("text",), cf_model="mf", n_layers=1, lambda_coeff=0.9)}
FILES = {"A": "lattice_tiny", "B": "lattice_tiny_B", "C": "lattice_tiny_C"}
KNN_K, REG_WEIGHT, WEIGHT_SIZE, BATCH = 5, 1e-3, [64, 64], 16
TRAJ_STEPS = ("build", "frozen", "frozen", "build")  # pre_epoch_processing() before the last one


def params_of(case):
    """The parameter names of a case in named_parameters() order ('.' as '_')."""
    mods = CASES[case]["mods"]
    return [p for p in ALL_PARAMS if p.split("_")[0] not in ("image", "text") or p.split("_")[0] in mods]


def case_params(g, case):
    """{name: fp32 array} of a golden case from the init stored in lattice_tiny.npz: cases A and C as drawn (C has no
    image parameters, so its text_trs takes the draws that are image_trs's in A: stored as C_init_text_trs_*), case B
    with the two embedding tables times 8."""
    out = {}
    for k in params_of(case):
        p = g[("C_init_" if case == "C" and k.startswith("text_trs") else "init_") + k]
        if case == "B" and k in ("user_embedding_weight", "item_id_embedding_weight"):
            p = p * np.float32(8.0)
        out[k] = p
    return out


def lattice_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": BATCH, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": REG_WEIGHT, "knn_k": KNN_K,
         "weight_size": list(WEIGHT_SIZE), "learning_rate": 0.001}
    d.update(over)
    return Config("LATTICE", "baby", d)


def set_params(m, P, names):
    with torch.no_grad():
        for p, k in zip(m._params(), names):
            p.copy_(torch.as_tensor(np.asarray(P[k], np.float32)).to(p.device))


def build_lattice(g, case="A", **over):
    """The model on the fixture's train edges and features, constructed under torch.manual_seed(3) as the fixture's
    reference model was, then given the case's parameters."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.lattice import LATTICE
    c = CASES[case]
    cfg = lattice_config(**dict({k: v for k, v in c.items() if k != "mods"}, **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    v = g["v_feat"] if "image" in c["mods"] else None
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, v, g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=BATCH)
    torch.manual_seed(3)
    m = LATTICE(cfg, tl)
    if case == "B":
        set_params(m, case_params(g, case), params_of(case))
    return m, cfg, ds, tl


# ----------------------------------------------------------------------------- restatement
def ui_adj_ref(U, I, rows, cols, dtype=torch.float64):
    """D^-1 (A + I) over the U + I nodes, dense."""
    rows, cols = torch.as_tensor(np.asarray(rows, np.int64)), torch.as_tensor(np.asarray(cols, np.int64))
    N = U + I
    a = torch.zeros((N, N), dtype=torch.float64)
    a[rows, U + cols] = 1
    a[U + cols, rows] = 1
    a = a + torch.eye(N, dtype=torch.float64)
    return (a / a.sum(1, keepdim=True)).to(dtype)


def orig_lists(feat, k, dtype=torch.float64):
    """The frozen graph of one modality as its I x k lists (idx, val): cosine similarity of the raw features, the k
    largest per row with their values, w_ij / sqrt(rowsum_i rowsum_j)."""
    f = torch.as_tensor(np.asarray(feat)).to(dtype)
    f = f / f.norm(dim=-1, keepdim=True)
    val, idx = torch.topk(f @ f.T, k, dim=-1)
    d = val.sum(-1).pow(-0.5)
    d[torch.isinf(d)] = 0
    return idx, d[:, None] * val * d[idx]


def learned_lists(T, mods, k):
    """Per modality (idx, v, n): the top-k lists of the normalised projections and their values as a function of the
    rows (the value and its derivative from one expression)."""
    out = []
    for m in mods:
        F = T[m + "_embedding_weight"] @ T[m + "_trs_weight"].T + T[m + "_trs_bias"]
        n = F / F.norm(dim=-1, keepdim=True)
        idx = torch.topk((n @ n.T).detach(), k, dim=-1).indices
        out.append((idx, (n[:, None, :] * n[idx]).sum(-1), n))
    return out


def build_graph_ref(T, mods, orig, k, lam):
    """item_adj in slot form: (col, val) of shape I x 2 M k, differentiable in val; also the per-modality lists."""
    lists = learned_lists(T, mods, k)
    M = len(mods)
    w = torch.softmax(T["modal_weight"], dim=0) if M == 2 else [1.0]
    a = [w[m] * lists[m][1] for m in range(M)]
    r = sum(x.sum(-1) for x in a)
    zero = r == 0
    s = torch.where(zero, torch.zeros_like(r), torch.where(zero, torch.ones_like(r), r).pow(-0.5))
    col = torch.cat([lists[m][0] for m in range(M)] + [orig[m][0] for m in range(M)], dim=1)
    val = torch.cat([(1 - lam) * (s[:, None] * a[m] * s[lists[m][0]]) for m in range(M)] +
                    [lam * (w[m] * orig[m][1]) for m in range(M)], dim=1)
    return col, val, lists, r


def dense_of_slots(col, val, I):
    """The I x I matrix of a slot list; a column listed several times in a row adds."""
    rows = torch.arange(I)[:, None].expand_as(col)
    return torch.zeros((I, I), dtype=val.dtype).index_put((rows, col), val, accumulate=True)


def tensors(P, names, dtype):
    return {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=True) for k in names}


def loss_ref(T, adj, col, val, users, pos, neg, n_layers, cf_model, n_ui_layers, reg_weight, batch_size):
    """(loss, ua, ia) of lattice.py:161-227 on the slot-form item graph."""
    Ei, Eu = T["item_id_embedding_weight"], T["user_embedding_weight"]
    h = Ei
    for _ in range(n_layers):
        h = (val[:, :, None] * h[col]).sum(1)
    if cf_model == "lightgcn":
        ego = torch.cat([Eu, Ei])
        layers = [ego]
        for _ in range(n_ui_layers):
            ego = adj @ ego
            layers.append(ego)
        ua, ia = torch.split(torch.stack(layers, dim=1).mean(dim=1), [Eu.shape[0], Ei.shape[0]])
    else:
        ua, ia = Eu, Ei
    ia = ia + Fn.normalize(h, p=2, dim=1)
    u, p, n = ua[users], ia[pos], ia[neg]
    bpr = -Fn.logsigmoid((u * p).sum(-1) - (u * n).sum(-1)).mean()
    reg = reg_weight * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / batch_size
    return bpr + reg, ua, ia


class Restatement:
    """The LATTICE of one golden case in plain torch at `dtype`."""

    def __init__(self, g, case, P=None, dtype=torch.float64, batch_size=BATCH):
        c = CASES[case]
        self.c, self.dtype, self.names = c, dtype, params_of(case)
        self.U, self.I = int(g["U"]), int(g["I"])
        self.T = tensors(P if P is not None else case_params(g, case), self.names, dtype)
        self.adj = ui_adj_ref(self.U, self.I, g["train_rows"], g["train_cols"], dtype)
        feats = {"image": g["v_feat"], "text": g["t_feat"]}
        self.orig = [orig_lists(feats[m], KNN_K, dtype) for m in c["mods"]]
        lt = lambda a: torch.as_tensor(np.asarray(a).astype(np.int64))  # noqa: E731
        self.batch = (lt(g["users"]), lt(g["pos"]), lt(g["neg"]))
        self.batch_size = batch_size
        self.graph = None  # (col, val) of the last build, detached

    def build(self):
        return build_graph_ref(self.T, self.c["mods"], self.orig, KNN_K, self.c["lambda_coeff"])

    def loss(self, build, batch=None):
        """The loss of a build step (the graph rebuilt and differentiated) or of a frozen step (the last build's)."""
        if build:
            col, val, self.lists, self.r = self.build()
            self.graph = (col, val.detach())
        else:
            col, val = self.graph
        loss, self.ua, self.ia = loss_ref(self.T, self.adj, col, val, *(batch or self.batch), self.c["n_layers"],
                                          self.c["cf_model"], len(WEIGHT_SIZE), REG_WEIGHT, self.batch_size)
        self.col, self.val = col, val
        return loss

    def step(self, build, batch=None):
        """dict(loss, grads in names order with None where autograd reaches nothing) of one step."""
        loss = self.loss(build, batch)
        grads = torch.autograd.grad(loss, [self.T[k] for k in self.names], allow_unused=True)
        return {"loss": loss.item(), "grads": [None if x is None else x.numpy() for x in grads]}

    def item_adj(self):
        return dense_of_slots(self.col, self.val.detach(), self.I).numpy()

    def scores(self):
        """full_sort_predict for all users: a graph built from the current parameters."""
        with torch.no_grad():
            col, val, _, _ = self.build()
            _, ua, ia = loss_ref(self.T, self.adj, col, val, *self.batch, self.c["n_layers"], self.c["cf_model"],
                                 len(WEIGHT_SIZE), REG_WEIGHT, self.batch_size)
            return (ua @ ia.T).numpy()

    def trajectory(self, lr=0.001):
        """The parameters after each of TRAJ_STEPS under torch.optim.Adam: [{name: array}, ...]."""
        params = [self.T[k] for k in self.names]
        opt = torch.optim.Adam(params, lr=lr, foreach=False)
        out, self.grad_log = [], []
        for kind in TRAJ_STEPS:
            opt.zero_grad(set_to_none=True)
            self.loss(kind == "build").backward()
            self.grad_log.append({k: None if self.T[k].grad is None else self.T[k].grad.numpy().copy()
                                  for k in self.names})
            opt.step()
            out.append({k: self.T[k].detach().numpy().copy() for k in self.names})
        return out


def adam_reach(g64, g32, lr=0.001, b2=0.999, eps=1e-8):
    """How far gradients within the gradient bar can move an Adam trajectory, per step and element (the bound of
    rfbm3_fixture.p1_bound, carried over several steps).  g64 / g32: the gradient logs of the fp64 and the fp32
    restatement ([{name: array or None}, ...]).  A step's update is u = lr mhat / (sqrt(vhat) + eps).  With every
    gradient within dg of the reference's, mhat moves by at most dg and so does sqrt(vhat) (a weighted 2-norm of the
    gradient history with weights that sum to 1), and |mhat| <= 1.1 sqrt(vhat) over the first four steps (the two
    weight sets differ by at most 5 %), so |du| <= lr 2.1 dg / (sqrt(vhat) + eps), and never more than 2.2 lr.  dg is
    the gradient bar itself: 1e-5 |g| + twice fp32 torch's own error on that gradient.  Returns [{name: array}, ...],
    the sums over the steps so far; a step without a gradient adds nothing."""
    out, acc, v, t = [], {}, {}, {}
    for s64, s32 in zip(g64, g32):
        for k, g in s64.items():
            acc.setdefault(k, 0.0)
            if g is None:
                continue
            t[k] = t.get(k, 0) + 1
            v[k] = b2 * v.get(k, 0.0) + (1 - b2) * g * g
            vhat = v[k] / (1 - b2 ** t[k])
            dg = 1e-5 * np.abs(g) + 2 * np.abs(s32[k].astype(np.float64) - g).max()
            acc[k] = acc[k] + lr * np.minimum(2.2, 2.1 * dg / (np.sqrt(vhat) + eps))
        out.append({k: np.array(a, dtype=np.float64) for k, a in acc.items()})
    return out


def bar(got, ref64, ref32, what, rtol=1e-5):
    """test_mgcn_kernels_gpu's bar: rtol 1e-5 against fp64 with an atol of twice fp32 torch's own error."""
    own = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    got = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    print(f"{what}: max abs error {np.abs(got - ref64).max():.3e} (fp32 torch {own:.3e})")
    np.testing.assert_allclose(got, ref64, rtol=rtol, atol=2 * own, err_msg=what)
