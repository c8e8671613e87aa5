"""Shared builders of the LGMRec tests: the model on the golden tiny data (lgmrec_tiny.npz, lgmrec_tiny_B.npz), a plain
torch restatement of the LGMRec step written from the formulas in the module docstring of gmr/lgmrec.py, with autograd
(lgmrec_step_ref) and with hand-written backward equations (lgmrec_step_hand; tests/test_lgmrec_restatement_cpu.py
pins both to the golden values and to each other), and row-level restatements of the gmr_lgm_* kernels."""
import numpy as np
import torch
import torch.nn.functional as Fn

from lattice_fixture import adam_reach, bar  # noqa: F401  (the bar and the Adam reach, re-exported)
from mgcn_fixture import dense_of  # noqa: F401  (re-exported)

DEV = "cuda"
STATE_KEYS = ["item_image_trs", "v_hyper", "item_text_trs", "t_hyper", "user_embedding.weight",
              "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight"]
PARAMS = [k.replace(".", "_") for k in STATE_KEYS[:6]]          # the trainable ones, named_parameters() order
TABLES = ["user_embedding_weight", "item_id_embedding_weight"]
HYPER = ["v_hyper", "t_hyper"]
CASES = {"A": dict(n_hyper_layer=1, hyper_num=4, keep_rate=1.0), "B": dict(n_hyper_layer=2, hyper_num=5, keep_rate=0.5)}
N_UI_LAYERS, N_MM_LAYERS, ALPHA, CL_WEIGHT, REG_WEIGHT, TAU, LR, EPS = 2, 2, 0.3, 1e-4, 1e-6, 0.2, 0.001, 1e-12
ADAM_STEPS = 3
TABLE_SCALE, HYPER_SCALE = 8.0, 2.0   # case B: the id tables as MGCN's case B; the hyperedge weights so that rows saturate


def case_params(g, case):
    """{name of PARAMS: fp32 array} of a golden case: case A is its stored init, case B its stored init with the two
    embedding tables times 8 and the two hyperedge weights times 2 (the maker asserts both against the reference)."""
    out = {}
    for k in PARAMS:
        p = g[f"{case}_init_{k}"]
        if case == "B" and k in TABLES:
            p = p * np.float32(TABLE_SCALE)
        elif case == "B" and k in HYPER:
            p = p * np.float32(HYPER_SCALE)
        out[k] = p
    return out


def lgmrec_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "cf_model": "lightgcn", "n_ui_layers": N_UI_LAYERS,
         "n_mm_layers": N_MM_LAYERS, "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 1.0, "alpha": ALPHA,
         "cl_weight": CL_WEIGHT, "reg_weight": REG_WEIGHT, "learning_rate": LR}
    d.update(over)
    return Config("LGMRec", "baby", d)


def set_params(m, P):
    with torch.no_grad():
        for p, k in zip(m._params(), PARAMS):
            p.copy_(torch.as_tensor(np.asarray(P[k], np.float32)).to(p.device))


def build_lgmrec(g, case="A", v_feat="v_feat", t_feat="t_feat", **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference model
    was, then given the case's parameters."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.utils import get_model
    cfg = lgmrec_config(**dict(CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g[v_feat] if v_feat else None,
                                g[t_feat] if t_feat else None)
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = get_model("LGMRec")(cfg, tl)
    if case != "A":
        set_params(m, case_params(g, case))
    return m, cfg, ds, tl


# ----------------------------------------------------------------------------- graphs
def graphs_ref(U, I, rows, cols, dtype=torch.float64):
    """(adj U x I 0/1, norm_adj dense N x N with d = (degree + 1e-7)^-1/2, inv_deg = fp32(1 / (user degree + 1e-7)))
    at `dtype`."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    R = np.zeros((U, I), np.float64)
    R[rows, cols] = 1.0
    deg = np.concatenate([R.sum(1), R.sum(0)])
    d = np.power(deg + 1e-7, -0.5)
    A = np.zeros((U + I, U + I), np.float64)
    A[:U, U:] = R
    A[U:, :U] = R.T
    A = d[:, None] * A * d[None, :]
    inv = (1.0 / (deg[:U] + 1e-7)).astype(np.float32)
    return (torch.tensor(R, dtype=dtype), torch.tensor(A, dtype=dtype), torch.tensor(inv.astype(np.float64), dtype=dtype))


# ----------------------------------------------------------------------------- the forward
def normalize(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)


def hyper_rows(Li, R, gm, keep, keep_rate, tau=TAU):
    """(S, h) of one modality over the N rows (users first): the softmax of (L + g) / tau and its dropout.  keep: N x H
    0/1 or None; F.dropout's arithmetic (the kept entries times 1 / keep_rate)."""
    L = torch.cat([R @ Li, Li])
    S = torch.softmax((L + gm) / tau, dim=1)
    if keep is None or keep_rate >= 1.0:
        return S, S
    return S, S * keep.to(S.dtype) * (1.0 / keep_rate)


def ssl_triple(a, b, table, tau=TAU):
    """ssl_triple_loss (lgmrec.py:159-166)."""
    na, nb, nt = normalize(a), normalize(b), normalize(table)
    return (torch.logsumexp(na @ nt.T / tau, dim=1) - (na * nb).sum(1) / tau).sum()


def lgmrec_forward(P, X, graphs, U, c, g, keep):
    """The forward of lgmrec.py:115-151 on torch tensors of one dtype.  P: dict of PARAMS; X: (image, text) features;
    c: dict(n_hyper_layer, keep_rate, alpha, n_ui_layers, n_mm_layers, cf_model); g: 2 x N x H; keep: 2 x N x H or
    None.  Returns dict(all, cge, mge [v, t], x [v, t], S, h, lat (per modality the list over the layers), ins)."""
    R, A, inv = graphs
    E = torch.cat([P["user_embedding_weight"], P["item_id_embedding_weight"]])
    if c.get("cf_model", "lightgcn") == "mf":
        cge = E
    else:
        layers = [E]
        for _ in range(c.get("n_ui_layers", N_UI_LAYERS)):
            layers.append(A @ layers[-1])
        cge = torch.stack(layers, dim=1).mean(dim=1)
    out = {"cge": cge, "mge": [], "x": [], "S": [], "h": [], "lat": [], "ins": []}
    for m, (w, hy) in enumerate((("item_image_trs", "v_hyper"), ("item_text_trs", "t_hyper"))):
        F_ = X[m] @ P[w]
        mge = torch.cat([inv[:, None] * (R @ F_), F_])
        for _ in range(c.get("n_mm_layers", N_MM_LAYERS)):
            mge = A @ mge
        S, h = hyper_rows(X[m] @ P[hy], R, g[m], None if keep is None else keep[m], c["keep_rate"])
        hu, hi = h[:U], h[U:]
        i, lats, ins = cge[U:], [], []
        for _ in range(c["n_hyper_layer"]):
            ins.append(i)
            lats.append(hi.T @ i)
            i = hi @ lats[-1]
        out["mge"].append(mge)
        out["x"].append(torch.cat([hu @ lats[-1], i]))
        out["S"].append(S)
        out["h"].append(h)
        out["lat"].append(lats)
        out["ins"].append(ins)
    ghe = out["x"][0] + out["x"][1]
    out["all"] = cge + normalize(out["mge"][0]) + normalize(out["mge"][1]) + c.get("alpha", ALPHA) * normalize(ghe)
    return out


def lgmrec_loss(P, X, graphs, U, users, pos, neg, c, g, keep):
    """(loss, [bpr, cl_users, cl_items, reg], forward dict) of calculate_loss (lgmrec.py:175-194)."""
    f = lgmrec_forward(P, X, graphs, U, c, g, keep)
    al, (xv, xt) = f["all"], f["x"]
    u, p, n = al[users], al[U + pos], al[U + neg]
    bpr = -Fn.logsigmoid((u * p).sum(1) - (u * n).sum(1)).mean()
    cl_u = ssl_triple(xv[users], xt[users], xt[:U])
    cl_i = ssl_triple(xv[U + pos], xt[U + pos], xt[U:])
    reg = (u.norm() + p.norm() + n.norm()) / users.numel()
    cw, rw = c.get("cl_weight", CL_WEIGHT), c.get("reg_weight", REG_WEIGHT)
    loss = bpr + cw * (cl_u + cl_i) + rw * reg
    return loss, (bpr, cw * cl_u, cw * cl_i, rw * reg), f


def _lt(a):
    return torch.as_tensor(np.asarray(a).astype(np.int64))


def _tens(P, feats, g, keep, dtype, grad=True):
    Pt = {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=grad) for k in PARAMS}
    X = [torch.tensor(np.asarray(f), dtype=dtype) for f in feats]
    gt = torch.tensor(np.asarray(g), dtype=dtype)
    kt = None if keep is None else torch.as_tensor(np.asarray(keep))
    return Pt, X, gt, kt


def lgmrec_step_ref(P, U, I, rows, cols, users, pos, neg, c, feats, g, keep=None, g_eval=None, dtype=torch.float64):
    """One LGMRec step in plain torch with autograd at `dtype`.  Returns dict(loss, terms [bpr, cl_users, cl_items, reg],
    grads in PARAMS order, all, cge, S, h (2 x N x H), x (N x 128), scores (evaluation with g_eval, no dropout), adj,
    norm_adj, inv_deg) as numpy."""
    Pt, X, gt, kt = _tens(P, feats, g, keep, dtype)
    graphs = graphs_ref(U, I, rows, cols, dtype)
    loss, terms, f = lgmrec_loss(Pt, X, graphs, U, _lt(users), _lt(pos), _lt(neg), c, gt, kt)
    grads = torch.autograd.grad(loss, [Pt[k] for k in PARAMS])
    out = {"loss": loss.item(), "terms": np.array([t.item() for t in terms]), "grads": [x.numpy() for x in grads]}
    out.update({k: f[k].detach().numpy() for k in ("all", "cge")})
    out["S"], out["h"] = (torch.stack(f[k]).detach().numpy() for k in ("S", "h"))
    out["x"] = torch.cat(f["x"], dim=1).detach().numpy()
    if g_eval is not None:
        with torch.no_grad():
            ev = lgmrec_forward(Pt, X, graphs, U, c, torch.tensor(np.asarray(g_eval), dtype=dtype), None)["all"]
        out["scores"] = (ev[:U] @ ev[U:].T).numpy()
    out.update({k: v.numpy() for k, v in zip(("adj", "norm_adj", "inv_deg"), graphs)})
    return out


# ----------------------------------------------------------------------------- the backward by hand
def nbwd(x, dy):
    """d x of y = x / max(|x|, eps) from d y: (d y - y <y, d y>) / nrm, without the projection where the norm is
    clamped."""
    nrm = x.norm(dim=1, keepdim=True)
    cl = nrm.clamp_min(EPS)
    y = x / cl
    dp = (y * dy).sum(1, keepdim=True) * (nrm > EPS).to(x.dtype)
    return (dy - y * dp) / cl


def ssl_triple_bwd(a, table, idx, coef, tau=TAU):
    """(d a, d table) of coef * T(a, table[idx], table) with respect to the unnormalised rows."""
    na, nt = normalize(a), normalize(table)
    sm = torch.softmax(na @ nt.T / tau, dim=1)
    sm[torch.arange(a.shape[0]), idx] -= 1.0
    sm = sm * (coef / tau)
    return nbwd(a, sm @ nt), nbwd(table, sm.T @ na)


def lgmrec_step_hand(P, U, I, rows, cols, users, pos, neg, c, feats, g, keep=None, dtype=torch.float64):
    """The gradients of one step from hand-written backward equations (no autograd), in PARAMS order, as numpy."""
    Pt, X, gt, kt = _tens(P, feats, g, keep, dtype, grad=False)
    R, A, inv = graphs = graphs_ref(U, I, rows, cols, dtype)
    users, pos, neg = _lt(users), _lt(pos), _lt(neg)
    f = lgmrec_forward(Pt, X, graphs, U, c, gt, kt)
    al, N, B = f["all"], U + I, users.numel()
    cw, rw, alpha = c.get("cl_weight", CL_WEIGHT), c.get("reg_weight", REG_WEIGHT), c.get("alpha", ALPHA)
    # d all: BPR and the Frobenius norms
    u, p, n = al[users], al[U + pos], al[U + neg]
    ds = -torch.sigmoid(-((u * p).sum(1) - (u * n).sum(1)))[:, None] / B
    dall = torch.zeros_like(al)
    dall.index_add_(0, users, ds * (p - n) + rw / B * u / u.norm())
    dall.index_add_(0, U + pos, ds * u + rw / B * p / p.norm())
    dall.index_add_(0, U + neg, -ds * u + rw / B * n / n.norm())
    # d x_v, d x_t: the two contrastive terms, then alpha n(ghe)
    xv, xt = f["x"]
    dxv, dxt = torch.zeros_like(xv), torch.zeros_like(xt)
    for idx, lo, hi in ((users, 0, U), (pos, U, N)):
        da, dt = ssl_triple_bwd(xv[lo + idx], xt[lo:hi], idx, cw)
        dxv.index_add_(0, lo + idx, da)
        dxt[lo:hi] += dt
    dg = alpha * nbwd(xv + xt, dall)
    dcge = dall.clone()
    grads = {}
    for m, (w, hy, dx) in enumerate((("item_image_trs", "v_hyper", dxv + dg), ("item_text_trs", "t_hyper", dxt + dg))):
        # the modal view: n_mm hops back over the symmetric graph, the users' mean to the items
        dm = nbwd(f["mge"][m], dall)
        for _ in range(c.get("n_mm_layers", N_MM_LAYERS)):
            dm = A @ dm
        grads[w] = X[m].T @ (dm[U:] + R.T @ (inv[:, None] * dm[:U]))
        # the hyperedge layers
        S, h, lats, ins = f["S"][m], f["h"][m], f["lat"][m], f["ins"][m]
        hi = h[U:]
        L = len(lats)
        dlat = h.T @ dx
        dh = dx @ lats[-1].T
        for l in range(L, 0, -1):
            dh[U:] += ins[l - 1] @ dlat.T
            di = hi @ dlat
            if l > 1:
                dlat = hi.T @ di
                dh[U:] += di @ lats[l - 2].T
        dcge[U:] += di
        # dropout, softmax, the logits
        if kt is not None and c["keep_rate"] < 1.0:
            dh = dh * kt[m].to(dtype) * (1.0 / c["keep_rate"])
        dL = S * (dh - (dh * S).sum(1, keepdim=True)) / TAU
        grads[hy] = X[m].T @ (dL[U:] + R.T @ dL[:U])
    if c.get("cf_model", "lightgcn") == "mf":
        dE = dcge
    else:
        n_ui = c.get("n_ui_layers", N_UI_LAYERS)
        dE, t = dcge.clone(), dcge
        for _ in range(n_ui):
            t = A @ t
            dE = dE + t
        dE = dE / (n_ui + 1)
    grads["user_embedding_weight"], grads["item_id_embedding_weight"] = dE[:U], dE[U:]
    return [grads[k].numpy() for k in PARAMS]


def trajectory(P, U, I, rows, cols, users, pos, neg, c, feats, gs, keeps, dtype=torch.float64, lr=LR):
    """len(gs) torch.optim.Adam steps of the restatement at `dtype`; returns ([{name: parameters after step j}],
    [{name: gradient of step j}]) as numpy."""
    Pt, X, _, _ = _tens(P, feats, gs[0], None, dtype)
    graphs = graphs_ref(U, I, rows, cols, dtype)
    opt = torch.optim.Adam([Pt[k] for k in PARAMS], lr=lr)
    traj, glog = [], []
    for gj, kj in zip(gs, keeps):
        opt.zero_grad()
        loss, _, _ = lgmrec_loss(Pt, X, graphs, U, _lt(users), _lt(pos), _lt(neg), c,
                                 torch.tensor(np.asarray(gj), dtype=dtype), torch.as_tensor(np.asarray(kj)))
        loss.backward()
        glog.append({k: Pt[k].grad.detach().numpy().copy() for k in PARAMS})
        opt.step()
        traj.append({k: Pt[k].detach().numpy().copy() for k in PARAMS})
    return traj, glog
