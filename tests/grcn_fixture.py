"""Shared builders of the GRCN tests: the model on the golden tiny data (grcn_tiny.npz, grcn_tiny_B.npz) and a plain
torch restatement of the GRCN step written from the formulas in the module docstring of gmr/grcn.py (index_add_ over
the edge list, no torch_geometric), with autograd (grcn_step_ref) and with hand-written backward equations
(grcn_step_hand; tests/test_grcn_restatement_cpu.py pins both to the golden values and to each other)."""
import numpy as np
import torch

from lattice_fixture import adam_reach, bar  # noqa: F401  (the bar and the Adam reach, re-exported)

DEV = "cuda"
D = 64
EPS = 1e-12
SLOPE = 0.01
LR = 0.001
ADAM_STEPS = 3
# named_parameters() of the reference: the module's own parameter, then id_gcn, v_gcn, t_gcn
STATE_KEYS = ["model_specific_conf", "id_gcn.id_embedding", "v_gcn.preference", "v_gcn.MLP.weight", "v_gcn.MLP.bias",
              "t_gcn.preference", "t_gcn.MLP.weight", "t_gcn.MLP.bias"]
PARAMS = [k.replace(".", "_") for k in STATE_KEYS]
CASES = {"A": dict(n_layers=3, reg_weight=0.001, mods="vt"), "B": dict(n_layers=1, reg_weight=0.1, mods="vt"),
         "C": dict(n_layers=3, reg_weight=0.001, mods="v")}


def params_of(case):
    return PARAMS if CASES[case]["mods"] == "vt" else PARAMS[:5]


def case_params(g, case):
    """{name: fp32 array} of a golden case: its stored init with model_specific_conf times the maker's conf_scale
    (the margins of the max and the ReLU, see tests/golden/make_golden_grcn.py)."""
    out = {k: g[f"{case}_init_{k}"] for k in params_of(case)}
    out["model_specific_conf"] = out["model_specific_conf"] * np.float32(g["conf_scale"])
    return out


def set_params(m, P):
    with torch.no_grad():
        for p, k in zip(m._params(), PARAMS):
            p.copy_(torch.as_tensor(np.asarray(P[k], np.float32)).to(p.device))


def grcn_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "embedding_size": 64, "latent_embedding": 64, "n_layers": 3,
         "reg_weight": 0.001, "learning_rate": LR}
    d.update(over)
    return Config("GRCN", "baby", d)


def build_grcn(g, case="A", v_feat="v_feat", t_feat="t_feat", as_drawn=False, **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference model
    was, then given the case's parameters (as_drawn: left at its init)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.utils import get_model
    c = dict(CASES[case])
    mods = c.pop("mods")
    cfg = grcn_config(**dict(c, **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g[v_feat] if v_feat else None,
                                g[t_feat] if (t_feat and "t" in mods) else None)
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = get_model("GRCN")(cfg, tl)
    if not as_drawn:
        set_params(m, case_params(g, case))
    return m, cfg, ds, tl


# ----------------------------------------------------------------------------- pieces
def normalize(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)


def normalize_bwd(y, nrm, dy):
    """d x of y = x / max(|x|, eps) (nrm = |x|, n x 1); a clamped row is a plain division."""
    free = (dy - y * (y * dy).sum(1, keepdim=True)) / nrm.clamp_min(EPS)
    return torch.where(nrm > EPS, free, dy / EPS)


def seg_softmax(s, idx, n):
    """torch_geometric.utils.softmax: the group's maximum subtracted (no gradient through it), the sum + 1e-16."""
    mx = torch.full((n,), -float("inf"), dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax")
    e = (s - mx[idx]).exp()
    den = torch.zeros(n, dtype=s.dtype).index_add_(0, idx, e) + 1e-16
    return e / den[idx]


def attend(xd, xs, didx, sidx):
    """(h, alpha): alpha_e = softmax over the edges of a destination of <xd[dest], xs[src]>, h[d] = sum alpha_e xs[src]."""
    a = seg_softmax((xd[didx] * xs[sidx]).sum(1), didx, xd.shape[0])
    return torch.zeros_like(xd).index_add_(0, didx, a[:, None] * xs[sidx]), a


def attend_bwd(xd, xs, didx, sidx, alpha, dh, dalpha):
    """(d xd, d xs) of attend from dh and dalpha (None: 0)."""
    t = (dh[didx] * xs[sidx]).sum(1)
    if dalpha is not None:
        t = t + dalpha
    tbar = torch.zeros(xd.shape[0], dtype=xd.dtype).index_add_(0, didx, alpha * t)
    ds = alpha * (t - tbar[didx])
    dxd = torch.zeros_like(xd).index_add_(0, didx, ds[:, None] * xs[sidx])
    dxs = torch.zeros_like(xs).index_add_(0, sidx, alpha[:, None] * dh[didx] + ds[:, None] * xd[didx])
    return dxd, dxs


def tensors(P, names, dtype, grad=True):
    return {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=grad) for k in names}


def _mods(T, feats):
    """[(preference, W, b, X), ...] of the modalities present."""
    out = []
    for m, X in zip("vt", feats):
        if X is not None and m + "_gcn_preference" in T:
            out.append((T[m + "_gcn_preference"], T[m + "_gcn_MLP_weight"], T[m + "_gcn_MLP_bias"], X))
    return out


def cgcn_forward(pref, W, b, X, rows, cols, n_layers, keep=None, route=False):
    """CGCN.forward (grcn.py:139-166): rep (N x 64) and alpha (2E: item-destination values in edge order, then the
    user-destination ones).  The routing rounds run over the E edges from the users to the items (:149-156), so the
    user rows receive no message there and a round is p <- n(p + 0); route = True routes over the user's items instead
    (the model's routing: items).  keep: a dict that receives the intermediates the hand-written backward reads."""
    U, I = pref.shape[0], X.shape[0]
    z = torch.nn.functional.leaky_relu(X @ W.T + b, SLOPE)
    f, p = normalize(z), normalize(pref)
    ps, hs = [p], []
    for _ in range(n_layers):
        h, a = attend(p, f, rows, cols) if route else (torch.zeros_like(p), None)
        hs.append(a)
        p = normalize(p + h)
        ps.append(p)
    hu, a = attend(p, f, rows, cols)
    hi, bb = attend(f, p, cols, rows)
    if keep is not None:
        keep.update(z=z, f=f, ps=ps, route_alpha=hs, a=a, b=bb)
    return torch.cat([p + hu, f + hi]), torch.cat([bb, a])


def refine(alphas, conf, rows, cols, U):
    """w (2E) = relu(max_m alpha_m conf[source, m]); also the argmax and the values."""
    src = torch.cat([rows, cols + U])
    val = torch.stack(alphas, dim=1) * conf[src]
    mx, arg = val.max(dim=1)
    return torch.relu(mx), arg, val


def id_forward(E, w, rows, cols, U):
    """EGCN.forward (grcn.py:93-109): x + x1 + x2 over the 2E directed edges with weights w."""
    src, dst = torch.cat([rows, cols + U]), torch.cat([cols + U, rows])
    x = normalize(E)
    x1 = torch.zeros_like(x).index_add_(0, dst, w[:, None] * x[src])
    x2 = torch.zeros_like(x).index_add_(0, dst, w[:, None] * x1[src])
    return x + x1 + x2, x, x1


def grcn_forward(T, feats, rows, cols, n_layers, keep=None, route=False):
    """GRCN.forward (grcn.py:224-298): (result N x 64 (1 + M), alpha 2E x M)."""
    U = T["v_gcn_preference"].shape[0]
    reps, alphas, kept = [], [], []
    for pref, W, b, X in _mods(T, feats):
        k = {} if keep is not None else None
        rep, al = cgcn_forward(pref, W, b, X, rows, cols, n_layers, k, route)
        reps.append(rep)
        alphas.append(al)
        kept.append(k)
    w, arg, val = refine(alphas, T["model_specific_conf"], rows, cols, U)
    id_rep, x, x1 = id_forward(T["id_gcn_id_embedding"], w, rows, cols, U)
    if keep is not None:
        keep.update(mods=kept, w=w, arg=arg, val=val, x=x, x1=x1, alphas=alphas)
    return torch.cat([id_rep] + reps, dim=1), torch.stack(alphas, dim=1)


def grcn_loss(T, result, users, pos, neg, reg_weight, has_t=True):
    """calculate_loss (grcn.py:300-333), the unused terms left out."""
    U = T["v_gcn_preference"].shape[0]
    ut = users.repeat_interleave(2)
    it = torch.stack([pos + U, neg + U]).t().reshape(-1)
    score = (result[ut] * result[it]).sum(1).view(-1, 2)
    loss = -torch.log(torch.sigmoid(score[:, 0] - score[:, 1])).mean()
    E = T["id_gcn_id_embedding"]
    reg = (E[ut] ** 2 + E[it] ** 2).mean() + (T["v_gcn_preference"] ** 2).mean()
    reg = reg + (T["v_gcn_preference"][ut] ** 2).mean()
    if has_t:
        reg = reg + (T["t_gcn_preference"][ut] ** 2).mean()
    return loss + reg_weight * reg


def _inputs(P, U, I, rows, cols, users, pos, neg, feats, names, dtype, grad=True):
    T = tensors(P, names, dtype, grad)
    fe = [None if x is None else torch.tensor(np.asarray(x), dtype=dtype) for x in feats]
    ix = [torch.as_tensor(np.asarray(a, np.int64)) for a in (rows, cols, users, pos, neg)]
    return T, fe, ix


def grcn_step_ref(P, U, I, rows, cols, users, pos, neg, cfg, feats, dtype=torch.float64):
    """One step by autograd: {"loss", "result", "alpha", "grads": [in params_of order]}."""
    names = [k for k in PARAMS if k in P]
    T, fe, (rows, cols, users, pos, neg) = _inputs(P, U, I, rows, cols, users, pos, neg, feats, names, dtype)
    result, alpha = grcn_forward(T, fe, rows, cols, cfg["n_layers"], route=cfg.get("routing") == "items")
    loss = grcn_loss(T, result, users, pos, neg, cfg["reg_weight"], "t_gcn_preference" in T)
    loss.backward()
    return {"loss": loss.item(), "result": result.detach().numpy(), "alpha": alpha.detach().numpy(),
            "grads": [T[k].grad.numpy() for k in names]}


def grcn_step_hand(P, U, I, rows, cols, users, pos, neg, cfg, feats, dtype=torch.float64):
    """The same step with the backward written out (the equations of gmr/grcn.py's docstring); no autograd."""
    names = [k for k in PARAMS if k in P]
    T, fe, (rows, cols, users, pos, neg) = _inputs(P, U, I, rows, cols, users, pos, neg, feats, names, dtype, False)
    R, rw, B, N, E = cfg["n_layers"], cfg["reg_weight"], len(users), U + I, len(rows)
    K = {}
    route = cfg.get("routing") == "items"
    result, alpha = grcn_forward(T, fe, rows, cols, R, K, route)
    mods = _mods(T, fe)
    M = len(mods)
    loss = grcn_loss(T, result, users, pos, neg, rw, M == 2)
    # ---- the loss rows
    ru, rp, rn = result[users], result[U + pos], result[U + neg]
    s = (ru * (rp - rn)).sum(1)
    c = -torch.sigmoid(-s) / B
    dres = torch.zeros_like(result)
    dres.index_add_(0, users, c[:, None] * (rp - rn))
    dres.index_add_(0, U + pos, c[:, None] * ru)
    dres.index_add_(0, U + neg, -c[:, None] * ru)
    G = {}
    Eid = T["id_gcn_id_embedding"]
    dE = torch.zeros_like(Eid)
    dE.index_add_(0, users, rw * Eid[users] / (32.0 * B))
    dE.index_add_(0, U + pos, rw * Eid[U + pos] / (64.0 * B))
    dE.index_add_(0, U + neg, rw * Eid[U + neg] / (64.0 * B))
    # ---- the id branch
    src, dst = torch.cat([rows, cols + U]), torch.cat([cols + U, rows])
    g, w, x, x1 = dres[:, :D], K["w"], K["x"], K["x1"]
    dx1 = g + torch.zeros_like(g).index_add_(0, src, w[:, None] * g[dst])
    dx = g + torch.zeros_like(g).index_add_(0, src, w[:, None] * dx1[dst])
    dw = (x[src] * dx1[dst]).sum(1) + (x1[src] * g[dst]).sum(1)
    G["id_gcn_id_embedding"] = dE + normalize_bwd(x, Eid.norm(dim=1, keepdim=True), dx)
    # ---- refine
    conf, arg, val = T["model_specific_conf"], K["arg"], K["val"]
    live = (val.gather(1, arg[:, None])[:, 0] > 0).to(dtype) * dw
    dconf = torch.zeros_like(conf)
    dalpha = []
    for m in range(M):
        sel = (arg == m).to(dtype) * live
        dalpha.append(sel * conf[src, m])
        dconf[:, m].index_add_(0, src, sel * K["alphas"][m])
    G["model_specific_conf"] = dconf
    # ---- the modalities
    for m, ((pref, W, b, X), k, name) in enumerate(zip(mods, K["mods"], "vt"[:M] if M == 2 else "v")):
        drep = dres[:, D * (1 + m):D * (2 + m)]
        f, ps = k["f"], k["ps"]
        p = ps[-1]
        dp1, df1 = attend_bwd(p, f, rows, cols, k["a"], drep[:U], dalpha[m][E:])
        df2, dp2 = attend_bwd(f, p, cols, rows, k["b"], drep[U:], dalpha[m][:E])
        dp, df = drep[:U] + dp1 + dp2, drep[U:] + df1 + df2
        for r in range(R - 1, -1, -1):
            if not route:
                dp = normalize_bwd(ps[r + 1], ps[r].norm(dim=1, keepdim=True), dp)
                continue
            h, _ = attend(ps[r], f, rows, cols)
            dy = normalize_bwd(ps[r + 1], (ps[r] + h).norm(dim=1, keepdim=True), dp)
            dpd, dfs = attend_bwd(ps[r], f, rows, cols, k["route_alpha"][r], dy, None)
            dp, df = dy + dpd, df + dfs
        dpref = normalize_bwd(ps[0], pref.norm(dim=1, keepdim=True), dp)
        dpref = dpref + torch.zeros_like(pref).index_add_(0, users, rw * pref[users] / (32.0 * B))
        if m == 0:
            dpref = dpref + rw * 2.0 * pref / pref.numel()
        z = k["z"]
        dz = normalize_bwd(f, z.norm(dim=1, keepdim=True), df)
        dz = torch.where(z > 0, dz, SLOPE * dz)
        G[name + "_gcn_preference"], G[name + "_gcn_MLP_weight"], G[name + "_gcn_MLP_bias"] = dpref, dz.T @ X, dz.sum(0)
    return {"loss": loss.item(), "result": result.numpy(), "alpha": alpha.numpy(), "grads": [G[k].numpy() for k in names]}


def trajectory(P, U, I, rows, cols, users, pos, neg, cfg, feats, dtype=torch.float64, steps=ADAM_STEPS, lr=LR):
    """`steps` torch.optim.Adam steps of the restatement on one batch: ([{name: parameter after step j}],
    [{name: gradient of step j}])."""
    names = [k for k in PARAMS if k in P]
    T, fe, (rows, cols, users, pos, neg) = _inputs(P, U, I, rows, cols, users, pos, neg, feats, names, dtype)
    opt = torch.optim.Adam([T[k] for k in names], lr=lr)
    traj, grads = [], []
    for _ in range(steps):
        opt.zero_grad()
        result, _ = grcn_forward(T, fe, rows, cols, cfg["n_layers"], route=cfg.get("routing") == "items")
        grcn_loss(T, result, users, pos, neg, cfg["reg_weight"], "t_gcn_preference" in T).backward()
        grads.append({k: T[k].grad.numpy().copy() for k in names})
        opt.step()
        traj.append({k: T[k].detach().numpy().copy() for k in names})
    return traj, grads
