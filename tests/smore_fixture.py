"""Shared builders of the SMORE tests: the model on the golden tiny data (smore_tiny.npz), a plain torch restatement of
the SMORE step written from the formulas in the module docstring of gmr/smore.py (real cosine / sine matrices, no
torch.fft; tests/test_smore_restatement_cpu.py pins it to the golden values and to torch.fft's autograd), and row-level
restatements of the spectrum step and the fuser (csrc/smore.hip)."""
import numpy as np
import torch
import torch.nn.functional as Fn

from lattice_fixture import adam_reach, bar  # noqa: F401  (the bar and the Adam reach, re-exported)
from mgcn_fixture import adj_ref, dense_of, knn_ref, nce_ref  # noqa: F401  (re-exported)

DEV = "cuda"
FILTERS = ["image_complex_weight", "text_complex_weight", "fusion_complex_weight"]
_LIN = ["image_trs", "text_trs"]
_Q = ["query_v", "query_t"]
_G = ["gate_v", "gate_t", "gate_f", "gate_image_prefer", "gate_text_prefer", "gate_fusion_prefer"]
STATE_KEYS = (FILTERS + ["user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight",
                         "text_embedding.weight"] + [f"{m}.{x}" for m in _LIN for x in ("weight", "bias")] +
              [f"{m}.{x}" for m in _Q for x in ("0.weight", "0.bias", "2.weight")] +
              [f"{m}.0.{x}" for m in _G for x in ("weight", "bias")])
PARAMS = [k.replace(".", "_") for k in STATE_KEYS]
TABLES = ["user_embedding_weight", "item_id_embedding_weight"]
# the 64-input weights case B scales by sqrt(8)
WIDE = [f"{m}_{x}" for m in _Q for x in ("0_weight", "2_weight")] + [f"{m}_0_weight" for m in _G]
CASES = {"A": dict(n_layers=1, dropout_rate=0.0, cl_loss=0.01), "B": dict(n_layers=2, dropout_rate=0.1, cl_loss=0.1)}
IMAGE_K, TEXT_K, N_UI_LAYERS, REG_WEIGHT, TEMP, LR = 5, 3, 2, 1e-4, 0.2, 0.001
ADAM_STEPS = 3


def case_params(g, case):
    """{name of PARAMS: fp32 array} of a golden case: case A is the stored init, case B the init with the two embedding
    tables times 8 and the 64-input weights times fp32(sqrt(8)) (the maker asserts both against the reference)."""
    s8 = np.float32(np.sqrt(8.0))
    out = {}
    for k in PARAMS:
        p = g["init_" + k]
        if case == "B" and k in TABLES:
            p = p * np.float32(8.0)
        elif case == "B" and k in WIDE:
            p = p * s8
        out[k] = p
    return out


def golden_keep(g, step=0):
    """The reference's three keep masks of case B's step (N x 192 uint8: [image | text | fusion])."""
    return np.ascontiguousarray(g["B_keep"][step])


def smore_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": REG_WEIGHT, "image_knn_k": IMAGE_K,
         "text_knn_k": TEXT_K, "n_ui_layers": N_UI_LAYERS, "n_layers": 1, "cl_loss": 0.01, "dropout_rate": 0.0,
         "learning_rate": LR}
    d.update(over)
    return Config("SMORE", "baby", d)


def set_params(m, P):
    """Load {name of PARAMS: array} into the model's slab through its parameter views."""
    with torch.no_grad():
        for p, k in zip(m._params(), PARAMS):
            p.copy_(torch.as_tensor(np.asarray(P[k], np.float32)).to(p.device))


def build_smore(g, case="A", **over):
    """The model on the fixture's train edges, constructed under torch.manual_seed(3) as the fixture's reference model
    was (its graphs come from the raw features), then given the case's parameters."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.utils import get_model
    cfg = smore_config(**dict(CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = get_model("SMORE")(cfg, tl)
    if case != "A":
        set_params(m, case_params(g, case))
    return m, cfg, ds, tl


# ----------------------------------------------------------------------------- the spectrum step
def trig(dtype=torch.float64):
    """(C, S, ck): C[k][n] = cos(theta k n) / 8, S[k][n] = sin(theta k n) / 8 for k = 0..32, n = 0..63, evaluated in
    double on the reduced angle index (k n mod 64), the sine rows of k = 0 and k = 32 exact zeros; ck = 1, 2, .., 2,
    1."""
    k, n = np.arange(33)[:, None], np.arange(64)[None, :]
    m = (k * n) % 64
    C = np.cos(2 * np.pi * m / 64) / 8
    S = np.sin(2 * np.pi * m / 64) / 8
    for tab in (C, S):           # the exact values at the multiples of a quarter turn
        tab[m % 16 == 0] = np.round(tab[m % 16 == 0] * 8) / 8
    assert not S[0].any() and not S[32].any()
    ck = np.full(33, 2.0)
    ck[[0, 32]] = 1.0
    return torch.tensor(C, dtype=dtype), torch.tensor(S, dtype=dtype), torch.tensor(ck, dtype=dtype)


def rfft_ref(x):
    """(Re, Im) of rfft(x, norm='ortho') over the last axis (64 -> 33 bins) as two real products."""
    C, S, _ = trig(x.dtype)
    return x @ C.T, -(x @ S.T)


def irfft_ref(yr, yi):
    """irfft(y, n=64, norm='ortho'): 1/8 sum_k c_k Re(Y_k e^{+i theta k n}); Im Y_0 and Im Y_32 meet zero sines."""
    C, S, ck = trig(yr.dtype)
    return (yr * ck) @ C - (yi * ck) @ S


def cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def spectrum_ref(V, T, Wi, Wt, Wf):
    """(image_conv, text_conv, fusion_conv) from the projected rows and the three (1, 33, 2) filters; also the two
    spectra as (Ar, Ai, Br, Bi)."""
    ar, ai = rfft_ref(V)
    br, bi = rfft_ref(T)
    w = [(W.reshape(33, 2)[:, 0], W.reshape(33, 2)[:, 1]) for W in (Wi, Wt, Wf)]
    ic = irfft_ref(*cmul(ar, ai, *w[0]))
    tc = irfft_ref(*cmul(br, bi, *w[1]))
    fc = irfft_ref(*cmul(*cmul(br, bi, ar, ai), *w[2]))
    return ic, tc, fc, (ar, ai, br, bi)


def spectrum_fft(V, T, Wi, Wt, Wf):
    """The same three rows through torch.fft, as smore.py:188-206."""
    a, b = torch.fft.rfft(V, dim=1, norm="ortho"), torch.fft.rfft(T, dim=1, norm="ortho")
    wi, wt, wf = (torch.view_as_complex(W.reshape(1, 33, 2).contiguous()) for W in (Wi, Wt, Wf))
    inv = lambda y: torch.fft.irfft(y, n=64, dim=1, norm="ortho")  # noqa: E731
    return inv(a * wi), inv(b * wt), inv(b * a * wf)


def layout64(re, im):
    """A spectrum (n x 33 real, n x 33 imaginary) in the kernels' 64-real layout: Re X_0..32, then Im X_1..31."""
    return torch.cat([re, im[:, 1:32]], dim=1)


def fusion_ref(av, at):
    """The union of two dense graphs: a shared entry takes the larger value, an entry of one graph keeps its value."""
    both = (av != 0) & (at != 0)
    return torch.where(both, torch.maximum(av, at), av + at)


# ----------------------------------------------------------------------------- the row blocks
def spectrum_rows_ref(d, dtype):
    """The spectrum kernel's rows with autograd at `dtype`.  d: V, T, E, dP (n x 192), dE0, Wi, Wt, Wf (33 x 2),
    Wgv, bgv, Wgt, bgt, Wgf, bgf.  Returns numpy: S (n x 128), conv, g, P (n x 192), dE, z (n x 192), dV, dT, dWi, dWt,
    dWf."""
    leaf = ("V", "T", "E", "Wi", "Wt", "Wf")
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=k in leaf) for k, v in d.items()}
    ic, tc, fc, (ar, ai, br, bi) = spectrum_ref(t["V"], t["T"], t["Wi"], t["Wt"], t["Wf"])
    ys = [x @ t["Wg" + s].T + t["bg" + s] for x, s in zip((ic, tc, fc), "vtf")]
    for y in ys:
        y.retain_grad()
    gs = [torch.sigmoid(y) for y in ys]
    P = torch.cat([t["E"] * g for g in gs], dim=1)
    (P * t["dP"]).sum().backward()
    o = {"S": torch.cat([layout64(ar, ai), layout64(br, bi)], dim=1), "conv": torch.cat([ic, tc, fc], dim=1),
         "g": torch.cat(gs, dim=1), "P": P, "dE": t["E"].grad + t["dE0"], "z": torch.cat([y.grad for y in ys], dim=1),
         "dV": t["V"].grad, "dT": t["T"].grad, "dWi": t["Wi"].grad, "dWt": t["Wt"].grad, "dWf": t["Wf"].grad}
    return {k: v.detach().numpy() for k, v in o.items()}


FUSE_W = ("Wv1", "bv1", "Wv2", "Wt1", "bt1", "Wt2", "Wi", "bi", "Wt", "bt", "Wf", "bf")


def fuse_rows(a, b, f, c, W, keep=None, p=0.0):
    """(side, all, parts) of the fuser on torch tensors of one dtype.  W: dict of FUSE_W; keep: n x 192 0/1 tensor
    ([image | text | fusion]) or None; parts: the pre-activations and saved rows by name."""
    y1v, y1t = f @ W["Wv1"].T + W["bv1"], f @ W["Wt1"].T + W["bt1"]
    hv, ht = torch.tanh(y1v), torch.tanh(y1t)
    y2v, y2t = hv @ W["Wv2"].T, ht @ W["Wt2"].T
    sv, st = torch.softmax(y2v, dim=-1), torch.softmax(y2t, dim=-1)
    yg = [c @ W["W" + s].T + W["b" + s] for s in "itf"]
    gs = [torch.sigmoid(y) for y in yg]
    if keep is not None and p > 0:
        # F.dropout's arithmetic: the kept entries times the rounded 1 / (1 - p)
        scale = 1.0 / (1.0 - p) if a.dtype == torch.float64 else float(np.float32(1.0) / np.float32(1.0 - p))
        gs = [g * keep[:, 64 * i:64 * i + 64].to(a.dtype) * scale for i, g in enumerate(gs)]
    side = (gs[0] * sv * a + gs[1] * st * b + gs[2] * f) / 3
    parts = {"y1v": y1v, "y2v": y2v, "y1t": y1t, "y2t": y2t, "yi": yg[0], "yt": yg[1], "yf": yg[2], "hv": hv, "ht": ht,
             "sv": sv, "st": st, "gi": gs[0], "gt": gs[1], "gf": gs[2]}
    return side, c + side, parts


def fuse_rows_ref(d, dtype, keep=None, p=0.0):
    """The fuser kernels' rows with autograd at `dtype`.  d: abf (n x 192), c, dall, dside, dcin and FUSE_W.  Returns
    numpy: side, all, saved (n x 448), dabf (n x 192), dc, z (n x 448: z1v, z2v, z1t, z2t, zi, zt, zf)."""
    t = {k: torch.tensor(v, dtype=dtype, requires_grad=k in ("abf", "c")) for k, v in d.items()}
    a, b, f = t["abf"][:, :64], t["abf"][:, 64:128], t["abf"][:, 128:]
    kp = None if keep is None else torch.as_tensor(np.asarray(keep))
    side, al, q = fuse_rows(a, b, f, t["c"], t, kp, p)
    ys = [q[k] for k in ("y1v", "y2v", "y1t", "y2t", "yi", "yt", "yf")]
    for y in ys:
        y.retain_grad()
    ((al * t["dall"]).sum() + (side * t["dside"]).sum() + (t["c"] * t["dcin"]).sum()).backward()
    o = {"side": side, "all": al, "saved": torch.cat([q[k] for k in ("hv", "ht", "sv", "st", "gi", "gt", "gf")], dim=1),
         "dabf": t["abf"].grad, "dc": t["c"].grad, "z": torch.cat([y.grad for y in ys], dim=1)}
    return {k: v.detach().numpy() for k, v in o.items()}


# ----------------------------------------------------------------------------- the step
def graphs_ref(U, I, rows, cols, feats, dtype=torch.float64, image_k=IMAGE_K, text_k=TEXT_K):
    """(adj, image_adj, text_adj, fusion_adj) dense at `dtype`."""
    av, at = knn_ref(feats[0], image_k, dtype), knn_ref(feats[1], text_k, dtype)
    return adj_ref(U, I, rows, cols, dtype), av, at, fusion_ref(av, at)


def smore_loss(P, graphs, U, users, pos, neg, n_layers, cl_loss, keep=None, p=0.0, n_ui_layers=N_UI_LAYERS,
               reg_weight=REG_WEIGHT, batch_size=None):
    """The loss of one SMORE step on a dict of torch parameters (names of PARAMS) and dense graphs; returns (loss,
    terms, tables) with tables = dict(a, b, f, c, side, all)."""
    adj, av, at, af = graphs
    R = adj[:U, U:]
    Ei = P["item_id_embedding_weight"]
    V = P["image_embedding_weight"] @ P["image_trs_weight"].T + P["image_trs_bias"]
    T = P["text_embedding_weight"] @ P["text_trs_weight"].T + P["text_trs_bias"]
    ic, tc, fc, _ = spectrum_ref(V, T, *[P[k] for k in FILTERS])
    views = []
    for x, gate, A in ((ic, "gate_v", av), (tc, "gate_t", at), (fc, "gate_f", af)):
        h = Ei * torch.sigmoid(x @ P[gate + "_0_weight"].T + P[gate + "_0_bias"])
        for _ in range(n_layers):
            h = A @ h
        views.append(torch.cat([R @ h, h]))
    a, b, f = views
    ego = torch.cat([P["user_embedding_weight"], Ei])
    layers = [ego]
    for _ in range(n_ui_layers):
        ego = adj @ ego
        layers.append(ego)
    c = torch.stack(layers, dim=1).mean(dim=1)
    W = {"Wv1": P["query_v_0_weight"], "bv1": P["query_v_0_bias"], "Wv2": P["query_v_2_weight"],
         "Wt1": P["query_t_0_weight"], "bt1": P["query_t_0_bias"], "Wt2": P["query_t_2_weight"],
         "Wi": P["gate_image_prefer_0_weight"], "bi": P["gate_image_prefer_0_bias"],
         "Wt": P["gate_text_prefer_0_weight"], "bt": P["gate_text_prefer_0_bias"],
         "Wf": P["gate_fusion_prefer_0_weight"], "bf": P["gate_fusion_prefer_0_bias"]}
    side, al, _ = fuse_rows(a, b, f, c, W, keep, p)
    u, pp, n = al[users], al[U + pos], al[U + neg]
    bpr = -Fn.logsigmoid((u * pp).sum(-1) - (u * n).sum(-1)).mean()
    reg = reg_weight * 0.5 * ((u ** 2).sum() + (pp ** 2).sum() + (n ** 2).sum()) / (batch_size or users.numel())
    nce_i = nce_ref(side[U + pos], c[U + pos])
    nce_u = nce_ref(side[users], c[users])
    loss = bpr + reg + cl_loss * (nce_i + nce_u)
    return loss, (bpr, reg, nce_i, nce_u), dict(a=a, b=b, f=f, c=c, side=side, all=al)


def _lt(a):
    return torch.as_tensor(np.asarray(a).astype(np.int64))


def smore_step_ref(P, U, I, rows, cols, users, pos, neg, n_layers, cl_loss, feats, keep=None, p=0.0,
                   batch_size=None, dtype=torch.float64, graphs=None):
    """One SMORE step in plain torch at `dtype`.  P: {name of PARAMS: array}; feats: the (image, text) features the
    frozen kNN graphs are built from; keep: N x 192 0/1 array (training with dropout p) or None.  Returns dict(loss,
    terms [bpr, reg, nce_items, nce_users], grads in PARAMS order, a, b, f, c, side, all, scores (evaluation: no
    dropout), adj, image_adj, text_adj, fusion_adj) as numpy."""
    P = {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=True) for k in PARAMS}
    graphs = graphs or graphs_ref(U, I, rows, cols, feats, dtype)
    kp = None if keep is None else torch.as_tensor(np.asarray(keep))
    loss, terms, tabs = smore_loss(P, graphs, U, _lt(users), _lt(pos), _lt(neg), n_layers, cl_loss, kp, p,
                                   batch_size=batch_size)
    grads = torch.autograd.grad(loss, [P[k] for k in PARAMS])
    with torch.no_grad():
        _, _, ev = smore_loss(P, graphs, U, _lt(users), _lt(pos), _lt(neg), n_layers, cl_loss)
    out = {"loss": loss.item(), "terms": np.array([t.item() for t in terms]), "grads": [x.numpy() for x in grads],
           "scores": (ev["all"][:U] @ ev["all"][U:].T).numpy()}
    out.update({k: v.detach().numpy() for k, v in tabs.items()})
    out.update({k: v.numpy() for k, v in zip(("adj", "image_adj", "text_adj", "fusion_adj"), graphs)})
    return out


def trajectory(P, U, I, rows, cols, users, pos, neg, n_layers, cl_loss, feats, keeps, p, dtype=torch.float64,
               lr=LR):
    """len(keeps) torch.optim.Adam steps of the restatement at `dtype`; returns ([{name: parameters after step j}],
    [{name: gradient of step j}]) as numpy."""
    P = {k: torch.tensor(np.asarray(P[k]), dtype=dtype, requires_grad=True) for k in PARAMS}
    graphs = graphs_ref(U, I, rows, cols, feats, dtype)
    opt = torch.optim.Adam([P[k] for k in PARAMS], lr=lr)
    traj, glog = [], []
    for keep in keeps:
        opt.zero_grad()
        loss, _, _ = smore_loss(P, graphs, U, _lt(users), _lt(pos), _lt(neg), n_layers, cl_loss,
                                torch.as_tensor(np.asarray(keep)), p)
        loss.backward()
        glog.append({k: P[k].grad.detach().numpy().copy() for k in PARAMS})
        opt.step()
        traj.append({k: P[k].detach().numpy().copy() for k in PARAMS})
    return traj, glog

