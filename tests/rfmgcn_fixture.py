"""Shared builders of the RFMGCN tests: the fp64 restatement of RFMGCN's RF inputs (X1 = all, cond = [a | b], the
two-segment centred prior) on top of tests/mgcn_fixture.py (the MGCN step) and tests/rfbm3_fixture.py (the generator's
losses with the prior term); tests/test_rfmgcn_cpu.py pins it to the reference's golden values
(tests/golden/make_golden_rfmgcn.py), the GPU tests use its fp64 run where the reference recorded nothing."""
import numpy as np
import torch

import mgcn_fixture as M
import rf_fixture as R
import rfbm3_fixture as RB

FILES = ("rfmgcn_tiny", "rfmgcn_tiny_param", "rfmgcn_tiny_grad", "rfmgcn_tiny_step")
RF_TINY = dict(R.RF_TINY)
DEV = M.DEV


def load_golden(golden):
    """The fixture of make_golden_rfmgcn.py: four files (size limit), one dict."""
    g = {}
    for name in FILES:
        g.update(golden(name))
    return g


def prior_ref(a, b, U):
    """rfmgcn.py:156-172 on torch tensors of one dtype: Z = (0 + a + b) / 2, the user rows minus the mean over the
    users, the item rows minus the mean over the items."""
    Z = (0 + a + b) / 2
    return torch.cat([Z[:U] - Z[:U].mean(dim=0, keepdim=True), Z[U:] - Z[U:].mean(dim=0, keepdim=True)])


def rf_inputs_ref(r, U, dtype=torch.float64):
    """(X1, cond, prior) of the RF step from mgcn_fixture.mgcn_step_ref's result: all, [a | b], prior_ref."""
    a, b = (torch.tensor(r[k], dtype=dtype) for k in ("a", "b"))
    return torch.tensor(r["all"], dtype=dtype), torch.cat([a, b], dim=1), prior_ref(a, b, U)


def rf_step_ref(VP, X1, cond, prior, dr, users, pos, U, n_layers, dtype=torch.float64):
    """rfbm3_fixture.train_losses on numpy velocity parameters VP {name: array} and draws dr; returns (result dict,
    {name: gradient})."""
    P = {n: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for n, v in VP.items()}
    c = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    li = lambda x: torch.as_tensor(np.asarray(x).astype(np.int64))  # noqa: E731
    out = RB.train_losses(P, c(X1), c(dr["X0"]), c(dr["t"]), c(cond), c(prior), li(users), li(pos),
                          li(dr["neg_items"]), li(dr["neg_users"]), U, n_layers)
    return out, R.grads_of(P, out["total"])


# ---------------------------------------------------------------------------------------------- GPU builders
def rfmgcn_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": M.REG_WEIGHT, "knn_k": M.KNN_K,
         "n_ui_layers": M.N_UI_LAYERS, "n_layers": 1, "cl_loss": 0.001}
    d.update(RF_TINY)
    d.update(over)
    return Config("RFMGCN", "baby", d)


def build_rfmgcn(g, case="A", **over):
    """RFMGCN on the data of mgcn_tiny.npz, constructed under torch.manual_seed(3) as the fixture's reference model
    was, then given the case's MGCN parameters.  Returns (model, cfg, dataset, loader)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rfmgcn import RFMGCN
    cfg = rfmgcn_config(**dict(M.CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = RFMGCN(cfg, tl)
    if case != "A":
        M.set_params(m, M.case_params(g, case))
    return m, cfg, ds, tl


def build_rfmgcn_mid(case="B", **over):
    """RFMGCN on mgcn_fixture.mid_data (U = 300, I = 1,100, widths 37 / 50, B = 700 with repeated users), with case
    B's scaling of the drawn MGCN parameters, as mgcn_fixture.build_mgcn_mid.  Returns (model, data)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rfmgcn import RFMGCN
    d = M.mid_data()
    batch = d["users"].size
    cfg = rfmgcn_config(**dict(M.CASES[case], train_batch_size=batch, knn_k=10, **over))
    ds = RecDataset.from_arrays(cfg, d["rows"], d["cols"], np.zeros(d["rows"].size), d["U"], d["I"], d["v_feat"],
                                d["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    m = RFMGCN(cfg, tl)
    g = {"init_" + k: p.detach().cpu().numpy() for k, p in zip(M.PARAMS, m._params())}
    M.set_params(m, M.case_params(g, "B"))
    return m, d


def draws(g, tag="A_", dev=DEV):
    return R.draws(g, tag, dev)
