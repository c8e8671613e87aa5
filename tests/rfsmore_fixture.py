"""Shared builders of the RFSMORE tests: the plain torch restatement of RFSMORE's RF inputs (X1 = all, cond =
[a | b | gf f] with the fusion preference gate gf of the step, dropout mask and scale included, and the two-segment
centred prior of (a + b + gf f) / 3) on top of tests/smore_fixture.py (the SMORE step), tests/rfbm3_fixture.py (the
generator's losses with the prior term) and tests/rf_fixture.py at C = 192; tests/test_rfsmore_cpu.py pins it to the
reference's golden values (tests/golden/make_golden_rfsmore.py), the GPU tests use its fp64 run where the reference
recorded nothing."""
import numpy as np
import torch

import mgcn_fixture as M
import rf_fixture as R
import rfmgcn_fixture as RM
import smore_fixture as F

FILES = ("rfsmore_tiny", "rfsmore_tiny_param", "rfsmore_tiny_grad", "rfsmore_tiny_step")
RF_TINY = dict(R.RF_TINY)
DEV = F.DEV
TAG = "B_"
N_PARAMS = 125760 + 128 * 64  # C = 192, two layers
rf_step_ref = RM.rf_step_ref


def load_golden(golden):
    """The fixture of make_golden_rfsmore.py: four files (size limit), one dict."""
    g = {}
    for name in FILES:
        g.update(golden(name))
    return g


def smore_golden(golden):
    return dict(golden("smore_tiny"), **golden("smore_tiny_B"))


def inputs_ref(a, b, f, g, U):
    """(cond, prior) of rfsmore.py:165-195 on torch tensors of one dtype: cond = [a | b | g f]; Z = (0 + a + b + g f)
    / 3, the user rows minus the mean over the users, the item rows minus the mean over the items."""
    gf = g * f
    Z = (0 + a + b + gf) / 3
    prior = torch.cat([Z[:U] - Z[:U].mean(dim=0, keepdim=True), Z[U:] - Z[U:].mean(dim=0, keepdim=True)])
    return torch.cat([a, b, gf], dim=1), prior


def gate_ref(P, c, keep=None, p=0.0):
    """The fusion preference gate of a step (smore.py: dropout(gate_fusion_prefer(content))) on the torch table c.  P:
    {name of smore_fixture.PARAMS: array}; keep: N x 192 0/1 array (its third block is the gate's) or None."""
    W = torch.tensor(np.asarray(P["gate_fusion_prefer_0_weight"]), dtype=c.dtype)
    bias = torch.tensor(np.asarray(P["gate_fusion_prefer_0_bias"]), dtype=c.dtype)
    g = torch.sigmoid(c @ W.T + bias)
    if keep is not None and p > 0:
        scale = 1.0 / (1.0 - p) if c.dtype == torch.float64 else float(np.float32(1.0) / np.float32(1.0 - p))
        g = g * torch.as_tensor(np.asarray(keep)[:, 128:]).to(c.dtype) * scale
    return g


def rf_inputs_ref(r, P, U, keep=None, p=0.0, dtype=torch.float64):
    """(X1, cond, prior) of the RF step from smore_fixture.smore_step_ref's result r (its a, b, f, c, all)."""
    a, b, f, c = (torch.tensor(r[k], dtype=dtype) for k in ("a", "b", "f", "c"))
    cond, prior = inputs_ref(a, b, f, gate_ref(P, c, keep, p), U)
    return torch.tensor(r["all"], dtype=dtype), cond, prior


# ---------------------------------------------------------------------------------------------- GPU builders
def rfsmore_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "reg_weight": F.REG_WEIGHT, "image_knn_k": F.IMAGE_K,
         "text_knn_k": F.TEXT_K, "n_ui_layers": F.N_UI_LAYERS, "n_layers": 1, "cl_loss": 0.01, "dropout_rate": 0.0,
         "learning_rate": F.LR}
    d.update(RF_TINY)
    d.update(over)
    return Config("RFSMORE", "baby", d)


def build_rfsmore(g, case="B", **over):
    """RFSMORE on the data of smore_tiny.npz, constructed under torch.manual_seed(3) as the fixture's reference model
    was, then given the case's SMORE parameters.  Returns (model, cfg, dataset, loader)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rfsmore import RFSMORE
    cfg = rfsmore_config(**dict(F.CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = RFSMORE(cfg, tl)
    if case != "A":
        F.set_params(m, F.case_params(g, case))
    return m, cfg, ds, tl


MID_K = (10, 10)  # mgcn_fixture's mid shape is tested at 10 neighbours: fp32 and fp64 select the same ones


def build_rfsmore_mid(**over):
    """RFSMORE on mgcn_fixture.mid_data with U = 300, I = 1,100 (3 + 9 blocks of 128 rows with both last blocks short;
    N = 1,400 is 43 sampler tiles and 24 rows), widths 37 / 50, B = 700 with repeated users; case B's settings
    (n_layers 2, dropout 0.1) and its scaling of the drawn SMORE parameters.  Returns (model, data)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rfsmore import RFSMORE
    d = M.mid_data()
    batch = d["users"].size
    cfg = rfsmore_config(**dict(F.CASES["B"], train_batch_size=batch, image_knn_k=MID_K[0], text_knn_k=MID_K[1],
                                **over))
    ds = RecDataset.from_arrays(cfg, d["rows"], d["cols"], np.zeros(d["rows"].size), d["U"], d["I"], d["v_feat"],
                                d["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    m = RFSMORE(cfg, tl)
    g = {"init_" + k: p.detach().cpu().numpy() for k, p in zip(F.PARAMS, m._params())}
    F.set_params(m, F.case_params(g, "B"))
    return m, d


def draws(g, tag=TAG, dev=DEV):
    return R.draws(g, tag, dev)
