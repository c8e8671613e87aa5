"""Shared builders of the RFLGMRec tests: the plain torch restatement of RFLGMRec's RF inputs (X1 = cge, cond =
[mge_v | mge_t], the two-segment centred prior of the *sum* mge_v + mge_t) and of its evaluation forward (the generated
rows mixed into cge before the hypergraph block) on top of tests/lgmrec_fixture.py (the LGMRec forward),
tests/rfmgcn_fixture.rf_step_ref (the generator's losses with the prior term) and tests/rf_fixture.py (the sampler);
tests/test_rflgmrec_cpu.py pins it to the reference's golden values (tests/golden/make_golden_rflgmrec.py), the GPU
tests use its fp64 run where the reference recorded nothing."""
import numpy as np
import torch

import lgmrec_fixture as F
import mgcn_fixture as M
import rf_fixture as R
import rfmgcn_fixture as RM

FILES = ("rflgmrec_tiny", "rflgmrec_tiny_param", "rflgmrec_tiny_grad", "rflgmrec_tiny_step")
RF_TINY = dict(R.RF_TINY)
DEV = F.DEV
TAG = "B_"
N_PARAMS = 125760  # C = 128, two layers
rf_step_ref = RM.rf_step_ref


def load_golden(golden):
    """The fixture of make_golden_rflgmrec.py: four files (size limit), one dict."""
    g = {}
    for name in FILES:
        g.update(golden(name))
    return g


def lgmrec_golden(golden):
    return dict(golden("lgmrec_tiny"), **golden("lgmrec_tiny_B"))


def prior_ref(a, b, U):
    """rflgmrec.py:125-143 on torch tensors of one dtype: Z = 0 + a + b (a sum, no mean of the views), the user rows
    minus the mean over the users, the item rows minus the mean over the items."""
    Z = 0 + a + b
    return torch.cat([Z[:U] - Z[:U].mean(dim=0, keepdim=True), Z[U:] - Z[U:].mean(dim=0, keepdim=True)])


def rf_inputs_ref(fw, U):
    """(X1, cond, prior) of the RF step from lgmrec_fixture.lgmrec_forward's result: cge, [mge_v | mge_t], prior_ref."""
    a, b = fw["mge"]
    return fw["cge"], torch.cat([a, b], dim=1), prior_ref(a, b, U)


def forward_ref(P, feats, U, I, rows, cols, c, g, keep=None, dtype=torch.float64):
    """lgmrec_fixture.lgmrec_forward from numpy inputs at `dtype` (no gradients)."""
    Pt, X, gt, kt = F._tens(P, feats, g, keep, dtype, grad=False)
    with torch.no_grad():
        return F.lgmrec_forward(Pt, X, F.graphs_ref(U, I, rows, cols, dtype), U, c, gt, kt)


def hyper_on(fw, cge, U, c):
    """LGMRec's forward from the hypergraph block on (lgmrec.py:139-145) with `cge` in place of fw's: the hyperedge
    layers on cge's item rows through fw's assignments h, and the combine.  Returns all."""
    xs = []
    for h in fw["h"]:
        hu, hi = h[:U], h[U:]
        i = cge[U:]
        for _ in range(c["n_hyper_layer"]):
            lat = hi.T @ i
            i = hi @ lat
        xs.append(torch.cat([hu @ lat, i]))
    ghe = xs[0] + xs[1]
    return cge + F.normalize(fw["mge"][0]) + F.normalize(fw["mge"][1]) + c.get("alpha", F.ALPHA) * F.normalize(ghe)


def eval_ref(fw, VP, z0, U, c, steps, n_layers, ratio, rule="cge"):
    """The warmed-up evaluation of rflgmrec.py:178-191 from an evaluation forward fw (no dropout): gen =
    generate([mge_v | mge_t]) from z0 on the velocity parameters VP {name: array}; rule "cge" (the model): cge' = cge +
    ratio gen, all = hyper_on(cge'); rule "all" (the other RF models' rule, which RFLGMRec is not): all = fw's all +
    ratio gen.  Returns dict(gen, cgemix, all)."""
    dt = fw["cge"].dtype
    Pv = {n: torch.tensor(np.asarray(v), dtype=dt) for n, v in VP.items()}
    with torch.no_grad():
        gen = R.generate(Pv, torch.cat(fw["mge"], dim=1), torch.tensor(np.asarray(z0), dtype=dt), steps, n_layers)
        mixc = fw["cge"] + ratio * gen
        al = hyper_on(fw, mixc, U, c) if rule == "cge" else fw["all"] + ratio * gen
    return {"gen": gen, "cgemix": mixc, "all": al}


# ---------------------------------------------------------------------------------------------- GPU builders
def rflgmrec_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "cf_model": "lightgcn", "n_ui_layers": F.N_UI_LAYERS,
         "n_mm_layers": F.N_MM_LAYERS, "n_hyper_layer": 1, "hyper_num": 4, "keep_rate": 1.0, "alpha": F.ALPHA,
         "cl_weight": F.CL_WEIGHT, "reg_weight": F.REG_WEIGHT, "learning_rate": F.LR}
    d.update(RF_TINY)
    d.update(over)
    return Config("RFLGMRec", "baby", d)


def build_rflgmrec(g, case="B", **over):
    """RFLGMRec on the data of lgmrec_tiny.npz, constructed under torch.manual_seed(3) as the fixture's reference
    model was, then given the case's LGMRec parameters.  Returns (model, cfg, dataset, loader)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rflgmrec import RFLGMRec
    cfg = rflgmrec_config(**dict(F.CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows, cols = g["train_rows"], g["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = RFLGMRec(cfg, tl)
    if case != "A":
        F.set_params(m, F.case_params(g, case))
    return m, cfg, ds, tl


def build_rflgmrec_mid(**over):
    """RFLGMRec on mgcn_fixture.mid_data with U = 300, I = 1,100 (3 + 9 blocks of 128 rows with both last blocks short;
    N = 1,400 is 43 sampler tiles and 24 rows), widths 37 / 50, B = 700 with repeated users; case B's settings
    (n_hyper_layer 2, hyper_num 5, keep_rate 0.5) and its scaling of the drawn LGMRec parameters.  Returns (model,
    data)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.rflgmrec import RFLGMRec
    d = M.mid_data()
    batch = d["users"].size
    cfg = rflgmrec_config(**dict(F.CASES["B"], train_batch_size=batch, **over))
    ds = RecDataset.from_arrays(cfg, d["rows"], d["cols"], np.zeros(d["rows"].size), d["U"], d["I"], d["v_feat"],
                                d["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=batch)
    torch.manual_seed(3)
    m = RFLGMRec(cfg, tl)
    g = {"B_init_" + k: p.detach().cpu().numpy() for k, p in zip(F.PARAMS, m._params())}
    F.set_params(m, F.case_params(g, "B"))
    return m, d


def draws(g, tag=TAG, dev=DEV):
    return R.draws(g, tag, dev)
