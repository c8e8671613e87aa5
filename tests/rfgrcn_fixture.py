"""Shared builders of the RFGRCN tests: the golden record of tests/golden/make_golden_rfgrcn.py (case A of
grcn_tiny.npz, generated rows and conditions 192 wide), the plain torch restatement of RFGRCN's RF inputs (X1 = cond =
the concatenated table, the per-segment centred prior) on top of tests/grcn_fixture.py (the GRCN forward),
tests/rfmgcn_fixture.rf_step_ref (the generator's losses with the prior term) and tests/rf_fixture.py (the velocity
net and the sampler, whose formulas take their widths from the tensors), the project's three bars, and the model
builders of the GPU tests."""
import numpy as np
import torch

import grcn_fixture as F
import rf_fixture as R
import rfmgcn_fixture as RM

FILES = ("rfgrcn_tiny", "rfgrcn_tiny_param", "rfgrcn_tiny_grad", "rfgrcn_tiny_step")
RF_TINY = dict(R.RF_TINY)
DEV = F.DEV
TAG = "A_"
CASE = "A"
L = 2
WIDTH = 192
N_PARAMS = 166848  # D = C = 192, two layers
N_PARAMS_128 = 142208  # D = C = 128 (image features alone)
rf_step_ref = RM.rf_step_ref


def load_golden(golden):
    """The fixture of make_golden_rfgrcn.py: four files (size limit), one dict.  The conditions are the target table
    (asserted by the maker), so A_cond is A_X1."""
    g = {}
    for name in FILES:
        g.update(golden(name))
    g[TAG + "cond"] = g[TAG + "X1"]
    return g


def case_config(**over):
    """The golden case's config keys: GRCN's case A and the RF settings of the record."""
    c = dict(F.CASES[CASE])
    c.pop("mods")
    return dict(c, **RF_TINY, **over)


def prior_ref(table, U):
    """rfgrcn.py:171-190: every 64-wide block minus its segment's column mean, which is the whole row minus its
    segment's column means."""
    return torch.cat([table[:U] - table[:U].mean(dim=0, keepdim=True), table[U:] - table[U:].mean(dim=0, keepdim=True)])


def result_ref(P, g, n_layers, dtype=torch.float64, mods="vt"):
    """GRCN's concatenated table from numpy parameters by grcn_fixture.grcn_forward."""
    names = [k for k in F.PARAMS if k in P]
    T = F.tensors(P, names, dtype, grad=False)
    feats = [torch.tensor(g["v_feat"], dtype=dtype), torch.tensor(g["t_feat"], dtype=dtype) if "t" in mods else None]
    lt = lambda a: torch.as_tensor(np.asarray(a, np.int64))  # noqa: E731
    with torch.no_grad():
        return F.grcn_forward(T, feats, lt(g["train_rows"]), lt(g["train_cols"]), n_layers)[0]


# ---------------------------------------------------------------------------------------------- the three bars
def sampler_bar(ref32, ref64):
    """4x the error of the fp32 CPU run of the same torch formula against its fp64 run, absolute, floored at 1e-6 of
    the largest value."""
    ref64 = np.asarray(ref64, np.float64)
    return max(4.0 * float(np.abs(np.asarray(ref32, np.float64) - ref64).max()), 1e-6 * float(np.abs(ref64).max()))


def grad_bar(g32, g64):
    """The same 4x rule relative to the parameter's largest gradient, floored at 1e-6."""
    return max(4.0 * R.rel_to_max(g32, g64), 1e-6)


TABLE = dict(rtol=1e-5, atol=2e-6)


def generate_ref(VP, cond, z0, steps, n_layers, dtype):
    P = {n: torch.tensor(np.asarray(v), dtype=dtype) for n, v in VP.items()}
    with torch.no_grad():
        return R.generate(P, torch.tensor(np.asarray(cond), dtype=dtype), torch.tensor(np.asarray(z0), dtype=dtype),
                          steps, n_layers).numpy()


def random_params(rng, C, n_layers, D, scale=1.0):
    """Velocity parameters of nn.Linear's scale for gmr.rf.param_specs(C, n_layers, D): {name: fp32 array}."""
    from gmr.rf import param_specs
    P = {}
    for name, sh in param_specs(C, n_layers, D):
        if len(sh) == 2:
            P[name] = (rng.uniform(-1, 1, sh) * scale / np.sqrt(sh[1])).astype(np.float32)
        elif name.endswith(".weight"):  # LayerNorm
            P[name] = (1.0 + 0.1 * rng.standard_normal(sh)).astype(np.float32)
        else:
            P[name] = (0.1 * rng.standard_normal(sh)).astype(np.float32)
    return P


# ---------------------------------------------------------------------------------------------- GPU builders
def rfgrcn_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "embedding_size": 64, "latent_embedding": 64, "n_layers": 3,
         "reg_weight": 0.001, "learning_rate": F.LR}
    d.update(RF_TINY)
    d.update(over)
    return Config("RFGRCN", "baby", d)


def build_rfgrcn(f, case=CASE, as_drawn=False, **over):
    """RFGRCN on the data of grcn_tiny.npz, constructed under torch.manual_seed(3) as the fixture's reference model
    was, then given the case's GRCN parameters.  Returns (model, cfg, dataset, loader)."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.utils import get_model
    c = dict(F.CASES[case])
    mods = c.pop("mods")
    cfg = rfgrcn_config(**dict(c, **over))
    U, I = int(f["U"]), int(f["I"])
    rows, cols = f["train_rows"], f["train_cols"]
    ds = RecDataset.from_arrays(cfg, rows, cols, np.zeros(len(rows)), U, I, f["v_feat"],
                                f["t_feat"] if "t" in mods else None)
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    m = get_model("RFGRCN")(cfg, tl)
    if not as_drawn:
        F.set_params(m, F.case_params(f, case))
    return m, cfg, ds, tl


def draws(g, tag=TAG, dev=DEV):
    return R.draws(g, tag, dev)
