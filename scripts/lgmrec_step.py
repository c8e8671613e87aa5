"""Time LGMRec on the synthetic baby shape (gmr/synthetic.py) with LGMRec.yaml's values, B = 2,048: the step, the
forward alone, the evaluation pass, each gmr_lgm_* launch of the global hypergraph embedding (GHE) block with the bytes
it has to move, the GHE block forward plus backward, and the same block in eager torch ops with autograd on the same
device (lgmrec.py:115-151 as the reference writes it: sparse.mm, F.gumbel_softmax, nn.Dropout, HGNNLayer, F.normalize).
Device work is timed with HIP events after a warm-up (medians over --reps calls, two alternating rounds); the
evaluation by a host clock around a device synchronise.  Prints one JSON line last.
python scripts/lgmrec_step.py [--shape baby] [--batch 2048] [--reps 100] [--profile N]
--profile N: N steps and one evaluation forward and nothing else, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-multimodal-recommendation_amd"))
ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="baby")
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--profile", type=int, default=0)
a = ap.parse_args()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gmr import _lib  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.kernels import ptr, stream  # noqa: E402
from gmr.lgmrec import LGMRec  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

PEAK_TBS = 8.0  # MI355X HBM3E peak, TB/s
D = 64

if not torch.cuda.is_available():
    raise SystemExit("lgmrec_step.py measures on the GPU; none found")
over = {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False, "epochs": 1}
cfg = Config("LGMRec", "baby", dict(over))
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
t0 = time.time()
m = LGMRec(cfg, tl)
torch.cuda.synchronize()
build_s = time.time() - t0
trainer = Trainer(cfg, m)
d = tl.epoch()
_, _, users, pos, neg, plan_bpr, plan_cl = next(iter(tl.batches(d)))
B, U, I, N, H = users.numel(), m.n_users, m.n_items, m.N, m.hyper_num
nnz = int(m.adj.nnz)


def step():
    m.rec_step(users, pos, neg, plan_bpr, plan_cl)


if a.profile:
    for _ in range(a.profile):
        step()
    m.forward_embeddings()
    torch.cuda.synchronize()
    print(json.dumps({"profiled_steps": a.profile, "I": I, "N": N, "B": B}), flush=True)
    raise SystemExit(0)


def events(fn, reps=a.reps, warmup=a.warmup):
    """Median / min ms of fn() by HIP events, one pair per call, after a warm-up."""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ts = [s.elapsed_time(e) for s, e in ev]
    return statistics.median(ts), min(ts)


def host(fn, reps=3, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.time()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.time() - t))
    return statistics.median(ts), min(ts)


res = {"shape": a.shape, "B": B, "U": U, "I": I, "nnz": nnz, "hyper_num": H, "n_hyper_layer": m.n_hyper_layer,
       "keep_rate": m.keep_rate, "n_ui_layers": m.n_ui_layers, "n_mm_layers": m.n_mm_layers,
       "feature_widths": [int(m.feat[k].shape[1]) for k in ("v", "t")], "construction_s": round(build_s, 3)}
step()
res["loss_first_step"] = round(float(m.loss_terms()[0]), 6)
cge = m.cge if m.cge is not None else m.slab.view("E")
pv, pt = m.proj["v"], m.proj["t"]
hi = m.h[U:]
dv, dt = m.dproj["v"], m.dproj["t"]


# ---- the launches of the GHE block, on the buffers the step left
def hyper_fwd():
    _lib.call("gmr_lgm_hyper_fwd", U, I, H, ptr(pv[:, D:]), pv.stride(0), ptr(pt[:, D:]), pt.stride(0),
              ptr(m.adj.rowptr), ptr(m.adj.col), None, None, H, None, None, H, m.tau, m.keep_rate,
              2 if m.keep_rate < 1 else 0, m.seed, 0, ptr(m.S), ptr(m.h), 2 * H, 0, stream())


def lat_fwd():
    m._lat(I, hi, cge[U:], cge[U:], m.lats[0])


def combine_fwd():
    _lib.call("gmr_lgm_combine_fwd", N, ptr(cge), D, ptr(m.mge), 2 * D, ptr(m.h), 2 * H, H, ptr(m.lats[-1]), m.alpha,
              ptr(m.all), D, ptr(m.CLN), ptr(m.nrmCL), ptr(m.nrm3), 0, stream())


def combine_bwd():
    _lib.call("gmr_lgm_combine_bwd", N, ptr(m.dall), D, ptr(m.mge), 2 * D, ptr(m.CLN), ptr(m.nrmCL), ptr(m.nrm3),
              m.alpha, ptr(m.dmge), 2 * D, ptr(m.dK), 0, stream())


def lat_bwd():
    m._lat(N, m.h, m.dK[:, :D], m.dK[:, D:], m.dlat[0])


def dh_items():
    m._dh(cge[U:], cge[U:], m.dlat[0], m.acc[U:])


def dh_rows():
    m._dh(m.dK[:, :D], m.dK[:, D:], m.lats[-1], m.dL, acc=m.acc, sbwd=True)


def apply_de():
    m._apply(hi, m.dlat[0], m.dall[U:], 1)


def logit_bwd():
    _lib.call("gmr_lgm_logit_bwd", U, I, H, ptr(m.dL), 2 * H, ptr(m.adj_t.rowptr), ptr(m.adj_t.col), ptr(dv[:, D:]),
              dv.stride(0), ptr(dt[:, D:]), dt.stride(0), 0, stream())


F4 = 4
tiles = lambda n: -(-n // int(_lib.load().gmr_lgm_tile_rows()))  # noqa: E731
ws = lambda n: 2 * tiles(n) * 2 * H * D  # noqa: E731  (the partials written, then read)
calls = {
    "gmr_lgm_hyper_fwd": (hyper_fwd, F4 * (I * 2 * H + nnz * 2 * H + nnz + 2 * N * 2 * H)),
    "gmr_lgm_lat (I rows)": (lat_fwd, F4 * (I * (2 * H + D) + ws(I))),
    "gmr_lgm_combine_fwd": (combine_fwd, F4 * N * (D + 2 * D + 2 * H + D + 2 * D + 5)),
    "gmr_lgm_combine_bwd": (combine_bwd, F4 * N * (D + 2 * D + 2 * D + 5 + 2 * D + 2 * 2 * D)),
    "gmr_lgm_lat (N rows)": (lat_bwd, F4 * (N * (2 * H + 2 * D) + ws(N))),
    "gmr_lgm_dh (I rows)": (dh_items, F4 * I * (D + 2 * H)),
    "gmr_lgm_dh (N rows, to d L)": (dh_rows, F4 * N * (2 * D + 4 * 2 * H)),
    "gmr_lgm_apply (d E_i)": (apply_de, F4 * I * (2 * H + 2 * D)),
    "gmr_lgm_logit_bwd": (logit_bwd, F4 * (N * 2 * H + nnz * 2 * H + nnz + I * 2 * H)),
}
if m.n_hyper_layer != 1:
    raise SystemExit("lgmrec_step.py times the one-layer block (LGMRec.yaml)")


def ghe_fwd():
    hyper_fwd(), lat_fwd(), combine_fwd()


def ghe_bwd():
    combine_bwd(), lat_bwd(), dh_items(), dh_rows(), apply_de(), logit_bwd()


# ---- the same block in eager torch ops with autograd (fresh Gumbel draws and masks per call, as the reference)
adj_sp = torch.sparse_coo_tensor(
    torch.stack([torch.repeat_interleave(torch.arange(U, device=cge.device),
                                         (m.adj.rowptr[1:] - m.adj.rowptr[:-1]).long()), m.adj.col.long()]),
    torch.ones(nnz, device=cge.device), (U, I)).coalesce()
leaf = {"Lv": pv[:, D:D + H], "Lt": pt[:, D:D + H], "cge": cge, "mge": m.mge}
leaf = {k: v.detach().clone().requires_grad_() for k, v in leaf.items()}
up_all, up_x = torch.randn(N, D, device=cge.device), torch.randn(N, 2 * D, device=cge.device) * 1e-4
drop = torch.nn.Dropout(p=1 - m.keep_rate)


def eager_ghe():
    c, xs = leaf["cge"], []
    for L in (leaf["Lv"], leaf["Lt"]):
        ih = drop(F.gumbel_softmax(L, m.tau, dim=1, hard=False))
        uh = drop(F.gumbel_softmax(torch.sparse.mm(adj_sp, L), m.tau, dim=1, hard=False))
        lat = ih.T @ c[U:]
        xs.append(torch.cat([uh @ lat, ih @ lat]))
    al = c + F.normalize(leaf["mge"][:, :D]) + F.normalize(leaf["mge"][:, D:]) + m.alpha * F.normalize(xs[0] + xs[1])
    return al, torch.cat([F.normalize(xs[0]), F.normalize(xs[1])], dim=1)


def eager_fwd_bwd():
    for p in leaf.values():
        p.grad = None
    al, x = eager_ghe()
    ((al * up_all).sum() + (x * up_x).sum()).backward()


res["kernels"] = {}
for rnd in range(2):  # alternating, twice: the spread
    res[f"step_ms_{rnd}"] = events(step)
    res[f"forward_ms_{rnd}"] = events(lambda: m._forward(train=True, step=0))
    res[f"ghe_fwd_ms_{rnd}"] = events(ghe_fwd)
    res[f"ghe_fwd_bwd_ms_{rnd}"] = events(lambda: (ghe_fwd(), ghe_bwd()))
    res[f"eager_ghe_fwd_ms_{rnd}"] = events(lambda: eager_ghe())
    res[f"eager_ghe_fwd_bwd_ms_{rnd}"] = events(eager_fwd_bwd)
# each launch: events around one call (an upper bound of the kernel's time: the launch gap is inside)
for name, (fn, nbytes) in calls.items():
    med, mn = events(fn)
    res["kernels"][name] = {"us_median": round(1e3 * med, 2), "us_min": round(1e3 * mn, 2), "bytes": nbytes,
                            "share_of_hbm_peak": round(nbytes / (med * 1e-3) / (PEAK_TBS * 1e12), 4)}
    print(name, res["kernels"][name], flush=True)
res["eager_over_kernels"] = round(res["eager_ghe_fwd_bwd_ms_1"][0] / res["ghe_fwd_bwd_ms_1"][0], 2)
res["evaluate_ms"] = host(lambda: trainer.evaluate(vl))
res["eval_forward_ms"] = events(lambda: m.forward_embeddings(), reps=20, warmup=3)
for key, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{key:48s} median {v[0]:10.4f} ms   min {v[1]:10.4f} ms", flush=True)
        res[key] = [round(v[0], 5), round(v[1], 5)]
print(json.dumps(res), flush=True)
