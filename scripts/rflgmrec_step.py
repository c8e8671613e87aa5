"""Time RFLGMRec on the synthetic baby shape (gmr/synthetic.py), B = 2,048, 1,024 InfoNCE negatives, rf_dropout 0.1,
rf_sampling_steps from the YAML: ms per rec_step of LGMRec and of RFLGMRec (the same model, use_rf toggled), the RF
step alone, the prior launches (gmr_rf_view_sum_prior) alone with their share of the HBM peak from the bytes they move,
and a warmed-up evaluation pass (forward_embeddings) in its two forms: the mix as the sampler's epilogue
(gmr_rf_sample_mix, what the model runs) against the same pass with gmr_rf_sample into a table of its own followed by
copy64 and gmr_axpy_dev_f32 (the composition the other RF models run: two more launches and three more passes over
N x 256 bytes, which the hyperedge reduction over the items waits on).  Device work is timed with HIP events after a
warm-up; the two evaluation forms are taken five times each in alternation in this one process, and the medians of
the five runs are reported next to the spread (max - min) of each.  Prints one JSON line last; run it under a time
limit (timeout -k 10 600 python scripts/rflgmrec_step.py).
python scripts/rflgmrec_step.py [--shape baby] [--batch 2048] [--reps 100] [--runs 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-multimodal-recommendation_amd"))
ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="baby")
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--runs", type=int, default=5)
a = ap.parse_args()
import torch  # noqa: E402

from gmr import _lib  # noqa: E402
from gmr.abstract_recommender import copy64  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import TrainDataLoader  # noqa: E402
from gmr.kernels import ptr, stream  # noqa: E402
from gmr.rflgmrec import RFLGMRec  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

PEAK_TBS = 8.0  # MI355X HBM3E peak, TB/s

if not torch.cuda.is_available():
    raise SystemExit("rflgmrec_step.py measures on the GPU; none found")
cfg = Config("RFLGMRec", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                                  "epochs": 1, "rf_dropout": 0.1, "rf_infonce_negatives": 1024})
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
m = RFLGMRec(cfg, tl)
m.pre_epoch_processing()
d = tl.epoch()
_, _, users, pos, neg, pb, pc = next(iter(tl.batches(d)))
B, N = users.numel(), m.N
g = m.rf_generator


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


# the prior kernel reads both views twice (sum pass, subtract pass) and writes N x 64
prior_bytes = N * 64 * 4 * (2 * 2 + 1)
res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "N": N, "rf_n_layers": g.L, "condition_dim": g.C,
       "n_neg": g.n_neg, "rf_dropout": g.dropout, "sampling_steps": g.sampling_steps, "prior_bytes": prior_bytes}
loss = float(m.rec_step(users, pos, neg, pb, pc))
res["loss_first_step"] = round(loss, 6)
res["rf_losses_first_step"] = [round(float(x), 6) for x in m.rf_loss_terms().cpu()]
# the RF step's tables as a forward leaves them (the backward reuses mge's buffer)
cge = m._forward(train=True, step=m._step)
X1, cond, prior = m.rf_step_inputs(cge)
X1, cond, prior = X1.clone(), cond.clone(), prior.clone()


def step(use_rf):
    m.use_rf = use_rf
    m.rec_step(users, pos, neg, pb, pc)
    m.use_rf = True


for rnd in range(2):
    res[f"lgmrec_rec_step_ms_{rnd}"] = events(lambda: step(False))
    res[f"rflgmrec_rec_step_ms_{rnd}"] = events(lambda: step(True))
    res[f"rf_train_step_ms_{rnd}"] = events(lambda: g.train_step(X1, cond, users, pos, prior=prior))
    m._forward(train=True, step=m._step)
    res[f"prior_ms_{rnd}"] = events(lambda: m.rf_step_inputs(cge))
    res[f"prior_share_of_peak_by_events_{rnd}"] = round(
        prior_bytes / (res[f"prior_ms_{rnd}"][0] * 1e-3) / (PEAK_TBS * 1e12), 4)

# the warmed-up evaluation pass: the mix as the sampler's epilogue against sample + copy64 + axpy
gen_rows = torch.empty(N, 64, device=m.device)
fused_hook = m._cge_for_hyper


def composed_hook(c):
    if not m._mixing:
        return c
    g.generate(m.mge, z0=m._z0, out=gen_rows)
    copy64(c, m._mixc)
    _lib.call("gmr_axpy_dev_f32", N * 64, ptr(g._ratio), ptr(gen_rows), ptr(m._mixc), stream())
    return m._mixc


g.set_epoch(g.warmup_epochs)
noise = torch.empty(2, N, m.hyper_num, device=m.device).exponential_().log_().neg_()
z0 = torch.randn(N, 64, device=m.device)
m.forward_embeddings(noise, z0)
want = m.all.clone()
m._cge_for_hyper = composed_hook
m.forward_embeddings(noise, z0)
res["fused_vs_composed_max_abs"] = float((m.all - want).abs().max())
runs = {"fused": [], "composed": []}
for _ in range(a.runs):
    for name, hook in (("composed", composed_hook), ("fused", fused_hook)):
        m._cge_for_hyper = hook
        runs[name].append(events(lambda: m.forward_embeddings(noise, z0))[0])
m._cge_for_hyper = fused_hook
g.set_epoch(0)
res["eval_tables_cold_ms"] = events(lambda: m.forward_embeddings(noise, z0))
for name, ts in runs.items():
    res[f"eval_tables_warm_{name}_runs_ms"] = [round(t, 5) for t in ts]
    res[f"eval_tables_warm_{name}_median_ms"] = round(statistics.median(ts), 5)
    res[f"eval_tables_warm_{name}_spread_ms"] = round(max(ts) - min(ts), 5)
res["fused_minus_composed_ms"] = round(res["eval_tables_warm_fused_median_ms"] -
                                       res["eval_tables_warm_composed_median_ms"], 5)
res["fused_not_slower_beyond_composed_spread"] = bool(
    res["fused_minus_composed_ms"] <= res["eval_tables_warm_composed_spread_ms"])
for k, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{k:36s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[k] = [round(v[0], 5), round(v[1], 5)]
for name in runs:
    med, spr = res[f"eval_tables_warm_{name}_median_ms"], res[f"eval_tables_warm_{name}_spread_ms"]
    print(f"warm evaluation tables, {name:8s}: median of {a.runs} runs {med:.4f} ms, spread {spr:.4f} ms", flush=True)
print(json.dumps(res), flush=True)
