"""Time RFSMORE on the synthetic baby shape (gmr/synthetic.py), B = 2,048, 1,024 InfoNCE negatives, rf_dropout 0.1,
10 sampling steps: ms per rec_step of SMORE and of RFSMORE (the same model, use_rf toggled; gmr/smore.py and
csrc/smore.hip are the ones SMORE itself runs), the RF step alone at C = 192 next to the same step of a C = 128
generator on the same N rows (RFMGCN's width), the fused sampler at C = 192 next to C = 128 (same N, L, steps), the
inputs launches (gmr_rf_view3_inputs) alone with their share of the HBM peak from the bytes they move, the sum of the
parts against the whole step, and the evaluation before and after warm-up.  Device work is timed with HIP events after
a warm-up (medians); every variant is taken twice in alternation in this one process, so a drift of the clock shows.
Prints one JSON line last; run it under a time limit (timeout -k 10 600 python scripts/rfsmore_step.py).  --profile N:
N steps and two warmed-up table builds only, for a kernel trace in a run of its own.
python scripts/rfsmore_step.py [--shape baby] [--batch 2048] [--reps 100] [--steps 10] [--profile 0]"""
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--profile", type=int, default=0)
a = ap.parse_args()
import torch  # noqa: E402

from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.rf import RFGenerator  # noqa: E402
from gmr.rfsmore import RFSMORE  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

PEAK_TBS = 8.0  # MI355X HBM3E peak, TB/s

if not torch.cuda.is_available():
    raise SystemExit("rfsmore_step.py measures on the GPU; none found")
cfg = Config("RFSMORE", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                                 "epochs": 1, "rf_sampling_steps": a.steps, "rf_dropout": 0.1,
                                 "rf_infonce_negatives": 1024})
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
m = RFSMORE(cfg, tl)
trainer = Trainer(cfg, m)
m.pre_epoch_processing()
d = tl.epoch()
_, _, users, pos, neg, pb, pc = next(iter(tl.batches(d)))
B, N = users.numel(), m.N
g = m.rf_generator


def set_warm(on):
    g.set_epoch(g.warmup_epochs if on else 0)


if a.profile:
    for _ in range(a.profile):
        m.rec_step(users, pos, neg, pb, pc)
    set_warm(True)
    for _ in range(2):
        m.forward_embeddings()
    torch.cuda.synchronize()
    print(json.dumps({"profiled_steps": a.profile, "N": N, "B": B}), flush=True)
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


def host(fn, reps=5, warmup=1):
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


# the inputs kernel reads a, b, f and the gate twice (sum pass, subtract pass) and writes N x 192 + N x 64
inputs_bytes = N * 64 * 4 * (2 * 4 + 4)
res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "N": N, "rf_n_layers": g.L, "condition_dim": g.C,
       "n_neg": g.n_neg, "rf_dropout": g.dropout, "sampling_steps": a.steps, "inputs_bytes": inputs_bytes}
loss = float(m.rec_step(users, pos, neg, pb, pc))
res["loss_first_step"] = round(loss, 6)
res["rf_losses_first_step"] = [round(float(x), 6) for x in m.rf_loss_terms().cpu()]
X1, cond, prior = m.rf_step_inputs()
# RFMGCN's width on the same rows: a C = 128 generator with the same settings, its conditions the first two views
g128 = RFGenerator(m.n_users, m.n_items, 128, m.device, n_layers=g.L, dropout=g.dropout, learning_rate=g.lr,
                   sampling_steps=a.steps, warmup_epochs=g.warmup_epochs, contrast_temp=g.temp,
                   contrast_weight=g.weight, n_negatives=g.n_neg, seed=g.seed)
cond128 = cond[:, :128].contiguous()
z0 = torch.randn(N, 64, device=m.device)
out = torch.empty(N, 64, device=m.device)


def step(use_rf):
    m.use_rf = use_rf
    m.rec_step(users, pos, neg, pb, pc)
    m.use_rf = True


for rnd in range(2):
    res[f"smore_rec_step_ms_{rnd}"] = events(lambda: step(False))
    res[f"rfsmore_rec_step_ms_{rnd}"] = events(lambda: step(True))
    res[f"rf_train_step_192_ms_{rnd}"] = events(lambda: g.train_step(X1, cond, users, pos, prior=prior))
    res[f"rf_train_step_128_ms_{rnd}"] = events(lambda: g128.train_step(X1, cond128, users, pos, prior=prior))
    res[f"sample_192_ms_{rnd}"] = events(lambda: g.generate(cond, z0=z0, out=out))
    res[f"sample_128_ms_{rnd}"] = events(lambda: g128.generate(cond128, z0=z0, out=out))
    res[f"inputs_ms_{rnd}"] = events(m._rf_inputs)
    set_warm(False)
    res[f"eval_tables_cold_ms_{rnd}"] = events(m.forward_embeddings)
    set_warm(True)
    res[f"eval_tables_warm_ms_{rnd}"] = events(m.forward_embeddings)
    set_warm(False)
res["eval_pass_cold_ms"] = host(lambda: trainer.evaluate(vl))
set_warm(True)
res["eval_pass_warm_ms"] = host(lambda: trainer.evaluate(vl))
for rnd in range(2):
    parts = sum(res[f"{k}_ms_{rnd}"][0] for k in ("smore_rec_step", "inputs", "rf_train_step_192"))
    res[f"sum_of_parts_ms_{rnd}"] = round(parts, 5)
    # three launches with their gaps, by events: an upper bound of the kernels' time, a lower one of their rate
    res[f"inputs_share_of_peak_by_events_{rnd}"] = round(
        inputs_bytes / (res[f"inputs_ms_{rnd}"][0] * 1e-3) / (PEAK_TBS * 1e12), 4)
    res[f"sample_192_over_128_{rnd}"] = round(res[f"sample_192_ms_{rnd}"][0] / res[f"sample_128_ms_{rnd}"][0], 4)
    res[f"rf_step_192_over_128_{rnd}"] = round(
        res[f"rf_train_step_192_ms_{rnd}"][0] / res[f"rf_train_step_128_ms_{rnd}"][0], 4)
for k, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{k:32s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[k] = [round(v[0], 5), round(v[1], 5)]
for rnd in range(2):
    print(f"sum of parts {rnd}: {res[f'sum_of_parts_ms_{rnd}']:.4f} ms against the whole step "
          f"{res[f'rfsmore_rec_step_ms_{rnd}'][0]:.4f} ms", flush=True)
print(json.dumps(res), flush=True)
