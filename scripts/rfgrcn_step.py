"""Time RFGRCN on the synthetic baby shape (gmr/synthetic.py), B = 2,048, 1,024 InfoNCE negatives, rf_dropout 0.1,
10 sampling steps: ms per rec_step of GRCN and of RFGRCN (the same model, use_rf toggled), the RF step alone at
(embedding_dim, condition_dim) = (192, 192), the fused sampler at (192, 192) next to (64, 192) on the same N, L and
steps (the widest 64-row sampler, RFSMORE's), the mixed sampler (gmr_rf_sample_mix_w, what rf_eval: mixed launches),
the centring launch (gmr_rf_center_segments) alone with its share of the HBM peak from the bytes it moves, and the sum
of the parts against the whole step.  Device work is timed with HIP events after a warm-up (medians); every variant is
taken twice in alternation in this one process, so a drift of the clock shows.  Prints one JSON line last; run it under
a time limit (timeout -k 10 600 python scripts/rfgrcn_step.py).
python scripts/rfgrcn_step.py [--shape baby] [--batch 2048] [--reps 100] [--steps 10]"""
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
ap.add_argument("--steps", type=int, default=10)
a = ap.parse_args()
import torch  # noqa: E402

from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import TrainDataLoader  # noqa: E402
from gmr.rf import RFGenerator  # noqa: E402
from gmr.rfgrcn import RFGRCN  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

PEAK_TBS = 8.0  # MI355X HBM3E peak, TB/s

if not torch.cuda.is_available():
    raise SystemExit("rfgrcn_step.py measures on the GPU; none found")
cfg = Config("RFGRCN", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                                "epochs": 1, "rf_sampling_steps": a.steps, "rf_dropout": 0.1,
                                "rf_infonce_negatives": 1024, "rf_eval": "mixed"})
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
m = RFGRCN(cfg, tl)
m.pre_epoch_processing()
d = tl.epoch()
_, _, users, pos, neg, pb, pc = next(iter(tl.batches(d)))
B, N, W = users.numel(), m.N, m.width
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


# the centring reads the N x W table twice (sum pass, subtract pass) and writes it once
center_bytes = N * W * 4 * 3
res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "N": N, "rf_n_layers": g.L, "embedding_dim": g.D,
       "condition_dim": g.C, "n_neg": g.n_neg, "rf_dropout": g.dropout, "sampling_steps": a.steps,
       "center_bytes": center_bytes}
loss = float(m.rec_step(users, pos, neg, pb))
res["loss_first_step"] = round(loss, 6)
res["rf_losses_first_step"] = [round(float(x), 6) for x in m.rf_loss_terms().cpu()]
X1, cond, prior = m.rf_step_inputs()
# the widest 64-row sampler on the same rows and conditions: embedding_dim 64, condition_dim W
g64 = RFGenerator(m.n_users, m.n_items, W, m.device, n_layers=g.L, dropout=g.dropout, learning_rate=g.lr,
                  sampling_steps=a.steps, warmup_epochs=g.warmup_epochs, contrast_temp=g.temp,
                  contrast_weight=g.weight, n_negatives=g.n_neg, seed=g.seed)
z0 = torch.randn(N, W, device=m.device)
z064 = z0[:, :64].contiguous()
out = torch.empty(N, W, device=m.device)
out64 = torch.empty(N, 64, device=m.device)


def step(use_rf):
    m.use_rf = use_rf
    m.rec_step(users, pos, neg, pb)
    m.use_rf = True


for rnd in range(2):
    res[f"grcn_rec_step_ms_{rnd}"] = events(lambda: step(False))
    res[f"rfgrcn_rec_step_ms_{rnd}"] = events(lambda: step(True))
    res[f"rf_train_step_{W}_ms_{rnd}"] = events(lambda: g.train_step(X1, cond, users, pos, prior=prior))
    res[f"sample_{W}_{W}_ms_{rnd}"] = events(lambda: g.generate(cond, z0=z0, out=out))
    res[f"sample_64_{W}_ms_{rnd}"] = events(lambda: g64.generate(cond, z0=z064, out=out64))
    res[f"sample_mix_{W}_{W}_ms_{rnd}"] = events(lambda: g.generate(cond, z0=z0, out=out, base=cond))
    res[f"center_ms_{rnd}"] = events(m.rf_step_inputs)
for rnd in range(2):
    parts = sum(res[f"{k}_ms_{rnd}"][0] for k in ("grcn_rec_step", "center", f"rf_train_step_{W}"))
    res[f"sum_of_parts_ms_{rnd}"] = round(parts, 5)
    # three launches with their gaps, by events: an upper bound of the kernels' time, a lower one of their rate
    res[f"center_share_of_peak_by_events_{rnd}"] = round(
        center_bytes / (res[f"center_ms_{rnd}"][0] * 1e-3) / (PEAK_TBS * 1e12), 4)
    res[f"sample_{W}_over_64_{rnd}"] = round(res[f"sample_{W}_{W}_ms_{rnd}"][0] / res[f"sample_64_{W}_ms_{rnd}"][0], 4)
for k, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{k:32s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[k] = [round(v[0], 5), round(v[1], 5)]
for rnd in range(2):
    print(f"sum of parts {rnd}: {res[f'sum_of_parts_ms_{rnd}']:.4f} ms against the whole step "
          f"{res[f'rfgrcn_rec_step_ms_{rnd}'][0]:.4f} ms", flush=True)
print(json.dumps(res), flush=True)
