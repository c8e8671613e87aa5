"""Time BM3 on the synthetic baby shape (gmr/synthetic.py), B = 2,048: ms per rec_step, and its three parts timed
on their own (forward: projections, encoder, the two squared norms; loss: the fused kernel and the reduce; backward),
so that the step can be compared with the sum of its parts, and ms per eval pass.  Device work is timed with HIP
events after a warm-up (medians), the parts and the step alternated twice so a drift of the clock shows; the eval
pass (host syncs inside) by a host clock around a device synchronise.  Prints one JSON line last.
python scripts/bm3_step.py [--shape baby] [--batch 2048] [--reps 500]"""
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
ap.add_argument("--reps", type=int, default=500)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
import torch  # noqa: E402

from gmr.bm3 import BM3  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bm3_step.py measures on the GPU; none found")
cfg = Config("BM3", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                             "epochs": 1})
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
m = BM3(cfg, tl)
trainer = Trainer(cfg, m)
d = tl.epoch()
_, _, users, pos, neg, _, plan = next(iter(tl.batches(d)))
B = users.numel()
w = m._work(B)


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


def host(fn, reps=7, warmup=2):
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


inv = 1.0 / B
loss = float(m.rec_step(users, pos, neg, plan_cl=plan))
res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "n_layers": m.n_layers, "dropout": m.dropout,
       "params": int(m.slab.numel), "loss": round(loss, 6)}
for rnd in range(2):
    res[f"forward_ms_{rnd}"] = events(m.step_forward)
    res[f"loss_ms_{rnd}"] = events(lambda: m.loss_fwd_bwd(users, pos, inv, w))
    res[f"backward_ms_{rnd}"] = events(lambda: m.step_backward(plan, w, B))
    res[f"rec_step_ms_{rnd}"] = events(lambda: m.rec_step(users, pos, neg, plan_cl=plan))
res["eval_pass_ms"] = host(lambda: trainer.evaluate(vl))
for k, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{k:24s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[k] = [round(v[0], 5), round(v[1], 5)]
print(json.dumps(res), flush=True)
