"""Time FREEDOM on the synthetic baby shape (gmr/synthetic.py), B = 2,048: ms per rec_step split into
forward / fused loss kernel / backward, ms per pre_epoch_processing (pruning + renormalised graph), ms
per eval pass, and the fused loss against the same three BPR terms composed from the older kernels (three
gmr_bpr_logsigmoid_f32 calls on [ua; ia], [ua; T], [ua; V], two adds of the user rows, three loss sums).
Device work is timed with HIP events after a warm-up (medians); the two passes with host syncs inside
(pruning, eval) by a host clock around a device synchronise.  Prints one JSON line last.
python scripts/freedom_step.py [--shape baby] [--batch 2048] [--reps 200]"""
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
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
a = ap.parse_args()
import torch  # noqa: E402

from gmr import _lib  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.freedom import FREEDOM  # noqa: E402
from gmr.kernels import ptr, stream  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("freedom_step.py measures on the GPU; none found")
cfg = Config("FREEDOM", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                                 "epochs": 1})
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
t0 = time.time()
m = FREEDOM(cfg, tl)
torch.cuda.synchronize()
build_s = time.time() - t0
trainer = Trainer(cfg, m)
m.pre_epoch_processing()
d = tl.epoch()
_, _, users, pos, neg, plan, _ = next(iter(tl.batches(d)))
B = users.numel()
w = m._work(B)
U, N = m.n_users, m.N


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


def host(fn, reps=10, warmup=2):
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
m.rec_step(users, pos, neg, plan)
fused_loss = m.loss_terms().clone()
fused_contrib = w["contrib"].clone()

# the composition: three contiguous (U + I) x 64 tables with the user rows ua (built outside the timed region)
tabs = [m.tab[:, :64].contiguous()]
for blk in (1, 2):
    t = m.tab[:, :64].contiguous()
    t[U:] = m.tab[U:, 64 * blk:64 * blk + 64]
    tabs.append(t)
c_loss = [torch.empty(B, device="cuda") for _ in range(3)]
c_contrib = [torch.empty((3 * B, 64), device="cuda") for _ in range(3)]
c_total = torch.zeros(4, device="cuda")
one = torch.ones(1, device="cuda")
reg = m.reg_weight


def composed():
    for j, (t, sc) in enumerate(zip(tabs, (inv, inv * reg, inv * reg))):
        _lib.call("gmr_bpr_logsigmoid_f32", B, U, ptr(t), ptr(users), ptr(pos), ptr(neg), ptr(c_loss[j]),
                  ptr(c_contrib[j]), sc, stream())
    for j in (1, 2):  # user rows: d/du of the three terms summed
        _lib.call("gmr_axpy_dev_f32", B * 64, ptr(one), ptr(c_contrib[j]), ptr(c_contrib[0]), stream())
    for j, sc in enumerate((inv, inv * reg, inv * reg)):
        _lib.call("gmr_sum_f32", B, ptr(c_loss[j]), sc, ptr(c_total), int(j > 0), stream())


composed()
torch.cuda.synchronize()
# the two forms compute the same thing (loss and user rows; pos / neg rows are scaled copies of ua)
assert abs(float(c_total[0]) - float(fused_loss[0])) <= 1e-5 * abs(float(fused_loss[0])), (c_total, fused_loss)
torch.testing.assert_close(c_contrib[0][:B], fused_contrib[:B, :64], rtol=1e-4, atol=1e-7)

res = {"shape": a.shape, "B": B, "U": U, "I": m.n_items, "edges": m.n_edges, "kept_edges": m.masked_adj.nnz // 2,
       "mm_adj_nnz": m.mm_adj.nnz, "construct_s": round(build_s, 2)}
# alternate the two loss forms, twice, so a drift of the clock shows
for rnd in range(2):
    res[f"loss_fused_ms_{rnd}"] = events(lambda: m.loss_fwd_bwd(users, pos, neg, inv, w))
    res[f"loss_composed_ms_{rnd}"] = events(composed)
res["forward_ms"] = events(m.step_forward)
res["backward_ms"] = events(lambda: m.step_backward(plan, w))
res["rec_step_ms"] = events(lambda: m.rec_step(users, pos, neg, plan))
res["pre_epoch_ms"] = host(m.pre_epoch_processing)
res["eval_pass_ms"] = host(lambda: trainer.evaluate(vl))
for k, v in res.items():
    if isinstance(v, tuple):
        print(f"{k:24s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[k] = [round(v[0], 5), round(v[1], 5)]
print(json.dumps(res), flush=True)
