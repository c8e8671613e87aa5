"""Time LD4MRec on the synthetic baby shape (gmr/synthetic.py), B = 2,048: ms per training step (rec_step: forward,
hand-derived backward, history update; the Adam step is timed apart), split by phase from HIP events recorded at
the phase boundaries of rec_step, the share of the step spent in the three big products (item_proj, output_proj
and their gradients: the B x I x H GEMMs), and ms per eval pass (full_sort_predict + mask + top-k over the
validation users).  Device work is timed with HIP events after a warm-up (medians and minima); the eval pass,
which has host syncs inside, by a host clock around a device synchronise.
--cpu times the plain-torch fp32 restatement of the same step (tests/ld4m_fixture.py: forward + autograd backward
on prepared inputs) at the same shape on --threads CPU threads instead: the "CPU baseline, kind: port".
Prints one JSON line last.
python scripts/ld4mrec_step.py [--shape baby] [--batch 2048] [--reps 400] [--cpu --threads 16]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-multimodal-recommendation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="baby")
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--reps", type=int, default=400)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gmr.configurator import Config  # noqa: E402
from gmr.synthetic import SHAPES  # noqa: E402

cfg = Config("LD4MRec", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                                 "epochs": 1})
H, L, T, k = cfg["cnet_hidden_size"], cfg["cnet_n_layers"], cfg["steps"], cfg["svd_k"]


def cpu_baseline():
    """Forward + backward of the restatement in fp32 on random parameters and inputs of the baby shape."""
    import ld4m_fixture as F
    torch.set_num_threads(a.threads)
    U, I, _, dv, dt = SHAPES[a.shape]
    B, D = a.batch, dv + dt
    gen = torch.Generator().manual_seed(0)
    r = lambda *s, sc=0.05: sc * torch.randn(*s, generator=gen)  # noqa: E731
    wide = {"mm_project": (64, D), "cnet.item_proj": (H, I), "cnet.cond_proj": (H, k + 64),
            "cnet.output_proj": (I, H)}   # every other Linear is H x H, norm1 holds two H vectors

    def shape_of(n):
        if n == "t_in":
            return (1,)
        base, kind = n.rsplit(".", 1)
        w = wide.get(base, (H, H))
        return w if kind == "weight" and "norm1" not in base else (w[0],)

    P = {n: r(*shape_of(n)).requires_grad_(n != "t_in") for n in F.param_names(L)}
    x_in = (torch.rand(B, I, generator=gen) < 0.001).float()
    target = x_in * 0.9 + (1 - x_in) * 0.1
    tt = torch.randint(0, T, (B,), generator=gen)
    x_t = 0.9 * x_in + 0.3 * torch.randn(B, I, generator=gen)
    svd, mm = r(B, k, sc=1.0), r(B, D, sc=1.0)
    masks = [(torch.rand(B, H, generator=gen) < 0.9) for _ in range(L)]
    params = [p for n, p in P.items() if n != "t_in"]

    def step():
        cond = torch.cat([svd, mm @ P["mm_project.weight"].T + P["mm_project.bias"]], 1)
        pred = F.cnet_ref(P, L, x_t, F.temb_ref(tt, H, torch.float32), cond, masks, 0.9)
        loss = ((pred - target) ** 2).mean(1).mean()
        torch.autograd.grad(loss, params)
        return loss.item()

    step()
    ts = []
    for _ in range(max(3, min(a.reps, 5))):
        t0 = time.time()
        step()
        ts.append(1e3 * (time.time() - t0))
    return {"kind": "port", "what": "fp32 torch restatement, forward + autograd backward", "threads": a.threads,
            "shape": a.shape, "B": B, "step_ms": [round(statistics.median(ts), 2), round(min(ts), 2)]}


if a.cpu:
    print(json.dumps({"cpu_baseline": cpu_baseline()}), flush=True)
    raise SystemExit(0)

from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.ld4mrec import LD4MRec  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("ld4mrec_step.py measures on the GPU; none found (--cpu times the CPU restatement)")
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
t0 = time.time()
m = LD4MRec(cfg, tl)
torch.cuda.synchronize()
build_s = time.time() - t0
trainer = Trainer(cfg, m)
d = tl.epoch()
users = next(iter(tl.batches(d)))[2]
B = users.numel()


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


def host(fn, reps=5, warmup=2):
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


step = lambda: m.rec_step(users)  # noqa: E731
res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "H": H, "L": L, "svd_k": k, "mm_dim": m.mm_dim,
       "construct_s": round(build_s, 2), "parameters": int(sum(p.numel() for p in m.parameters()))}
res["rec_step_ms"] = events(step)
res["adam_ms"] = events(trainer.optimizer.step)
# phases: events at the boundaries inside rec_step (their own cost is in these numbers, not in rec_step_ms above)
phases = {}
for _ in range(a.reps):
    m._marks = []
    step()
    marks, m._marks = m._marks, None
    torch.cuda.synchronize()
    for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
        phases.setdefault(name, []).append(e0.elapsed_time(e1))
res["phase_ms"] = {n: round(statistics.median(v), 4) for n, v in phases.items()}
total = sum(res["phase_ms"].values())
big = sum(res["phase_ms"][n] for n in ("item_proj", "output_proj", "output_proj_bwd", "item_proj_bwd"))
res["phase_sum_ms"] = round(total, 4)
res["big_products_share"] = round(big / total, 4)
# the useful work of the step's products (2 M N K each), over the step time: a whole-step rate, not a kernel's
I, D, C = m.n_items, m.mm_dim, m.cond_dim
flops = 2 * B * (5 * I * H            # item_proj: forward, dW; output_proj: forward, dW, dh
                 + 12 * L * H * H     # linear1, linear2 (forward, dW, dx each) and the 2LH-wide modulation product
                 + 2 * C * H + 64 * H  # cond_proj: forward, dW, and the 64 condition columns that need a gradient
                 + 2 * D * 64)        # mm_project: forward, dW
flops += 2 * 2 * T * H * H            # the time table and its weight gradient
res["step_product_tflops"] = round(flops / (res["rec_step_ms"][0] * 1e-3) / 1e12, 2)
res["rec_step_ms_again"] = events(step)   # the same measurement once more: the spread of this run
eu = torch.arange(min(cfg["eval_batch_size"], m.n_users), device="cuda")
res["predict_batch_ms"] = events(lambda: m.full_sort_predict([eu]), warmup=3)
res["wi_transpose_ms"] = events(lambda: m._transpose_wi(m._w["WiT"]), warmup=3)  # its share of a predict call
res["eval_pass_ms"] = host(lambda: trainer.evaluate(vl))
for kk, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{kk:24s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[kk] = [round(v[0], 5), round(v[1], 5)]
for n, v in res["phase_ms"].items():
    print(f"  phase {n:18s} {v:9.4f} ms  ({100 * v / total:5.1f} %)", flush=True)
print(json.dumps(res), flush=True)
