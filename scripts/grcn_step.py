"""Time GRCN on the synthetic baby shape (gmr/synthetic.py) with GRCN.yaml's values, B = 2,048: the step, the graph
block forward plus backward (routing, final attention, refining and the weighted id propagation of both modalities:
GRCN.block_forward / block_backward), the same block in eager torch ops with autograd on the same device (the
index_add_ restatement of tests/grcn_fixture.py moved to the device), every C-ABI call of a step by name, and the
evaluation pass.  Both routing settings are timed ('reference': the users receive no routing message, as in grcn.py;
'items': routed over the user's items).  Device work is timed with HIP events after a warm-up (medians over --reps
calls, two alternating rounds).  Prints one JSON line last.
python scripts/grcn_step.py [--shape baby] [--batch 2048] [--reps 50]"""
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
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()
import torch  # noqa: E402

from gmr import _lib  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.grcn import GRCN  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

D = 64
if not torch.cuda.is_available():
    raise SystemExit("grcn_step.py measures on the GPU; none found")


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


def n(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def seg_softmax(s, idx, size):
    mx = torch.full((size,), -float("inf"), device=s.device).scatter_reduce(0, idx, s.detach(), "amax")
    e = (s - mx[idx]).exp()
    return e / (torch.zeros(size, device=s.device).index_add_(0, idx, e) + 1e-16)[idx]


def attend(xd, xs, di, si):
    al = seg_softmax((xd[di] * xs[si]).sum(1), di, xd.shape[0])
    return torch.zeros_like(xd).index_add_(0, di, al[:, None] * xs[si]), al


def run(routing):
    over = {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False, "epochs": 1,
            "routing": routing}
    cfg = Config("GRCN", "baby", dict(over))
    init_seed(999)
    ds = make_dataset(cfg, a.shape, seed=0)
    tr, va, te = ds.split()
    pop, warm, _, _ = popularity_groups(cfg, tr)
    cfg["pop_items"], cfg["warm_users"] = pop, warm
    tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
    vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
    t0 = time.time()
    m = GRCN(cfg, tl)
    torch.cuda.synchronize()
    res = {"routing": routing, "construction_s": round(time.time() - t0, 3)}
    trainer = Trainer(cfg, m)
    d = tl.epoch()
    _, _, users, pos, neg, plan_bpr, plan_cl = next(iter(tl.batches(d)))
    U, I, E, M, R = m.n_users, m.n_items, m.E, m.M, m.n_layers
    res.update(B=users.numel(), U=U, I=I, E=E, M=M, n_layers=R,
               max_item_degree=int((m.graph.trp[1:] - m.graph.trp[:-1]).max()),
               max_user_degree=int((m.graph.rowptr[1:] - m.graph.rowptr[:-1]).max()))

    def step():
        m.rec_step(users, pos, neg, plan_bpr, plan_cl)

    step()
    res["loss_first_step"] = round(float(m.loss_terms()[0]), 6)

    def block():
        m.block_forward()
        m.block_backward()

    # ---- the C-ABI calls of a step and of the block, counted and timed by name (events around each call: an upper
    # bound of the kernel's time, the launch gap is inside)
    real = _lib.call
    log = []

    def counting(name, *args):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = real(name, *args)
        e.record()
        log.append((name, s, e))
        return rc

    per = {}
    for what, fn in (("step", step), ("block", block)):
        times = {}
        for rep in range(7):
            log.clear()
            _lib.call = counting
            try:
                fn()
            finally:
                _lib.call = real
            torch.cuda.synchronize()
            for k, (name, s, e) in enumerate(log):
                times.setdefault(f"{k:02d} {name}", []).append(s.elapsed_time(e))
        res[what + "_calls"] = len(log)
        per[what] = {k: round(1e3 * statistics.median(v[2:]), 2) for k, v in times.items()}
    res["block_call_us"] = per["block"]
    res["step_call_us"] = per["step"]
    new = {k: v for k, v in per["block"].items() if "gmr_grcn_" in k}
    res["slowest_new_launch"] = max(new, key=new.get)

    # ---- the same block in eager torch ops with autograd
    g = m.graph
    rows = torch.repeat_interleave(torch.arange(U, device=m.device), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols = g.col.long()
    src, dst = torch.cat([rows, cols + U]), torch.cat([cols + U, rows])
    s = m.slab
    leaf = {"F": m.F, "P0": m.P[0], "conf": s.view("conf"), "E": s.view("E")}
    leaf = {k: v.detach().clone().requires_grad_() for k, v in leaf.items()}
    up = torch.randn_like(m.result)

    def eager():
        reps, als = [], []
        for k in range(M):
            f, p = leaf["F"][:, D * k:D * k + D], leaf["P0"][:, D * k:D * k + D]
            for _ in range(R):
                h = attend(p, f, rows, cols)[0] if routing == "items" else torch.zeros_like(p)
                p = n(p + h)
            hu, al = attend(p, f, rows, cols)
            hi, be = attend(f, p, cols, rows)
            reps.append(torch.cat([p + hu, f + hi]))
            als.append(torch.cat([be, al]))
        w = torch.relu((torch.stack(als, 1) * leaf["conf"][src]).max(dim=1)[0])
        x = n(leaf["E"])
        x1 = torch.zeros_like(x).index_add_(0, dst, w[:, None] * x[src])
        x2 = torch.zeros_like(x).index_add_(0, dst, w[:, None] * x1[src])
        return torch.cat([x + x1 + x2] + reps, dim=1)

    def eager_fwd_bwd():
        for p in leaf.values():
            p.grad = None
        (eager() * up).sum().backward()

    with torch.no_grad():
        err = float((eager() - m.result).abs().max())
    res["eager_vs_kernels_max_abs"] = err
    for rnd in range(2):  # alternating, twice: the spread
        res[f"step_ms_{rnd}"] = events(step)
        res[f"block_fwd_ms_{rnd}"] = events(m.block_forward)
        res[f"block_fwd_bwd_ms_{rnd}"] = events(block)
        res[f"eager_block_fwd_bwd_ms_{rnd}"] = events(eager_fwd_bwd, reps=max(5, a.reps // 5), warmup=2)
    res["eager_over_kernels"] = round(res["eager_block_fwd_bwd_ms_1"][0] / res["block_fwd_bwd_ms_1"][0], 2)
    t = time.time()
    trainer.evaluate(vl)
    torch.cuda.synchronize()
    res["evaluate_ms"] = round(1e3 * (time.time() - t), 2)
    for key, v in list(res.items()):
        if isinstance(v, tuple):
            print(f"{routing:10s} {key:32s} median {v[0]:10.4f} ms   min {v[1]:10.4f} ms", flush=True)
            res[key] = [round(v[0], 5), round(v[1], 5)]
    for k, v in per["block"].items():
        print(f"{routing:10s} block call {k:40s} {v:10.2f} us", flush=True)
    if res["eager_over_kernels"] < 1.0:
        print("THE HIP BLOCK IS SLOWER THAN EAGER TORCH", flush=True)
    return res


out = [run(r) for r in ("reference", "items")]
print(json.dumps(out), flush=True)
