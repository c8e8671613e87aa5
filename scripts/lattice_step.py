"""Time LATTICE on the synthetic baby shape (gmr/synthetic.py), B = 2,048: the epoch, the build step against the
frozen step, the frozen step against FREEDOM's step on the same data, each gmr_lat_* kernel with the bytes it has to
move, and the graph build plus its backward against the same computation in eager dense torch ops on the GPU
(lattice.py:133-163 as the reference writes it: I x I matrices through autograd), with the peak device memory of
both.  Device work is timed with HIP events after a warm-up (medians); whatever has a host sync inside (the build
step wraps a CSR, the epoch, the evaluation) by a host clock around a device synchronise.  Prints one JSON line last.
python scripts/lattice_step.py [--shape baby] [--batch 2048] [--reps 100] [--profile N]
--profile N: N build steps and 4 N frozen steps and nothing else, for a kernel trace."""
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
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--profile", type=int, default=0)
a = ap.parse_args()
import torch  # noqa: E402

from gmr import _lib  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.freedom import FREEDOM  # noqa: E402
from gmr.kernels import ptr, stream  # noqa: E402
from gmr.lattice import LATTICE  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

PEAK_TBS = 8.0  # MI355X HBM3E peak, TB/s

if not torch.cuda.is_available():
    raise SystemExit("lattice_step.py measures on the GPU; none found")
over = {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False, "epochs": 1}
cfg = Config("LATTICE", "baby", dict(over))
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
t0 = time.time()
m = LATTICE(cfg, tl)
torch.cuda.synchronize()
build_s = time.time() - t0
trainer = Trainer(cfg, m)
d = tl.epoch()
_, _, users, pos, neg, plan, _ = next(iter(tl.batches(d)))
B, U, I, N, k, M = users.numel(), m.n_users, m.n_items, m.N, m.knn_k, m.M
Mk, R = M * k, 2 * M * k


def build_step():
    m.pre_epoch_processing()
    m.rec_step(users, pos, neg, plan)


def frozen_step():
    m.rec_step(users, pos, neg, plan)


if a.profile:
    for _ in range(a.profile):
        build_step()
        for _ in range(4):
            frozen_step()
    m.forward_embeddings()
    torch.cuda.synchronize()
    print(json.dumps({"profiled_build_steps": a.profile, "I": I, "B": B}), flush=True)
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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return [round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)]


res = {"shape": a.shape, "B": B, "U": U, "I": I, "knn_k": k, "M": M, "R": R, "n_layers": m.n_layers,
       "construction_s": round(build_s, 3)}
build_step()
res["loss_first_step"] = round(float(m.loss_terms()[0]), 6)
res["build_step_peak_mb_above_resident_and_total"] = peak_mb(build_step)

# ---- the steps, and FREEDOM's on the same data
fcfg = Config("FREEDOM", "baby", dict(over))
fcfg["pop_items"], fcfg["warm_users"] = pop, warm
fm = FREEDOM(fcfg, tl)
fm.pre_epoch_processing()
for rnd in range(2):  # alternating, twice: the spread
    res[f"build_step_ms_{rnd}"] = host(build_step)
    res[f"frozen_step_ms_{rnd}"] = events(frozen_step)
    res[f"freedom_step_ms_{rnd}"] = events(lambda: fm.rec_step(users, pos, neg, plan))
G = m.graph


def graph_only():
    """The graph build and its backward as a build step runs them (g_l and h_l of the last step)."""
    m._build(G)
    G.build_transpose(M, k)
    m.gslab.zero_grad()
    m._graph_backward(G)


res["graph_build_plus_backward_ms"] = host(graph_only)
res["graph_build_ms"] = host(lambda: m._build(G))
res["graph_transpose_and_lists_ms"] = host(lambda: G.build_transpose(M, k))
res["graph_backward_ms"] = events(lambda: m._graph_backward(G))
res["graph_build_plus_backward_peak_mb_above_resident"] = peak_mb(graph_only)[0]

# ---- each new kernel: events around one call (an upper bound of the kernel's time: the launch gap is inside)
n0, n1 = m._nf(0), m._nf(M - 1)
d0, d1 = m._nf(0, m.dn), m._nf(M - 1, m.dn)
mw, lam, ldc = m._mw(), m.lambda_coeff, G.col.stride(0)
g1, h0 = m._g[m.n_layers - 1], m.slab.view("E")[U:]
row = 256
calls = {
    "gmr_lat_edge_fwd": (lambda: _lib.call("gmr_lat_edge_fwd", I, k, M, ptr(n0), n0.stride(0), ptr(m.idx[0]), k, ptr(n1),
                                           n1.stride(0), ptr(m.idx[M - 1]), k, ptr(mw), ptr(G.v), ptr(G.col), ldc,
                                           ptr(G.r), ptr(G.s), stream()),
                         M * I * row + 3 * I * Mk * 4 + 8 * I, I * Mk * row),
    "gmr_lat_adj_fwd": (lambda: _lib.call("gmr_lat_adj_fwd", I, k, M, ptr(G.v), ptr(G.s), ptr(G.col), ldc, ptr(m.oval),
                                          ptr(mw), lam, ptr(G.val), stream()),
                        3 * I * Mk * 4 + 4 * I + I * R * 4, I * Mk * 4),
    "gmr_lat_sddmm": (lambda: _lib.call("gmr_lat_sddmm", I, R, ptr(G.col), ldc, ptr(g1), g1.stride(0), ptr(h0),
                                        h0.stride(0), 0, ptr(m.dA), stream()),
                      2 * I * row + 2 * I * R * 4, I * R * row),
    "gmr_lat_bwd_ds": (lambda: _lib.call("gmr_lat_bwd_ds", I, k, M, ptr(m.dA), ptr(G.v), ptr(G.r), ptr(G.s), ptr(G.col),
                                         ldc, ptr(G.in_ptr), ptr(G.in_edge), ptr(mw), lam, ptr(m.dr), stream()),
                       4 * I * Mk * 4 + 4 * (3 * I + M * I), 2 * I * Mk * 12),
    "gmr_lat_bwd_da": (lambda: _lib.call("gmr_lat_bwd_da", I, k, M, ptr(m.dA), ptr(G.v), ptr(G.s), ptr(m.dr), ptr(G.col),
                                         ldc, ptr(m.oval), ptr(mw), lam, ptr(m.dv), ptr(m.parts), stream()),
                       I * R * 4 + 4 * I * Mk * 4 + 16 * I, I * Mk * 4),
    "gmr_lat_bwd_dn": (lambda: _lib.call("gmr_lat_bwd_dn", I, k, M, ptr(m.dv), ptr(n0), n0.stride(0), ptr(n1),
                                         n1.stride(0), ptr(G.col), ldc, ptr(G.in_ptr), ptr(G.in_edge), ptr(d0),
                                         d0.stride(0), ptr(d1), d1.stride(0), stream()),
                       2 * M * I * row + 3 * I * Mk * 4 + 4 * M * I, 2 * I * Mk * row),
}
if M == 2:
    calls["gmr_lat_dw_reduce"] = (lambda: _lib.call("gmr_lat_dw_reduce", I, ptr(m.parts), ptr(mw),
                                                    ptr(m.gslab.gview("modal_weight")), stream()), 8 * I + 16, 0)
res["kernels"] = {}
for name, (fn, unique, gathered) in calls.items():
    med, mn = events(fn)
    # unique: every array once (the least HBM has to move); gathered: the rows and scalars fetched through the lists,
    # which the caches serve when the table fits (7,050 x 256 B = 1.8 MB per table at baby)
    res["kernels"][name] = {"us_median": round(1e3 * med, 2), "us_min": round(1e3 * mn, 2), "unique_bytes": unique,
                            "gathered_bytes": gathered,
                            "unique_bytes_share_of_hbm_peak": round(unique / (med * 1e-3) / (PEAK_TBS * 1e12), 4),
                            "gathered_rate_tbs": round(gathered / (med * 1e-3) / 1e12, 3)}
    print(name, res["kernels"][name], flush=True)

# ---- the same graph computation in eager dense torch ops (what models/lattice.py runs), with autograd
gs = m.gslab
P = {n_: gs.view(n_).detach().clone().requires_grad_() for n_ in gs.layout}
Ei, up = h0.detach().clone(), g1.detach().clone()
odense = []
for j in range(M):
    o = torch.zeros((I, I), device="cuda")
    o.scatter_add_(1, m.ocol[:, j * k:(j + 1) * k].long(), m.oval[:, j * k:(j + 1) * k])
    odense.append(o)


def dense_graph():
    w = torch.softmax(P["modal_weight"], 0)
    learned, orig = 0, 0
    for j, (name, _) in enumerate(m.mods):
        f = P[name + "_embedding"] @ P[name + "_W"].T + P[name + "_b"]
        f = f / f.norm(dim=-1, keepdim=True)
        sim = f @ f.T
        val, ind = torch.topk(sim, k, dim=-1)
        adj = torch.zeros_like(sim).scatter_(-1, ind, val)
        learned = learned + (w[j] if M == 2 else 1.0) * adj
        orig = orig + (w[j] if M == 2 else 1.0) * odense[j]
    dinv = learned.sum(-1).pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    item_adj = (1 - lam) * (dinv[:, None] * learned * dinv[None, :]) + lam * orig
    h = Ei
    for _ in range(m.n_layers):
        h = item_adj @ h
    return h


def dense_fwd_bwd():
    for p in P.values():
        p.grad = None
    (dense_graph() * up).sum().backward()


try:
    res["dense_eager_graph_fwd_bwd_ms"] = host(dense_fwd_bwd)
    res["dense_eager_peak_mb_above_resident"] = peak_mb(dense_fwd_bwd)[0]
    if m.n_layers == 1:  # the same upstream gradient, so the same parameter gradients
        graph_only()
        worst = 0.0
        for n_ in gs.layout:
            if n_ == "modal_weight" and M == 1:
                continue
            ours, ref = gs.gview(n_), P[n_].grad
            worst = max(worst, float((ours - ref).abs().max() / ref.abs().max()))
        res["dense_vs_sparse_worst_grad_diff_rel_to_max"] = worst
    res["dense_over_sparse"] = round(res["dense_eager_graph_fwd_bwd_ms"][0] / res["graph_build_plus_backward_ms"][0], 2)
except torch.cuda.OutOfMemoryError as e:  # that the dense form does not fit is itself a result
    res["dense_eager_graph_fwd_bwd_ms"] = "out of memory: " + str(e)[:120]
del odense

# ---- epochs through the trainer, and an evaluation
ep = []
for e in range(a.epochs):
    torch.cuda.synchronize()
    t = time.time()
    m.pre_epoch_processing()
    loss, _ = trainer._train_epoch(tl, e)
    torch.cuda.synchronize()
    ep.append(round(time.time() - t, 4))
res["steps_per_epoch"] = len(list(tl.batches(tl.epoch())))
res["epoch_s"] = ep
res["epoch_loss"] = float(loss)
res["evaluate_ms"] = host(lambda: trainer.evaluate(vl), reps=3, warmup=1)
for key, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{key:48s} median {v[0]:10.4f} ms   min {v[1]:10.4f} ms", flush=True)
        res[key] = [round(v[0], 5), round(v[1], 5)]
print(json.dumps(res), flush=True)
