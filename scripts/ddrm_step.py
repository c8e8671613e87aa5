"""Time DDRM on the synthetic baby shape (gmr/synthetic.py), B = 2,048: ms per training step (rec_step: encoder,
both fused denoiser forwards, row loss, backward; the Adam step is timed apart) and ms per eval pass (generation +
fused score -> mask -> top-K over the validation users) at sampling_steps 0 and 10.  Device work is timed with HIP
events after a warm-up (medians and minima, and the step a second time for the spread of the run); the eval pass,
which has host syncs inside, by a host clock around a device synchronise.
--cpu times the plain-torch fp32 restatement (tests/ddrm_fixture.py: forward + autograd backward of the step, and
the prediction at both step counts) at the same shape on --threads CPU threads instead: the "CPU baseline, kind:
port".  Prints one JSON line last.
python scripts/ddrm_step.py [--shape baby] [--batch 2048] [--reps 300] [--cpu --threads 16]"""
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
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gmr.configurator import Config  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402

cfg = Config("DDRM", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                              "epochs": 1})
H, T, L = int(cfg["dims"][0]), int(cfg["steps"]), int(cfg["lightGCN_n_layers"])
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()


def cpu_baseline():
    """The restatement in fp32 with a sparse adjacency (the dense one of the tests does not fit this shape)."""
    import ddrm_fixture as F
    from gmr.ddrm import ddrm_schedule, init_parameters
    torch.set_num_threads(a.threads)
    U, I = ds.user_num, ds.item_num
    rows, cols = tr.df[cfg["USER_ID_FIELD"]].values, tr.df[cfg["ITEM_ID_FIELD"]].values
    N, B = U + I, a.batch
    deg = np.bincount(np.concatenate([rows, U + cols]), minlength=N).astype(np.float64)
    d = np.where(deg > 0, deg ** -0.5, 0.0)
    idx = torch.as_tensor(np.stack([np.concatenate([rows, U + cols]), np.concatenate([U + cols, rows])]))
    val = torch.as_tensor((d[idx[0].numpy()] * d[idx[1].numpy()]).astype(np.float32))
    adj = torch.sparse_coo_tensor(idx, val, (N, N)).coalesce()
    R = torch.sparse_coo_tensor(torch.as_tensor(np.stack([rows, cols])), torch.ones(len(rows)), (U, I)).coalesce()
    cnt = torch.as_tensor(np.maximum(np.bincount(rows, minlength=U), 1).astype(np.float32))[:, None]
    torch.manual_seed(0)
    P = {n: v.clone().requires_grad_(True) for n, v in zip(F.param_names(), init_parameters(U, I, H))}
    sch = ddrm_schedule(T, 1e-4, 5e-4, 5e-3)
    gen = torch.Generator().manual_seed(0)
    users, pos, neg = (torch.randint(0, n, (B,), generator=gen) for n in (U, I, I))
    t = torch.randint(0, T, (B,), generator=gen)
    nu, ni = torch.randn(B, 64, generator=gen), torch.randn(B, 64, generator=gen)
    ku, ki = (torch.rand(B, 64, generator=gen) < 0.5).float(), (torch.rand(B, 64, generator=gen) < 0.5).float()
    sa = F.f32_table(sch["sqrt_alphas_cumprod"], torch.float32)
    s1 = F.f32_table(sch["sqrt_one_minus_alphas_cumprod"], torch.float32)

    def encode():
        E = torch.cat([P["rec_model.embedding_user.weight"], P["rec_model.embedding_item.weight"]])
        tabs = [E]
        for _ in range(L):
            tabs.append(torch.sparse.mm(adj, tabs[-1]))
        return E, torch.stack(tabs, 1).mean(1)

    def step():
        E, G = encode()
        u, p, n = G[users], G[U + pos], G[U + neg]
        ou, _, _ = F.dnn_ref(P, "user_reverse_model", sa[t][:, None] * u + s1[t][:, None] * nu, p, t, ku)
        oi, _, _ = F.dnn_ref(P, "item_reverse_model", sa[t][:, None] * p + s1[t][:, None] * ni, u, t, ki)
        reg = 0.5 * ((E[users] ** 2).sum() + (E[U + pos] ** 2).sum() + (E[U + neg] ** 2).sum()) / B
        loss = F.row_loss_ref(u, p, n, ou, oi, reg, 0.1, 0.1, 1e-4)[0]
        torch.autograd.grad(loss, list(P.values()))
        return loss.item()

    def predict(S):
        with torch.no_grad():
            _, G = encode()
            ua, ia = G[:U], G[U:]
            x = sa[T - 1] * (torch.sparse.mm(R, ia) / cnt) + s1[T - 1] * torch.randn(U, 64, generator=gen)
            x = F.chain_ref(P, x, ua, S, sch, None, torch.float32)
            return x  # the score product and the top-K are not part of this baseline

    def clock(fn, reps=5):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.time()
            fn()
            ts.append(1e3 * (time.time() - t0))
        return [round(statistics.median(ts), 2), round(min(ts), 2)]

    return {"kind": "port", "what": "fp32 torch restatement; step = forward + autograd backward, generate = encoder + "
            "history mean + chain (no scoring, no top-K)", "threads": a.threads, "shape": a.shape, "B": B,
            "step_ms": clock(step), "generate_s0_ms": clock(lambda: predict(0)), "generate_s10_ms": clock(lambda: predict(10))}


if a.cpu:
    print(json.dumps({"cpu_baseline": cpu_baseline()}), flush=True)
    raise SystemExit(0)

from gmr.dataloader import EvalDataLoader, TrainDataLoader  # noqa: E402
from gmr.ddrm import DDRM  # noqa: E402
from gmr.quick_start import popularity_groups  # noqa: E402
from gmr.trainer import Trainer  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("ddrm_step.py measures on the GPU; none found (--cpu times the CPU restatement)")
init_seed(999)
pop, warm, _, _ = popularity_groups(cfg, tr)
cfg["pop_items"], cfg["warm_users"] = pop, warm
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
vl = EvalDataLoader(cfg, va, additional_dataset=tr, batch_size=cfg["eval_batch_size"])
t0 = time.time()
m = DDRM(cfg, tl)
torch.cuda.synchronize()
build_s = time.time() - t0
trainer = Trainer(cfg, m)
d = tl.epoch()
_, _, users, pos, neg, pb, _ = next(iter(tl.batches(d)))
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


m.train()
step = lambda: m.rec_step(users, pos, neg, pb)  # noqa: E731
res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "H": H, "T": T, "n_layers": L,
       "construct_s": round(build_s, 2), "parameters": int(sum(p.numel() for p in m.parameters()))}
res["rec_step_ms"] = events(step)
res["adam_ms"] = events(trainer.optimizer.step)
res["encoder_fwd_ms"] = events(lambda: m._forward(m.tab))
res["rec_step_ms_again"] = events(step)   # the same measurement once more: the spread of this run
m.eval()
for S in (0, 10):
    m.sampling_steps = S
    res[f"generate_s{S}_ms"] = events(m.forward_embeddings, warmup=3)
    res[f"eval_pass_s{S}_ms"] = host(lambda: trainer.evaluate(vl))
for kk, v in list(res.items()):
    if isinstance(v, tuple):
        print(f"{kk:24s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[kk] = [round(v[0], 5), round(v[1], 5)]
print(json.dumps(res), flush=True)
