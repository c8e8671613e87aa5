"""Time RFFREEDOM on the synthetic baby shape (gmr/synthetic.py), B = 2,048: ms per rec_step with and without the
rectified-flow step, the RF training step by phase (draws + interpolation, net forward, head + InfoNCE + scatter,
backward, AdamW), and the rf_sampling_steps-step sampler in its two forms: gmr_rf_sample (one launch) and the same
integration composed per layer from the GEMM and the row kernels.  The two forms are checked against each other
first (the sampler bar of DESIGN section 11) and then timed alternately, twice, in this one process.  Device work
is timed with HIP events after a warm-up (medians).  Prints one JSON line last; run it under a time limit
(timeout -k 10 600 python scripts/rffreedom_step.py).
python scripts/rffreedom_step.py [--shape baby] [--batch 2048] [--reps 50] [--steps 5]"""
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
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--bar", type=float, default=2.048e-6, help="max abs difference allowed between the two samplers")
a = ap.parse_args()
import torch  # noqa: E402

from gmr import _lib  # noqa: E402
from gmr.configurator import Config  # noqa: E402
from gmr.dataloader import TrainDataLoader  # noqa: E402
from gmr.kernels import ptr, stream  # noqa: E402
from gmr.rf import D, SITE_T, SITE_X0  # noqa: E402
from gmr.rffreedom import RFFREEDOM  # noqa: E402
from gmr.synthetic import make_dataset  # noqa: E402
from gmr.utils import init_seed  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("rffreedom_step.py measures on the GPU; none found")
cfg = Config("RFFREEDOM", "baby", {"synthetic": a.shape, "train_batch_size": a.batch, "save_recommended_topk": False,
                                   "epochs": 1, "rf_sampling_steps": a.steps})
init_seed(999)
ds = make_dataset(cfg, a.shape, seed=0)
tr, va, te = ds.split()
tl = TrainDataLoader(cfg, tr, batch_size=a.batch, shuffle=True)
m = RFFREEDOM(cfg, tl)
m.pre_epoch_processing()
d = tl.epoch()
_, _, users, pos, neg, plan, _ = next(iter(tl.batches(d)))
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


res = {"shape": a.shape, "B": B, "U": m.n_users, "I": m.n_items, "N": N, "rf_n_layers": g.L, "condition_dim": g.C,
       "n_neg": g.n_neg, "sampling_steps": a.steps}
m.rec_step(users, pos, neg, plan)
torch.cuda.synchronize()
res["rf_losses_first_step"] = [round(float(x), 6) for x in m.rf_loss_terms().cpu()]

# ---- rec_step with and without the RF step (the same model: use_rf toggled)
res["rec_step_rf_ms"] = events(lambda: m.rec_step(users, pos, neg, plan))
m.use_rf = False
res["rec_step_freedom_ms"] = events(lambda: m.rec_step(users, pos, neg, plan))
m.use_rf = True

# ---- the RF training step by phase, on the tables of the last step
X1, cond, _ = m.rf_step_inputs()
w = g._work(B)
res["rf_train_step_ms"] = events(lambda: g.train_step(X1, cond, users, pos))


def ph_draws():
    _lib.call("gmr_rf_randn", N * D, g.seed, g.step_ctr, SITE_X0, ptr(w["X0"]), stream())
    _lib.call("gmr_rf_rand", N, g.seed, g.step_ctr, SITE_T, ptr(w["t"]), stream())
    _lib.call("gmr_rf_interp", N, ptr(X1), X1.stride(0), ptr(w["X0"]), ptr(w["t"]), ptr(w["Xt"]), stream())
    _lib.call("gmr_rf_time_embed", N, ptr(w["t"]), ptr(w["S"]), stream())


def ph_head():
    _lib.call("gmr_rf_head_fwd", N, ptr(w["V"]), ptr(w["Xt"]), ptr(X1), X1.stride(0), ptr(w["X0"]), ptr(w["t"]), 0.1,
              ptr(w["pred"]), ptr(w["rowparts"]), stream())
    cp, cb = w["clparts"], w["contrib"]
    g.infonce(w["pred"], X1, 0, g.U, users, cp[:B], cb[:B], None, 3, g.weight / B)
    g.infonce(w["pred"], X1, g.U, g.I, pos, cp[B:2 * B], cb[B:2 * B], None, 2, g.weight / B)
    _lib.call("gmr_rf_losses", N, ptr(w["rowparts"]), B, ptr(cp), g.weight, ptr(w["loss"]), stream())


res["rf_phase_draws_ms"] = events(ph_draws)
res["rf_phase_net_fwd_ms"] = events(lambda: g._net_fwd(w, w["Xt"], w["S"], cond, None))
res["rf_phase_head_infonce_ms"] = events(ph_head)
res["rf_phase_net_bwd_ms"] = events(lambda: g._net_bwd(w, w["Xt"], w["S"], cond))
res["rf_phase_adamw_ms"] = events(g.adamw_step)
# the three products of one 128 x 128 Linear's backward, alone: dW = dY^T X (k = N), db = colsum(dY), dX = dY W
from gmr import kernels as K  # noqa: E402
name = "res_blocks.0.net.4"
res["rf_bwd_dw_gemm_ms"] = events(lambda: K.gemm(w["G2"], w["A"]["block0a"], g.slab.gview(name + ".weight"),
                                                 trans_a=True))
res["rf_bwd_db_colsum_ms"] = events(lambda: K.colsum(w["G2"], g.slab.gview(name + ".bias")))
res["rf_bwd_dx_gemm_ms"] = events(lambda: K.gemm(w["G2"], g.slab.view(name + ".weight"), w["G1"]))
res["rf_bwd_act_ms"] = events(lambda: g._act_bwd(w, w["Y"]["block0a"], "res_blocks.0.net.1", w["G1"], w["G2"]))

# ---- the sampler: one launch against the per-layer composition
z0 = torch.randn((N, D), device="cuda")
o1, o2 = torch.empty((N, D), device="cuda"), torch.empty((N, D), device="cuda")
g.generate(cond, z0=z0, n_steps=a.steps, out=o1, fused=True)
g.generate(cond, z0=z0, n_steps=a.steps, out=o2, fused=False)
torch.cuda.synchronize()
diff = float((o1 - o2).abs().max())
res["sampler_max_abs_diff"] = diff
res["sampler_max_abs"] = float(o2.abs().max())
res["sampler_agree"] = bool(diff <= a.bar and torch.isfinite(o1).all())  # reported; the exit status says it too
print(f"samplers: max abs difference {diff:.3e} (bar {a.bar:.3e}), max |z| {res['sampler_max_abs']:.3f}", flush=True)
for rnd in range(2):  # alternate, twice, so a drift of the clock shows
    res[f"sample_fused_ms_{rnd}"] = events(lambda: g.generate(cond, z0=z0, n_steps=a.steps, out=o1, fused=True))
    res[f"sample_composed_ms_{rnd}"] = events(lambda: g.generate(cond, z0=z0, n_steps=a.steps, out=o2, fused=False))
# MFMA work of the fused kernel: 2 * rows * (in * out) per Linear; the condition encoder once, the rest per step
per_step = 2 * (64 * 128 + g.L * 2 * 128 * 128 + 128 * 128 + 128 * 64)
flop = N * (2 * g.C * 128 + a.steps * per_step)
res["sample_gflop"] = round(flop / 1e9, 3)
res["sample_fused_tflops"] = round(flop / (min(res["sample_fused_ms_0"][0], res["sample_fused_ms_1"][0]) * 1e-3) / 1e12, 3)
g.set_epoch(g.warmup_epochs)  # warmed up: the evaluation tables carry the mix
res["eval_tables_ms"] = events(lambda: m.forward_embeddings(z0))
for k, v in res.items():
    if isinstance(v, tuple):
        print(f"{k:28s} median {v[0]:9.4f} ms   min {v[1]:9.4f} ms", flush=True)
        res[k] = [round(v[0], 5), round(v[1], 5)]
print(json.dumps(res), flush=True)
sys.exit(0 if res["sampler_agree"] else 1)
