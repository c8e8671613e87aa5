"""Generate tests/golden/ddrm_tiny.npz by running the reference DDRM (models/ddrm.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  U = 37, I = 41, B = 16 (a user and an item three times in the batch), dims [300], lightGCN_n_layers 3,
steps 100 with the YAML's schedule, constructed under torch.manual_seed(3).  Recorded: the parameters, the fp64
schedule tables, one training step (t with 0, T - 1 and a repeated value, both noises, both dropout keep masks, the
loss, the per-row w / softplus / recon terms, every gradient) and the scores of all users at sampling_steps 0 and 3
and with sampling_noise at 3 steps (q_sample noise and step noises recorded; step_noise is indexed by timestep).

The train edges are stored (and given to the reference) sorted by (user, item), the order of the package's user CSR.

Usage:  python tests/golden/make_golden_ddrm.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Cfg, MockLoader, OUT, _import_reference, make_interactions  # noqa: E402

TABLES = ("betas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_variance",
          "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def key(name):
    return name.replace(".", "_")


def gen_ddrm():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    _import_reference()
    import models.ddrm as ddrm

    U, I, B, H, T = 37, 41, 16, 300, 100
    rng = np.random.default_rng(17)
    rows, cols = make_interactions(rng, U, I)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    users[2] = users[3] = users[1]
    pos[7] = pos[9] = pos[5]
    t = rng.integers(0, T, B)
    t[0], t[1], t[3] = 0, T - 1, t[2]

    cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
              device=torch.device("cpu"), end2end=False, is_multimodal_model=False, embedding_size=64,
              lightGCN_n_layers=3, keep_prob=0.6, A_split=False, dropout=False, steps=T, noise_schedule="linear-var",
              noise_scale=0.0001, noise_min=0.0005, noise_max=0.005, sampling_steps=0, sampling_noise=False,
              dims=[H], act="tanh", norm=False, alpha=0.1, beta=0.1, reg_weight=0.0001)
    torch.manual_seed(3)
    m = ddrm.DDRM(cfg, MockLoader(U, I, rows, cols))
    names = [n for n, _ in m.named_parameters()]
    out = {"U": np.int64(U), "I": np.int64(I), "H": np.int64(H), "T": np.int64(T), "train_rows": rows,
           "train_cols": cols, "users": users, "pos": pos, "neg": neg, "t": t.astype(np.int64),
           "param_names": np.array(names)}
    for n, p in m.named_parameters():
        out["p_" + key(n)] = p.detach().numpy().copy()
    d = m.diffusion
    for k in TABLES:
        out["sch_" + k] = getattr(d, k).numpy().astype(np.float64).copy()

    class RecDrop(nn.Module):  # nn.Dropout that keeps the mask it drew
        def __init__(self, p, sink):
            super().__init__()
            self.p, self.sink = p, sink

        def forward(self, x):
            y = F.dropout(x, self.p, self.training)
            self.sink.append(((y != 0) | (x == 0)).numpy().astype(np.uint8))
            return y

    # ---- one training step with everything recorded
    sink_u, sink_i, noises, recs, sps, ws = [], [], [], [], [], []
    m.user_reverse_model.drop = RecDrop(0.5, sink_u)
    m.item_reverse_model.drop = RecDrop(0.5, sink_i)
    randn_like, softplus, tpow = torch.randn_like, F.softplus, torch.pow
    get_rec = d.get_reconstruct_loss

    def rec_randn(x):
        noises.append(randn_like(x))
        return noises[-1]

    def rec_softplus(x):
        sps.append(softplus(x))
        return sps[-1]

    def rec_pow(a, b):
        ws.append(tpow(a, b))
        return ws[-1]

    def rec_loss(a, b, pt):
        recs.append(get_rec(a, b, pt))
        return recs[-1]

    d.sample_timesteps = lambda n, dev, method="uniform": (torch.as_tensor(t), torch.ones(n))
    d.get_reconstruct_loss = rec_loss
    m.train()
    m.zero_grad()
    torch.manual_seed(13)
    torch.randn_like, F.softplus, torch.pow = rec_randn, rec_softplus, rec_pow
    try:
        loss = m.calculate_loss([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    finally:
        torch.randn_like, F.softplus, torch.pow = randn_like, softplus, tpow
    loss.backward()
    assert len(noises) == 2 and len(sink_u) == 1 and len(sink_i) == 1 and len(recs) == 2 and len(sps) == 2
    out["noise_u"], out["noise_i"] = noises[0].numpy().copy(), noises[1].numpy().copy()
    out["keep_u"], out["keep_i"] = sink_u[0], sink_i[0]
    assert 0.4 < out["keep_u"].mean() < 0.6 and 0.4 < out["keep_i"].mean() < 0.6
    out["loss"] = np.float32(loss.item())
    out["row_w"] = ws[-1].detach().numpy().copy()
    out["row_sp"] = sps[-1].detach().numpy().copy()
    out["row_rec"] = ((recs[0] + recs[1]) / 2).detach().numpy().copy()
    for n, p in m.named_parameters():
        out["g_" + key(n)] = p.grad.numpy().copy()

    # ---- prediction: all users, recorded noise
    m.eval()
    allu = [torch.arange(U)]

    def scores(S, noisy, seed):
        cfg["sampling_steps"], cfg["sampling_noise"] = S, noisy
        draws = []

        def rr(x):
            draws.append(randn_like(x))
            return draws[-1]

        torch.manual_seed(seed)
        torch.randn_like = rr
        try:
            with torch.no_grad():
                sc = m.full_sort_predict(allu).numpy().copy()
        finally:
            torch.randn_like = randn_like
        return sc, [x.numpy().copy() for x in draws]

    out["scores_s0"], dr = scores(0, False, 21)
    out["noise_s0"] = dr[0]
    out["scores_s3"], dr = scores(3, False, 22)
    out["noise_s3"] = dr[0]
    out["scores_s3n"], dr = scores(3, True, 23)
    assert len(dr) == 4
    out["noise_s3n"] = dr[0]
    out["step_noise_s3n"] = np.stack(dr[1:][::-1])  # draws run i = 2, 1, 0: index by timestep
    assert not np.allclose(out["scores_s3"], out["scores_s0"])
    return out


def main():
    out = gen_ddrm()
    # random fp32 does not compress: the gradients go to a file of their own so that each stays under 1 MiB
    grads = {k: out.pop(k) for k in [k for k in out if k.startswith("g_")]}
    for name, d in (("ddrm_tiny.npz", out), ("ddrm_tiny_grad.npz", grads)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)
    print("loss", out["loss"])


if __name__ == "__main__":
    main()
