"""Generate tests/golden/ld4mrec_tiny.npz by running the reference LD4MRec (models/ld4mrec.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is
data only.  U = 37, I = 41, Dv = 40, Dt = 25, B = 16, svd_k = 8, cnet_hidden_size = 64, cnet_n_layers = 2,
steps = 100, constructed under torch.manual_seed(3).  Case d0: dropout 0; case d1: dropout 0.1 with the keep
masks the reference drew recorded (same parameters, SVD table, batch, t and noise).

The train edges are stored (and given to the reference) sorted by (user, item), the order of the package's
user CSR.

Usage:  python tests/golden/make_golden_ld4mrec.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Cfg, MockLoader, OUT, _import_reference, make_interactions  # noqa: E402


def key(name):
    return name.replace(".", "_")


def gen_ld4mrec(tmp):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    _import_reference()
    import models.ld4mrec as ld4

    U, I, DV, DT, B, k, H, L, T = 37, 41, 40, 25, 16, 8, 64, 2, 100
    rng = np.random.default_rng(11)
    rows, cols = make_interactions(rng, U, I)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
    t = rng.standard_normal((I, DT)).astype(np.float32)
    os.makedirs(os.path.join(tmp, "tf"), exist_ok=True)
    np.save(os.path.join(tmp, "tf", "image_feat.npy"), v)
    np.save(os.path.join(tmp, "tf", "text_feat.npy"), t)
    users = rng.integers(0, U, B)
    users[2], users[3] = users[1], users[1]  # a user three times
    assert len(set(users.tolist())) < B - 1

    def cfg(dropout):
        return Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                   device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/",
                   dataset="tf", vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy",
                   embedding_size=64, n_layers=2, reg_weight=1e-4, steps=T, noise_schedule="linear",
                   noise_min=0.0001, noise_max=0.02, sampling_steps=0, reweight=True, norm=True,
                   cnet_hidden_size=H, cnet_n_layers=L, dropout=dropout, svd_k=k, smoothing_gamma=0.1,
                   min_noise_level=0.001)

    def fresh(dropout):
        torch.manual_seed(3)
        np.random.seed(5)
        return ld4.LD4MRec(cfg(dropout), MockLoader(U, I, rows, cols))

    out = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
           "users": users, "svd_k": np.int64(k), "H": np.int64(H), "L": np.int64(L), "T": np.int64(T)}
    inter = [torch.as_tensor(users)]
    rec = {}

    class RecDrop(nn.Module):  # nn.Dropout that keeps the mask it drew
        def __init__(self, p, sink):
            super().__init__()
            self.p, self.sink = p, sink

        def forward(self, x):
            y = F.dropout(x, self.p, self.training)
            self.sink.append(((y != 0) | (x == 0)).numpy().astype(np.uint8))
            return y

    def step(m, tag, masks=None):
        """One calculate_loss + backward with t / noise recorded (first call) or replayed (later calls)."""
        choice, mse = np.random.choice, ld4.F.mse_loss

        def pick(n, size=None, p=None):
            if "t" not in rec:
                np.random.seed(7)
                tt = choice(n, size=size, p=p)
                tt[5] = tt[6] = tt[4]  # one value three times: its loss_history entry compounds
                rec["t"] = tt.copy()
            return rec["t"].copy()

        def q_sample(x, tt):
            if "noise" not in rec:
                torch.manual_seed(13)
                rec["noise"] = torch.randn_like(x)
            ab = m.alpha_bar[tt].unsqueeze(1)
            return torch.sqrt(ab) * x + torch.sqrt(1 - ab) * rec["noise"], rec["noise"]

        def mse_rows(a, b, reduction="mean"):
            r = mse(a, b, reduction=reduction)
            rec["rows"] = r.mean(dim=1).detach().numpy().copy()
            return r

        m.q_sample = q_sample
        m.train()
        m.zero_grad()
        np.random.choice, ld4.F.mse_loss = pick, mse_rows
        try:
            loss = m.calculate_loss(inter)
        finally:
            np.random.choice, ld4.F.mse_loss = choice, mse
        loss.backward()
        out[tag + "loss"] = np.float32(loss.item())
        out[tag + "row_loss"] = rec["rows"]
        for n, p in m.named_parameters():
            out[tag + "g_" + key(n)] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
        out[tag + "loss_history"] = m.loss_history.numpy().copy()

    # ---- case d0
    m = fresh(0.0)
    names = [n for n, _ in m.named_parameters()]
    out["param_names"] = np.array(names)
    for n, p in m.named_parameters():
        out["p_" + key(n)] = p.detach().numpy().copy()
    assert np.all(out["p_t_in"] == 0)
    out["user_svd_emb"] = m.user_svd_emb.numpy().copy()
    out["user_mm_emb"] = m.user_mm_emb.numpy().copy()
    out["alpha_bar"] = m.alpha_bar.numpy().copy()
    m.eval()
    with torch.no_grad():
        out["scores_t0"] = m.full_sort_predict([torch.arange(U)]).numpy().copy()
        m.t_in.data.fill_(-0.37)
        out["scores_tneg"] = m.full_sort_predict([torch.arange(U)]).numpy().copy()
        m.t_in.data.fill_(0.0)
    out["t_in_neg"] = np.float32(-0.37)
    step(m, "d0_")
    out["t"], out["noise"] = rec["t"].astype(np.int64), rec["noise"].numpy().copy()
    vals, counts = np.unique(out["t"], return_counts=True)
    assert counts.max() >= 3
    assert not np.allclose(out["scores_t0"], out["scores_tneg"])

    # ---- case d1: same everything, dropout 0.1 with recorded masks
    m1 = fresh(0.1)
    for n, p in m1.named_parameters():
        assert np.array_equal(p.detach().numpy(), out["p_" + key(n)])
    m1.user_svd_emb = m.user_svd_emb
    sink = []
    for blk in m1.cnet.layers:
        blk.dropout = RecDrop(0.1, sink)
    torch.manual_seed(29)
    step(m1, "d1_")
    assert len(sink) == L
    out["d1_masks"] = np.stack(sink)
    assert 0.8 < out["d1_masks"].mean() < 0.97 and out["d1_masks"].min() == 0
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_ld4mrec(tmp)
    path = os.path.join(OUT, "ld4mrec_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; loss d0", out["d0_loss"], "loss d1", out["d1_loss"])


if __name__ == "__main__":
    main()
