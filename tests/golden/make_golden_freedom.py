"""Generate tests/golden/freedom_tiny.npz by running the reference FREEDOM (models/freedom.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the
output is data only.  Case A: knn_k=5, n_mm_layers=1, n_ui_layers=2, dropout=0.8 (the pruned graph
the reference drew is stored with its draw); case B: the same data and initial parameters with
n_mm_layers=2, n_ui_layers=3, dropout=0.

The train edges are stored (and given to the reference) sorted by (user, item), so the reference's
edge ids are the positions of the package's user CSR.

Usage:  python tests/golden/make_golden_freedom.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Cfg, MockLoader, OUT, _import_reference, coo_of, make_interactions  # noqa: E402

PARAMS = ["user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "image_trs.weight",
          "image_trs.bias", "text_embedding.weight", "text_trs.weight", "text_trs.bias"]


def _check_knn_gap(feat, k):
    """Every row's k-th and (k+1)-th largest cosine similarity differ by more than 1e-4."""
    f = feat.astype(np.float64)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    s = -np.sort(-(f @ f.T), axis=1)
    return (s[:, k - 1] - s[:, k]).min() > 1e-4


def gen_freedom(tmp):
    import scipy.sparse as sp
    import torch
    sp.dok_matrix._update = lambda self, d: self._dict.update(d)  # removed from scipy; freedom.py:111 calls it
    _import_reference()
    import models.freedom as freedom

    U, I, DV, DT, B, k = 37, 41, 40, 25, 16, 5
    for seed in range(11, 64):  # the first seed from 11 whose features give well-separated top-k lists
        rng = np.random.default_rng(seed)
        rows, cols = make_interactions(rng, U, I)
        v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
        t = rng.standard_normal((I, DT)).astype(np.float32)
        if _check_knn_gap(v, k) and _check_knn_gap(t, k):
            break
    else:
        raise AssertionError("no seed with a kNN gap above 1e-4")
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    os.makedirs(os.path.join(tmp, "tf"), exist_ok=True)
    np.save(os.path.join(tmp, "tf", "image_feat.npy"), v)
    np.save(os.path.join(tmp, "tf", "text_feat.npy"), t)
    users = rng.integers(0, U, B)
    pos = rng.integers(0, I, B)
    neg = rng.integers(0, I, B)
    neg[0] = pos[0]                      # a pos == neg row
    users[2], users[3] = users[1], users[1]  # a user three times
    pos[5], neg[6] = pos[4], pos[4]      # an item twice as positive and once as negative
    assert len(set(users.tolist())) < B and len(set(pos.tolist()) | set(neg.tolist())) < 2 * B

    def cfg(**kw):
        base = dict(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                    device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/",
                    dataset="tf", vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy",
                    embedding_size=64, feat_embed_dim=64, knn_k=k, lambda_coeff=0.9, cf_model="lightgcn",
                    mm_image_weight=0.1, degree_ratio=1.0, reg_weight=0.001)
        base.update(kw)
        return Cfg(**base)

    def fresh(c):
        mm = os.path.join(tmp, "tf", "mm_adj_freedomdsp_{}_{}.pt".format(k, 1))
        if os.path.exists(mm):
            os.remove(mm)  # the reference caches mm_adj on disk; every case builds its own
        torch.manual_seed(3)
        return freedom.FREEDOM(c, MockLoader(U, I, rows, cols))

    def knn_ind(feat):
        n = feat.div(torch.norm(feat, p=2, dim=-1, keepdim=True))
        return torch.topk(torch.mm(n, n.t()), k, dim=-1)[1].numpy()

    out = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
           "users": users, "pos": pos, "neg": neg, "data_seed": np.int64(seed)}
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])

    def step(m, tag):
        m.zero_grad()
        ua, ia = m.forward(m.masked_adj)
        u = ua[inter[0]]
        terms = [m.bpr_loss(u, ia[inter[1]], ia[inter[2]])]
        tf_, vf_ = m.text_trs(m.text_embedding.weight), m.image_trs(m.image_embedding.weight)
        terms.append(m.bpr_loss(u, tf_[inter[1]], tf_[inter[2]]))
        terms.append(m.bpr_loss(u, vf_[inter[1]], vf_[inter[2]]))
        loss = m.calculate_loss(inter)
        loss.backward()
        out[tag + "loss"] = np.float32(loss.item())
        out[tag + "loss_terms"] = np.asarray([x.item() for x in terms], np.float32)  # graph, text, image
        params = dict(m.named_parameters())
        for n in PARAMS:
            out[tag + "g_" + n.replace(".", "_")] = params[n].grad.numpy().copy()
        with torch.no_grad():
            out[tag + "scores"] = m.full_sort_predict([torch.arange(U)]).numpy()
        return ua, ia

    # ---- case A
    m = fresh(cfg(n_mm_layers=1, n_ui_layers=2, dropout=0.8))
    params = dict(m.named_parameters())
    assert list(params) == PARAMS
    for n in PARAMS:
        out["p_" + n.replace(".", "_")] = params[n].detach().numpy().copy()
    out["norm_adj_idx"], out["norm_adj_val"] = coo_of(m.norm_adj)
    out["mm_adj_idx"], out["mm_adj_val"] = coo_of(m.mm_adj)
    out["knn_ind_image"] = knn_ind(m.image_embedding.weight.detach())
    out["knn_ind_text"] = knn_ind(m.text_embedding.weight.detach())
    a, b = out["knn_ind_image"], out["knn_ind_text"]
    share = [len(set(x) & set(y)) for x, y in zip(a.tolist(), b.tolist())]
    assert max(share) >= 1 and min(share) < k, "the two kNN lists must share an index in some row and differ in some"
    out["edge_values"] = m.edge_values.numpy().copy()
    assert np.array_equal(m.edge_indices.numpy(), np.stack([rows, cols]))
    # pre_epoch_processing (freedom.py:128-143) with the draw kept
    torch.manual_seed(17)
    degree_len = int(m.edge_values.size(0) * (1. - m.dropout))
    degree_idx = torch.multinomial(m.edge_values, degree_len)
    torch.manual_seed(17)
    m.pre_epoch_processing()
    out["degree_idx"] = degree_idx.numpy()
    out["masked_adj_idx"], out["masked_adj_val"] = coo_of(m.masked_adj)
    kept = np.stack([rows[out["degree_idx"]], cols[out["degree_idx"]] + U])
    assert set(map(tuple, kept.T)) == set(map(tuple, out["masked_adj_idx"][:, out["masked_adj_idx"][0] < U].T))
    ua, ia = step(m, "A_")
    out["A_ua"], out["A_ia"] = ua.detach().numpy(), ia.detach().numpy()

    # ---- case B: same data and parameters, deeper propagation, no pruning
    mb = fresh(cfg(n_mm_layers=2, n_ui_layers=3, dropout=0.0))
    for n, p in mb.named_parameters():
        assert np.array_equal(p.detach().numpy(), out["p_" + n.replace(".", "_")])
    mb.pre_epoch_processing()
    step(mb, "B_")
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_freedom(tmp)
    path = os.path.join(OUT, "freedom_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; loss A", out["A_loss"], "loss B", out["B_loss"])


if __name__ == "__main__":
    main()
