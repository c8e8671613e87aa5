"""Generate tests/golden/bm3_tiny.npz by running the reference BM3 (models/bm3.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through the helpers make_golden_freedom.py imports);
the output is data only.  Case A: n_layers=1, dropout=0.3; case B: the same data and initial parameters with
n_layers=2, dropout=0.5.

The four dropout masks of calculate_loss (drawn in the order u, i, t, v on whole tables) are captured by replaying
the generator: seed, draw F.dropout(ones(n, 64), p) for n = U, I, I, I, seed again, run calculate_loss.  The replay
is asserted: the loss recomputed here from the captured masks equals the reference's exactly.

The train edges are stored (and given to the reference) sorted by (user, item).

Usage:  python tests/golden/make_golden_bm3.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_freedom import Cfg, MockLoader, OUT, _import_reference, coo_of, make_interactions  # noqa: E402

PARAMS = ["user_embedding.weight", "item_id_embedding.weight", "predictor.weight", "predictor.bias",
          "image_embedding.weight", "image_trs.weight", "image_trs.bias", "text_embedding.weight", "text_trs.weight",
          "text_trs.bias"]
CASES = {"A": dict(n_layers=1, dropout=0.3), "B": dict(n_layers=2, dropout=0.5)}
MASK_SEED = 17


def gen_bm3(tmp):
    import scipy.sparse as sp
    import torch
    import torch.nn.functional as F
    sp.dok_matrix._update = lambda self, d: self._dict.update(d)  # removed from scipy; bm3.py:67 calls it
    _import_reference()
    import models.bm3 as bm3

    U, I, DV, DT, B = 37, 41, 40, 25, 16
    rng = np.random.default_rng(29)
    rows, cols = make_interactions(rng, U, I)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
    t = rng.standard_normal((I, DT)).astype(np.float32)
    os.makedirs(os.path.join(tmp, "tf"), exist_ok=True)
    np.save(os.path.join(tmp, "tf", "image_feat.npy"), v)
    np.save(os.path.join(tmp, "tf", "text_feat.npy"), t)
    users = rng.integers(0, U, B)
    items = rng.integers(0, I, B)
    users[2], users[3] = users[1], users[1]  # a user three times
    items[5] = items[4]                      # an item twice
    assert sorted(np.bincount(users))[-1] >= 3 and sorted(np.bincount(items))[-1] >= 2

    def cfg(**kw):
        base = dict(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                    device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/",
                    dataset="tf", vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy",
                    embedding_size=64, feat_embed_dim=64, reg_weight=0.1, cl_weight=2.0)
        base.update(kw)
        return Cfg(**base)

    out = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
           "users": users, "items": items, "mask_seed": np.int64(MASK_SEED)}
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(items)])

    def replay(m, keep):
        """calculate_loss of bm3.py:97-147 with the four masks given."""
        cos = F.cosine_similarity
        sc = 1.0 / (1.0 - m.dropout)
        ua, ib = m.forward()
        tf_, vf_ = m.text_trs(m.text_embedding.weight), m.image_trs(m.image_embedding.weight)
        us, it = inter[0], inter[1]
        tu, ti = (ua.detach() * keep[0] * sc)[us], (ib.detach() * keep[1] * sc)[it]
        tt, tvv = (tf_.detach() * keep[2] * sc)[it], (vf_.detach() * keep[3] * sc)[it]
        pu, pi, pt, pv = (m.predictor(x) for x in (ua, ib, tf_, vf_))
        terms = [1 - cos(pu[us], ti, dim=-1).mean(), 1 - cos(pi[it], tu, dim=-1).mean(),
                 1 - cos(pt[it], ti, dim=-1).mean(), 1 - cos(pv[it], ti, dim=-1).mean(),
                 1 - cos(pt[it], tt, dim=-1).mean(), 1 - cos(pv[it], tvv, dim=-1).mean()]
        reg = m.reg_loss(ua, ib)
        loss = (terms[0] + terms[1]).mean() + m.reg_weight * reg + m.cl_weight * (terms[2] + terms[3] + terms[4] +
                                                                                 terms[5]).mean()
        return loss, terms, reg

    for case, kw in CASES.items():
        tag = case + "_"
        torch.manual_seed(3)
        m = bm3.BM3(cfg(**kw), MockLoader(U, I, rows, cols))
        params = dict(m.named_parameters())
        assert list(params) == PARAMS
        for n in PARAMS:
            key = "p_" + n.replace(".", "_")
            val = params[n].detach().numpy().copy()
            if key in out:
                assert np.array_equal(out[key], val), n  # both cases start from the same parameters
            out[key] = val
        if case == "A":
            out["norm_adj_idx"], out["norm_adj_val"] = coo_of(m.norm_adj)
        # the masks calculate_loss will draw
        p = m.dropout
        torch.manual_seed(MASK_SEED)
        keep = [(F.dropout(torch.ones(n, 64), p) != 0) for n in (U, I, I, I)]
        for name, k in zip("uitv", keep):
            out[tag + "keep_" + name] = k.numpy().astype(np.uint8)
        m.zero_grad()
        torch.manual_seed(MASK_SEED)
        loss = m.calculate_loss(inter)
        loss.backward()
        with torch.no_grad():
            again, terms, reg = replay(m, [k.float() for k in keep])
            ua, ib = m.forward()
        assert float((again - loss.detach()).abs().max()) == 0.0, (case, float(again), float(loss.detach()))
        out[tag + "loss"] = np.float32(loss.item())
        out[tag + "loss_terms"] = np.asarray([x.item() for x in terms], np.float32)  # ui, iu, t, v, tv, vt
        out[tag + "reg"] = np.float32(reg.item())
        out[tag + "ua"], out[tag + "ib"] = ua.numpy().copy(), ib.numpy().copy()
        for n in PARAMS:
            out[tag + "g_" + n.replace(".", "_")] = params[n].grad.numpy().copy()
        with torch.no_grad():
            out[tag + "scores"] = m.full_sort_predict([torch.arange(U)]).numpy()
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_bm3(tmp)
    path = os.path.join(OUT, "bm3_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; loss A", out["A_loss"], "loss B", out["B_loss"])


if __name__ == "__main__":
    main()
