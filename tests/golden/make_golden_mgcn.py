"""Generate tests/golden/mgcn_tiny.npz by running the reference MGCN (models/mgcn.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  The reference needs three things to run on a CPU: a scatter_add stand-in for the absent torch_scatter,
torch.Tensor.cuda as the identity (mgcn.py:59,69) and a temporary data_path for its kNN cache files.

The parameters are stored once (init_*): case_params() gives a case's parameters from them, and the maker asserts that
they equal the reference model's bit for bit; all = c + side (fp32) is asserted likewise and not stored.

Case A: the init as drawn under torch.manual_seed(3), n_layers = 1, cl_loss = 0.001.
Case B: the same init with the two embedding tables times 8 and the six 64-input weights times sqrt(8), n_layers = 2,
cl_loss = 0.1: at the raw init the attention gradients are about 1e-7 of the loss scale and too small to test.

Usage:  python tests/golden/make_golden_mgcn.py
"""
import os
import sys
import tempfile
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Cfg, MockLoader, OUT, _import_reference, coo_of, make_interactions  # noqa: E402
from make_golden_freedom import _check_knn_gap  # noqa: E402

PARAMS = ["user_embedding.weight", "item_id_embedding.weight", "image_embedding.weight", "text_embedding.weight",
          "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias", "query_common.0.weight",
          "query_common.0.bias", "query_common.2.weight", "gate_v.0.weight", "gate_v.0.bias", "gate_t.0.weight",
          "gate_t.0.bias", "gate_image_prefer.0.weight", "gate_image_prefer.0.bias", "gate_text_prefer.0.weight",
          "gate_text_prefer.0.bias"]
WIDE = ["query_common.0.weight", "query_common.2.weight", "gate_v.0.weight", "gate_t.0.weight",
        "gate_image_prefer.0.weight", "gate_text_prefer.0.weight"]
CASES = {"A": dict(n_layers=1, cl_loss=0.001), "B": dict(n_layers=2, cl_loss=0.1)}


def case_params(init, case):
    """The parameters of a case from the stored init {name: fp32 array}: case A as drawn, case B with the two
    embedding tables times 8 and the six 64-input weights times fp32(sqrt(8))."""
    if case == "A":
        return dict(init)
    s8 = np.float32(np.sqrt(8.0))
    return {n: (p * np.float32(8.0) if n in ("user_embedding.weight", "item_id_embedding.weight") else
                p * s8 if n in WIDE else p) for n, p in init.items()}


def _kth_positive(feat, k):
    """Every row's k-th largest cosine similarity is positive."""
    f = feat.astype(np.float64)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    return (-np.sort(-(f @ f.T), axis=1))[:, k - 1].min() > 0


def gen_mgcn(tmp):
    import torch
    ts = types.ModuleType("torch_scatter")

    def scatter_add(src, index, dim=0, dim_size=None):
        return torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, src)

    ts.scatter_add = scatter_add
    sys.modules["torch_scatter"] = ts
    _import_reference()
    torch.Tensor.cuda = lambda self, *a, **kw: self
    import models.mgcn as mgcn

    U, I, DV, DT, B, k, L = 37, 41, 40, 25, 16, 5, 2
    for seed in range(11, 256):
        rng = np.random.default_rng(seed)
        rows, cols = make_interactions(rng, U, I)
        v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
        t = rng.standard_normal((I, DT)).astype(np.float32)
        if all(_check_knn_gap(f, k) and _kth_positive(f, k) for f in (v, t)):
            break
    else:
        raise AssertionError("no seed with a kNN gap above 1e-4 and positive k-th similarities")
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    os.makedirs(os.path.join(tmp, "tm"), exist_ok=True)
    np.save(os.path.join(tmp, "tm", "image_feat.npy"), v)
    np.save(os.path.join(tmp, "tm", "text_feat.npy"), t)
    users = rng.integers(0, U, B)
    pos = rng.integers(0, I, B)
    neg = rng.integers(0, I, B)
    users[3] = users[1]  # a user twice
    pos[5] = pos[4]      # a positive item twice
    assert len(set(users.tolist())) < B and len(set(pos.tolist())) < B
    n_isolated = I - len(set(cols.tolist()))

    def fresh(case):
        for f in os.listdir(os.path.join(tmp, "tm")):
            if f.endswith(".pt"):
                os.remove(os.path.join(tmp, "tm", f))  # the reference caches the kNN graphs; every case builds its own
        c = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset="tm",
                vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64, knn_k=k,
                n_ui_layers=L, reg_weight=1e-4, lambda_coeff=0.9, **CASES[case])
        torch.manual_seed(3)
        return mgcn.MGCN(c, MockLoader(U, I, rows, cols))

    out = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
           "users": users, "pos": pos, "neg": neg, "data_seed": np.int64(seed), "n_isolated": np.int64(n_isolated)}
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    init = None
    for case in ("A", "B"):
        m = fresh(case)
        params = dict(m.named_parameters())
        assert list(params) == PARAMS
        if case == "A":
            init = {n: p.detach().clone() for n, p in params.items()}
            for n in PARAMS:
                out["init_" + n.replace(".", "_")] = init[n].numpy().copy()
            out["adj_idx"], out["adj_val"] = coo_of(m.norm_adj)
            out["R_idx"], out["R_val"] = coo_of(m.R)
            out["image_adj_idx"], out["image_adj_val"] = coo_of(m.image_original_adj)
            out["text_adj_idx"], out["text_adj_val"] = coo_of(m.text_original_adj)
        else:
            with torch.no_grad():
                for n, p in params.items():
                    assert torch.equal(p, init[n])
                    if n in ("user_embedding.weight", "item_id_embedding.weight"):
                        p.mul_(8.0)
                    elif n in WIDE:
                        p.mul_(float(np.sqrt(8.0)))
        tag = case + "_"
        # the parameters of a case are stored once: case_params() below gives them from the init, bit for bit
        want = case_params({n: init[n].numpy() for n in PARAMS}, case)
        for n in PARAMS:
            assert np.array_equal(params[n].detach().numpy(), want[n]), n
        m.zero_grad()
        ua, ia, side, content = m.forward(m.norm_adj, train=True)
        # the two modal views (mgcn.py:148-185), which forward does not return
        with torch.no_grad():
            views = []
            for emb, trs, gate, adj in ((m.image_embedding, m.image_trs, m.gate_v, m.image_original_adj),
                                        (m.text_embedding, m.text_trs, m.gate_t, m.text_original_adj)):
                h = m.item_id_embedding.weight * gate(trs(emb.weight))
                for _ in range(m.n_layers):
                    h = torch.sparse.mm(adj, h)
                views.append(torch.cat([torch.sparse.mm(m.R, h), h]).numpy())
        out[tag + "a"], out[tag + "b"] = views
        out[tag + "c"], out[tag + "side"] = content.detach().numpy(), side.detach().numpy()
        # all = c + side in fp32 (mgcn.py:201) is not stored: the sum of the two stored tables gives it bit for bit
        assert np.array_equal(torch.cat([ua, ia]).detach().numpy(), out[tag + "c"] + out[tag + "side"])
        mf, emb, _ = m.bpr_loss(ua[inter[0]], ia[inter[1]], ia[inter[2]])
        su, si = torch.split(side, [U, I])
        cu, ci = torch.split(content, [U, I])
        nce_i = m.InfoNCE(si[inter[1]], ci[inter[1]], 0.2)
        nce_u = m.InfoNCE(su[inter[0]], cu[inter[0]], 0.2)
        loss = m.calculate_loss(inter)
        loss.backward()
        out[tag + "loss"] = np.float32(loss.item())
        out[tag + "loss_terms"] = np.asarray([mf.item(), emb.item(), nce_i.item(), nce_u.item()], np.float32)
        for n in PARAMS:
            out[tag + "g_" + n.replace(".", "_")] = params[n].grad.numpy().copy()
        with torch.no_grad():
            out[tag + "scores"] = m.full_sort_predict([torch.arange(U)]).numpy()
        print(case, "loss", loss.item(), "terms", out[tag + "loss_terms"], "smallest max |grad|",
              min(float(np.abs(out[tag + "g_" + n.replace(".", "_")]).max()) for n in PARAMS))
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_mgcn(tmp)
    path = os.path.join(OUT, "mgcn_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; seed", out["data_seed"], "isolated items", out["n_isolated"])


if __name__ == "__main__":
    main()
