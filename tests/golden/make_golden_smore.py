"""Generate tests/golden/smore_tiny.npz (data, init, case A) and smore_tiny_B.npz (case B) by running the reference
SMORE (models/smore.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  The reference needs the same three things as MGCN's to run on a CPU: a scatter_add stand-in for the absent
torch_scatter, torch.Tensor.cuda as the identity (smore.py:63,73) and a temporary data_path for its kNN cache files.

Every case is run twice: in fp32 as the reference computes (loss32, loss_terms32, scores32 and the Adam trajectory; its
gradients are only compared here), and rerun in double (the entries without a suffix: the values the tests pin).  The
double rerun is the reference's own module after .double(), with its graphs replaced by the same graphs evaluated in
double (the dense restatements of tests/smore_fixture.py, asserted here against the reference's fp32 graphs in pattern
and at 2e-6 in value; the union of the fusion graph is exact) and its dropout replaced by the masks its fp32 run drew.

The parameters are stored once (init_*): smore_fixture.case_params() gives a case's parameters from them, and the maker
asserts that they equal the reference model's bit for bit.

Case A: the init as drawn under torch.manual_seed(3), n_layers 1, dropout 0, image_knn_k 5, text_knn_k 3, cl_loss 0.01.
Case B: the same init with the two embedding tables times 8 and the 64-input weights times sqrt(8) (as MGCN's case B),
n_layers 2, dropout 0.1, cl_loss 0.1; then three torch.optim.Adam steps (lr 0.001) of the fp32 reference on the same
batch, each with its own three masks (B_keep: 3 x N x 192; the first step's gradients are the case's), the parameters
after the third step stored as traj3_*.

Usage:  python tests/golden/make_golden_smore.py
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import Cfg, MockLoader, OUT, _import_reference, coo_of, make_interactions  # noqa: E402
from make_golden_freedom import _check_knn_gap  # noqa: E402
from make_golden_mgcn import _kth_positive  # noqa: E402
import smore_fixture as F  # noqa: E402

U, I, DV, DT, B = 37, 41, 40, 25, 16


def _sparse64(dense):
    return dense.to_sparse().coalesce()


def gen_smore(tmp):
    import torch
    import torch.nn as nn
    ts = types.ModuleType("torch_scatter")
    ts.scatter_add = lambda src, index, dim=0, dim_size=None: torch.zeros(dim_size, dtype=src.dtype).index_add_(
        0, index, src)
    sys.modules["torch_scatter"] = ts
    _import_reference()
    torch.Tensor.cuda = lambda self, *a, **kw: self
    import models.smore as smore

    ks = (F.IMAGE_K, F.TEXT_K)
    for seed in range(11, 512):
        rng = np.random.default_rng(seed)
        rows, cols = make_interactions(rng, U, I)
        v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
        t = rng.standard_normal((I, DT)).astype(np.float32)
        if all(_check_knn_gap(f, k) and _kth_positive(f, k) for f, k in zip((v, t), ks)):
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
    n_isolated = I - len(set(cols.tolist()))

    class Recorder(nn.Module):
        """The reference's nn.Dropout, with the mask of every call read off its output (a sigmoid is never 0)."""

        def __init__(self, drop):
            super().__init__()
            self.drop, self.masks = drop, []

        def forward(self, x):
            y = self.drop(x)
            if self.training and self.drop.p > 0:
                self.masks.append((y != 0).numpy().astype(np.uint8))
            return y

    class Replay(nn.Module):
        """Dropout with given masks, in the module's dtype."""

        def __init__(self, masks, p):
            super().__init__()
            self.masks, self.p, self.i = masks, p, 0

        def forward(self, x):
            if not self.training or self.p == 0:
                return x
            k = torch.as_tensor(self.masks[self.i % 3]).to(x.dtype)
            self.i += 1
            return x * k / (1.0 - self.p)

    def fresh(case):
        for f in os.listdir(os.path.join(tmp, "tm")):
            if f.endswith(".pt"):
                os.remove(os.path.join(tmp, "tm", f))  # the reference caches the kNN graphs; every case builds its own
        cs = F.CASES[case]
        c = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset="tm",
                vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64,
                image_knn_k=ks[0], text_knn_k=ks[1], n_ui_layers=F.N_UI_LAYERS, reg_weight=F.REG_WEIGHT,
                lambda_coeff=0.9, temperature=0.2, **cs)
        torch.manual_seed(3)
        m = smore.SMORE(c, MockLoader(U, I, rows, cols))
        m.dropout = Recorder(m.dropout)
        return m

    def step(m, inter):
        """One calculate_loss + backward; returns (loss, terms, tables)."""
        m.zero_grad()
        ua, ia, side, content = m.forward(m.norm_adj, train=True)
        # forward is run once more inside calculate_loss; with dropout that would draw other masks, so the loss is
        # assembled here from the reference's own pieces, as calculate_loss does (smore.py:316-336)
        mf, emb, reg = m.bpr_loss(ua[inter[0]], ia[inter[1]], ia[inter[2]])
        su, si = torch.split(side, [U, I])
        cu, ci = torch.split(content, [U, I])
        nce_i = m.InfoNCE(si[inter[1]], ci[inter[1]], 0.2)
        nce_u = m.InfoNCE(su[inter[0]], cu[inter[0]], 0.2)
        loss = mf + emb + reg + m.cl_loss * (nce_i + nce_u)
        loss.backward()
        return loss, [mf.item(), emb.item(), nce_i.item(), nce_u.item()], (side, content, ua, ia)

    out = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
           "users": users, "pos": pos, "neg": neg, "data_seed": np.int64(seed), "n_isolated": np.int64(n_isolated)}
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    g64 = F.graphs_ref(U, I, rows, cols, (v, t), torch.float64)
    init = None
    for case in ("A", "B"):
        cs, tag = F.CASES[case], case + "_"
        m = fresh(case)
        params = dict(m.named_parameters())
        assert [n.replace("dropout.drop.", "") for n in params] == F.STATE_KEYS, list(params)
        names = dict(zip(F.PARAMS, params.values()))
        if case == "A":
            init = {k: p.detach().clone() for k, p in names.items()}
            for k in F.PARAMS:
                out["init_" + k] = init[k].numpy().copy()
            for key, sp_t in (("adj", m.norm_adj), ("R", m.R), ("image_adj", m.image_original_adj),
                              ("text_adj", m.text_original_adj), ("fusion_adj", m.fusion_adj)):
                out[key + "_idx"], out[key + "_val"] = coo_of(sp_t)
            # the graphs in double against the reference's: the same pattern, the values at 2e-6
            for key, d64, shape in (("adj", g64[0], (U + I, U + I)), ("image_adj", g64[1], (I, I)),
                                    ("text_adj", g64[2], (I, I)), ("fusion_adj", g64[3], (I, I))):
                ref = F.dense_of(out[key + "_idx"], out[key + "_val"], shape)
                assert np.array_equal(ref != 0, d64.numpy() != 0), key
                np.testing.assert_allclose(d64.numpy(), ref, rtol=2e-6, atol=0, err_msg=key)
            # the fusion graph of the reference's own fp32 graphs through the fixture's union: exact
            av32 = torch.tensor(F.dense_of(out["image_adj_idx"], out["image_adj_val"], (I, I)), dtype=torch.float32)
            at32 = torch.tensor(F.dense_of(out["text_adj_idx"], out["text_adj_val"], (I, I)), dtype=torch.float32)
            fa = F.dense_of(out["fusion_adj_idx"], out["fusion_adj_val"], (I, I))
            assert np.array_equal(F.fusion_ref(av32, at32).numpy().astype(np.float64), fa)
            # rows with shared columns (and both orders of the larger value), rows with columns of one graph only
            a_, t_ = av32.numpy(), at32.numpy()
            both, only = (a_ != 0) & (t_ != 0), (a_ != 0) ^ (t_ != 0)
            off = ~np.eye(I, dtype=bool)
            assert (both & off).any(1).sum() >= 3 and only.any(1).sum() >= 3
            assert (both & (a_ > t_)).any() and (both & (t_ > a_)).any()
            out["fusion_shared_rows"] = np.int64((both & off).any(1).sum())
        else:
            with torch.no_grad():
                for k, p in names.items():
                    assert torch.equal(p, init[k])
                    if k in F.TABLES:
                        p.mul_(8.0)
                    elif k in F.WIDE:
                        p.mul_(float(np.sqrt(8.0)))
        want = F.case_params({"init_" + k: init[k].numpy() for k in F.PARAMS}, case)
        for k in F.PARAMS:
            assert np.array_equal(names[k].detach().numpy(), want[k]), k
        start = {k: p.detach().clone() for k, p in names.items()}
        # ---- fp32, as the reference computes
        opt = torch.optim.Adam(m.parameters(), lr=F.LR)
        n_steps = F.ADAM_STEPS if case == "B" else 1
        for j in range(n_steps):
            loss, terms, (side, content, ua, ia) = step(m, inter)
            if j == 0:
                if case == "A":  # without dropout the assembled loss is calculate_loss's, bit for bit
                    assert m.calculate_loss(inter).item() == loss.item()
                out[tag + "loss32"] = np.float32(loss.item())
                out[tag + "loss_terms32"] = np.asarray(terms, np.float32)
                g32 = {k: names[k].grad.numpy().copy() for k in F.PARAMS}
                m.eval()
                with torch.no_grad():
                    out[tag + "scores32"] = m.full_sort_predict([torch.arange(U)]).numpy()
                m.train()
            if case == "B":
                opt.step()
        if case == "B":
            for k in F.PARAMS:
                out[f"traj{n_steps}_{k}"] = names[k].detach().numpy().copy()
        masks = m.dropout.masks
        if case == "B":
            assert len(masks) == 3 * n_steps
            keep = np.stack([np.concatenate(masks[3 * j:3 * j + 3], axis=1) for j in range(n_steps)])
            assert keep.shape == (n_steps, U + I, 192)
            share = keep.mean()
            assert 0.85 < share < 0.95, share
            out["B_keep"] = keep
        else:
            assert not masks
        # ---- the rerun in double
        with torch.no_grad():
            for k, p in names.items():
                p.copy_(start[k])
        m.double()
        m.norm_adj, m.R = _sparse64(g64[0]), _sparse64(g64[0][:U, U:])
        m.image_original_adj, m.text_original_adj, m.fusion_adj = (_sparse64(x) for x in g64[1:])
        m.dropout = Replay(masks[:3], cs["dropout_rate"])
        loss, terms, (side, content, ua, ia) = step(m, inter)
        out[tag + "loss"] = np.float64(loss.item())
        out[tag + "loss_terms"] = np.asarray(terms, np.float64)
        out[tag + "c"], out[tag + "side"] = content.detach().numpy(), side.detach().numpy()
        for k in F.PARAMS:
            g = names[k].grad.numpy().copy()
            out[tag + "g_" + k] = g
            own = np.abs(g32[k].astype(np.float64) - g).max()
            # twice fp32 torch's own error stays below 1e-3 of the gradient's largest entry: the bar can tell a
            # wrong gradient from a right one
            assert 2 * own < 1e-3 * np.abs(g).max(), (case, k, own, np.abs(g).max())
        m.eval()
        with torch.no_grad():
            out[tag + "scores"] = m.full_sort_predict([torch.arange(U)]).numpy()
        print(case, "loss", loss.item(), "fp32", out[tag + "loss32"], "terms", out[tag + "loss_terms"],
              "smallest max |grad|", min(float(np.abs(out[tag + "g_" + k]).max()) for k in F.PARAMS))
    # fp32 and fp64 select the same neighbours: the gaps of both graphs, and the fp32 reference's patterns above
    assert all(_check_knn_gap(f, k) for f, k in zip((v, t), ks))
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = gen_smore(tmp)
    # two files, each under the size limit of a committed file: the data, the init and case A; case B
    second = {k: out.pop(k) for k in list(out) if k.startswith(("B_", "traj"))}
    for name, d in (("smore_tiny.npz", out), ("smore_tiny_B.npz", second)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")
    print("seed", out["data_seed"], "isolated items", out["n_isolated"])


if __name__ == "__main__":
    main()
