"""Generate tests/golden/lattice_tiny*.npz by running the reference LATTICE (models/lattice.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  The reference needs two things to run on a CPU: torch.Tensor.cuda as the identity (lattice.py:76,87) and a
temporary data_path for its kNN cache files, which are removed between the cases.

lattice_tiny.npz holds the data, the init (stored once: case_params() gives a case's parameters from it, and the
maker asserts that they equal the reference model's bit for bit), case A and its four-step Adam trajectory;
lattice_tiny_B.npz and lattice_tiny_C.npz hold the other cases.

Case A: both modalities, lightgcn, n_layers = 1, lambda = 0.9, the init as drawn under torch.manual_seed(3).
Case B: both modalities, lightgcn, n_layers = 2, lambda = 0.5, the two embedding tables times 8.
Case C: text only, mf, n_layers = 1, lambda = 0.9, as drawn (text_trs takes the draws that are image_trs's in A).

Every loss, gradient, item_adj and score is the reference rerun in double: the model converted with .double() and its
graphs (norm_adj, the original item graphs) rebuilt in fp64.  The fp32 reference gives the init, the trajectory
(torch.optim.Adam, lr 0.001: build, frozen, frozen, pre_epoch_processing, build) and the size of fp32's own error.

Conditions on the inputs, asserted here (the data seed is searched until they hold):
  every recorded graph (original, learned, learned again after each trajectory step) has a gap above 1e-4 between each
  row's k-th and (k+1)-th similarity and positive row sums; for every stored gradient, twice the error of the fp32
  reference against the fp64 one is below 1e-3 of the gradient's largest entry.

Usage:  python tests/golden/make_golden_lattice.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import Cfg, MockLoader, OUT, _import_reference, make_interactions  # noqa: E402
from make_golden_freedom import _check_knn_gap  # noqa: E402

CASES = {"A": dict(mods=("image", "text"), cf_model="lightgcn", n_layers=1, lambda_coeff=0.9),
         "B": dict(mods=("image", "text"), cf_model="lightgcn", n_layers=2, lambda_coeff=0.5),
         "C": dict(mods=("text",), cf_model="mf", n_layers=1, lambda_coeff=0.9)}
U, I, DV, DT, B, K = 37, 41, 40, 25, 16, 5
TABLES = ("user_embedding.weight", "item_id_embedding.weight")


class Retry(Exception):
    pass


def _need(ok, what):
    if not ok:
        raise Retry(what)


def _key(n):
    return n.replace(".", "_")


def _kth_rowsum_positive(sim, k):
    return bool((np.sort(sim, axis=1)[:, -k:].sum(1) > 0).all())


def gen_lattice(tmp, seed):
    import torch
    import models.lattice as lattice
    from utils.utils import build_knn_neighbourhood, build_sim, compute_normalized_laplacian

    rng = np.random.default_rng(seed)
    rows, cols = make_interactions(rng, U, I)
    v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
    t = rng.standard_normal((I, DT)).astype(np.float32)
    for f in (v, t):
        _need(_check_knn_gap(f, K), "raw kNN gap")
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    for d, with_image in (("tl", True), ("tc", False)):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
        if with_image:
            np.save(os.path.join(tmp, d, "image_feat.npy"), v)
        np.save(os.path.join(tmp, d, "text_feat.npy"), t)
    users = rng.integers(0, U, B)
    pos = rng.integers(0, I, B)
    neg = rng.integers(0, I, B)
    users[3] = users[1]  # a user twice
    pos[5] = pos[4]      # a positive item twice
    assert len(set(users.tolist())) < B and len(set(pos.tolist())) < B
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])

    def fresh(case):
        c = CASES[case]
        ds = "tl" if "image" in c["mods"] else "tc"
        for f in os.listdir(os.path.join(tmp, ds)):
            if f.endswith(".pt"):
                os.remove(os.path.join(tmp, ds, f))  # the reference caches the kNN graphs; every model builds its own
        cfg = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                  device=torch.device("cpu"), end2end=False, is_multimodal_model=True, data_path=tmp + "/", dataset=ds,
                  vision_feature_file="image_feat.npy", text_feature_file="text_feat.npy", embedding_size=64,
                  feat_embed_dim=64, weight_size=[64, 64], knn_k=K, reg_weight=1e-3, mess_dropout=[0.1, 0.1],
                  cf_model=c["cf_model"], n_layers=c["n_layers"], lambda_coeff=c["lambda_coeff"])
        torch.manual_seed(3)
        m = lattice.LATTICE(cfg, MockLoader(U, I, rows, cols))
        if case == "B":
            with torch.no_grad():
                for n, p in m.named_parameters():
                    if n in TABLES:
                        p.mul_(8.0)
        return m

    def in_double(m):
        """The model in fp64 with its graphs rebuilt in fp64."""
        m = m.double()
        coo = m.get_adj_mat().tocoo()
        m.norm_adj = torch.sparse_coo_tensor(np.vstack((coo.row, coo.col)).astype(np.int64),
                                             torch.as_tensor(coo.data.astype(np.float64)), coo.shape).coalesce()
        for name in ("image", "text"):
            if hasattr(m, name + "_embedding"):
                w = getattr(m, name + "_embedding").weight.detach()
                setattr(m, name + "_original_adj",
                        compute_normalized_laplacian(build_knn_neighbourhood(build_sim(w), topk=K)))
        return m

    def check_learned(m, what):
        """The gap and the row-sum conditions on the graph the model's current parameters give."""
        with torch.no_grad():
            w = torch.softmax(m.modal_weight.double(), 0)
            mix = 0
            for j, name in enumerate(n_ for n_ in ("image", "text") if hasattr(m, n_ + "_trs")):
                trs, emb = getattr(m, name + "_trs"), getattr(m, name + "_embedding")
                f = trs(emb.weight).double().numpy()
                _need(_check_knn_gap(f, K), what + " kNN gap, " + name)
                kept = build_knn_neighbourhood(build_sim(torch.as_tensor(f)), topk=K)
                mix = mix + (w[j] if hasattr(m, "image_trs") and hasattr(m, "text_trs") else 1.0) * kept
            _need(bool((mix.sum(-1) > 0).all()), what + " row sums")

    def lists_of(dense, k):
        """(idx, val) of the k kept entries per row, columns ascending."""
        d = dense.detach().numpy()
        idx = np.stack([np.flatnonzero(r) for r in d])
        assert idx.shape == (I, k), "a kept entry is zero"
        return idx.astype(np.int64), np.take_along_axis(d, idx, 1)

    main = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
            "users": users, "pos": pos, "neg": neg, "data_seed": np.int64(seed)}
    files = {"A": main, "B": {}, "C": {}}
    init = None
    for case, c in CASES.items():
        out, tag = files[case], case + "_"
        m32 = fresh(case)
        names = [n for n, _ in m32.named_parameters()]
        out[tag + "params"] = np.asarray([_key(n) for n in names])
        if case == "A":
            init = {n: p.detach().numpy().copy() for n, p in m32.named_parameters()}
            for n in names:
                main["init_" + _key(n)] = init[n]
        for n, p in m32.named_parameters():  # the stored init gives every case's parameters
            want = init[n] * np.float32(8.0) if case == "B" and n in TABLES else init[n]
            if case == "C" and n.startswith("text_trs"):
                main["C_init_" + _key(n)] = p.detach().numpy().copy()
            else:
                assert np.array_equal(p.detach().numpy(), want), (case, n)
        check_learned(m32, case + " learned")
        m64 = in_double(fresh(case))
        for name in c["mods"]:
            orig = getattr(m64, name + "_original_adj")
            _need(bool((orig.sum(-1) > 0).all()), "original row sums")
            out[tag + "orig_" + name + "_idx"], out[tag + "orig_" + name + "_val"] = lists_of(orig, K)
        # build step, then the frozen step (same batch, no optimiser step in between)
        for step in ("build", "frozen"):
            g32 = {}
            for m in (m32, m64):
                m.zero_grad(set_to_none=True)
                loss = m.calculate_loss(inter)
                loss.backward()
                if m is m32:
                    g32 = {n: (None if p.grad is None else p.grad.numpy().copy()) for n, p in m.named_parameters()}
            out[tag + step + "_loss"] = np.float64(loss.item())
            has = []
            for n, p in m64.named_parameters():
                has.append(p.grad is not None)
                assert (p.grad is None) == (g32[n] is None)
                if p.grad is None:
                    continue
                g64 = p.grad.numpy().copy()
                own = float(np.abs(g32[n].astype(np.float64) - g64).max())
                _need(2 * own < 1e-3 * np.abs(g64).max(), f"{case} {step} {n}: fp32 error {own:.2e} of "
                                                           f"{np.abs(g64).max():.2e}")
                out[tag + step + "_g_" + _key(n)] = g64
            out[tag + step + "_has_grad"] = np.asarray(has)
            if step == "build":
                for name in c["mods"]:
                    kept = getattr(m64, name + "_adj")  # the top-k values before the mix (lattice.py:141-148)
                    out[tag + "learn_" + name + "_idx"], out[tag + "learn_" + name + "_val"] = lists_of(kept, K)
                out[tag + "item_adj"] = m64.item_adj.detach().numpy().copy()
            else:
                graph_side = [n for n in names if n not in TABLES]
                assert [n for n, h in zip(names, has) if not h] == graph_side  # .grad is None on the graph side
        with torch.no_grad():
            out[tag + "scores"] = m64.full_sort_predict([torch.arange(U)]).numpy()
        if case == "A":
            # four Adam steps of the fp32 reference across an epoch boundary
            m = fresh(case)
            opt = torch.optim.Adam(m.parameters(), lr=0.001)
            for j, kind in enumerate(("build", "frozen", "frozen", "build")):
                if j == 3:
                    m.pre_epoch_processing()
                assert m.build_item_graph == (kind == "build")
                opt.zero_grad(set_to_none=True)
                m.calculate_loss(inter).backward()
                opt.step()
                check_learned(m, f"after step {j + 1}")
                for n, p in m.named_parameters():
                    main[f"traj{j + 1}_" + _key(n)] = p.detach().numpy().copy()
        print(case, "loss", out[tag + "build_loss"], "smallest max |grad|",
              min(float(np.abs(a).max()) for k_, a in out.items() if "_build_g_" in k_))
    return files


def main():
    _import_reference()
    import torch
    torch.Tensor.cuda = lambda self, *a, **kw: self
    for seed in range(11, 256):
        with tempfile.TemporaryDirectory() as tmp:
            try:
                files = gen_lattice(tmp, seed)
            except Retry as e:
                print("seed", seed, "rejected:", e)
                continue
        break
    else:
        raise AssertionError("no data seed satisfies the conditions")
    for case, name in (("A", "lattice_tiny"), ("B", "lattice_tiny_B"), ("C", "lattice_tiny_C")):
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **files[case])
        print("wrote", path, os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
