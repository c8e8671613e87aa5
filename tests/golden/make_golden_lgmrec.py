"""Generate tests/golden/lgmrec_tiny.npz (data, case A) and lgmrec_tiny_B.npz (case B) by running the reference LGMRec
(models/lgmrec.py) on CPU.

Runs only where make_golden.py runs (it imports the reference through that module's helpers); the output is data
only.  The reference imports torch, numpy and scipy only; it needs one stand-in to run, scipy's removed
dok_matrix._update (as BM3's and FREEDOM's makers).

Every case is run twice: in fp32 as the reference computes (loss32, the Adam trajectory; its gradients give the stored
distances <case>_own_<param>), and rerun in double (the entries without a suffix: the values the tests pin).  The double
rerun is the reference's own module after .double(), with its graphs replaced by the same graphs evaluated in double
(tests/lgmrec_fixture.py's, asserted here against the reference's fp32 graphs), inv_deg kept at its fp32 value, and
its draws replaced by the ones its fp32 run drew:
  Gumbel   F.gumbel_softmax is replaced by a wrapper that draws g by torch's own formula, records it and returns
           softmax((x + g) / tau); the wrapper is asserted bit-equal to the real function under the same RNG state.
  dropout  every mask is recorded by applying the module's dropout to a tensor of ones under the RNG state of the real
           call (a softmax at tau 0.2 underflows to exactly 0, so zeros of the output say nothing).

Case A: the init as drawn under torch.manual_seed(3), n_hyper_layer 1, hyper_num 4, keep_rate 1.
Case B: its own init (hyper_num 5) with the two embedding tables times 8 and the two hyperedge weights times 2, so that
softmax rows saturate (the maker asserts an entry below 1e-30), n_hyper_layer 2, keep_rate 0.5; then three
torch.optim.Adam steps (lr 0.001) of the fp32 reference on the same batch, each with its own draws (B_g: 3 x 2 x N x H,
B_keep likewise; the first step's gradients are the case's), the parameters after the third step stored as traj3_*.
Evaluation scores use one more recorded set of Gumbel draws (<case>_g_eval).

Usage:  python tests/golden/make_golden_lgmrec.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import Cfg, MockLoader, OUT, _import_reference, coo_of, make_interactions  # noqa: E402
import lgmrec_fixture as F  # noqa: E402

U, I, DV, DT, B = 37, 41, 40, 25, 16


def gen_lgmrec():
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn
    import scipy.sparse as sp
    sp.dok_matrix._update = lambda self, d: self._dict.update(d)  # removed from scipy; lgmrec.py:76 calls it
    _import_reference()
    import models.lgmrec as lgmrec

    rng = np.random.default_rng(23)
    rows, cols = make_interactions(rng, U, I)
    keep_e = rows != U - 1                       # the last user has no interactions
    rows, cols = rows[keep_e], cols[keep_e]
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    assert len(set(rows.tolist())) < U and len(set(cols.tolist())) < I, "an empty user and an untouched item"
    v = np.abs(rng.standard_normal((I, DV))).astype(np.float32)
    t = rng.standard_normal((I, DT)).astype(np.float32)
    users = rng.integers(0, U - 1, B)
    pos = rng.integers(0, I, B)
    neg = rng.integers(0, I, B)
    users[3] = users[1]  # a user twice
    pos[5] = pos[4]      # a positive item twice
    real_gumbel = Fn.gumbel_softmax
    rec = {"g": [], "keep": []}

    def gumbel_softmax(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        state = torch.get_rng_state()
        want = real_gumbel(logits, tau, hard=hard, dim=dim)
        torch.set_rng_state(state)
        g = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
        y = ((logits + g) / tau).softmax(dim)
        assert torch.equal(y, want)
        rec["g"].append(g.detach().clone())
        return y

    lgmrec.F.gumbel_softmax = gumbel_softmax

    class Recorder(nn.Module):
        """The reference's nn.Dropout, the mask of every call recorded from a tensor of ones under the same RNG state."""

        def __init__(self, drop):
            super().__init__()
            self.drop = drop

        def forward(self, x):
            if self.training and self.drop.p > 0:
                state = torch.get_rng_state()
                rec["keep"].append((self.drop(torch.ones_like(x)) != 0).numpy().astype(np.uint8))
                torch.set_rng_state(state)
            return self.drop(x)

    class Replay(nn.Module):
        def __init__(self, masks, keep_rate):
            super().__init__()
            self.masks, self.keep_rate, self.i = masks, keep_rate, 0

        def forward(self, x):
            if not self.training or self.keep_rate >= 1.0:
                return x
            k = torch.as_tensor(self.masks[self.i]).to(x.dtype)
            self.i += 1
            return x * k * (1.0 / self.keep_rate)

    def fresh(case):
        c = Cfg(USER_ID_FIELD="userID", ITEM_ID_FIELD="itemID", NEG_PREFIX="neg__", train_batch_size=B,
                device=torch.device("cpu"), end2end=True, is_multimodal_model=True, embedding_size=64,
                feat_embed_dim=64, cf_model="lightgcn", n_ui_layers=F.N_UI_LAYERS, n_mm_layers=F.N_MM_LAYERS,
                alpha=F.ALPHA, cl_weight=F.CL_WEIGHT, reg_weight=F.REG_WEIGHT, **F.CASES[case])
        # end2end: the base class loads no feature file; the features are set before the constructor reads them
        base = lgmrec.GeneralRecommender.__init__

        def init(self, config, dataset):
            base(self, config, dataset)
            self.v_feat, self.t_feat = torch.as_tensor(v), torch.as_tensor(t)

        lgmrec.GeneralRecommender.__init__ = init
        try:
            torch.manual_seed(3)
            m = lgmrec.LGMRec(c, MockLoader(U, I, rows, cols))
        finally:
            lgmrec.GeneralRecommender.__init__ = base
        m.drop = Recorder(m.drop)
        return m

    def stack_draws(lst, N, H):
        """[iv, uv, it, ut] (the order of the reference's calls) as 2 x N x H, user rows first."""
        iv, uv, it, ut = lst
        return np.stack([np.concatenate([uv, iv]), np.concatenate([ut, it])])

    def step(m, inter, rw):
        m.zero_grad()
        ua, ia, hyper = m.forward()
        u, p, n = ua[inter[0]], ia[inter[1]], ia[inter[2]]
        bpr = m.bpr_loss(u, p, n)
        uv, iv, ut, it = hyper
        cl_u = m.ssl_triple_loss(uv[inter[0]], ut[inter[0]], ut)
        cl_i = m.ssl_triple_loss(iv[inter[1]], it[inter[1]], it)
        reg = m.reg_loss(u, p, n)
        loss = bpr + m.cl_weight * (cl_u + cl_i) + rw * reg
        loss.backward()
        terms = [bpr.item(), m.cl_weight * cl_u.item(), m.cl_weight * cl_i.item(), rw * reg.item()]
        return loss, terms, torch.cat([ua, ia]), torch.cat([torch.cat([uv, iv]), torch.cat([ut, it])], dim=1)

    out = {"U": np.int64(U), "I": np.int64(I), "train_rows": rows, "train_cols": cols, "v_feat": v, "t_feat": t,
           "users": users, "pos": pos, "neg": neg}
    inter = torch.stack([torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg)])
    R64, A64, inv64 = F.graphs_ref(U, I, rows, cols, torch.float64)
    N = U + I
    for case in ("A", "B"):
        cs, tag = F.CASES[case], case + "_"
        H = cs["hyper_num"]
        m = fresh(case)
        params = dict(m.named_parameters())
        assert [n.replace("drop.drop.", "") for n in params] == F.STATE_KEYS, list(params)
        names = {k: params[s] for k, s in zip(F.PARAMS, F.STATE_KEYS)}
        for k in F.PARAMS:
            out[tag + "init_" + k] = names[k].detach().numpy().copy()
        if case == "A":
            out["norm_adj_idx"], out["norm_adj_val"] = coo_of(m.norm_adj)
            out["adj_idx"], out["adj_val"] = coo_of(m.adj)
            out["inv_deg"] = m.num_inters[:U].numpy().reshape(-1).copy()   # an N x 1 column in the reference
            ref = F.dense_of(out["norm_adj_idx"], out["norm_adj_val"], (N, N))
            assert np.array_equal(ref != 0, A64.numpy() != 0)
            assert np.array_equal(A64.numpy().astype(np.float32), ref.astype(np.float32)), "norm_adj rounds the same"
            assert np.array_equal(F.dense_of(out["adj_idx"], out["adj_val"], (U, I)), R64.numpy())
            assert np.array_equal(out["inv_deg"].astype(np.float64), inv64.numpy())
        else:
            with torch.no_grad():
                for k in F.TABLES:
                    names[k].mul_(F.TABLE_SCALE)
                for k in F.HYPER:
                    names[k].mul_(F.HYPER_SCALE)
        want = F.case_params(out, case)
        for k in F.PARAMS:
            assert np.array_equal(names[k].detach().numpy(), want[k]), k
        start = {k: p.detach().clone() for k, p in names.items()}
        # ---- fp32, as the reference computes
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=F.LR)
        n_steps = F.ADAM_STEPS if case == "B" else 1
        gs, keeps = [], []
        for j in range(n_steps):
            rec["g"], rec["keep"] = [], []
            loss, terms, al, x = step(m, inter, m.reg_weight)
            gs.append(stack_draws([a.numpy() for a in rec["g"]], N, H))
            if cs["keep_rate"] < 1.0:
                keeps.append(stack_draws(rec["keep"], N, H))
            else:
                assert not rec["keep"]
            if j == 0:
                if case == "A":  # without dropout the assembled loss is calculate_loss's under the same RNG state
                    state = torch.get_rng_state()
                    torch.manual_seed(77)
                    a = m.calculate_loss(inter).item()
                    torch.manual_seed(77)
                    b = step(m, inter, m.reg_weight)[0].item()
                    torch.set_rng_state(state)
                    assert a == b, (a, b)
                    m.zero_grad()
                    rec["g"] = []
                    loss, terms, al, x = step(m, inter, m.reg_weight)
                    gs[0] = stack_draws([a.numpy() for a in rec["g"]], N, H)
                out[tag + "loss32"] = np.float32(loss.item())
                g32 = {k: names[k].grad.numpy().copy() for k in F.PARAMS}
                m.eval()
                rec["g"] = []
                with torch.no_grad():
                    out[tag + "scores32"] = m.full_sort_predict([torch.arange(U)]).numpy()
                g_eval = stack_draws([a.numpy() for a in rec["g"]], N, H)
                m.train()
            if case == "B":
                opt.step()
        if case == "B":
            for k in F.PARAMS:
                out[f"traj{n_steps}_{k}"] = names[k].detach().numpy().copy()
            out["B_keep"] = np.stack(keeps)
            share = out["B_keep"].mean()
            assert 0.45 < share < 0.55, share
        out[tag + "g"] = np.stack(gs).astype(np.float32)
        out[tag + "g_eval"] = g_eval.astype(np.float32)
        # ---- the rerun in double
        with torch.no_grad():
            for k, p in names.items():
                p.copy_(start[k])
        m.double()
        m.norm_adj, m.adj = A64.to_sparse().coalesce(), R64.to_sparse().coalesce()
        m.num_inters = torch.cat([inv64, torch.zeros(I, dtype=torch.float64)])[:, None]
        m.drop = Replay([a for a in rec_order(keeps[0])] if keeps else [], cs["keep_rate"])
        replay = [torch.as_tensor(a).double() for a in rec_order(gs[0])]

        def replay_gumbel(logits, tau=1, hard=False, eps=1e-10, dim=-1, _i=[0]):
            gg = replay[_i[0] % 4]
            _i[0] += 1
            return ((logits + gg) / tau).softmax(dim)

        lgmrec.F.gumbel_softmax = replay_gumbel
        loss, terms, al, x = step(m, inter, m.reg_weight)
        out[tag + "loss"] = np.float64(loss.item())
        out[tag + "loss_terms"] = np.asarray(terms, np.float64)
        out[tag + "all"], out[tag + "x"] = al.detach().numpy(), x.detach().numpy()
        for k in F.PARAMS:
            gr = names[k].grad.numpy().copy()
            out[tag + "g_" + k] = gr
            out[tag + "own_" + k] = np.float64(np.abs(g32[k].astype(np.float64) - gr).max())
            print(case, k, "max |grad|", np.abs(gr).max(), "fp32 torch's distance", out[tag + "own_" + k])
        if case == "B":  # the underflow path: a probability below 1e-30 (or exactly 0) in the fp32 softmax
            P32 = {k: torch.tensor(want[k]) for k in F.PARAMS}
            f32 = F.lgmrec_forward(P32, [torch.as_tensor(v), torch.as_tensor(t)],
                                   F.graphs_ref(U, I, rows, cols, torch.float32), U, dict(cs),
                                   torch.as_tensor(out["B_g"][0]), torch.as_tensor(out["B_keep"][0]))
            smin = min(float(s.min()) for s in f32["S"])
            assert smin < 1e-30, smin
            out["B_softmax_min"] = np.float64(smin)
        m.eval()
        replay[:] = [torch.as_tensor(a).double() for a in rec_order(g_eval)]
        with torch.no_grad():
            out[tag + "scores"] = m.full_sort_predict([torch.arange(U)]).numpy()
        lgmrec.F.gumbel_softmax = gumbel_softmax
        print(case, "loss", loss.item(), "fp32", out[tag + "loss32"], "terms", out[tag + "loss_terms"])
    return out


def rec_order(st):
    """2 x N x H (user rows first) back into the reference's call order [iv, uv, it, ut]."""
    return [st[0][U:], st[0][:U], st[1][U:], st[1][:U]]


def main():
    out = gen_lgmrec()
    second = {k: out.pop(k) for k in list(out) if k.startswith(("B_", "traj"))}
    for name, d in (("lgmrec_tiny.npz", out), ("lgmrec_tiny_B.npz", second)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
