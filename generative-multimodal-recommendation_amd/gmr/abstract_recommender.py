"""Model base classes — mirror common/abstract_recommender.py of the reference.

GeneralRecommender(config, dataloader) reads n_users / n_items from the dataloader's dataset
and loads the modality features (image/text) as fp32 device tensors
(reference abstract_recommender.py:75-103).  Feature files are read with numpy's safe
loader (allow_pickle=False); in-memory datasets may carry the arrays directly.

EmbeddingRecommender is the base of the models whose scores are usr[users] @ itm^T over fp32 tables (VBPR, FREEDOM,
BM3, MGCN, DDRM and the RF models on them): the autograd bridge of calculate_loss, the scoring paths and the small
host helpers those models share.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import kernels as K
from .kernels import ptr, stream


def r4(n):
    """n rounded up to a multiple of 4: fp32 rows padded to 16 bytes."""
    return (n + 3) // 4 * 4


def config_seed(config):
    """The run's seed: the first of a seed list, 0 when unset."""
    s = config["seed"]
    return int((s[0] if isinstance(s, (list, tuple)) else s) or 0)


def sort_plan(keys, key_add):
    """The sorted-scatter plan of one batch (gmr_sort_batch_keys): keys, the int32 index vectors of B rows each;
    key_add, the table row offset of each (a tuple, or an int32 device tensor kept by the caller).  Padded to the
    next power of two."""
    nk, B, dev = len(keys), keys[0].numel(), keys[0].device
    kt = torch.stack(keys).contiguous()
    offs = torch.tensor([0, B], dtype=torch.int64, device=dev)
    ka = key_add if torch.is_tensor(key_add) else torch.tensor(key_add, dtype=torch.int32, device=dev)
    n2 = 1 << max(1, (nk * B - 1).bit_length())
    plan = torch.empty((1, n2), dtype=torch.int64, device=dev)
    _lib.call("gmr_sort_batch_keys", 1, ptr(kt), ptr(offs), ptr(ka), nk, B, ptr(plan), n2, n2, stream())
    return plan[0]


def copy64(src, dst, res=None):
    """dst = src over n x 64 views of any row stride, + res on the last res.shape[0] rows (gmr_frd_mean_fwd with one
    layer)."""
    n = src.shape[0]
    _lib.call("gmr_frd_mean_fwd", n, n - res.shape[0] if res is not None else n, 1,
              (ctypes.c_void_p * 1)(src.data_ptr()), (ctypes.c_int64 * 1)(src.stride(0)), ptr(res),
              res.stride(0) if res is not None else 0, ptr(dst), dst.stride(0), stream())


class AbstractRecommender(nn.Module):
    def pre_epoch_processing(self):
        pass

    def post_epoch_processing(self):
        pass

    def calculate_loss(self, interaction):
        raise NotImplementedError

    def predict(self, interaction):
        raise NotImplementedError

    def full_sort_predict(self, interaction):
        raise NotImplementedError

    def __str__(self):
        n = sum(int(np.prod(p.size())) for p in self.parameters())
        return super().__str__() + "\nTrainable parameters: {}".format(n)


class GeneralRecommender(AbstractRecommender):
    def __init__(self, config, dataloader):
        super().__init__()
        self.USER_ID = config["USER_ID_FIELD"]
        self.ITEM_ID = config["ITEM_ID_FIELD"]
        self.NEG_ITEM_ID = (config["NEG_PREFIX"] or "neg__") + (self.ITEM_ID or "")
        self.n_users = dataloader.dataset.get_user_num()
        self.n_items = dataloader.dataset.get_item_num()
        self.batch_size = config["train_batch_size"]
        self.device = config["device"]
        self.v_feat, self.t_feat = None, None
        if not config["end2end"] and config["is_multimodal_model"]:
            ds = dataloader.dataset
            v = getattr(ds, "v_feat", None)
            t = getattr(ds, "t_feat", None)
            if v is None and t is None:
                path = os.path.abspath((config["data_path"] or "") + (config["dataset"] or ""))
                vf = os.path.join(path, config["vision_feature_file"] or "")
                tf = os.path.join(path, config["text_feature_file"] or "")
                if os.path.isfile(vf):
                    v = np.load(vf, allow_pickle=False)
                if os.path.isfile(tf):
                    t = np.load(tf, allow_pickle=False)
            if v is not None:
                self.v_feat = torch.as_tensor(np.asarray(v, np.float32)).to(self.device)
            if t is not None:
                self.t_feat = torch.as_tensor(np.asarray(t, np.float32)).to(self.device)
            assert self.v_feat is not None or self.t_feat is not None, "Features all NONE"


class _StepLoss(torch.autograd.Function):
    """calculate_loss as an autograd node: rec_step has left every gradient in the slab's twin."""

    @staticmethod
    def forward(ctx, model, users, pos, neg, *params):
        loss = model.rec_step(users, pos, neg)
        ctx.model = model
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        return (None, None, None, None, *[gv * g for gv in ctx.model.grad_views()])


class EmbeddingRecommender(GeneralRecommender):
    """A model with rec_step / grad_views over one Slab and forward_embeddings() -> (usr, itm).  Registers no
    parameter, buffer or submodule of its own: parameters() is the model's."""
    LOSS_ROWS = 3  # rows of the interaction calculate_loss reads: users, pos, neg (BM3 has no negatives: 2)

    def _params(self):
        """The parameters in grad_views() order (every model registers them in the reference's order)."""
        return list(self.parameters())

    def calculate_loss(self, interaction):
        users, pos, neg = ([interaction[i].to(torch.int32).contiguous() for i in range(self.LOSS_ROWS)] + [None])[:3]
        params = self._params()
        for p in params:
            p.grad = None
        return _StepLoss.apply(self, users, pos, neg, *params)

    def _proj_bwd(self, name, dT):
        """The gradients of one modality's projection T = name_trs(name_embedding) from dT."""
        s = self.slab
        K.gemm(dT, s.view(name + "_embedding"), s.gview(name + "_W"), trans_a=True)   # dW = dT^T raw
        K.colsum(dT, s.gview(name + "_b"))                                              # db
        K.gemm(dT, s.view(name + "_W"), s.gview(name + "_embedding"))                   # draw = dT W

    @torch.no_grad()
    def topk_from_embeddings(self, usr, itm, users_i32, mask_rows, mask_cols, k, out_idx, scores_buf, out_val=None):
        E = users_i32.numel()
        ub = scores_buf.new_empty((E, usr.shape[1]))
        K.gather_rows(usr, users_i32, ub)
        sc = scores_buf[:E, :self.n_items]
        K.gemm(ub, itm, sc, trans_b=True)
        K.mask_scores(sc, mask_rows, mask_cols)
        K.topk_rows(sc, k, out_idx, out_val)
        return out_idx

    @torch.no_grad()
    def full_sort_predict(self, interaction, *draws, **draws_kw):
        """Scores of the users of interaction[0]; draws go to forward_embeddings (injected noise)."""
        users = interaction[0].to(torch.int32).contiguous()
        usr, itm = self.forward_embeddings(*draws, **draws_kw)
        E = users.numel()
        ub = torch.empty((E, usr.shape[1]), device=self.device)
        K.gather_rows(usr, users, ub)
        scores = torch.empty((E, self.n_items), device=self.device)
        K.gemm(ub, itm, scores, trans_b=True)
        return scores
