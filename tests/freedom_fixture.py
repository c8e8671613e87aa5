"""Shared builders of the FREEDOM GPU tests: the model on the golden tiny data (freedom_tiny.npz)."""
import numpy as np
import torch

DEV = "cuda"
PARAMS = ["user_embedding_weight", "item_id_embedding_weight", "image_embedding_weight", "image_trs_weight",
          "image_trs_bias", "text_embedding_weight", "text_trs_weight", "text_trs_bias"]
CASES = {"A": dict(n_mm_layers=1, n_ui_layers=2, dropout=0.8), "B": dict(n_mm_layers=2, n_ui_layers=3, dropout=0.0)}


def freedom_config(**over):
    from gmr.configurator import Config
    d = {"train_batch_size": 16, "eval_batch_size": 16, "seed": [999], "save_recommended_topk": False,
         "topk": [5, 10], "valid_metric": "Recall@10", "knn_k": 5, "mm_image_weight": 0.1, "reg_weight": 0.001,
         "n_mm_layers": 1, "n_ui_layers": 2, "dropout": 0.8}
    d.update(over)
    return Config("FREEDOM", "baby", d)


def build_freedom(g, case="A", rows=None, cols=None, labels=None, **over):
    """The model on the fixture's train edges (or the given interactions), constructed under
    torch.manual_seed(3) as the fixture's reference model was."""
    from gmr.dataloader import TrainDataLoader
    from gmr.dataset import RecDataset
    from gmr.freedom import FREEDOM
    cfg = freedom_config(**dict(CASES[case], **over))
    U, I = int(g["U"]), int(g["I"])
    rows = g["train_rows"] if rows is None else rows
    cols = g["train_cols"] if cols is None else cols
    labels = np.zeros(len(rows)) if labels is None else labels
    ds = RecDataset.from_arrays(cfg, rows, cols, labels, U, I, g["v_feat"], g["t_feat"])
    tl = TrainDataLoader(cfg, ds, batch_size=16)
    torch.manual_seed(3)
    return FREEDOM(cfg, tl), cfg, ds, tl


def csr_keys(a):
    """(row * n_cols + col keys in CSR order, values) of a gmr CSR, on the host."""
    rp = a.rowptr.cpu().numpy().astype(np.int64)
    col = a.col.cpu().numpy().astype(np.int64)
    row = np.repeat(np.arange(a.n_rows), np.diff(rp))
    assert rp[-1] == col.size == a.nnz
    return row * a.n_cols + col, a.val.cpu().numpy()


def coo_keys(idx, val, n_cols):
    """The same of a coalesced COO (row-major order)."""
    key = idx[0].astype(np.int64) * n_cols + idx[1]
    o = np.argsort(key, kind="stable")
    return key[o], val[o]
