"""The plain torch restatement of the FREEDOM step (tests/freedom_fixture.py::freedom_step_ref) pinned to the
reference's golden values (freedom_tiny.npz, cases A and B), in fp32 and in fp64, at the bars of
test_freedom_gpu.py: with it pinned, the GPU tests may use its fp64 autograd at shapes the reference recorded
nothing for."""
import numpy as np
import pytest
import torch

from freedom_fixture import CASES, PARAMS, check_grads, freedom_step_ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_pinned(golden, case, dtype):
    g = golden("freedom_tiny")
    tag = case + "_"
    rows, cols = g["train_rows"], g["train_cols"]
    if case == "A":  # the reference's draw: edge ids are positions in the (user, item)-sorted edge list
        assert np.array_equal(np.lexsort((cols, rows)), np.arange(rows.size))
        rows, cols = rows[g["degree_idx"]], cols[g["degree_idx"]]
    c = CASES[case]
    r = freedom_step_ref({k: g["p_" + k] for k in PARAMS}, int(g["U"]), int(g["I"]), rows, cols, g["knn_ind_image"],
                         g["knn_ind_text"], g["users"], g["pos"], g["neg"], c["n_mm_layers"], c["n_ui_layers"],
                         dtype=dtype)
    np.testing.assert_allclose(r["loss"], g[tag + "loss"], rtol=1e-5)
    np.testing.assert_allclose(r["terms"], g[tag + "loss_terms"], rtol=1e-5)
    check_grads(r["grads"], [g[tag + "g_" + k] for k in PARAMS], show=f"{case} {dtype}")
