"""The functional restatement of the rectified-flow generator (tests/rf_fixture.py) pinned to the reference's
values at dropout 0 (tests/golden/make_golden_rffreedom.py): with it pinned, the GPU tests may use its autograd
as the expected gradient where the reference recorded none (dropout masks, other shapes)."""
import numpy as np
import pytest
import torch

import rf_fixture as R

RECORDS = [("A_", 2, 128), ("B_", 1, 64)]


@pytest.fixture(scope="module")
def g(golden):
    return R.load_golden(golden)


@pytest.mark.parametrize("tag,L,C", RECORDS)
def test_train_step_pinned(g, tag, L, C):
    assert g[tag + "cond"].shape == (78, C) and not g[tag + "cond"][:37].any()  # zero user rows
    P = {n: torch.tensor(g[tag + "p0_" + R.key(n)], requires_grad=True) for n in R.param_names(L)}
    X1, X0, t, cond, users, pos, ni, nu = R.record_inputs(g, tag)
    r = R.train_losses(P, X1, X0, t, cond, users, pos, ni, nu, 37, L)
    np.testing.assert_allclose(r["v"].detach().numpy(), g[tag + "v"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["rf_loss"].item(), g[tag + "rf_loss"], rtol=1e-5)
    np.testing.assert_allclose(r["cl_loss"].item(), g[tag + "cl_loss"], rtol=1e-5)
    for n, v in R.grads_of(P, r["total"]).items():
        want = g[tag + "g_" + R.key(n)]
        np.testing.assert_allclose(v.numpy(), want, rtol=1e-4, atol=R.grad_bar(g, tag) * np.abs(want).max(), err_msg=n)
    # one torch.optim.AdamW step on the recorded gradients gives the recorded parameters
    ps = [torch.nn.Parameter(torch.tensor(g[tag + "p0_" + R.key(n)])) for n in R.param_names(L)]
    for p, n in zip(ps, R.param_names(L)):
        p.grad = torch.tensor(g[tag + "g_" + R.key(n)])
    torch.optim.AdamW(ps, lr=float(g["lr"])).step()
    for p, n in zip(ps, R.param_names(L)):
        np.testing.assert_array_equal(p.detach().numpy(), g[tag + "p1_" + R.key(n)], err_msg=n)


@pytest.mark.parametrize("tag,L,C", RECORDS)
def test_generate_pinned(g, tag, L, C):
    P = R.params_from(g, tag, L, prefix="p1_")
    z = R.generate(P, torch.tensor(g[tag + "cond"]), torch.tensor(g[tag + "z0"]), int(g["steps"]), L)
    np.testing.assert_allclose(z.numpy(), g[tag + "gen"], rtol=0, atol=4 * float(g[tag + "err_sample"]))


def test_fixture_covers_the_collision_rule_and_duplicates(g):
    for tag in ("A_", "B_"):
        ni, pos = g[tag + "neg_items"], g[tag + "pos"]
        assert not (ni == pos[:, None]).any() and not (g[tag + "neg_users"] == g[tag + "users"][:, None]).any()
        assert any(len(set(r.tolist())) < r.size for r in ni)  # a duplicate negative within a row
    assert len(set(g["A_users"].tolist())) < 16 and len(set(g["A_pos"].tolist())) < 16  # repeated anchors
    assert R.collide(np.array([[3, 40]]), np.array([40]), 41).tolist() == [[3, 0]]  # n - 1 wraps to 0
