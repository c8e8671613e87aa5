"""The sparse slot-form restatement of tests/lattice_fixture.py against the reference's dense formulation
(tests/golden/lattice_tiny*.npz, models/lattice.py rerun in double): item_adj, the loss and every gradient of a build
step and of the frozen step after it, and the scores, to rtol 1e-9.  The slot lists hold a column several times in a
row where the image, text and original lists share it; the dense form scatters them into one entry.  That the two
agree is what lets the GPU tests take the restatement as their reference."""
import numpy as np
import pytest
import torch

import lattice_fixture as F

RTOL = 1e-9


@pytest.fixture(scope="module")
def g(golden):
    main = golden("lattice_tiny")
    return {c: (main if c == "A" else dict(main, **golden(F.FILES[c]))) for c in F.CASES}


@pytest.mark.parametrize("case", list(F.CASES))
def test_parameter_names(g, case):
    assert [str(n) for n in g[case][case + "_params"]] == F.params_of(case)


@pytest.mark.parametrize("case", list(F.CASES))
def test_lists(g, case):
    """The original and the learned lists: the same columns per row, the same values."""
    d, tag = g[case], case + "_"
    r = F.Restatement(d, case)
    r.loss(build=True)
    for j, name in enumerate(F.CASES[case]["mods"]):
        for kind, (idx, val) in (("orig", r.orig[j]), ("learn", r.lists[j][:2])):
            order = torch.argsort(idx, dim=1)
            assert np.array_equal(torch.gather(idx, 1, order).numpy(), d[tag + kind + "_" + name + "_idx"]), (kind, name)
            np.testing.assert_allclose(torch.gather(val.detach(), 1, order).numpy(),
                                       d[tag + kind + "_" + name + "_val"], rtol=RTOL, atol=0, err_msg=kind + name)
    assert (r.r > 0).all()


def test_slot_lists_hold_duplicate_columns(g):
    """The case the dense scatter form hides: a row whose lists share columns."""
    r = F.Restatement(g["A"], "A")
    r.loss(build=True)
    col = r.col.numpy()
    assert any(len(set(row.tolist())) < len(row) for row in col)


@pytest.mark.parametrize("case", list(F.CASES))
def test_steps(g, case):
    d, tag = g[case], case + "_"
    r = F.Restatement(d, case)
    names = F.params_of(case)
    for step in ("build", "frozen"):
        out = r.step(build=step == "build")
        np.testing.assert_allclose(out["loss"], d[tag + step + "_loss"], rtol=RTOL)
        if step == "build":
            np.testing.assert_allclose(r.item_adj(), d[tag + "item_adj"], rtol=RTOL, atol=1e-18)
        has = d[tag + step + "_has_grad"]
        for k, gr, h in zip(names, out["grads"], has):
            assert (gr is not None) == bool(h), (step, k)
            if h:
                want = d[tag + step + "_g_" + k]
                np.testing.assert_allclose(gr, want, rtol=RTOL, atol=1e-12 * np.abs(want).max(), err_msg=step + k)
        if step == "frozen":
            assert [k for k, h in zip(names, has) if not h] == [k for k in names if k in F.GRAPH_SIDE]
    np.testing.assert_allclose(r.scores(), d[tag + "scores"], rtol=RTOL, atol=1e-15)


def test_trajectory_in_fp32_follows_the_reference(g):
    """The four Adam steps of the fp32 restatement stay near the fp32 reference's: the size of this difference is the
    margin of the GPU trajectory test."""
    d = g["A"]
    traj = F.Restatement(d, "A", dtype=torch.float32).trajectory()
    for j, P in enumerate(traj):
        for k, v in P.items():
            want = d[f"traj{j + 1}_{k}"]
            err = np.abs(v - want).max()
            # a step moves an entry by about lr = 1e-3 times its gradient over the gradient's running size; the maker
            # holds fp32's gradient error below 1e-3 of the largest entry, so a step adds at most lr * 1e-3
            assert err <= (j + 1) * 1e-3 * 1e-3, (j, k, err)
    # the graph side does not move on the frozen steps
    for k in F.GRAPH_SIDE:
        assert np.array_equal(traj[1][k], traj[0][k]) and np.array_equal(traj[2][k], traj[0][k])
        assert np.array_equal(d["traj2_" + k], d["traj1_" + k]) and np.array_equal(d["traj3_" + k], d["traj1_" + k])
        assert not np.array_equal(d["traj4_" + k], d["traj3_" + k])
