"""Checkpoint / resume of RFGRCN, in the manner of tests/test_rfmgcn_resume_gpu.py: save after epoch 1 -> fresh model
and trainer -> resume -> epoch 2 equals the uninterrupted run bit for bit (same kernels, same Philox draws).  Covers
GRCN's parameters, the 192-wide velocity parameters, the AdamW moments and the RF step / epoch counters (GRCN itself has
no counters: the extra state is the RF's alone); the checkpoint is read back with torch.load(weights_only=True)."""
import numpy as np
import pytest
import torch

import rfgrcn_fixture as RG

pytestmark = pytest.mark.gpu


def test_resume_continues_the_same_run(golden, tmp_path):
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    f = golden("grcn_tiny")

    def fresh():
        init_seed(999)
        m, cfg, ds, tl = RG.build_rfgrcn(f, "A", rf_dropout=0.1, checkpoint_dir=str(tmp_path))
        return tl, m, Trainer(cfg, m)

    def epoch(tl, m, tr, e):
        m.pre_epoch_processing()
        loss = tr._train_epoch(tl, e)[0]
        return loss, m.loss_terms().cpu().numpy().copy(), m.rf_loss_terms().cpu().numpy().copy()

    tl, m, tr = fresh()
    tr._train_data = tl
    runs = []
    for e in range(3):
        runs.append(epoch(tl, m, tr, e))
        if e == 1:
            tr._save_checkpoint(1)
    gen = m.rf_generator
    assert gen.D == 192 and gen.slab.numel == RG.N_PARAMS
    want = (m.slab.data.cpu().numpy(), gen.slab.data.cpu().numpy(), gen.exp_avg.cpu().numpy(),
            gen.exp_avg_sq.cpu().numpy(), m.extra_state())
    assert want[4] == {"rf_epoch": 2, "rf_step": 3 * len(tl)} and gen.step_ctr == 3 * len(tl) > 0
    assert np.isfinite(runs[2][0]) and np.isfinite(runs[2][2]).all()

    tl2, m2, tr2 = fresh()
    path = str(tmp_path / "RFGRCN-baby.pth")
    tr2.resume_checkpoint(path, train_data=tl2)
    assert tr2.start_epoch == 2 and m2._training_epoch == 1 and m2.rf_generator.epoch == 1
    assert m2.rf_generator.step_ctr == 2 * len(tl2)
    loss, terms, rf_terms = epoch(tl2, m2, tr2, 2)
    assert loss == runs[2][0] and np.array_equal(terms, runs[2][1]) and np.array_equal(rf_terms, runs[2][2])
    g2 = m2.rf_generator
    np.testing.assert_array_equal(m2.slab.data.cpu().numpy(), want[0])
    np.testing.assert_array_equal(g2.slab.data.cpu().numpy(), want[1])
    np.testing.assert_array_equal(g2.exp_avg.cpu().numpy(), want[2])
    np.testing.assert_array_equal(g2.exp_avg_sq.cpu().numpy(), want[3])
    assert m2.extra_state() == want[4]
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["generated_graphs"] == {"rf_epoch": 1, "rf_step": 2 * len(tl)}
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(ck["state_dict"])
