"""Checkpoint / resume of RFBM3, in the manner of tests/test_rffreedom_resume_gpu.py: save after epoch 1 -> fresh
model and trainer -> resume -> epoch 2 equals the uninterrupted run bit for bit (same kernels, same Philox draws).
Covers BM3's parameters and its mask counter, the velocity parameters, the AdamW moments and the RF step / epoch
counters; the checkpoint is read back with torch.load(weights_only=True)."""
import numpy as np
import pytest
import torch

import rfbm3_fixture as RB

pytestmark = pytest.mark.gpu


def test_resume_continues_the_same_run(golden, tmp_path):
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    b = golden("bm3_tiny")

    def fresh():
        init_seed(999)
        m, cfg, ds, tl = RB.build_rfbm3(b, rf_dropout=0.1, checkpoint_dir=str(tmp_path))
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
    want = (m.slab.data.cpu().numpy(), gen.slab.data.cpu().numpy(), gen.exp_avg.cpu().numpy(),
            gen.exp_avg_sq.cpu().numpy(), m.extra_state())
    assert want[4]["rf_epoch"] == 2 and want[4]["rf_step"] == gen.step_ctr == want[4]["counters"]["step"] > 0

    tl2, m2, tr2 = fresh()
    path = str(tmp_path / "RFBM3-baby.pth")
    tr2.resume_checkpoint(path, train_data=tl2)
    assert tr2.start_epoch == 2 and m2._training_epoch == 1 and m2.rf_generator.epoch == 1
    assert m2._step == m2.rf_generator.step_ctr == 2 * len(tl2)
    loss, terms, rf_terms = epoch(tl2, m2, tr2, 2)
    assert loss == runs[2][0] and np.array_equal(terms, runs[2][1]) and np.array_equal(rf_terms, runs[2][2])
    g2 = m2.rf_generator
    np.testing.assert_array_equal(m2.slab.data.cpu().numpy(), want[0])
    np.testing.assert_array_equal(g2.slab.data.cpu().numpy(), want[1])
    np.testing.assert_array_equal(g2.exp_avg.cpu().numpy(), want[2])
    np.testing.assert_array_equal(g2.exp_avg_sq.cpu().numpy(), want[3])
    assert m2.extra_state() == want[4]
    ck = torch.load(path, map_location="cpu", weights_only=True)
    gg = ck["generated_graphs"]
    assert gg["rf_epoch"] == 1 and isinstance(gg["rf_step"], int) and gg["counters"]["step"] == gg["rf_step"]
    assert "rf_generator.exp_avg_sq" in ck["state_dict"]
