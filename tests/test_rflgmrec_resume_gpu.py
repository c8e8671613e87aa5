"""Checkpoint / resume of RFLGMRec, in the manner of tests/test_rfsmore_resume_gpu.py: with rf_warmup_epochs 1, save
after epoch 1 (warmed up, after one evaluation pass has advanced LGMRec's evaluation counter) -> fresh model and
trainer -> resume -> epoch 2 equals the uninterrupted run bit for bit (same kernels, same Philox draws).  Covers
LGMRec's parameters and its two Philox counters (training step, evaluation pass), the trainer's optimiser state, the
velocity parameters, the AdamW moments, the RF step / epoch counters and the warmed-up evaluation table (its Gumbel
draws are keyed on the evaluation-pass counter, its start noise on the RF step counter); the checkpoint is read back
with torch.load(weights_only=True)."""
import numpy as np
import pytest
import torch

import rflgmrec_fixture as RL

pytestmark = pytest.mark.gpu


def _opt_state(tr):
    out = []
    for st in tr.optimizer.state_dict()["state"]:   # one entry per slab: step, exp_avg, exp_avg_sq
        out += [v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v) for _, v in sorted(st.items())]
    return out


def test_resume_continues_the_same_run(golden, tmp_path):
    from gmr.trainer import Trainer
    from gmr.utils import init_seed
    f = RL.lgmrec_golden(golden)

    def fresh():
        init_seed(999)
        m, cfg, ds, tl = RL.build_rflgmrec(f, "B", rf_dropout=0.1, rf_warmup_epochs=1, checkpoint_dir=str(tmp_path))
        return tl, m, Trainer(cfg, m)

    def epoch(tl, m, tr, e):
        m.pre_epoch_processing()
        loss = tr._train_epoch(tl, e)[0]
        return loss, m.loss_terms().cpu().numpy().copy(), m.rf_loss_terms().cpu().numpy().copy()

    def table(m):
        return torch.cat([x.clone() for x in m.forward_embeddings()])

    tl, m, tr = fresh()
    tr._train_data = tl
    runs = []
    for e in range(3):
        if e == 1:
            assert not m.rf_warm()
        runs.append(epoch(tl, m, tr, e))
        if e == 1:
            assert m.rf_warm()
            mid_table = table(m)    # evaluation pass 0, mixed
            tr._save_checkpoint(1)
    gen = m.rf_generator
    n = len(tl)
    final = table(m)    # evaluation pass 1
    want = (m.slab.data.cpu().numpy(), gen.slab.data.cpu().numpy(), gen.exp_avg.cpu().numpy(),
            gen.exp_avg_sq.cpu().numpy(), m.extra_state(), _opt_state(tr), final)
    assert want[4] == {"counters": {"step": 3 * n, "eval_pass": 2}, "rf_epoch": 2, "rf_step": 3 * n}
    assert gen.step_ctr == 3 * n > 0 and np.isfinite(runs[2][0]) and np.isfinite(runs[2][2]).all()
    assert not torch.equal(want[6], mid_table)

    tl2, m2, tr2 = fresh()
    path = str(tmp_path / "RFLGMRec-baby.pth")
    tr2.resume_checkpoint(path, train_data=tl2)
    assert tr2.start_epoch == 2 and m2._training_epoch == 1 and m2.rf_generator.epoch == 1 and m2.rf_warm()
    assert m2.rf_generator.step_ctr == 2 * n and m2._step == 2 * n and m2._eval_pass == 1
    loss, terms, rf_terms = epoch(tl2, m2, tr2, 2)
    assert loss == runs[2][0] and np.array_equal(terms, runs[2][1]) and np.array_equal(rf_terms, runs[2][2])
    g2 = m2.rf_generator
    np.testing.assert_array_equal(m2.slab.data.cpu().numpy(), want[0])
    np.testing.assert_array_equal(g2.slab.data.cpu().numpy(), want[1])
    np.testing.assert_array_equal(g2.exp_avg.cpu().numpy(), want[2])
    np.testing.assert_array_equal(g2.exp_avg_sq.cpu().numpy(), want[3])
    got = _opt_state(tr2)
    assert len(got) == len(want[5]) > 0
    for a, b in zip(got, want[5]):
        np.testing.assert_array_equal(a, b)
    assert torch.equal(table(m2), want[6])
    assert m2.extra_state() == want[4]
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["generated_graphs"] == {"counters": {"step": 2 * n, "eval_pass": 1}, "rf_epoch": 1, "rf_step": 2 * n}
    assert {"rf_generator.velocity_params", "rf_generator.exp_avg", "rf_generator.exp_avg_sq"} <= set(ck["state_dict"])
