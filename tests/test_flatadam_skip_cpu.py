"""FlatAdam.step skips a slab whose model marks it as having no gradient this step (Slab.has_grad = False), as
torch.optim.Adam skips a parameter whose .grad is None: the data, both moments and the step counter stay.  An unmarked
slab steps exactly as before.  The HIP update (gmr_adam_f32) is replaced by its arithmetic in fp32 torch, so the test
runs without a GPU; what it checks is the host side: which slabs are stepped, with which step number."""
import numpy as np
import torch

from gmr import slab as S


def _adam_fp32(param, grad, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """gmr.kernels.adam: csrc/optim.hip's update, every product and sum rounded on its own."""
    f = np.float32
    step_size, bc2_sqrt = f(lr / (1.0 - beta1 ** step)), f((1.0 - beta2 ** step) ** 0.5)
    g = grad if weight_decay == 0.0 else grad + f(weight_decay) * param
    m.copy_(m + f(1.0 - f(beta1)) * (g - m))
    v.copy_(v * f(beta2) + f(1.0 - f(beta2)) * g * g)
    param.copy_(param - step_size * (m / (torch.sqrt(v) / bc2_sqrt + f(eps))))


def _parent_step(opt):
    """FlatAdam.step as it was before has_grad: every slab, every call."""
    for s, st in zip(opt.slabs, opt.state):
        st["step"] += 1
        S.K.adam(s.data, s.grad, st["exp_avg"], st["exp_avg_sq"], opt.lr, opt.betas[0], opt.betas[1], opt.eps,
                 opt.weight_decay, st["step"])


def _slabs(seed):
    g = torch.Generator().manual_seed(seed)
    a = S.Slab([("E", (7, 64), None)], "cpu")
    b = S.Slab([("W", (5, 10), 12), ("b", (5,), None), ("mw", (2,), None)], "cpu")
    for s in (a, b):
        s.data.copy_(torch.randn(s.numel, generator=g))
    return a, b


def _grads(slabs, seed):
    g = torch.Generator().manual_seed(seed)
    for s in slabs:
        s.grad.copy_(torch.randn(s.numel, generator=g))


def _snap(opt):
    return [(s.data.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"])
            for s, st in zip(opt.slabs, opt.state)]


def _same(x, y):
    return all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(x, y))


def test_has_grad_defaults_to_true():
    a, _ = _slabs(0)
    assert a.has_grad is True


def test_marked_slab_keeps_data_moments_and_step(monkeypatch):
    monkeypatch.setattr(S.K, "adam", _adam_fp32)
    new, old = S.FlatAdam(_slabs(1), lr=1e-3), S.FlatAdam(_slabs(1), lr=1e-3)
    # step 1: both slabs step, as the parent's loop does, bit for bit
    for opt in (new, old):
        _grads(opt.slabs, 10)
    new.step()
    _parent_step(old)
    assert all(_same(x, y) for x, y in zip(_snap(new), _snap(old)))
    # steps 2 and 3: the second slab is marked; a zero gradient in its twin must not decay its moments
    before = _snap(new)[1]
    new.slabs[1].has_grad = False
    for k in (11, 12):
        _grads(new.slabs[:1], k)
        _grads(old.slabs[:1], k)
        new.slabs[1].grad.zero_()
        new.step()
        _parent_step(_View(old, 0))
    after = _snap(new)[1]
    assert _same(before, after) and after[3] == 1
    assert _same(_snap(new)[0], _snap(old)[0]) and new.state[0]["step"] == 3
    # step 4: unmarked again, it takes its second step (step counter 2, not 4)
    new.slabs[1].has_grad = True
    _grads(new.slabs, 13)
    _grads(old.slabs, 13)
    new.step()
    _parent_step(old)
    assert new.state[1]["step"] == 2 and new.state[0]["step"] == 4
    assert all(_same(x, y) for x, y in zip(_snap(new), _snap(old)))


class _View:
    """The parent's loop over a subset of an optimiser's slabs."""

    def __init__(self, opt, idx):
        self.slabs, self.state = [opt.slabs[idx]], [opt.state[idx]]
        self.lr, self.betas, self.eps, self.weight_decay = opt.lr, opt.betas, opt.eps, opt.weight_decay


def test_unmarked_slabs_follow_torch_adam(monkeypatch):
    """The stand-in is torch.optim.Adam's arithmetic: three steps of both slabs against torch's single-tensor Adam."""
    monkeypatch.setattr(S.K, "adam", _adam_fp32)
    opt = S.FlatAdam(_slabs(2), lr=1e-3)
    ps = [torch.nn.Parameter(s.data.clone()) for s in opt.slabs]
    ref = torch.optim.Adam(ps, lr=1e-3, foreach=False)
    for k in range(3):
        _grads(opt.slabs, 20 + k)
        for p, s in zip(ps, opt.slabs):
            p.grad = s.grad.clone()
        opt.step()
        ref.step()
    for p, s in zip(ps, opt.slabs):
        np.testing.assert_allclose(s.data.numpy(), p.detach().numpy(), rtol=1e-6, atol=1e-7)


def test_state_dict_round_trip_keeps_per_slab_steps(monkeypatch):
    monkeypatch.setattr(S.K, "adam", _adam_fp32)
    opt = S.FlatAdam(_slabs(3), lr=1e-3)
    _grads(opt.slabs, 30)
    opt.step()
    opt.slabs[1].has_grad = False
    opt.step()
    sd = opt.state_dict()
    assert [st["step"] for st in sd["state"]] == [2, 1]
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    other = S.FlatAdam(_slabs(3), lr=1e-3)
    other.load_state_dict(sd)
    assert [st["step"] for st in other.state] == [2, 1]
    assert all(torch.equal(a["exp_avg"], b["exp_avg"]) for a, b in zip(other.state, opt.state))
