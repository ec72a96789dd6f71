"""eprecon_amd.optim.FusedAdam (csrc/optim.hip) against clip_grad_norm_ + torch.optim.Adam on float64 host copies.

The yardstick of every accuracy check is torch's own fp32 device path on the same inputs: the error of FusedAdam against
float64 may be at most twice that path's error plus k * 2^-24 * max(1, max |x|) after k steps (one rounding of the stored
value per step).  Errors are maxima over the whole parameter set.  The norm is held to a relative 2^-22 of the float64
norm: the squares are exact in double, the n * 2^-53 of their sum is negligible, and one rounding to float remains.
"""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 27 * 96 * 96]
VIEW = 1000            # floats of the parameter that is a view one float into its storage: the scalar path
FROZEN = 100
NONCONTIG = SIZES.index(256)      # this parameter is [16, 16] and gets a transposed (non-contiguous) gradient
N_STEPS = 10
SNAPSHOTS = (1, 2, 3, 10)
LR = 1e-3


class Problem:
    """seeded values ~N(0, 1) and, per step, gradients of magnitudes 1e-6 .. 1e2 (fp32, host)"""

    def __init__(self, seed=20):
        gen = torch.Generator().manual_seed(seed)
        self.n = SIZES + [VIEW]
        self.values = [torch.randn(n, generator=gen) for n in self.n]
        self.frozen = torch.randn(FROZEN, generator=gen)
        self.grads = [[torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 8.0 - 6.0) for n in self.n]
                      for _ in range(N_STEPS)]
        self.norms = [float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs))) for gs in self.grads]

    def gradients(self, k, mode):
        """step k's gradients; mode "inactive": scaled so that their norm is 0.5"""
        scale = 0.5 / self.norms[k] if mode == "inactive" else 1.0
        return [(g.double() * scale).float() for g in self.grads[k]]

    def parameters(self, device, dtype):
        ps = []
        for i, v in enumerate(self.values):
            v = v.to(device=device, dtype=dtype)
            if i == len(self.values) - 1:
                store = torch.zeros(VIEW + 1, device=device, dtype=dtype)
                store[1:] = v
                ps.append(torch.nn.Parameter(store[1:]))
            else:
                ps.append(torch.nn.Parameter(v.reshape(16, 16).clone() if i == NONCONTIG else v.clone()))
        frozen = torch.nn.Parameter(self.frozen.to(device=device, dtype=dtype).clone(), requires_grad=False)
        return ps, frozen


@pytest.fixture(scope="module")
def prob():
    return Problem()


def set_grads(ps, grads, skip=()):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if i in skip:
            p.grad = None
            continue
        g = g.to(device=p.device, dtype=p.dtype)
        if i == NONCONTIG:
            g = g.reshape(16, 16).t().contiguous().t()
            assert not g.is_contiguous()
        elif i == len(ps) - 1:           # the view's gradient is one float into its storage too: the norm's scalar path
            store = torch.zeros(VIEW + 1, device=p.device, dtype=p.dtype)
            store[1:] = g
            g = store[1:]
        p.grad = g


def flat(ps, opt, key):
    out = []
    for p in ps:
        t = p.detach() if key == "p" else opt.state[p][key] if key in opt.state.get(p, {}) else torch.zeros_like(p)
        out.append(t.detach().double().cpu().reshape(-1))
    return torch.cat(out)


def run(kind, prob, mode="active", wd=0.0, steps=N_STEPS, skip_at=None, skip=(), finish="launch", nan_at=None):
    """kind: "f64" (the witness, host), "torch" (fp32, device), "fused".  -> {step: {"p", "exp_avg", "exp_avg_sq"} as
    float64 host vectors}, norms, the optimiser, the parameters, the frozen tensor"""
    from eprecon_amd.optim import FusedAdam
    device, dtype = ("cpu", torch.float64) if kind == "f64" else ("cuda", torch.float32)
    ps, frozen = prob.parameters(device, dtype)
    every = ps + [frozen]
    max_norm = None if mode == "off" else 1.0
    if kind == "fused":
        opt = FusedAdam(every, lr=LR, weight_decay=wd, finish=finish)
    else:
        opt = torch.optim.Adam(every, lr=LR, weight_decay=wd)
    snaps, norms = {}, []
    for k in range(steps):
        grads = prob.gradients(k, mode)
        if nan_at is not None and k == nan_at[0]:
            grads[nan_at[1]][nan_at[2]] = float("nan")
        set_grads(ps, grads, skip if k == skip_at else ())
        if kind == "fused":
            norm = opt.clip_and_step(max_norm)
        else:
            norm = torch.nn.utils.clip_grad_norm_(every, max_norm) if max_norm is not None else None
            opt.step()
        norms.append(None if norm is None else norm.detach().clone())
        if k + 1 in SNAPSHOTS or k + 1 == steps:
            snaps[k + 1] = {key: flat(ps, opt, key) for key in ("p", "exp_avg", "exp_avg_sq")}
    return snaps, norms, opt, ps, frozen


def check_against_witness(got, yard, want, k, what):
    for key in ("p", "exp_avg", "exp_avg_sq"):
        err = float((got[key] - want[key]).abs().max())
        err_torch = float((yard[key] - want[key]).abs().max())
        bound = 2.0 * err_torch + k * 2.0 ** -24 * max(1.0, float(want[key].abs().max()))
        print(f"{what} k={k} {key}: fused {err:.3e} torch-fp32 {err_torch:.3e} bound {bound:.3e}")
        assert err <= bound, (what, k, key, err, err_torch, bound)


@pytest.fixture(scope="module")
def witnesses(prob):
    """the float64 witness and torch's fp32 device run of every (mode, wd): computed once, read by the tests below"""
    out = {}
    for mode in ("active", "inactive", "off"):
        for wd in (0.0, 1e-2):
            out[mode, wd] = (run("f64", prob, mode, wd), run("torch", prob, mode, wd))
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("mode", ["active", "inactive", "off"])
def test_values_and_norm_against_float64(prob, witnesses, mode, wd):
    (want, want_norms, *_), (yard, *_ ) = witnesses[mode, wd]
    got, norms, opt, ps, frozen = run("fused", prob, mode, wd)
    for k in SNAPSHOTS:
        check_against_witness(got[k], yard[k], want[k], k, f"{mode} wd={wd}")
    assert torch.equal(frozen.detach().cpu(), prob.frozen) and frozen not in opt.state
    if mode == "off":
        assert all(n is None for n in norms)
        return
    for n, w in zip(norms, want_norms):
        rel = abs(float(n.double()) - float(w)) / float(w)
        print(f"{mode} wd={wd} norm {float(n):.9g} float64 {float(w):.17g} rel {rel:.3e}")
        assert n.is_cuda and n.dtype == torch.float32 and rel <= 2.0 ** -22
    if mode == "active":
        assert float(want_norms[0]) > 100.0
    else:
        assert abs(float(want_norms[0]) - 0.5) < 1e-6


def test_gradients_stay_unclipped(prob):
    ps, frozen = prob.parameters("cuda", torch.float32)
    from eprecon_amd.optim import FusedAdam
    opt = FusedAdam(ps + [frozen], lr=LR)
    grads = prob.gradients(0, "active")
    set_grads(ps, grads)
    opt.clip_and_step(1.0)
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad.cpu().reshape(-1), g)


def test_skipped_gradients(prob):
    skip = tuple(range(0, len(SIZES) + 1, 3))
    want, _, wopt, wps, _ = run("f64", prob, steps=3, skip_at=1, skip=skip)
    yard, *_ = run("torch", prob, steps=3, skip_at=1, skip=skip)
    one, *_ = run("fused", prob, steps=1)
    two, _, opt, ps, frozen = run("fused", prob, steps=2, skip_at=1, skip=skip)
    got, _, opt, ps, frozen = run("fused", prob, steps=3, skip_at=1, skip=skip)
    check_against_witness(got[3], yard[3], want[3], 3, "skip")
    assert [float(opt.state[p]["step"]) for p in ps] == [float(wopt.state[p]["step"]) for p in wps]
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0 if i in skip else 3.0 for i in range(len(ps))]
    # step 2 left the skipped tensors and their moments as step 1 had them, bit for bit
    at = np.cumsum([0] + prob.n)
    for i in skip:
        for key in ("p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(one[1][key][at[i]:at[i + 1]], two[2][key][at[i]:at[i + 1]]), (i, key)
    assert torch.equal(frozen.detach().cpu(), prob.frozen)


def test_zero_gradients_change_nothing(prob):
    from eprecon_amd.optim import FusedAdam
    ps, frozen = prob.parameters("cuda", torch.float32)
    before = [p.detach().clone() for p in ps]
    opt = FusedAdam(ps + [frozen], lr=LR)
    for _ in range(2):
        set_grads(ps, [torch.zeros(n) for n in prob.n])
        norm = opt.clip_and_step(1.0)
        assert float(norm) == 0.0
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)
        assert torch.isfinite(opt.state[p]["exp_avg"]).all() and torch.isfinite(opt.state[p]["exp_avg_sq"]).all()


def test_nan_gradient_spreads_as_in_torch(prob):
    nan_at = (1, len(SIZES) - 1, 77)
    yard, *_ = run("torch", prob, steps=2, nan_at=nan_at)
    got, norms, *_ = run("fused", prob, steps=2, nan_at=nan_at)
    assert torch.isnan(norms[1]) and not torch.isnan(norms[0])
    for key in ("p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(torch.isnan(got[2][key]), torch.isnan(yard[2][key])), key
        assert torch.isnan(got[2][key]).any()


def test_two_runs_give_the_same_bits(prob):
    a, na, *_ = run("fused", prob, wd=1e-2, steps=3)
    b, nb, *_ = run("fused", prob, wd=1e-2, steps=3)
    c, nc, *_ = run("fused", prob, wd=1e-2, steps=3, finish="resum")
    for other, norms in ((b, nb), (c, nc)):
        for key in ("p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[3][key], other[3][key]), key
        assert all(torch.equal(x, y) for x, y in zip(na, norms))


@pytest.mark.parametrize("first", ["fused", "torch"])
def test_state_interchanges_with_torch_adam(prob, first):
    """three steps with one class, its state_dict loaded into the other, two more steps with both"""
    from eprecon_amd.optim import FusedAdam
    (want, *_), (yard, *_) = run("f64", prob, steps=5), run("torch", prob, steps=5)
    _, _, opt, ps, frozen = run(first, prob, steps=3)
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps[:-1]]
    store = torch.zeros(VIEW + 1, device="cuda")
    store[1:] = ps[-1].detach()
    ps2.append(torch.nn.Parameter(store[1:]))
    frozen2 = torch.nn.Parameter(frozen.detach().clone(), requires_grad=False)
    other = (torch.optim.Adam if first == "fused" else FusedAdam)(ps2 + [frozen2], lr=LR)
    other.load_state_dict(copy.deepcopy(opt.state_dict()))     # (load_state_dict keeps tensors that need no cast: no sharing)
    for p in ps2:
        st = other.state[p]
        assert float(st["step"]) == 3.0 and st["step"].dtype == torch.float32 and not st["step"].is_cuda
        assert st["exp_avg"].dtype == torch.float32 and st["exp_avg"].is_cuda
    for k in (3, 4):
        for o, params in ((opt, ps), (other, ps2)):
            set_grads(params, prob.gradients(k, "active"))
            if isinstance(o, FusedAdam):
                o.clip_and_step(1.0)
            else:
                torch.nn.utils.clip_grad_norm_(params, 1.0)
                o.step()
    for o, params, what in ((opt, ps, first), (other, ps2, "loaded from " + first)):
        got = {key: flat(params, o, key) for key in ("p", "exp_avg", "exp_avg_sq")}
        check_against_witness(got, yard[5], want[5], 5, what)
        assert all(float(o.state[p]["step"]) == 5.0 for p in params)


def test_unsupported_parameters_are_named():
    from eprecon_amd.optim import FusedAdam
    with pytest.raises(ValueError, match="float64"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64, device="cuda"))])
    with pytest.raises(ValueError, match="cpu"):
        FusedAdam([("layer.weight", torch.nn.Parameter(torch.zeros(4)))])
    with pytest.raises(ValueError, match="layer.weight"):
        FusedAdam([("layer.weight", torch.nn.Parameter(torch.zeros(4)))])
    FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64), requires_grad=False),
               torch.nn.Parameter(torch.zeros(4, device="cuda"))])


def test_train_step_runs_on_the_fused_optimizer():
    from eprecon_amd.fragment_step import TrainStep
    from eprecon_amd.optim import FusedAdam
    s = TrainStep(seed=0, lr=2e-6, height=240, width=320, optimizer="fused")
    assert isinstance(s.optimizer, FusedAdam)
    before = {n: p.detach().clone() for n, p in s.net.named_parameters()}
    versions = {n: p._version for n, p in s.net.named_parameters()}
    a = s.run()
    # norm (with its finish launch, if that is the form in use), update and the ONE repack of every operand-order weight copy: the step's writes are known to autograd
    # (the version counters the weight caches key on), so nothing is left stale for the next forward
    assert s.optimizer.launches == (4 if s.optimizer.finish == "launch" else 3)
    assert all(p._version > versions[n] for n, p in s.net.named_parameters() if p.grad is not None)
    from eprecon_amd.sparse import repack_registered
    assert repack_registered() == 0
    b = s.run()
    assert np.isfinite(a["total_loss"]) and np.isfinite(b["total_loss"])
    assert any(not torch.equal(p.detach(), before[n]) for n, p in s.net.named_parameters())
