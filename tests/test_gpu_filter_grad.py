"""Training through the particle filter on the GPU: torchsde.sdeint_filter(..., differentiable=True).  B = 4 input rows, S = 4
particles, the lean Euler kernel at H = 32, three observations four steps apart, a Gaussian likelihood of three state components
through engine.sample_loglik(..., stats=True).

The forward values are those of the default (no_grad) filter bit for bit under the same seed and generator.  The FIVO loss
-logz[-1].mean() fills every parameter gradient, and those gradients are compared with the chain composed by hand - differentiable
sdeint pieces (sample_grad, resume_grad) and `sample_resample_tensor_ops(differentiable=True)` on the same uniforms.  The two
chains take the same ancestors (asserted first) and run the same deterministic fused adjoints between the steps, so what separates
them is the round-off of the resampling step alone, carried on linearly.  Its size per step k is the bound of
tests/test_gpu_sample_resample_grad.py on the weights w_n = e_n / P (unit = 2^-24, x_n = mx - a_n):
    rel_n = (x_n + 6) unit + BP / P + 2 unit,     delta_k = max over the rows of sum_n w_n rel_n
- the weighted mean, because every weight gradient is c w_n with one c per row: a particle far below the maximum has a large rel_n and
no weight.  The forward values the kernel hands on (logz, the resampled log_weight) differ from the statement's within the same
pieces and move the next step's weights by as much again, so a tensor's gradients may differ by
    TOL = 2 (delta_1 + delta_2 + delta_3)      of the tensor's largest entry,
formed from the weights of the run itself (about 6e-6 here; never the project's 1e-4 against float64, which both chains' common
adjoint error would need and which cancels between them).  With SNSDE_FILTER_GRAD_MARGINS set the measured differences and TOL are
appended to that file (profiles/filter_grad_margins.txt is such a run: at most 0.20 of TOL, TOL = 6.1e-6)."""
import math
import os

import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests import sample_resample_reference as R
from tests.buffer_arena import same_bits
from tests.helpers import launched_kernels, make_problem
from tests.kernel_cases import STEP_OFFSET_CASES

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

CASE = STEP_OFFSET_CASES[1]      # 'lean general': the lean 4-row-tile kernel, H = 32
ROWS, SN = 4, 4
TS = torch.tensor([0.0, 1.0, 2.0, 3.0])      # 3 observations, 4 steps of dt = 0.25 each


def step_bound(a):
    """delta_k of the docstring from the (B, S) log-weights a = log_weight + log_increment of one resampling step."""
    a = a.detach().double().cpu()
    x = a.max(dim=-1, keepdim=True).values - a
    e = torch.exp(-x)
    P = torch.cumsum(e, dim=-1)
    tot = P[:, -1:]
    BP = R.U32 * (P.sum(-1, keepdim=True) + (e * (x + 6.0)).sum(-1, keepdim=True))
    rel = (x + 6.0) * R.U32 + BP / tot + 2 * R.U32
    return float(((e / tot) * rel).sum(-1).max())


def _module():
    c = CASE
    assert c.fwd == 'lean' and c.H == 32
    pr = make_problem(9, c.io, c.no, c.NL, ROWS, c.H, c.C, 7)
    m = S.Diffusion_model(c.C, c.H, c.H, c.NL, input_option=c.io, noise_option=c.no)
    with torch.no_grad():
        for name, q in m.named_parameters():
            q.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(DEV)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    return m, torch.from_numpy(pr['y0']).to(DEV)


def _likelihood(k, yk):
    obs = torch.full((yk.shape[0] // SN, 3), 0.1 * k, device=yk.device)
    return engine.sample_loglik(yk[:, :3].contiguous(), SN, obs, std=0.5, stats=True)[1]


OPTIONS = {'samples': SN, 'seed': 77, 'kernel': CASE.kernel}


@pytest.mark.parametrize('threshold', [1.0, 0.0], ids=['always', 'never'])
def test_the_differentiable_filter(threshold):
    m, y0 = _module()
    ts = TS.to(DEV)
    gen = lambda: torch.Generator(DEV).manual_seed(5)
    m.requires_grad_(False)
    plain = S.sdeint_filter(m, y0, ts, _likelihood, method='euler', dt=0.25, options=OPTIONS, threshold=threshold, generator=gen())
    m.requires_grad_(True)
    with launched_kernels() as lk:
        r = S.sdeint_filter(m, y0, ts, _likelihood, method='euler', dt=0.25, options=OPTIONS, threshold=threshold, generator=gen(),
                            differentiable=True)
        # the forward values of the default filter, bit for bit
        for name, a, b in zip(r._fields, r, plain):
            assert same_bits(a.detach(), b), name
        assert r.logz.requires_grad and r.log_weight.requires_grad and r.ys.requires_grad
        assert not r.ancestor.requires_grad and not r.ess.requires_grad
        assert int(r.ancestor.ne(torch.arange(SN, device=DEV, dtype=torch.int32)).sum()) > 0 or threshold == 0.0
        (-r.logz[-1].mean()).backward()
    assert lk.fwd == ['lean'] and lk.rev == ['general'], (lk.fwd, lk.rev)
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    assert sum(float(g.abs().max()) > 0 for g in got.values()) >= len(got) - 1
    # the default stays what it was: an input that requires grad does not make the default filter differentiable
    assert not S.sdeint_filter(m, y0, ts, _likelihood, method='euler', dt=0.25, options=OPTIONS, threshold=threshold,
                               generator=gen()).logz.requires_grad
    # the chain by hand, the resampling in tensor ops on the same uniforms
    m.zero_grad()
    g, y, state, lw, tol = gen(), y0, None, torch.zeros(ROWS, SN, device=DEV), 0.0
    for k in (1, 2, 3):
        piece, state = S.sdeint(m, y, ts[k - 1:k + 1], dt=0.25, method='euler', options=dict(OPTIONS, sample_grad=True, resume_grad=True),
                                extra=True, extra_solver_state=state)
        assert same_bits(piece[1].detach(), plain.ys[k]), k
        u = torch.rand((ROWS,), device=DEV, dtype=torch.float32, generator=g)
        inc = _likelihood(k, piece[1])
        tol += 2 * step_bound(lw + inc)
        step = engine.sample_resample_tensor_ops(piece[1], SN, lw, inc, u, threshold, False, differentiable=True)
        assert torch.equal(step.ancestor, plain.ancestor[k]), (k, 'the two chains take the same ancestors')
        assert float((step.logz.detach() - plain.logz[k]).abs().max()) <= 1e-5 * (1 + float(plain.logz[k].abs().max()) + math.log(SN))
        y, lw = step.state, step.log_weight
    (-step.logz.mean()).backward()
    assert 1e-7 < tol < 2e-5, tol      # (a few units of float32 round-off per step: the bound is no stand-in for a loose tolerance)
    worst = []
    for n, p in m.named_parameters():
        diff, scale = float((got[n] - p.grad).abs().max()), float(p.grad.abs().max())
        line = f'threshold={threshold} {n}: |fused - by hand| {diff:.3e} of {scale:.3e} = {diff / (scale + 1e-300):.3e}, TOL {tol:.3e}'
        print(line)
        if os.environ.get('SNSDE_FILTER_GRAD_MARGINS'):
            with open(os.environ['SNSDE_FILTER_GRAD_MARGINS'], 'a') as fh:
                fh.write(line + '\n')
        worst.append((diff - tol * scale, n, diff, scale))
    assert max(worst)[0] <= 0, ('fused against the chain by hand, beyond TOL of the largest entry', tol, max(worst)[1:])
