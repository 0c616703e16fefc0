"""The solve chain on poisoned allocations (tests/buffer_arena.py: poisoned_allocations): every torch.empty / empty_like of
engine.py - ys, traj, dW_out, act_save, stage_save, adj, delta, the gradients and every workspace - returns memory filled bytewise
with 0x00, 0xFF (NaN as float, -1 as int32) or 0x3F (0.747.. as float), and what the API returns must not depend on which.

The determinism tests of the suite ("two launches, the same bits") cannot see this: their second call gets from the caching allocator
the block the first call freed, still holding the first call's correct values, so an element a kernel forgot to write, or a
workspace word it read before writing, looks fine.  Here the claim is bit equality across the three fills, or it is nothing: no
tolerance.  Only what the API returns is compared; the regions of act_save / stage_save and of the workspaces that
csrc/snsde_save_layout.h documents as unused are not.

Forward, inference: one Philox-driven launch per forward kernel (kernel_cases.STEP_OFFSET_CASES).  Training: one case per adjoint
kernel (kernel_cases.POISONED_TRAINING_CASES) through sdeint and .backward().  tests/test_kernel_census_cpu.py holds both tables
to the kernels they name; every launch here asserts its kernels again on the descriptor it launched.  Every test asserts that the
proxy filled something, so a refactor that allocates past it fails loudly (tests/test_buffer_arena_cpu.py scans engine.py for that).

No kernel waits on or counts in a word of global memory (no global atomics, no spin loops in csrc/; the two hipMemsetAsync calls
zero outputs), so a poisoned workspace can change values, never make a kernel wait."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests import kernel_cases as K
from tests.buffer_arena import FILLS, bits, poisoned_allocations, same_bits
from tests.helpers import assert_kernels, launched_kernels, make_problem, param_spec
from tests.test_gpu_step_offset import _Problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
SEED = 0x0123_4567_89AB_CDEF


def _assert_same(got, want, what):
    """Two dicts of tensors (or None), bit for bit."""
    assert got.keys() == want.keys(), what
    for k in want:
        a, b = got[k], want[k]
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert same_bits(a, b), f'{what}: {k} depends on what the allocations held ' \
                                    f'({int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()} elements differ)'


def _over_fills(run, what):
    """run() -> dict of tensors, once under each fill; everything equal to the 0x00 run bit for bit."""
    first = None
    for fill in FILLS:
        with poisoned_allocations(engine, fill) as proxy:
            out = run()
            torch.cuda.synchronize()
        assert proxy.count > 0, f'{what}: no allocation went through the proxy'
        out = {k: (None if v is None else v.detach().clone()) for k, v in out.items()}
        if first is None:
            first = out
            assert any(v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in out.values()), what
        else:
            _assert_same(out, first, f'{what} fill {fill:#04x}')
    return first


@pytest.mark.parametrize('case', K.STEP_OFFSET_CASES, ids=[c.test for c in K.STEP_OFFSET_CASES])
def test_inference_on_every_forward_kernel(case):
    p = _Problem(case)

    def run():
        call = p.call(p.grid, p.y0)      # (SolveCall allocates ys and the workspace)
        assert_kernels(call, fwd=case.fwd)
        # the poison is where the kernel will write: before the launch every byte of ys and of the workspace holds the fill
        assert all(bool((bits(t) == engine.torch.fill).all()) for t in (call.ys, call.workspace))
        return dict(ys=call.launch())
    out = _over_fills(run, case.test)
    assert bool(torch.isfinite(out['ys']).all())


def _flat(pr):
    spec = param_spec(pr['io'], pr['no'], pr['NL'], pr['C'], pr['H'])
    return torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in spec])).to(DEV)


def _model(c, pr, coeffs_grad=False):
    m = S.Diffusion_model(c.C, c.H, c.H, c.NL, input_option=c.io, noise_option=c.no)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(DEV)
    coeffs = torch.from_numpy(pr['coeffs']).to(DEV).requires_grad_(coeffs_grad)
    m.set_X(coeffs, torch.from_numpy(pr['times']).to(DEV))
    return m, coeffs


@pytest.mark.parametrize('case', K.POISONED_TRAINING_CASES, ids=[c.test for c in K.POISONED_TRAINING_CASES])
def test_training_on_every_adjoint_kernel(case):
    c = case
    pr = make_problem(7100 + c.H + c.B, c.io, c.no, c.NL, c.B, c.H, c.C, c.L)
    ts = torch.from_numpy(np.asarray(c.ts, np.float32)).to(DEV)
    w = torch.from_numpy(np.random.default_rng(c.H + c.B).standard_normal((len(c.ts), c.B, c.H)).astype(np.float32)).to(DEV)
    want_coeffs = c.rev not in ('w4_fused', 'generic')      # the adjoints that leave delta planes (snsde_coeff_gradients reads them)

    def run():
        m, coeffs = _model(c, pr, want_coeffs)
        y0 = torch.from_numpy(pr['y0']).to(DEV).requires_grad_(True)
        with launched_kernels() as ran:
            ys = S.sdeint(m, y0, ts, method=c.method, dt=c.dt, options={'seed': SEED, 'strict': True, 'kernel': c.kernel})
            (ys * w).sum().backward()
        assert (ran.fwd, ran.rev) == ([c.fwd], [c.rev]), (ran.fwd, ran.rev, 'meant', (c.fwd, c.rev))
        out = dict(ys=ys, y0_grad=y0.grad, **{name: q.grad for name, q in m.named_parameters()})
        if want_coeffs:
            out['coeffs_grad'] = coeffs.grad
        return out
    out = _over_fills(run, c.test)
    assert out['y0_grad'] is not None and float(out['y0_grad'].abs().max()) > 0
    assert sum(v is not None for k, v in out.items() if k not in ('ys', 'y0_grad', 'coeffs_grad')) >= 4
    if want_coeffs and c.io not in (1, 3, 5):      # (those drifts do not read X: no path to the coefficients)
        assert out['coeffs_grad'] is not None


def test_the_small_probes_and_the_two_call_backward():
    """engine.initial_state, engine.eval_fg, and solve_backward -> param_gradients -> coeff_gradients (the two-call form of the
    backward, which hands the adjoint's workspace and delta planes from one call to the next)."""
    c = K.POISONED_TRAINING_CASES[-1]
    assert c.test == 'lean / general'
    pr = make_problem(7300, c.io, c.no, c.NL, c.B, c.H, c.C, c.L)
    model = engine.model_struct(c.C, c.H, c.H, c.NL, c.io, c.no)
    flat, coeffs, y0 = _flat(pr), torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['y0']).to(DEV)
    grid = engine.step_grid(np.asarray(c.ts, np.float32), c.dt, pr['times'], torch.device(DEV))
    gen = torch.Generator(device=DEV).manual_seed(5)
    weight, bias = torch.randn(c.H, c.C, device=DEV, generator=gen), torch.randn(c.H, device=DEV, generator=gen)
    gy = torch.randn(len(c.ts), c.B, c.H, device=DEV, generator=gen)

    _over_fills(lambda: dict(z0=engine.initial_state(weight, bias, coeffs, grid)), 'initial_state')

    def fg():
        f, g = engine.eval_fg(model, flat, coeffs, pr['times'], np.float32(2.5), y0)
        return dict(f=f, g=g)
    _over_fills(fg, 'eval_fg')

    def two_calls():
        call = engine.SolveCall(model, flat, coeffs, grid, y0, method=c.method, seed=11, kernel=c.kernel, save_traj=True, save_dW=True,
                                save_act=True)
        ys = call.launch()
        assert_kernels(call, fwd=c.fwd, rev=c.rev)
        adj, delta = engine.solve_backward(call, gy, save_delta=True)
        grad = engine.param_gradients(call, adj, delta)
        return dict(ys=ys, adj=adj, grad=grad, coeffs_grad=engine.coeff_gradients(call, adj, delta), traj=call.traj, dW=call.dW_out)
    _over_fills(two_calls, 'solve_backward + param_gradients + coeff_gradients')


def test_a_graph_captured_under_poison_replays_to_the_eager_bits():
    """The fills are ordinary kernels, so they are captured with the solve: every replay poisons the solve's buffers again (0xFF)
    and must give the bits of the eager run on zero-filled ones."""
    c = K.STEP_OFFSET_CASES[1]
    pr = make_problem(7400, c.io, c.no, c.NL, c.B, c.H, c.C, c.L)
    m, _ = _model(c, pr)
    y0 = torch.from_numpy(pr['y0']).to(DEV)
    ts = torch.from_numpy(np.asarray(c.ts, np.float32)).to(DEV)
    key = 1234567
    state = S.torchsde.prepare_graph_capture(DEV)
    with torch.no_grad():
        with poisoned_allocations(engine, 0x00) as zeroed:
            eager = S.sdeint(m, y0, ts, dt=c.dt, method=c.method, options={'seed': key}).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            S.sdeint(m, y0, ts, dt=c.dt, method=c.method, options={'seed': 1})
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with poisoned_allocations(engine, 0xFF) as poisoned:
            with torch.cuda.graph(g):
                static = S.sdeint(m, y0, ts, dt=c.dt, method=c.method, options={})
    assert zeroed.count > 0 and poisoned.count > 0
    for _ in range(2):
        state.fill_(key - 1)           # the recorded solve advances the key by one, then reads it
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(static, eager)
        static.zero_()
    assert bool(torch.isfinite(eager).all()) and float(eager.abs().max()) > 0
