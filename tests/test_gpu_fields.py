"""GPU parity of the fused path for tutorial-style fields (fields.py; reference tutorial/*.ipynb cell 7) against the
float64 tensor-op loop over the module's own f / g with the same Brownian increments.  Tolerance: the fp32 kernel vs
the fp64 loop, 2e-4 of the trajectory's scale (north_star's fp32 tolerance for the path)."""
import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import fields
from tests.helpers import grad_close, make_problem

GRAD_TOL = 1e-4      # measured <= 2.3e-5 over 887 tensors (profiles/r05_grad_margins_small.txt); it was 2e-3
from tests.tutorial_fields import COMPOSITION_CASES, TutorialField

pytestmark = pytest.mark.gpu


class Replay:
    levy_area_approximation = 'space-time'

    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb, return_U=False):
        i, self.n = self.n, self.n + 1
        return (self.dW[i], self.dU[i]) if return_U else self.dW[i]


def problem(seed, B, H, C, L, kind, layers, act, dev):
    pr = make_problem(seed, 4, 17, 2, B, H, C, L, times=np.linspace(0.0, 2.0, L))
    times = torch.from_numpy(pr['times'])
    coeffs = torch.from_numpy(pr['coeffs'])
    torch.manual_seed(seed)
    field = TutorialField(kind, C, H, layers, act)
    with torch.no_grad():
        for p in field.parameters():       # livelier than the default init, still a stable drift
            p.mul_(1.5)
    y0 = torch.rand(B, H) * 0.5 + 0.25
    return field, times, coeffs, y0


CASES = [(kind, H, layers, act, method)
         for kind in ('lsde', 'lnsde', 'lnsde_additive', 'gsde')
         for H, layers, act, method in ((32, 1, 'lipswish', 'euler'), (64, 2, 'lipswish', 'euler'), (128, 2, 'lipswish', 'euler'),
                                        (128, 1, 'silu', 'milstein'), (64, 3, 'relu', 'euler'), (32, 2, 'lipswish', 'milstein'),
                                        (64, 3, 'lipswish', 'milstein'), (256, 2, 'lipswish', 'euler'), (256, 1, 'silu', 'milstein'))]


@pytest.mark.parametrize('kind,H,layers,act,method', CASES)
def test_tutorial_field_fused_vs_fp64_loop(kind, H, layers, act, method):
    dev = torch.device('cuda')
    B, C, L = 37, 3, 11
    field, times, coeffs, y0 = problem(H + layers, B, H, C, L, kind, layers, act, dev)
    dt = 0.05
    grid = S.engine.StepGrid(times.numpy(), dt, times.numpy(), None)
    h = (grid.t1 - grid.t0).astype(np.float64)
    dW = torch.from_numpy(np.random.default_rng(3).standard_normal((grid.N, B, H)) * np.sqrt(h)[:, None, None] * 0.5)
    # float64 loop over the module's own f / g (CPU)
    f64 = TutorialField(kind, C, H, layers, act).double()
    f64.load_state_dict({k: v.double() for k, v in field.state_dict().items()})
    f64.set_X(coeffs.double(), times.double())
    with torch.no_grad():
        want = S.sdeint(f64, y0.double(), times.double(), bm=Replay(dW), dt=dt, method=method, options={'backend': 'torch'})
    # fused: must be the composed-field path (the generic stepper is disabled for the call)
    field = field.to(dev)
    field.set_X(coeffs.to(dev), times.to(dev))
    cf = fields.compose(field)
    assert cf is not None, 'tutorial-style module not recognised'
    generic = S.torchsde._sdeint_torch
    S.torchsde._sdeint_torch = lambda *a, **k: (_ for _ in ()).throw(AssertionError('fell back to the generic stepper'))
    try:
        with torch.no_grad():
            got = S.sdeint(field, y0.to(dev), times.to(dev), bm=Replay(dW.float().to(dev)), dt=dt, method=method)
    finally:
        S.torchsde._sdeint_torch = generic
    assert cf.verified.get(str(y0.to(dev).device)) is True
    assert cf.model.drift_output == (fields.DRIFT_TIMES_Y if kind == 'gsde' else fields.DRIFT_LINEAR)
    assert cf.model.noise_option == (12 if kind in ('lsde', 'lnsde_additive') else 13)
    scale = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    assert np.isfinite(scale) and err <= 2e-4 * max(scale, 1.0), (err, scale)


def test_tutorial_field_philox_rows_are_shard_invariant():
    dev = torch.device('cuda')
    B, H, C, L = 48, 64, 2, 9
    field, times, coeffs, y0 = problem(5, B, H, C, L, 'lnsde', 2, 'lipswish', dev)
    field = field.to(dev)
    with torch.no_grad():
        field.set_X(coeffs.to(dev), times.to(dev))
        full = S.sdeint(field, y0.to(dev), times.to(dev), dt=0.05, method='euler', options={'seed': 9})
        field.set_X(coeffs[16:40].to(dev), times.to(dev))
        part = S.sdeint(field, y0[16:40].to(dev), times.to(dev), dt=0.05, method='euler', options={'seed': 9, 'row_offset': 16})
    assert torch.equal(part, full[:, 16:40])


@pytest.mark.parametrize('H,layers', [(48, 1), (128, 3)])
def test_unrecognised_variants_take_the_generic_stepper(H, layers):
    dev = torch.device('cuda')
    B, C, L = 8, 2, 7        # H = 48 / (128, 3 layers): no lean-kernel instantiation -> probe fails -> generic path
    field, times, coeffs, y0 = problem(6, B, H, C, L, 'lsde', layers, 'lipswish', dev)
    field = field.to(dev)
    field.set_X(coeffs.to(dev), times.to(dev))
    dW = torch.randn(32, B, H, device=dev) * 0.1          # times span 2.0, dt = 1/16
    with torch.no_grad():
        got = S.sdeint(field, y0.to(dev), times.to(dev), bm=Replay(dW), dt=0.0625, method='euler')
        want = S.sdeint(field, y0.to(dev), times.to(dev), bm=Replay(dW), dt=0.0625, method='euler', options={'backend': 'torch', 'graph': False})
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    # a Tanh-terminated MLP is not an affine chain the kernel implements: structural reject
    field2 = TutorialField('lsde', C, 64, 1)
    field2.f_net._model.append(torch.nn.Tanh())
    assert fields.compose(field2) is None


GRAD_CASES = [(kind, H, layers, act, method)
              for kind in ('lsde', 'lnsde', 'lnsde_additive', 'gsde')
              for H, layers, act, method in ((32, 1, 'lipswish', 'euler'), (64, 2, 'lipswish', 'milstein'), (128, 2, 'silu', 'euler'),
                                             (32, 3, 'relu', 'milstein'))]
# the Neural ODE notebook's field (drift only, scalar-noise shape)
GRAD_CASES += [('ode', H, layers, act, 'euler') for H, layers, act in ((32, 2, 'lipswish'), (64, 1, 'relu'), (128, 2, 'silu'))]
# SRK (the GSDE-SRK notebook trains with it): the general kernel's SRK variant + the SRK adjoint kernel's variant switches
GRAD_CASES += [(kind, H, layers, act, 'srk') for kind in ('lsde', 'lnsde', 'lnsde_additive', 'gsde')
               for H, layers, act in ((32, 1, 'lipswish'), (64, 2, 'relu'), (128, 1, 'silu'), (64, 3, 'lipswish'))]
# NeuralSDEFunc-shaped fields (drift and diffusion both MLPs of [t, y]): Euler, the net kernels + the general adjoint kernel
GRAD_CASES += [('nsde', H, 1, act, 'euler') for H, act in ((16, 'lipswish'), (32, 'lipswish'), (64, 'relu'), (64, 'silu'),
                                                            (128, 'lipswish'), (128, 'relu'))]
# ... and under SRK (torchsde's default method): the net kernels' SRK forward with the pre-activations saved, the SRK net adjoint's
# variant switches (snsde_m4n_srk_reverse_kernel<CfgNR<.., VAR>>)
GRAD_CASES += [('nsde', H, 1, act, 'srk') for H, act in ((16, 'lipswish'), (32, 'lipswish'), (64, 'silu'), (64, 'relu'), (128, 'lipswish'),
                                                          (128, 'relu'))]
# ... and under Milstein (snsde_m4n_mil_reverse_kernel<CfgNM<.., VAR>>: the tangent's cotangent reaches the hidden pre-activation
# through the activation's SECOND derivative)
GRAD_CASES += [('nsde', H, 1, act, 'milstein') for H, act in ((16, 'lipswish'), (32, 'silu'), (64, 'lipswish'), (64, 'relu'), (128, 'lipswish'),
                                                               (128, 'silu'))]


@pytest.mark.parametrize('kind,H,layers,act,method', GRAD_CASES)
def test_tutorial_field_training_step_fused_vs_fp64_autograd(kind, H, layers, act, method):
    """loss.backward() through the fused solve of a tutorial-style field (forward + adjoint + weight-gradient kernels, the
    composition and the module's own g in autograd around them) against float64 autograd through the tensor-op loop on
    the same increments: dL/dy0 and every parameter of the module."""
    dev = torch.device('cuda')
    B, C, L = 19, 3, 9
    field, times, coeffs, y0 = problem(50 + H + layers, B, H, C, L, kind, layers, act, dev)
    dt = 0.125
    grid = S.engine.StepGrid(times.numpy(), dt, times.numpy(), None)
    h = (grid.t1 - grid.t0).astype(np.float64)
    rng = np.random.default_rng(4)
    dW = torch.from_numpy(rng.standard_normal((grid.N, B, H)) * np.sqrt(h)[:, None, None] * 0.5)
    dU = None
    if method == 'srk':       # the space-time Levy integral that goes with dW
        hc = torch.from_numpy(h)[:, None, None]
        dU = hc * (0.5 * dW + (hc / 12).sqrt() * torch.from_numpy(rng.standard_normal((grid.N, B, H))) * 0.5)
    wsum = torch.from_numpy(rng.standard_normal((L, B, H)))
    f64 = TutorialField(kind, C, H, layers, act).double()
    f64.load_state_dict({k: v.double() for k, v in field.state_dict().items()})
    f64.set_X(coeffs.double(), times.double())
    y64 = y0.double().requires_grad_(True)
    want = S.sdeint(f64, y64, times.double(), bm=Replay(dW, dU), dt=dt, method=method, options={'backend': 'torch'})
    (want * wsum).sum().backward()

    field = field.to(dev)
    field.set_X(coeffs.to(dev), times.to(dev))
    yg = y0.to(dev).requires_grad_(True)
    generic = S.torchsde._sdeint_torch
    S.torchsde._sdeint_torch = lambda *a, **k: (_ for _ in ()).throw(AssertionError('fell back to the tensor-op loop'))
    try:
        got = S.sdeint(field, yg, times.to(dev), bm=Replay(dW.float().to(dev), None if dU is None else dU.float().to(dev)), dt=dt,
                       method=method)
        (got * wsum.float().to(dev)).sum().backward()
    finally:
        S.torchsde._sdeint_torch = generic
    assert float((got.detach().double().cpu() - want.detach()).abs().max()) <= 2e-4 * max(float(want.detach().abs().max()), 1.0)

    def close(g, ref, name):
        # (round 6: scalar parameters under SRK - `time_rate` of the additive LNSDE field is -0.02 as a sum of O(1) terms over 19 x 128 x 8
        #  row-steps - measured 1.2e-4 once the block is composed natively in float32; the matrices stay at 1e-4)
        tol = 3e-4 if (method == 'srk' and ref.numel() == 1) else GRAD_TOL
        grad_close(g, ref, name, tol, 'fields')
    close(yg.grad, y64.grad, 'y0')
    ref = dict(f64.named_parameters())
    for name, p in field.named_parameters():
        gr = ref[name].grad
        if gr is None or float(gr.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6, name
            continue
        assert p.grad is not None, name
        close(p.grad, gr, name)


@pytest.mark.parametrize('kind', ['lsde', 'lnsde', 'gsde'])
def test_tutorial_workflow_trains_on_the_fused_path(kind, monkeypatch):
    """examples/tutorial_ou_process.py = the tutorial notebooks' workflow (OU data, Hermite coefficients, batch 16, hidden 32,
    ts = every knot, dt = 0.05, Adam, MSE): every solve of training and evaluation must take the fused kernels (the
    tensor-op loop is disabled), and the test error must fall."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'tutorial_ou_process.py')
    spec = importlib.util.spec_from_file_location('tutorial_ou_process', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def no_loop(*a, **k):
        raise AssertionError('the tensor-op loop ran')
    monkeypatch.setattr(S.torchsde, '_sdeint_torch', no_loop)
    hist = mod.main(['--field', kind, '--epochs', '3', '--samples', '320', '--device', 'cuda'])
    assert len(hist) == 4 and all(np.isfinite(hist)) and hist[-1] < 0.7 * hist[0], hist


def test_composed_block_and_table_caches_follow_parameter_updates():
    """Inference solves reuse the composed parameter block and the diffusion table while no parameter changed; an in-place
    update (what an optimizer step does) or a re-assigned parameter must be seen by the next solve."""
    import copy
    dev = torch.device('cuda')
    B, H, C, L = 16, 32, 2, 9
    field, times, coeffs, y0 = problem(77, B, H, C, L, 'lnsde', 1, 'lipswish', dev)
    field = field.to(dev)
    field.set_X(coeffs.to(dev), times.to(dev))

    def solve(f):
        with torch.no_grad():
            return S.sdeint(f, y0.to(dev), times.to(dev), dt=0.05, method='euler', options={'seed': 3})
    a1, a2 = solve(field), solve(field)
    assert torch.equal(a1, a2)
    cf = fields.compose(field)
    assert cf._flat_cache is not None and cf._tab_cache is not None
    with torch.no_grad():
        field.linear_out.weight.mul_(1.25)           # in-place: version counter
        field.g_net._model[0].bias.add_(0.05)
    b1 = solve(field)
    fresh = copy.deepcopy(field)
    assert fresh.__dict__['_snsde_cache'].composed is None      # the memoised mapping / device tensors do not travel with a copy
    fresh.set_X(coeffs.to(dev), times.to(dev))
    assert not torch.equal(a1, b1) and torch.equal(b1, solve(fresh))
    field.emb.bias.data.add_(0.2)                    # through .data: no version bump - caught by the content fingerprint
    fresh3 = copy.deepcopy(field)
    fresh3.set_X(coeffs.to(dev), times.to(dev))
    c1 = solve(field)
    assert not torch.equal(c1, b1) and torch.equal(c1, solve(fresh3))
    b1 = c1
    field.linear_X.weight = torch.nn.Parameter(field.linear_X.weight.detach() * 0.5)     # re-assigned parameter: new address
    fresh2 = copy.deepcopy(field)
    fresh2.set_X(coeffs.to(dev), times.to(dev))
    assert torch.equal(solve(field), solve(fresh2)) and not torch.equal(solve(field), b1)


def test_tutorial_field_solve_records_into_a_graph():
    """A no-grad solve of a composed field inside a CUDA/HIP graph capture: no host read-back (the parameter fingerprint of the
    inference cache is skipped, the composition is part of the recording), fresh increments on every replay, and a parameter
    update between replays is seen (the recorded composition re-reads the module's weights)."""
    from stable_neural_sdes_amd import torchsde as T
    dev = torch.device('cuda')
    B, H, C, L = 16, 32, 2, 9
    field, times, coeffs, y0 = problem(78, B, H, C, L, 'lnsde', 1, 'lipswish', dev)
    field = field.to(dev)
    times, y0 = times.to(dev), y0.to(dev)
    field.set_X(coeffs.to(dev), times)
    T.prepare_graph_capture(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        S.sdeint(field, y0, times, dt=0.05, method='euler')
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = S.sdeint(field, y0, times, dt=0.05, method='euler')
    g.replay(); torch.cuda.synchronize()
    a = out.clone()
    g.replay(); torch.cuda.synchronize()
    b = out.clone()
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, b)      # fresh Brownian increments
    assert torch.equal(a[0], y0) and torch.equal(b[0], y0)
    with torch.no_grad():
        field.linear_out.weight.zero_(); field.linear_out.bias.zero_()        # drift off, ...
        for m in field.g_net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.zero_(); m.bias.zero_()                               # ... diffusion factor g(t) = const
    g.replay(); torch.cuda.synchronize()
    c = out.clone()
    assert not torch.allclose(c, b)


@pytest.mark.parametrize('kind,method', [('lnsde', 'euler'), ('gsde', 'srk'), ('nsde', 'euler'), ('nsde', 'srk')])
def test_tutorial_field_training_step_records_into_a_graph(kind, method):
    """Forward + loss.backward() + Adam step of a composed field recorded into ONE CUDA/HIP graph (composition, fused solve,
    adjoint, weight-gradient pass with its side-stream fork / join, the composition's backward, the optimizer): replays draw
    fresh increments from the device-resident key, train the module, and never touch the tensor-op loop."""
    from stable_neural_sdes_amd import torchsde as T
    dev = torch.device('cuda')
    B, H, C, L = 32, 32, 2, 9
    field, times, coeffs, y0 = problem(91, B, H, C, L, kind, 1, 'lipswish', dev)
    field = field.to(dev)
    times, y0 = times.to(dev), y0.to(dev)
    field.set_X(coeffs.to(dev), times)
    target = torch.zeros(B, H, device=dev)
    opt = torch.optim.Adam(field.parameters(), lr=2e-3, capturable=True)
    torch.manual_seed(1234)                          # (the eager warm-up steps draw their keys from torch's CPU generator)
    T.prepare_graph_capture(dev).fill_(20240917)     # the recorded solves' device-resident key: the same noise whatever ran before

    def step():
        out = S.sdeint(field, y0, times, dt=0.05, method=method)
        loss = (out[-1] - target).square().mean()
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        return loss
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    generic = T._sdeint_torch
    T._sdeint_torch = lambda *a, **k: (_ for _ in ()).throw(AssertionError('fell back to the tensor-op loop'))
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_loss = step()
    finally:
        T._sdeint_torch = generic
    before = [p.detach().clone() for p in field.parameters()]
    losses = []
    for _ in range(40):
        g.replay()
        losses.append(static_loss.detach().clone())
    torch.cuda.synchronize()
    losses = [float(v) for v in losses]
    assert all(np.isfinite(losses)) and len(set(losses)) > 30, 'replays must draw fresh increments'
    assert np.mean(losses[-10:]) < np.mean(losses[:10]), losses
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, field.parameters()))


# ---- the notebooks' own vector fields (tests/golden/tutorial.npz: generated by executing tutorial/*.ipynb cell 7) ------------
from tests.helpers import group, load, params_of      # noqa: E402
TUT = load('tutorial.npz')
T1_CASES = sorted({k.split('/')[1] for k in TUT.files if k.startswith('T1/')})


@pytest.mark.parametrize('case', T1_CASES)
def test_fused_path_vs_trajectories_of_the_reference_notebooks_fields(case):
    """State_dict of the notebook's Neural{LSDE, LNSDE, GSDE}Func loaded into the test-side class (strict: same parameter
    names and shapes), solved on the fused path with the fixture's increments, against the float64 trajectory that the
    notebook's own f / g produced under the fixed-step scheme."""
    dev = torch.device('cuda')
    g = group(TUT, f'T1/{case}')
    C, H, layers = (int(v) for v in g['meta'])
    field = TutorialField(str(g['kind']), C, H, layers, str(g['activation']))
    field.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params_of(TUT, f'T1/{case}').items()}, strict=True)
    field = field.to(dev)
    times = torch.from_numpy(g['times']).to(dev)
    field.set_X(torch.from_numpy(g['coeffs']).to(dev), times)
    method = str(g['method'])
    dU = torch.from_numpy(g['dU']).to(dev) if 'dU' in g else None
    with torch.no_grad():
        ys = S.sdeint(field, torch.from_numpy(g['y0']).to(dev), times, dt=float(g['dt']), method=method,
                      bm=Replay(torch.from_numpy(g['dW']).to(dev), dU))
    cf = fields.compose(field)
    assert cf is not None and any(v is True for v in cf.verified.values()), 'the field did not take the fused path'
    B, L = g['y0'].shape[0], g['times'].shape[0]
    assert S.engine.forward_path(cf.model, B, L, g['dW'].shape[0], method=method, kernel='auto', table=cf.tabulated) != 'none', \
        f'no fused kernel for this field under {method}'
    ref = g['ys64']
    scale = np.abs(ref).max()
    err = np.abs(ys.double().cpu().numpy() - ref).max()
    assert err <= 2e-4 * max(scale, 1.0), (err, scale)
    # no further from the float64 trajectory than the float32 tensor-op evaluation of the notebook's module (x4)
    assert err <= 4 * np.abs(g['ys32'].astype(np.float64) - ref).max() + 1e-5 * scale


@pytest.mark.parametrize('kind,method', [('gsde', 'srk'), ('nsde', 'euler'), ('nsde', 'srk'), ('nsde', 'milstein')])
def test_field_training_step_at_the_timed_size_vs_fp64_autograd(kind, method):
    """The sizes tools/time_fields.py / bench.py time (1024 rows, H = 128; 40 steps here to bound the float64 loop): loss.backward()
    through the fused solve against float64 autograd through the tensor-op loop on the same increments."""
    dev = torch.device('cuda')
    B, H, C, L, n = 1024, 128, 2, 5, 40
    field, times, coeffs, y0 = problem(123, B, H, C, L, kind, 1, 'lipswish', dev)
    times = torch.linspace(0.0, 1.0, L, dtype=torch.float64)
    dt = 1.0 / n
    grid = S.engine.StepGrid(times.numpy().astype(np.float32), dt, times.numpy().astype(np.float32), None)
    h = (grid.t1 - grid.t0).astype(np.float64)
    gen = torch.Generator(device=dev).manual_seed(9)
    hc = torch.from_numpy(h).to(dev)[:, None, None]
    dW = torch.randn(grid.N, B, H, generator=gen, device=dev, dtype=torch.float64) * hc.sqrt() * 0.5
    dU = hc * (0.5 * dW + (hc / 12).sqrt() * torch.randn(grid.N, B, H, generator=gen, device=dev, dtype=torch.float64) * 0.5) if method == 'srk' else None
    wsum = torch.randn(L, B, H, generator=gen, device=dev, dtype=torch.float64)
    f64 = TutorialField(kind, C, H, 1, 'lipswish').double().to(dev)
    f64.load_state_dict({k: v.double() for k, v in field.state_dict().items()})
    f64.set_X(coeffs.double().to(dev), times.to(dev))
    y64 = y0.double().to(dev).requires_grad_(True)
    want = S.sdeint(f64, y64, times.to(dev), bm=Replay(dW, dU), dt=dt, method=method, options={'backend': 'torch'})
    (want * wsum).sum().backward()
    field = field.to(dev)
    field.set_X(coeffs.to(dev), times.float().to(dev))
    yg = y0.to(dev).requires_grad_(True)
    generic = S.torchsde._sdeint_torch
    S.torchsde._sdeint_torch = lambda *a, **k: (_ for _ in ()).throw(AssertionError('fell back to the tensor-op loop'))
    try:
        got = S.sdeint(field, yg, times.float().to(dev), bm=Replay(dW.float(), None if dU is None else dU.float()), dt=dt, method=method)
        (got * wsum.float()).sum().backward()
    finally:
        S.torchsde._sdeint_torch = generic
    assert float((got.detach().double() - want.detach()).abs().max()) <= 2e-4 * max(float(want.detach().abs().max()), 1.0)

    def close(g, ref, name):
        grad_close(g, ref, name, GRAD_TOL, 'fields-big')
    close(yg.grad, y64.grad, 'y0')
    ref = dict(f64.named_parameters())
    for name, p in field.named_parameters():
        gr = ref[name].grad
        if gr is None or float(gr.abs().max()) == 0.0:
            continue
        assert p.grad is not None, name
        close(p.grad, gr, name)


@pytest.mark.parametrize('kind,H,layers', COMPOSITION_CASES)
def test_native_block_composition_matches_the_torch_composition(kind, H, layers):
    """snsde_affine_compose / _backward (one launch each; round 6) against the torch formulation of ComposedField._flat they replace in
    training: the same parameter block to float32 round-off, and the same gradients for a random cotangent of the block."""
    dev = torch.device('cuda')
    field, times, coeffs, y0 = problem(900 + H, 7, H, 3, 9, kind, layers, 'lipswish', dev)
    field = field.to(dev)
    field.set_X(coeffs.to(dev), times.to(dev))
    cf = S.fields.compose(field)
    assert cf is not None
    cot = torch.randn(cf.numel, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    out = {}
    for native in (True, False):
        field.zero_grad(set_to_none=True)
        saved = S.fields._native_block
        if not native:
            S.fields._native_block = lambda *a, **k: None
        try:
            flat = cf.flat(dev, grad=True)
        finally:
            S.fields._native_block = saved
        assert (flat.grad_fn is not None) and (type(flat.grad_fn).__name__.startswith('_ComposeAffine') == native)
        (flat * cot).sum().backward()
        out[native] = (flat.detach().clone(), {n: p.grad.clone() for n, p in field.named_parameters() if p.grad is not None})
    fa, ga = out[True]
    fb, gb = out[False]
    assert float((fa - fb).abs().max()) <= 2e-6 * (1.0 + float(fb.abs().max()))
    assert ga.keys() == gb.keys() and len(ga) >= 8 - (2 if kind == 'lsde' else 0)
    for n in gb:
        assert float((ga[n] - gb[n]).abs().max()) <= 2e-5 * (1.0 + float(gb[n].abs().max())), n
