"""Training through the bf16-operand solve on the GPU (options={'precision': 'bf16', 'bf16_grad': True}, SNSDE_FLAG_BF16_GRAD):
the states against the inference kernel (bit for bit), the gradients against fp64 autograd through the straight-through reference
(tests/bf16_grad_reference.py) with the float32 run of the same reference as the yardstick, what separates them from the fp32
training solve, the split parameter pass, the refusals, a wrapper training step and a captured graph.
Cases and references: tests/bf16_grad_cases.py (the float32 yardstick of every case is checked on the CPU first,
tests/test_bf16_grad_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests import bf16_grad_cases as K
from tests.helpers import make_problem, param_spec

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
ON = {'precision': 'bf16', 'bf16_grad': True}
SELECTED = K.selected()


class _ReplayBM:
    def __init__(self, dW):
        self.dW, self.n = dW, 0

    def __call__(self, ta, tb):
        i, self.n = self.n, self.n + 1
        return self.dW[i]


def _field(pr, grad=True, zero_weights=False):
    m = S.Diffusion_model(pr['C'], pr['H'], pr['H'], pr['NL'], input_option=pr['io'], noise_option=pr['no'])
    sd = {k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()}
    if zero_weights:      # every weight matrix of the drift MLP; biases, theta and the diffusion's parameters kept
        sd = {k: (torch.zeros_like(v) if k.endswith('weight') and not k.startswith('noise') else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m = m.to(DEV).requires_grad_(grad)
    times = torch.from_numpy(pr['times']).to(DEV)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), times)
    return m, times


def _solve(pr, method, dW=None, grad=True, options=ON, zero_weights=False):
    """-> (model, y0, ys) of one sdeint on the case's inputs (supplied increments, or Philox with options['seed'])"""
    m, times = _field(pr, grad, zero_weights)
    y0 = torch.from_numpy(pr['y0']).to(DEV).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        ys = S.sdeint(m, y0, times, dt=1.0, method=method, bm=None if dW is None else _ReplayBM(torch.from_numpy(dW).to(DEV)),
                      options=dict(options))
    return m, y0, ys


def _grads(pr, method, dW, G, options=ON, zero_weights=False):
    m, y0, ys = _solve(pr, method, dW, True, options, zero_weights)
    (ys * torch.from_numpy(G).to(DEV)).sum().backward()
    out = {'y0': y0.grad.detach().clone()}
    for n, p in m.named_parameters():
        out[n] = torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()
    return ys.detach(), out


# ---- 1. the states are the inference kernel's --------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SELECTED, ids=K.case_id)
def test_states_equal_the_inference_solve_bitwise(case):
    pr, ts, dW, _ = K.inputs(case)
    _, _, train = _solve(pr, case[7], dW, True)
    assert type(train.grad_fn).__name__.startswith('_FusedSolve') and train.grad_fn.call.desc.flags & engine._lib.FLAG_BF16_GRAD
    assert train.grad_fn.call.act_save is not None
    _, _, infer = _solve(pr, case[7], dW, False, {'precision': 'bf16'})
    assert torch.equal(train.detach(), infer)
    _, _, train = _solve(pr, case[7], None, True, dict(ON, seed=77))
    _, _, infer = _solve(pr, case[7], None, False, {'precision': 'bf16', 'seed': 77})
    _, _, other = _solve(pr, case[7], None, False, {'precision': 'bf16', 'seed': 78})
    assert torch.equal(train.detach(), infer) and (case[1] == 0 or not torch.equal(infer, other))


# ---- 2. the gradients --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', SELECTED, ids=K.case_id)
def test_gradients_against_the_straight_through_reference(case):
    """dL/dy0 and every parameter gradient of L = (ys * G).sum() against fp64 autograd through the reference on the same increments:
    relative L2 <= max(4 e32, 1e-4) per tensor, e32 = the float32 run of the same reference against fp64 (4x: the project's
    criterion; 1e-4: what tests/test_gpu_bf16.py pins for the same one-bf16-ulp operand flips on the forward of these
    shapes).  Rows whose dL/dy0 leaves the reference by more than ROW_TOL of the batch maximum are set aside - at most
    KINK_ROWS_FRAC * B + 1 of them - and taken out of the loss in a second pass (tests/bigcase.py's rule).
    The reference rounds the float32 folded products the prepare launch forms (bf16_grad_reference: folded='prepare'), the numbers
    both passes of the library multiply; with fp64 products instead, a folded weight of typical size that rounds to the other bf16
    neighbour moved ten of 23 and 19 of 64 rows beyond ROW_TOL (Training).
    SNSDE_BF16_GRAD_MARGINS names a file the measured ratios are appended to (profiles/bf16_grad_margins.txt is such a run: worst
    tensor at 0.25 of its bound, five cases with one row set aside, none with more)."""
    pr, ts, dW, G = K.inputs(case)
    ys64, g64, g32 = K.reference(case)
    ys, got = _grads(pr, case[7], dW, G)
    rows = K.kink_rows(got['y0'], g64['y0'])
    # where the rows set aside come from: the forward states of those rows against the arbiter's (an operand that rounded to the
    # other bf16 neighbour moves the row's trajectory by ~2^-9 of one product, and everything behind it)
    fdev = ((ys.double().cpu() - ys64).abs().amax(dim=(0, 2)) / ys64.abs().amax(dim=(0, 2)).clamp(min=1.0)).numpy()
    keep = np.setdiff1d(np.arange(case[3]), rows)
    print(K.case_id(case), 'kink rows (first pass)', rows, 'cap', K.kink_cap(case[3]), '| forward deviation of a row from the arbiter, max over '
          f'its states / max(1, |y|): rows kept median {np.median(fdev[keep]):.1e} max {fdev[keep].max():.1e}'
          + (f'; rows set aside min {fdev[list(rows)].min():.1e} median {np.median(fdev[list(rows)]):.1e}' if rows else ''))
    if rows and len(rows) <= case[3] // 2:
        G2 = G.copy()
        G2[:, list(rows), :] = 0.0
        _, g64, g32 = K.reference(case, rows)
        _, got = _grads(pr, case[7], dW, G2)
    report, bad = [], {}
    for n, ref in g64.items():
        if float(ref.abs().max()) == 0.0:
            assert float(got[n].abs().max()) == 0.0, n
            continue
        assert bool(torch.isfinite(got[n]).all()), n
        e, e32 = K.rel_l2(got[n], ref), K.rel_l2(g32[n], ref)
        bound = max(4 * e32, 1e-4)
        report.append(f'{K.case_id(case)} rows_set_aside={len(rows)} {n} rel_l2={e:.3e} e32={e32:.3e} bound={bound:.3e} ratio={e / bound:.3f}')
        if e > bound:
            bad[n] = (e, bound)
    print('\n'.join(report))
    if os.environ.get('SNSDE_BF16_GRAD_MARGINS'):
        with open(os.environ['SNSDE_BF16_GRAD_MARGINS'], 'a') as fh:
            fh.write('\n'.join(report) + '\n')
    assert len(rows) <= K.kink_cap(case[3]), rows
    assert not bad, bad


# ---- 3. it is not the fp32 gradient ------------------------------------------------------------------------------------------------

def test_parameter_gradients_differ_from_the_fp32_training_solve():
    case = K.K2_CASES[0]
    pr, ts, dW, G = K.inputs(case)
    ys16, g16 = _grads(pr, 'euler', dW, G)
    ys32, g32 = _grads(pr, 'euler', dW, G, options={})
    assert not torch.equal(ys16, ys32)
    for n in g16:
        if n != 'y0' and float(g32[n].abs().max()) > 0:
            assert not torch.equal(g16[n], g32[n]), n


@pytest.mark.parametrize('method', ['euler', 'milstein'])
def test_zero_drift_weights_give_the_fp32_gradients_bitwise(method):
    """Every drift weight matrix zero: no operand is left in the forward or in the adjoint, so dL/dy0 and the gradients of the
    diffusion's parameters (theta, noise_t) are the fp32 training solve's to the bit."""
    pr, ts, dW, G = K.inputs(K.K2_CASES[0])
    ys16, g16 = _grads(pr, method, dW, G, zero_weights=True)
    ys32, g32 = _grads(pr, method, dW, G, options={}, zero_weights=True)
    assert torch.equal(ys16, ys32) and float(g16['y0'].abs().max()) > 0
    for n in g16:
        if n == 'y0' or n == 'theta' or n.startswith('noise'):
            assert torch.equal(g16[n], g32[n]) and float(g16[n].abs().max()) > 0, n


# ---- 4. the split parameter pass ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', [K.K2_CASES[1]] + SELECTED[2:5], ids=K.case_id)
def test_split_parameter_pass_equals_the_fused_call(case):
    pr, ts, dW, G = K.inputs(case)
    _, a = _grads(pr, case[7], dW, G)
    _, b = _grads(pr, case[7], dW, G, options=dict(ON, param_pass='split'))
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ---- 5. refusals and the wrapper ---------------------------------------------------------------------------------------------------

def test_refusals_raise_and_launch_nothing(monkeypatch):
    launched = []
    monkeypatch.setattr(engine.SolveCall, 'launch', lambda self, *a, **k: launched.append(1))
    for case, kw, opts in (((4, 17, 2, 16, 64, 5, 6, 'srk'), {}, {}), ((4, 18, 2, 16, 64, 5, 6, 'euler'), {}, {}),
                           ((4, 17, 2, 16, 256, 5, 6, 'euler'), {}, {}), ((4, 17, 2, 16, 32, 5, 6, 'euler'), {}, {}),
                           ((4, 17, 2, 16, 64, 5, 6, 'euler'), dict(samples=2), dict(samples=2)),
                           ((4, 17, 2, 16, 64, 5, 6, 'euler'), dict(samples=2, sample_grad=True), dict(samples=2, sample_grad=True)),
                           ((4, 17, 2, 16, 64, 5, 6, 'euler'), dict(kernel='generic'), dict(kernel='generic')),
                           ((4, 17, 2, 16, 64, 5, 6, 'euler'), dict(kernel='mfma16'), dict(kernel='mfma16')),
                           ((4, 17, 2, 16, 64, 5, 6, 'euler'), dict(bf16_grad=False), None)):
        io, no, NL, B, H, C, L, method = case
        assert K.mode(case, **kw) == 0, (case, kw)
        pr = make_problem(3, io, no, NL, B, H, C, L)
        m, times = _field(pr)
        y0 = torch.from_numpy(pr['y0']).to(DEV).requires_grad_(True)
        with pytest.raises(ValueError):
            S.sdeint(m, y0, times, dt=1.0, method=method, options=dict(ON, **opts) if opts is not None else {'precision': 'bf16'})
    assert K.mode((4, 13, 2, 16, 64, 5, 6, 'euler'), table=True) == 0 and K.mode((4, 17, 2, 16, 64, 5, 6, 'euler'), kl_column=3) == 0
    # the tutorial-field variants (activation / drift output / diffusion output / raw time switches of include/snsde.h)
    times6 = np.arange(6, dtype=np.float32)
    grid6 = engine.StepGrid(times6, 1.0, times6, None)
    for switches in (dict(activation=1), dict(drift_output=1), dict(diffusion_output=1), dict(time_feature=1), dict(activation=2, drift_output=1)):
        model = engine.model_struct(5, 64, 64, 2, 4, 0, **switches)
        assert engine.backward_mode(model, 16, 6, grid6, 'euler', precision='bf16', bf16_grad=True) == 0, switches
        assert engine.forward_path(model, 16, 6, 5, precision='bf16', bf16_grad=True, training=True) == 'none', switches
    pr = make_problem(3, 4, 17, 2, 16, 64, 5, 6)
    m, times = _field(pr)
    y0 = torch.from_numpy(pr['y0']).to(DEV)
    for extra in (dict(recompute=2), dict(param_pass='torch'), dict(backend='torch')):
        with pytest.raises(ValueError):
            S.sdeint(m, y0, times, dt=1.0, method='euler', options=dict(ON, **extra))
    with pytest.raises(ValueError):      # strict or not: never the tensor-op loop, never an f32 kernel
        S.sdeint(m, y0, times, dt=1.0, method='srk', options=dict(ON, strict=False))
    m.coeffs.requires_grad_(True)
    with pytest.raises(ValueError, match='control path'):
        S.sdeint(m, y0, times, dt=1.0, method='euler', options=ON)
    assert not launched


def test_library_refuses_training_planes_and_coefficient_gradients():
    """The C ABI itself, no Python guard in front: a supplied noise_table or a path-integral column with the training planes is
    refused by the forward launch under both flags, and snsde_coeff_gradients returns SNSDE_ERR_UNSUPPORTED after a bf16_grad
    solve whose adjoint and parameter pass ran."""
    pr = make_problem(3, 4, 13, 2, 16, 64, 5, 6)
    ts = pr['times']
    model = engine.model_struct(5, 64, 64, 2, 4, 13)
    flat = torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in param_spec(4, 13, 2, 5, 64)])).to(DEV)
    coeffs, y0 = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['y0']).to(DEV)
    grid = engine.step_grid(ts, 1.0, pr['times'], torch.device(DEV))
    kw = dict(seed=3, save_traj=True, save_act=True, precision='bf16', bf16_grad=True)
    table = torch.rand(grid.N, 64, device=DEV)
    for extra in (dict(noise_table=table), dict(kl_column=(3, 0.0, 0.0))):
        with pytest.raises(engine._lib.SnsdeError) as exc:
            engine.SolveCall(model, flat, coeffs, grid, y0, **dict(kw, **extra)).launch()
        assert exc.value.code == engine._lib.SNSDE_ERR_UNSUPPORTED
    with pytest.raises(engine._lib.SnsdeError) as exc:      # the training planes without the second flag: as before
        engine.SolveCall(model, flat, coeffs, grid, y0, **dict(kw, bf16_grad=False)).launch()
    assert exc.value.code == engine._lib.SNSDE_ERR_UNSUPPORTED
    call = engine.SolveCall(model, flat, coeffs, grid, y0, **kw)
    ys = call.launch()
    assert engine.backward_supported(call) == 1
    adj, gflat, delta = engine.backward_with_gradients(call, torch.ones_like(ys), return_delta=True)
    assert delta is not None and bool(torch.isfinite(gflat).all()) and float(gflat.abs().max()) > 0
    with pytest.raises(engine._lib.SnsdeError) as exc:
        engine.coeff_gradients(call, adj, delta)
    assert exc.value.code == engine._lib.SNSDE_ERR_UNSUPPORTED


def test_wrapper_training_step():
    B, Cn, H, L = 24, 5, 64, 9
    rng = np.random.default_rng(4)
    times = torch.arange(L, dtype=torch.float32, device=DEV)
    X = torch.from_numpy((rng.standard_normal((B, L, Cn)) * 0.1).cumsum(1).astype(np.float32)).to(DEV)
    coeffs = S.torchcde.hermite_cubic_coefficients_with_backward_differences(X, times)
    fi = torch.from_numpy(rng.integers(1, L, size=B)).to(DEV)
    torch.manual_seed(5)
    func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=17)
    net = S.NeuralSDE(func, Cn, H, 2).to(DEV).train()
    out = net(times, (coeffs,), fi, method='euler', options=dict(ON, seed=21))
    out.square().sum().backward()
    for n, p in func.named_parameters():
        if not n.startswith('noise') and n != 'theta':
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    assert float(net.initial_network.weight.grad.abs().max()) > 0


# ---- 6. hipGraph -------------------------------------------------------------------------------------------------------------------

def test_captured_forward_and_backward_replay_to_the_eager_gradient():
    pr = make_problem(21, 4, 17, 2, 96, 128, 21, 12)
    m, times = _field(pr)
    y0 = torch.from_numpy(pr['y0']).to(DEV).requires_grad_(True)
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((len(pr['times']), 96, 128)).astype(np.float32)).to(DEV)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    params = list(m.parameters())

    def step():
        ys = S.sdeint(m, y0, times, dt=0.5, method='euler', options=dict(ON, seed=seed))
        return torch.autograd.grad((ys * G).sum(), [y0] + params, allow_unused=True)

    eager = [None if g is None else g.clone() for g in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    for t in static:
        if t is not None:
            t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0].abs().max()) > 0
    for a, b in zip(static, eager):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
