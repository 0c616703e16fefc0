"""Training through sample paths on the GPU: options={'samples': S, 'sample_grad': True} (SNSDE_FLAG_SAMPLE_GRAD) against the
same solve with the coefficients replicated row-wise S times by hand - the parent's route - and against the fp64 tensor-op loop.

What is compared, and why it can be exact.  The sampled descriptor runs the kernels the replicated one runs (same forced kernel,
seed, row_offset and cotangent): the forward maps path p to coefficient row p / S in its prologue, the adjoint reads no
coefficients, the weight-gradient pass reduces over the same (pass, path) rows in the same order - so the states, dL/dy0 per path
and every parameter gradient are torch.equal.  The coefficient gradient is the one new sum,
    grad_coeffs[b, k, j C + c] = sum_{p : k_p = k} sum_{s < S} phi_j(r_p) v_p[b S + s, c];
with the cotangent on ONE path of every group the other paths add exact zeros, so coeffs.grad[b] must be torch.equal to the
replicated solve's row b S + s* whatever order the kernel sums in; with every path live it is held to the fp64 loop by the
project's gradient yardstick (tests/test_gpu_parity.py: max and mean relative error < 1e-4).

Shapes: the knots, output times and (io, no) -> (H, C, NL, dt) shapes of tests/test_gpu_coeff_grad.py with its row count replaced
by the (input rows, samples) pairs of tests/test_gpu_samples.py - (3,3), (2,4), (5,5), (1,7): two input rows in one 4-row tile, a
ragged last tile, a tile with a single input row - and (5,7) = 35 paths for the 16-row tiles."""
import signal
import warnings

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import grad_close, make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0], np.float32)
TS = np.array([0.0, 2.5, 6.0], np.float32)
GRAD_TOL_MAX = GRAD_TOL_MEAN = 1e-4      # (tests/test_gpu_parity.py)
PAIRS = [(3, 3), (2, 4), (5, 5), (1, 7), (5, 7)]      # (input rows B, samples S): paths = B S
# (io, no) -> (H, C, NL, dt)
SHAPES = {(4, 17): (128, 21, 2, 0.5), (2, 16): (32, 3, 1, 1.0), (6, 17): (64, 69, 2, 0.5), (0, 17): (64, 3, 2, 1.0)}


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('sample-gradient GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class _ReplayBM:
    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb, return_U=False):
        out = self.dW[self.n]
        u = self.dU[self.n] if self.dU is not None else None
        self.n += 1
        return (out, u) if return_U else out


_CASES = {}


def _case(io, no, B, Sn, method, dt=None, shape=None, seed=0):
    """Inputs of one configuration: B input rows, B S paths (y0, increments and loss weights per path).  Computed once, shared,
    never modified; the fp64 reference is added by _reference on first use."""
    H, C_, NL, dt0 = shape or SHAPES[(io, no)]
    dt = dt0 if dt is None else dt
    key = (io, no, B, Sn, method, dt, H, C_, NL, seed)
    if key in _CASES:
        return _CASES[key]
    P = B * Sn
    sd = 900 + seed + 11 * io + no + H + C_ + 7 * B + Sn
    pr = make_problem(sd, io, no, NL, B, H, C_, len(TIMES), times=TIMES)
    grid = engine.StepGrid(TS, dt, TIMES, None)
    rng = np.random.default_rng(sd)
    hh = (grid.t1 - grid.t0).astype(np.float32).reshape(-1, 1, 1)
    y0 = (0.5 * rng.standard_normal((P, H))).astype(np.float32)
    dW = (rng.standard_normal((grid.N, P, H)).astype(np.float32) * np.sqrt(hh)).astype(np.float32)
    dU = None
    if method == 'srk':
        dU = (hh * (0.5 * dW + np.sqrt(hh / 12) * rng.standard_normal(dW.shape).astype(np.float32))).astype(np.float32)
    wsum = rng.standard_normal((len(TS), P, H)).astype(np.float32)
    c = dict(pr=pr, y0=y0, dW=dW, dU=dU, wsum=wsum, grid=grid, io=io, no=no, NL=NL, B=B, S=Sn, P=P, H=H, C=C_, dt=dt, method=method)
    _CASES[key] = c
    return c


def _build(c, dtype, device, replicate, rows=None):
    """Module, y0 (per path) and the coefficient leaf: (B, ..) in place, or the hand-replicated (B S, ..) leaf."""
    pr, Sn = c['pr'], c['S']
    rows = slice(None) if rows is None else rows
    m = S.Diffusion_model(c['C'], c['H'], c['H'], c['NL'], input_option=c['io'], noise_option=c['no'])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(device=device, dtype=dtype)
    coeffs = torch.from_numpy(pr['coeffs'][rows]).to(device=device, dtype=dtype)
    if replicate:
        coeffs = coeffs.repeat_interleave(Sn, 0).contiguous()
    coeffs.requires_grad_(True)
    m.set_X(coeffs, torch.from_numpy(pr['times']).to(device))
    prow = slice(None) if rows == slice(None) else slice(rows.start * Sn, rows.stop * Sn)
    y0 = torch.from_numpy(c['y0'][prow]).to(device=device, dtype=dtype).requires_grad_(True)
    return m, y0, coeffs, prow


def _reference(c):
    """fp64 CPU tensor-op loop on replicated coefficients with the case's increments; autograd sums dL/d coeffs over S."""
    if 'ref' not in c:
        m, y0, coeffs, _ = _build(c, torch.float64, 'cpu', replicate=False)
        m.set_X(coeffs.repeat_interleave(c['S'], 0), m.times)
        bm = _ReplayBM(torch.from_numpy(c['dW']).double(), None if c['dU'] is None else torch.from_numpy(c['dU']).double())
        ys = S.sdeint(m, y0, torch.from_numpy(TS), bm=bm, method=c['method'], dt=c['dt'], options={'backend': 'torch'})
        (ys * torch.from_numpy(c['wsum']).double()).sum().backward()
        c['ref'] = dict(ys=ys.detach(), y0=y0.grad, coeffs=coeffs.grad, params={n: p.grad for n, p in m.named_parameters()})
    return c['ref']


def _assert_sampled_node(ys, c, rows_B=None):
    """1. Route: a green comparison is the fused node on the sampled descriptor with the coefficients in place."""
    node = ys.grad_fn
    assert type(node).__name__.startswith('_FusedSolve'), type(node).__name__
    assert node.mode == 1 and node.call.delta_slots > 0
    assert int(node.call.desc.samples) == c['S'] and int(node.call.desc.flags) & engine._lib.FLAG_SAMPLE_GRAD
    assert node.call.keep[1].shape[0] == (c['B'] if rows_B is None else rows_B)
    assert node.call.act_save.shape[2] == node.call.keep[1].shape[0] * c['S']      # the saved planes are per path


def _gpu(c, options, sampled, philox=False, wsum=None, rows=None, backward=True, coeff_grad=True):
    """One solve + backward on the GPU.  sampled: options samples / sample_grad on (B, ..) coefficients; else the replicated solve."""
    m, y0, coeffs, prow = _build(c, torch.float32, DEV, replicate=not sampled, rows=rows)
    if not coeff_grad:
        coeffs.requires_grad_(False)
    bm = None
    if not philox:
        dW = torch.from_numpy(c['dW'][:, prow]).to(DEV).contiguous()
        dU = None if c['dU'] is None else torch.from_numpy(c['dU'][:, prow]).to(DEV).contiguous()
        bm = _ReplayBM(dW, dU)
    opts = dict(options)
    if sampled:
        opts.update(samples=c['S'], sample_grad=True)
    if philox:
        opts.setdefault('seed', 1234)
    with warnings.catch_warnings():
        warnings.filterwarnings('error', module='stable_neural_sdes_amd')      # (no route of this file warns)
        ys = S.sdeint(m, y0, torch.from_numpy(TS).to(DEV), bm=bm, method=c['method'], dt=c['dt'], options=opts)
        if backward:
            w = c['wsum'] if wsum is None else wsum
            (ys * torch.from_numpy(w[:, prow]).to(DEV)).sum().backward()
    return m, y0, coeffs, ys


def _equal_but_coeffs(a, b, tag):
    """ys, dL/dy0 per path and every parameter gradient of two runs: torch.equal."""
    (ma, y0a, _, ysa), (mb, y0b, _, ysb) = a, b
    assert torch.equal(ysa.detach(), ysb.detach()), (tag, 'ys')
    assert y0a.grad is not None and torch.equal(y0a.grad, y0b.grad), (tag, 'y0')
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (p.grad is None) == (q.grad is None), (tag, n)
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), (tag, n)
    assert float(y0a.grad.abs().max()) > 0


def _grid(dt):
    return engine.step_grid(TS, dt, TIMES, torch.device(DEV))


# ---- 1. route -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,Sn', PAIRS)
def test_the_library_plans_the_sampled_adjoint_and_the_node_holds_the_coefficients_in_place(B, Sn):
    for (io, no), (H, C_, NL, dt) in SHAPES.items():
        model = engine.model_struct(C_, H, H, NL, io, no)
        for kernel in ('mfma4', 'mfma16'):
            for method in ('euler', 'milstein'):
                assert engine.backward_mode(model, B * Sn, len(TIMES), _grid(dt), method, kernel, samples=Sn, sample_grad=True) == 1
                assert engine.backward_mode(model, B * Sn, len(TIMES), _grid(dt), method, kernel, samples=Sn) == 0
    H, C_, NL, dt = SHAPES[(4, 17)]
    model = engine.model_struct(C_, H, H, NL, 4, 17)
    assert engine.backward_mode(model, B * Sn, len(TIMES), _grid(dt), 'euler', 'auto', samples=Sn, sample_grad=True) == 1
    assert engine.backward_mode(model, B * Sn, len(TIMES), _grid(1.0), 'srk', 'mfma4', samples=Sn, sample_grad=True) == 1
    c = _case(4, 17, B, Sn, 'euler')
    m, y0, coeffs, ys = _gpu(c, {'kernel': 'mfma4', 'strict': True, 'row_offset': 2 * Sn}, sampled=True, backward=False)
    _assert_sampled_node(ys, c)
    assert tuple(ys.shape) == (len(TS), B * Sn, H)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    assert tuple(coeffs.grad.shape) == tuple(coeffs.shape) == (B, len(TIMES) - 1, 4 * C_) and float(coeffs.grad.abs().max()) > 0


# ---- 2. bit identity with the replicated fused solve -------------------------------------------------------------------------------

@pytest.mark.parametrize('B,Sn', PAIRS)
@pytest.mark.parametrize('method', ['euler', 'milstein'])
@pytest.mark.parametrize('io,no', [(4, 17), (2, 16), (6, 17), (0, 17)])
@pytest.mark.parametrize('kernel', ['mfma4', 'mfma16'])
def test_states_and_gradients_equal_the_replicated_solve_bit_for_bit(kernel, io, no, method, B, Sn):
    c = _case(io, no, B, Sn, method)
    for philox in (True, False):
        opts = {'kernel': kernel, 'strict': True, 'row_offset': 2 * Sn}
        a = _gpu(c, opts, sampled=True, philox=philox)
        _assert_sampled_node(a[3], c)
        b = _gpu(c, opts, sampled=False, philox=philox)
        assert int(b[3].grad_fn.call.desc.samples) == 0 and b[3].grad_fn.mode == 1
        _equal_but_coeffs(a, b, f'{kernel} ({io},{no}) {method} ({B},{Sn}) philox={philox}')
        assert tuple(a[2].grad.shape) == (B, len(TIMES) - 1, 4 * c['C'])


@pytest.mark.parametrize('B,Sn', PAIRS)
@pytest.mark.parametrize('method', ['euler', 'milstein'])
def test_auto_at_128_is_the_lean_kernel_specialised_and_general(method, B, Sn):
    c = _case(4, 17, B, Sn, method)
    for philox in (True, False):
        runs = []
        for general in (False, True):
            opts = {'strict': True, 'row_offset': 2 * Sn, 'lean_general': general}
            a = _gpu(c, opts, sampled=True, philox=philox)
            _assert_sampled_node(a[3], c)
            want = 'specialised' if (philox and method == 'euler' and not general) else 'general'
            assert engine.lean_variant(a[3].grad_fn.call) == want
            b = _gpu(c, opts, sampled=False, philox=philox)      # (lean_general is the sampled route's switch: ignored here, as before)
            assert engine.lean_variant(b[3].grad_fn.call) == ('specialised' if philox and method == 'euler' else 'general')
            _equal_but_coeffs(a, b, f'auto {method} ({B},{Sn}) philox={philox} general={general}')
            runs.append(a)
        _equal_but_coeffs(runs[0], runs[1], 'specialised against general')
        assert torch.equal(runs[0][2].grad, runs[1][2].grad)


@pytest.mark.parametrize('B,Sn', PAIRS)
def test_srk_on_the_general_kernel_equals_the_replicated_solve(B, Sn):
    c = _case(4, 17, B, Sn, 'srk', dt=1.0)
    for philox in (True, False):
        opts = {'kernel': 'mfma4', 'strict': True, 'row_offset': 2 * Sn}
        a = _gpu(c, opts, sampled=True, philox=philox)
        _assert_sampled_node(a[3], c)
        b = _gpu(c, opts, sampled=False, philox=philox)
        _equal_but_coeffs(a, b, f'srk ({B},{Sn}) philox={philox}')


def test_split_parameter_pass_equals_the_fused_call():
    c = _case(4, 17, 3, 3, 'euler')
    a = _gpu(c, {'kernel': 'mfma4', 'strict': True}, sampled=True)
    b = _gpu(c, {'kernel': 'mfma4', 'strict': True, 'param_pass': 'split'}, sampled=True)
    _assert_sampled_node(b[3], c)
    _equal_but_coeffs(a, b, 'split')
    assert torch.equal(a[2].grad, b[2].grad)
    with pytest.raises(ValueError, match='sample_grad'):
        _gpu(c, {'kernel': 'mfma4', 'param_pass': 'torch'}, sampled=True)


# ---- 3. exactness of the path sum ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,Sn', [(3, 3), (2, 4)])
@pytest.mark.parametrize('method,kernel', [('euler', 'mfma4'), ('euler', 'mfma16'), ('srk', 'mfma4')])
def test_one_live_path_per_group_gives_that_paths_own_gradient_exactly(method, kernel, B, Sn):
    """The cotangent on path s* = b % S of every group, zero elsewhere: coeffs.grad[b] of the solve in place is, bit for bit, row
    b S + s* of the replicated solve's gradient, whose other rows are exactly zero.  A wrong p / S, or a sum that is not exact
    over zero terms, fails without a tolerance.  SRK at dt = 1: the stage times revisit intervals (t0 = 0 visits 0, 1, 0)."""
    c = _case(4, 17, B, Sn, method, dt=1.0 if method == 'srk' else None)
    live = np.zeros((1, B * Sn, 1), np.float32)
    for b in range(B):
        live[0, b * Sn + b % Sn, 0] = 1.0
    wsum = c['wsum'] * live
    opts = {'kernel': kernel, 'strict': True, 'row_offset': 2 * Sn}
    _, _, ca, ysa = _gpu(c, opts, sampled=True, wsum=wsum)
    _assert_sampled_node(ysa, c)
    _, _, cb, _ = _gpu(c, opts, sampled=False, wsum=wsum)
    for b in range(B):
        for s in range(Sn):
            row = cb.grad[b * Sn + s]
            if s == b % Sn:
                assert float(row.abs().max()) > 0
                assert torch.equal(ca.grad[b], row), (b, s)
            else:
                assert float(row.abs().max()) == 0.0, (b, s)


@pytest.mark.parametrize('Sn', [30, 240])
def test_many_paths_per_row_take_the_narrow_and_the_chunked_rounds(Sn):
    """C = 69 channels x S paths = the floats of one (pass, input row): 2070 at S = 30 (fewer than eight passes fit an LDS round of
    the grouped walk) and 16560 at S = 240 (past the LDS: one pass per round, in two chunks of its paths).  One live path, the last of
    the group: exact.  Every path live: the replicated solve's gradient summed over S in float64, to the project's 1e-4 (a chain
    of S fp32 terms per pass: at most S 2^-24 = 1.4e-5 relative at S = 240)."""
    c = _case(6, 17, 1, Sn, 'euler')
    opts = {'kernel': 'mfma4', 'strict': True}
    live = np.zeros((1, Sn, 1), np.float32)
    live[0, Sn - 1, 0] = 1.0
    _, _, ca, ysa = _gpu(c, opts, sampled=True, wsum=c['wsum'] * live)
    _assert_sampled_node(ysa, c)
    _, _, cb, _ = _gpu(c, opts, sampled=False, wsum=c['wsum'] * live)
    assert torch.equal(ca.grad[0], cb.grad[Sn - 1]) and float(cb.grad[:Sn - 1].abs().max()) == 0.0 and float(ca.grad.abs().max()) > 0
    _, _, ca, _ = _gpu(c, opts, sampled=True)
    _, _, ca2, _ = _gpu(c, opts, sampled=True)
    _, _, cb, _ = _gpu(c, opts, sampled=False)
    assert torch.equal(ca.grad, ca2.grad)
    grad_close(ca.grad, cb.grad.double().sum(0, keepdim=True), 'coeffs', GRAD_TOL_MAX, f'S = {Sn}')


# ---- 4. against fp64 ------------------------------------------------------------------------------------------------------------

def _compare_fp64(c, run, tag, replicated):
    m, y0, coeffs, ys = run
    ref = _reference(c)
    fscale = float(ref['ys'].abs().max()) + 1e-12
    ferr = float((ys.detach().double().cpu() - ref['ys']).abs().max()) / fscale
    g = coeffs.grad.reshape(c['B'], c['S'], *coeffs.shape[1:]).sum(1) if replicated else coeffs.grad
    e = (g.double().cpu() - ref['coeffs']).abs()
    print(f"{tag}: forward {ferr:.3e} coeffs max {float(e.max()) / float(ref['coeffs'].abs().max()):.3e} "
          f"mean {float(e.mean()) / float(ref['coeffs'].abs().mean()):.3e}")
    assert ferr < 2e-4, (tag, 'forward', ferr)
    assert tuple(g.shape) == tuple(ref['coeffs'].shape) and bool(torch.isfinite(g).all())
    grad_close(g, ref['coeffs'], 'coeffs', GRAD_TOL_MAX, tag)
    grad_close(y0.grad, ref['y0'], 'y0', GRAD_TOL_MAX, tag)
    for name, p in m.named_parameters():
        gref = ref['params'][name]
        if gref is None or float(gref.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6, name
            continue
        grad_close(p.grad, gref, name, GRAD_TOL_MAX, tag)


# the pair each shape is held to the fp64 loop at (every pair is met; (5,7) on the widest control path)
FP64_PAIR = {(4, 17): (3, 3), (2, 16): (2, 4), (6, 17): (5, 7), (0, 17): (1, 7)}
FP64_CASES = [(k, io, no, meth) for k in ('mfma4', 'mfma16') for (io, no) in SHAPES for meth in ('euler', 'milstein')] + \
             [('mfma4', 4, 17, 'srk'), ('mfma4', 4, 17, 'euler55')]


@pytest.mark.parametrize('kernel,io,no,method', FP64_CASES)
def test_against_the_fp64_loop_on_replicated_coefficients(kernel, io, no, method):
    """A seed is acceptable only if the replicated fused solve - the parent's route - passes the same comparison at it: that run
    comes first, so a failure of the yardstick on a relu kink shows there and not as a defect of the path sum."""
    B, Sn = FP64_PAIR[(io, no)]
    if method == 'euler55':
        method, (B, Sn) = 'euler', (5, 5)
    c = _case(io, no, B, Sn, method, dt=1.0 if method == 'srk' else None)
    opts = {'kernel': kernel, 'strict': True}
    tag = f'{kernel} ({io},{no}) {method} ({B},{Sn})'
    _compare_fp64(c, _gpu(c, opts, sampled=False), tag + ' replicated', True)
    run = _gpu(c, opts, sampled=True)
    _assert_sampled_node(run[3], c)
    _compare_fp64(c, run, tag + ' in place', False)


# ---- 5. empty intervals ---------------------------------------------------------------------------------------------------------

def _empty_intervals(c):
    """Intervals no drift pass falls into, from the solver's own tables."""
    grid = c['grid']
    if c['method'] == 'srk':
        tab = np.zeros((grid.N, 4, 8), np.float32)
        engine._lib.check(engine._lib.lib().snsde_grid_srk_build(grid.step_tab.ctypes.data, grid.N, grid._times32.ctypes.data,
                                                                 grid._times32.shape[0], tab.ctypes.data))
        hit = set(tab[:, (0, 3, 2), 4].copy().view(np.int32).reshape(-1).tolist())
    else:
        hit = set(grid.step_tab[:, 5].copy().view(np.int32).tolist())
    return [k for k in range(len(TIMES) - 1) if k not in hit]


@pytest.mark.parametrize('B,Sn', [(3, 3), (1, 7)])
def test_intervals_without_a_pass_get_exact_zeros(B, Sn):
    c = _case(4, 17, B, Sn, 'euler', dt=2.0, shape=(64, 3, 2, 2.0))
    assert _empty_intervals(c) == [1, 3, 5]
    run = _gpu(c, {'kernel': 'mfma4', 'strict': True}, sampled=True)
    _assert_sampled_node(run[3], c)
    g = run[2].grad
    for k in (1, 3, 5):
        assert float(g[:, k].abs().max()) == 0.0 and float(_reference(c)['coeffs'][:, k].abs().max()) == 0.0, k
    assert float(g[:, 0].abs().max()) > 0
    _compare_fp64(c, run, f'dt=2 ({B},{Sn})', False)


# ---- 6. determinism and shards --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_two_runs_and_a_shard_of_whole_groups_are_bit_equal(method):
    c = _case(4, 17, 4, 4, method, shape=(64, 21, 2, 0.5))
    _, y1, c1, ys1 = _gpu(c, {'kernel': 'mfma4', 'strict': True}, sampled=True)
    _, y2, c2, _ = _gpu(c, {'kernel': 'mfma4', 'strict': True}, sampled=True)
    assert torch.equal(c1.grad, c2.grad) and torch.equal(y1.grad, y2.grad) and float(c1.grad.abs().max()) > 0
    _, ysh, csh, yss = _gpu(c, {'kernel': 'mfma4', 'strict': True, 'row_offset': 8, 'global_rows': 16}, sampled=True, rows=slice(2, 4))
    _assert_sampled_node(yss, c, rows_B=2)
    assert torch.equal(yss.detach(), ys1.detach()[:, 8:16])
    assert torch.equal(csh.grad, c1.grad[2:4])
    assert torch.equal(ysh.grad, y1.grad[8:16])


# ---- 7. fallback ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('what,io,no,H,kernel,coeff_grad', [('wave pairs', 1, 18, 64, 'auto', False), ('diffusion net', 4, 14, 64, 'mfma4', True),
                                                            ('H = 256', 4, 17, 256, 'auto', True)])
def test_uncovered_configurations_take_the_replicated_differentiable_solve(what, io, no, H, kernel, coeff_grad):
    """No sampled adjoint route: the coefficients are replicated and the ordinary fused solve runs - no exception, no warning
    (_gpu turns warnings into errors), the states and gradients of the hand-replicated call.  (The wave-pair adjoint returns no
    coefficient gradient with or without samples: that configuration is run for y0 and the parameters.)"""
    B, Sn = 4, 3
    c = _case(io, no, B, Sn, 'euler', shape=(H, 3, 2, 1.0))
    model = engine.model_struct(3, H, H, 2, io, no)
    assert engine.backward_mode(model, B * Sn, len(TIMES), _grid(1.0), 'euler', kernel, samples=Sn, sample_grad=True) == 0
    assert engine.backward_mode(model, B * Sn, len(TIMES), _grid(1.0), 'euler', kernel) == 1
    if what == 'wave pairs':
        assert engine.forward_path(model, B * Sn, len(TIMES), _grid(1.0).N, 'euler') == 'w4'
    opts = {'kernel': kernel, 'seed': 77}
    a = _gpu(c, opts, sampled=True, philox=True, coeff_grad=coeff_grad)
    node = a[3].grad_fn
    assert type(node).__name__.startswith('_FusedSolve') and int(node.call.desc.samples) == 0 and node.call.keep[1].shape[0] == B * Sn
    # by hand: the same replication op in the graph, so autograd's sum over S is the same operation in both
    m, y0, coeffs, _ = _build(c, torch.float32, DEV, replicate=False)
    if not coeff_grad:
        coeffs.requires_grad_(False)
    m.set_X(coeffs.repeat_interleave(Sn, 0), m.times)
    ys = S.sdeint(m, y0, torch.from_numpy(TS).to(DEV), method='euler', dt=1.0, options=opts)
    (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    _equal_but_coeffs(a, (m, y0, coeffs, ys), what)
    if coeff_grad:
        assert tuple(a[2].grad.shape) == (B, len(TIMES) - 1, 12) and torch.equal(a[2].grad, coeffs.grad) and float(coeffs.grad.abs().max()) > 0


def test_the_recompute_environment_variable_takes_the_replicated_route(monkeypatch):
    """SNSDE_RECOMPUTE_STEPS is the process-wide form of options['recompute'] (which sample_grad refuses by name): recompute mode
    re-runs the forward on one coefficient row per path, so such a process trains on the replicated route - the states and gradients
    of the hand-replicated call under the same variable, and no sampled node."""
    monkeypatch.setenv('SNSDE_RECOMPUTE_STEPS', '2')
    c = _case(4, 17, 3, 3, 'euler')
    opts = {'kernel': 'mfma4', 'seed': 5}
    a = _gpu(c, opts, sampled=True, philox=True, coeff_grad=False)
    node = a[3].grad_fn
    assert type(node).__name__.startswith('_FusedSolve') and int(node.call.desc.samples) == 0 and node.recompute == 2
    assert node.call.keep[1].shape[0] == 9
    b = _gpu(c, opts, sampled=False, philox=True, coeff_grad=False)
    _equal_but_coeffs(a, b, 'recompute env')
    # with a coefficient gradient the replicated solve follows its own rule under recompute (the tensor-op loop, one warning)
    m, y0, coeffs, prow = _build(c, torch.float32, DEV, replicate=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ys = S.sdeint(m, y0, torch.from_numpy(TS).to(DEV), bm=_ReplayBM(torch.from_numpy(c['dW']).to(DEV)), method='euler', dt=c['dt'],
                      options={'kernel': 'mfma4', 'samples': 3, 'sample_grad': True})
        (ys * torch.from_numpy(c['wsum']).to(DEV)).sum().backward()
    monkeypatch.delenv('SNSDE_RECOMPUTE_STEPS')
    ref = _gpu(c, {'kernel': 'mfma4', 'strict': True}, sampled=True)
    assert tuple(coeffs.grad.shape) == tuple(coeffs.shape)
    grad_close(coeffs.grad, ref[2].grad, 'coeffs', GRAD_TOL_MAX, 'recompute env')
    grad_close(y0.grad, ref[1].grad, 'y0', GRAD_TOL_MAX, 'recompute env')


# ---- 8. wrapper -----------------------------------------------------------------------------------------------------------------

def test_wrapper_trains_through_sample_paths_back_to_the_observations():
    B, Cn, H, Sn = 5, 3, 32, 3
    rng = np.random.default_rng(9)
    X0 = torch.from_numpy((rng.standard_normal((B, len(TIMES), Cn)) * 0.3).cumsum(1).astype(np.float32)).to(DEV)
    fi = torch.tensor([6, 3, 6, 2, 4], device=DEV)
    w = torch.from_numpy(rng.standard_normal((B, 2)).astype(np.float32)).to(DEV)
    times = torch.from_numpy(TIMES).to(DEV)
    torch.manual_seed(5)
    func = S.Diffusion_model(Cn, H, H, 2, input_option=4, noise_option=17)
    net = S.NeuralSDE(func, Cn, H, 2).to(DEV).train()
    # the in-place run below is the sampled fused node (the readout hides it): the library plans it for this model and grid
    assert engine.backward_mode(engine.model_struct(Cn, H, H, 2, 4, 17), B * Sn, len(TIMES), _grid(0.5), 'euler', samples=Sn, sample_grad=True) == 1

    def run(in_place):
        X = X0.clone().requires_grad_(True)
        net.zero_grad()
        coeffs = S.torchcde.hermite_cubic_coefficients_with_backward_differences(X, times)
        torch.manual_seed(11)      # (the head's dropout mask: the same (B S, H) draw in both runs)
        if in_place:
            out = net(times, (coeffs,), fi, method='euler', options={'samples': Sn, 'sample_grad': True, 'seed': 21})
        else:
            out = net(times, (coeffs.repeat_interleave(Sn, 0),), fi.repeat_interleave(Sn), method='euler', options={'seed': 21})
        assert tuple(out.shape) == (B * Sn, 2)
        mean = S.sample_stats(out, Sn)[0]
        (mean * w).sum().backward()
        return X.grad.clone(), out.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters()}
    with warnings.catch_warnings():
        warnings.filterwarnings('error', module='stable_neural_sdes_amd')
        ga, outa, pa = run(True)
    gb, outb, pb = run(False)
    assert torch.equal(outa, outb)
    assert bool(torch.isfinite(ga).all()) and float(ga.abs().max()) > 0
    grad_close(ga, gb, 'X', GRAD_TOL_MAX, 'wrapper')
    for n in pa:      # the field's gradients come out of the fused node alone: the same bits; initial_network sees B rows, not B S
        if n.startswith('func.'):
            assert torch.equal(pa[n], pb[n]), n
        else:
            grad_close(pa[n], pb[n], n, GRAD_TOL_MAX, 'wrapper')


# ---- 9. hipGraph ----------------------------------------------------------------------------------------------------------------

def test_captured_sampled_forward_and_backward_replay_to_the_eager_gradient():
    c = _case(4, 17, 3, 3, 'euler', shape=(64, 21, 2, 0.5))
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    ts = torch.from_numpy(TS).to(DEV)
    wsum = torch.from_numpy(c['wsum']).to(DEV)
    m, y0, coeffs, _ = _build(c, torch.float32, DEV, replicate=False)

    def step():
        ys = S.sdeint(m, y0, ts, method='euler', dt=0.5, options={'kernel': 'mfma4', 'strict': True, 'seed': seed, 'samples': 3,
                                                                  'sample_grad': True})
        assert int(ys.grad_fn.call.desc.samples) == 3
        return torch.autograd.grad((ys * wsum).sum(), [coeffs, y0])

    eager = [g.clone() for g in step()]
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
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[0].abs().max()) > 0 and tuple(eager[0].shape) == tuple(coeffs.shape)
    assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])


# ---- 10. sample_stats backward --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('groups,Sn,width', [(1, 2, 1), (7, 3, 33), (64, 8, 128)])
def test_sample_stats_backward_against_float64_autograd(groups, Sn, width):
    """grad_ys = gm / S + gv 2 (y - mean) / (S - 1).  Bound per element, derived from the formula's fp32 roundings (a division, a
    product, a subtraction, one fma per term - a handful of 2^-24 relative errors, taken as 2^-19 of the terms' magnitudes with
    |y - mean| <= 2 max_s |y|) plus the fp32 mean's own error, at most S 2^-24 max_s |y|, carried through 2 gv / (S - 1)."""
    rng = np.random.default_rng(groups + Sn + width)
    x = rng.standard_normal((groups, Sn, width)).astype(np.float32)
    gm = rng.standard_normal((groups, width)).astype(np.float32)
    gv = rng.standard_normal((groups, width)).astype(np.float32)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    m64 = x64.sum(1) / Sn
    v64 = (x64 - m64.unsqueeze(1)).square().sum(1) / (Sn - 1)
    (m64 * torch.from_numpy(gm).double()).sum().backward(retain_graph=True)
    ref_m = x64.grad.clone()
    x64.grad = None
    ((m64 * torch.from_numpy(gm).double()).sum() + (v64 * torch.from_numpy(gv).double()).sum()).backward()
    ref = x64.grad.numpy()
    ymax = np.abs(x).max(1).astype(np.float64)
    agm, agv = np.abs(gm.astype(np.float64)), np.abs(gv.astype(np.float64))
    bound = 2.0 ** -19 * (agm / Sn + 4 * agv * ymax / (Sn - 1)) + 2 * agv / (Sn - 1) * Sn * 2.0 ** -24 * ymax
    bound_m = 2.0 ** -19 * agm / Sn

    def run(xd, var=True):
        xd = xd.requires_grad_(True)
        mean, v = S.sample_stats(xd, Sn, var=var)
        assert 'SampleStats' in type(mean.grad_fn).__name__
        loss = (mean * torch.from_numpy(gm).to(DEV)).sum()
        if var:
            loss = loss + (v * torch.from_numpy(gv).to(DEV)).sum()
        else:
            assert v is None
        loss.backward()
        return xd.grad
    xd = torch.from_numpy(x).to(DEV).reshape(groups * Sn, width)
    g1, g2 = run(xd.clone()), run(xd.clone())
    assert torch.equal(g1, g2) and tuple(g1.shape) == (groups * Sn, width)
    err = np.abs(g1.double().cpu().numpy().reshape(groups, Sn, width) - ref)
    print(f'sample_stats backward ({groups}, {Sn}, {width}): err / bound max {np.max(err / bound[:, None, :]):.3f}')
    assert np.all(err <= bound[:, None, :])
    gmo = run(xd.clone(), var=False)      # var=False: the mean's term alone
    err_m = np.abs(gmo.double().cpu().numpy().reshape(groups, Sn, width) - ref_m.numpy())
    assert np.all(err_m <= bound_m[:, None, :])
    # an unaligned view (the scalar route of the kernels): the same numbers
    buf = torch.zeros(groups * Sn * width + 1, device=DEV)
    buf[1:] = xd.reshape(-1)
    gu = run(buf[1:].reshape(groups * Sn, width).detach())
    assert torch.equal(gu, g1)
    # an input without grad builds no node
    mean, v = S.sample_stats(xd, Sn)
    assert mean.grad_fn is None and not mean.requires_grad and v.grad_fn is None
    with torch.no_grad():
        mean2, _ = S.sample_stats(xd.clone().requires_grad_(True), Sn)
    assert mean2.grad_fn is None and torch.equal(mean2, mean)
