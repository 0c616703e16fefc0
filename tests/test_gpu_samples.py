"""snsde_solve::samples on the GPU: a solve of S paths per input row with the coefficients in place against the same descriptor with
samples = 0 and the coefficients replicated row-wise S times - same forced kernel, seed and row_offset, the states bit for bit
(torch.equal, no tolerance) - for every kernel family that takes the option; a shard; the Python fallback; snsde_sample_stats.

Shapes: irregular knots and six solver steps (the spline interval moves), (input rows, samples) pairs that put two input rows into
one 4-row tile, leave the last tile ragged, or give a tile one input row; 16-row tiles with a ragged third tile."""
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import make_problem, param_spec

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0], np.float32)      # knots: six steps of dt = 1 cross five intervals
TS = np.array([0.0, 2.5, 6.0], np.float32)
PAIRS = [(3, 3), (2, 4), (5, 5), (1, 7), (4, 1)]      # (input rows B, samples S): paths = B S


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('sample-path GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


_PROBLEMS = {}


def _problem(io, no, H, C_, B, NL=2):
    key = (io, no, H, C_, B, NL)
    if key not in _PROBLEMS:
        pr = make_problem(100 + 7 * B + H + C_, io, no, NL, B, H, C_, len(TIMES), times=TIMES)
        flat = torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in param_spec(io, no, NL, C_, H)])).to(DEV)
        _PROBLEMS[key] = (engine.model_struct(C_, H, H, NL, io, no), flat, torch.from_numpy(pr['coeffs']).to(DEV))
    return _PROBLEMS[key]


def _sampled_and_replicated(io, no, H, C_, B, Sn, method='euler', kernel='auto', precision='fp32', lean_general=False,
                            row_out=False, expect=None, variant=None, seed=41):
    """ys of the sampled solve and of the replicated one; asserts the route first, so that a green comparison is the kernel meant."""
    model, flat, coeffs = _problem(io, no, H, C_, B)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert 5 <= grid.N <= 9
    P = B * Sn
    gen = torch.Generator().manual_seed(seed + P)
    y0 = (0.5 * torch.randn(P, H, generator=gen)).to(DEV)
    ro = torch.randint(0, len(TS), (P,), generator=gen).to(device=DEV, dtype=torch.int32) if row_out else None
    path = engine.forward_path(model, P, len(TIMES), grid.N, method, kernel, precision=precision, row_offset=2 * Sn,
                               samples=Sn, lean_general=lean_general)
    assert path == expect, (path, expect)
    kw = dict(method=method, seed=seed, row_offset=2 * Sn, kernel=kernel, precision=precision, lean_general=lean_general, row_out=ro)
    a = engine.SolveCall(model, flat, coeffs, grid, y0, samples=Sn, **kw)
    b = engine.SolveCall(model, flat, coeffs.repeat_interleave(Sn, 0).contiguous(), grid, y0, **kw)
    assert int(a.desc.samples) == (Sn if Sn > 1 else 0) and int(b.desc.samples) == 0
    if variant is not None:
        assert engine.lean_variant(a) == engine.lean_variant(b) == variant
    ya, yb = a.launch().clone(), b.launch().clone()
    torch.cuda.synchronize()
    assert tuple(ya.shape) == ((P, H) if row_out else (len(TS), P, H))
    assert torch.isfinite(ya).all()
    return ya, yb


def _check(*args, **kw):
    ya, yb = _sampled_and_replicated(*args, **kw)
    assert torch.equal(ya, yb)
    return ya


@pytest.mark.parametrize('B,Sn', PAIRS)
@pytest.mark.parametrize('C_', [3, 21])
@pytest.mark.parametrize('H', [32, 64, 128])
def test_lean_kernel_general_and_specialised(H, C_, B, Sn):
    """kernel = 'mfma4' on the reference's (4, 17) field: the lean kernel, its specialised instantiation where one exists (forced
    off with SNSDE_FLAG_LEAN_GENERAL), every output time and the per-row output."""
    model, _, _ = _problem(4, 17, H, C_, B)
    probe = engine.SolveCall(model, *_problem(4, 17, H, C_, B)[1:], engine.step_grid(TS, 1.0, TIMES, torch.device(DEV)),
                             torch.zeros(B, H, device=DEV), kernel='mfma4', seed=1)
    auto_variant = engine.lean_variant(probe)
    assert auto_variant in ('general', 'specialised')
    if (H, C_) == (128, 21):
        assert auto_variant == 'specialised'      # the K2 instantiation
    outs = []
    for general in (False, True):
        for row_out in (False, True):
            ys = _check(4, 17, H, C_, B, Sn, kernel='mfma4', lean_general=general, row_out=row_out, expect='lean',
                        variant='general' if general else auto_variant)
            if not row_out:
                outs.append(ys)
    assert torch.equal(outs[0], outs[1])      # (the two instantiations agree, as everywhere)
    if Sn > 1:      # the paths of one input row start together and part
        v = outs[0].reshape(len(TS), B, Sn, H)
        assert (v[-1, :, 0] - v[-1, :, 1]).abs().max() > 1e-4


def test_one_sample_is_the_plain_solve():
    """(4, 1): samples = 1 is samples = 0 - the descriptor, the route and the bits."""
    model, flat, coeffs = _problem(4, 17, 64, 3, 4)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    y0 = torch.full((4, 64), 0.25, device=DEV)
    a = engine.SolveCall(model, flat, coeffs, grid, y0, seed=9, samples=1)
    b = engine.SolveCall(model, flat, coeffs, grid, y0, seed=9)
    assert int(a.desc.samples) == 0
    assert torch.equal(a.launch().clone(), b.launch().clone())


@pytest.mark.parametrize('B,Sn', PAIRS)
@pytest.mark.parametrize('H,C_', [(64, 3), (128, 21)])
@pytest.mark.parametrize('method', ['euler', 'milstein'])
def test_lean_kernel_with_bf16_operands(method, H, C_, B, Sn):
    for row_out in (False, True):
        _check(4, 17, H, C_, B, Sn, method=method, kernel='mfma4', precision='bf16', row_out=row_out, expect='lean-bf16')


@pytest.mark.parametrize('B,Sn', PAIRS)
@pytest.mark.parametrize('H,C_', [(32, 3), (64, 21), (128, 3)])
def test_lean_kernel_under_milstein_and_without_time_features(H, C_, B, Sn):
    _check(2, 13, H, C_, B, Sn, method='milstein', kernel='mfma4', expect='lean')
    _check(0, 16, H, C_, B, Sn, method='euler', kernel='mfma4', expect='lean', row_out=True)


@pytest.mark.parametrize('B,Sn', PAIRS)
@pytest.mark.parametrize('H,C_', [(32, 21), (64, 3), (128, 21)])
def test_general_kernel_srk_on_four_row_tiles(H, C_, B, Sn):
    for row_out in (False, True):
        _check(4, 17, H, C_, B, Sn, method='srk', kernel='mfma4', row_out=row_out, expect='mfma-srk')


@pytest.mark.parametrize('B,Sn', PAIRS + [(5, 7)])
@pytest.mark.parametrize('H,C_', [(32, 3), (64, 21), (128, 3)])
def test_general_kernel_on_sixteen_row_tiles(H, C_, B, Sn):
    """kernel = 'mfma16': Euler and Milstein on the general kernel ((5, 7) = 35 paths: a ragged third tile), SRK where it has
    16-row tiles (H = 64 / 128)."""
    _check(4, 17, H, C_, B, Sn, method='euler', kernel='mfma16', expect='mfma16')
    _check(6, 13, H, C_, B, Sn, method='milstein', kernel='mfma16', row_out=True, expect='mfma16')
    if H != 32:
        _check(4, 17, H, C_, B, Sn, method='srk', kernel='mfma16', expect='mfma-srk')


@pytest.mark.parametrize('B,Sn', PAIRS)
def test_general_kernel_on_four_row_tiles_with_a_diffusion_net(B, Sn):
    """Euler through a one-layer diffusion net at H = 64 under kernel = 'mfma4': the general kernel's 4-row flavour, behind a
    control embedding - and with a latent-only drift (input_option 1), where no coefficient is read: a no-op."""
    _check(4, 14, 64, 3, B, Sn, kernel='mfma4', expect='mfma4')
    _check(4, 14, 64, 21, B, Sn, kernel='mfma4', row_out=True, expect='mfma4')
    ya = _check(1, 14, 64, 3, B, Sn, kernel='mfma4', expect='mfma4')
    # no control path: the same paths whatever the coefficients hold
    model, flat, coeffs = _problem(1, 14, 64, 3, B)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    P = B * Sn
    y0 = (0.5 * torch.randn(P, 64, generator=torch.Generator().manual_seed(41 + P))).to(DEV)
    other = engine.SolveCall(model, flat, torch.zeros_like(coeffs), grid, y0, seed=41, row_offset=2 * Sn, kernel='mfma4', samples=Sn)
    assert torch.equal(other.launch(), ya)


@pytest.mark.parametrize('B,Sn', PAIRS + [(5, 7)])
@pytest.mark.parametrize('H,C_', [(32, 3), (48, 21)])
def test_generic_family(H, C_, B, Sn):
    """kernel = 'generic': its Euler / Milstein kernel, its SRK kernel and its Milstein-through-a-net kernel (8-row tiles)."""
    _check(4, 17, H, C_, B, Sn, kernel='generic', expect='generic')
    _check(2, 7, H, C_, B, Sn, kernel='generic', row_out=True, expect='generic')
    _check(4, 17, H, C_, B, Sn, method='srk', kernel='generic', expect='generic-srk')
    _check(0, 14, H, C_, B, Sn, method='milstein', kernel='generic', expect='generic')


def test_auto_routes_and_uncovered_families():
    """`auto` at these sizes is the lean kernel; the wave pairs, the diffusion-net kernels and H = 256 are left uncovered: no
    kernel, and the library refuses the launch."""
    _check(4, 17, 128, 21, 3, 3, expect='lean')
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    for io, no, H, method in ((1, 18, 64, 'euler'), (4, 17, 256, 'euler'), (1, 18, 64, 'srk')):
        model, flat, coeffs = _problem(io, no, H, 3, 3)
        assert engine.forward_path(model, 12, len(TIMES), grid.N, method) != 'none'
        assert engine.forward_path(model, 12, len(TIMES), grid.N, method, samples=4) == 'none'
        call = engine.SolveCall(model, flat, coeffs, grid, torch.zeros(12, H, device=DEV), method=method, samples=4)
        with pytest.raises(engine._lib.SnsdeError) as err:
            call.launch()
        assert err.value.code == -4


def test_a_shard_of_a_sampled_solve():
    """Paths 8 .. 15 of a (4 rows, 4 samples) problem - row_offset = 8, the coefficient rows 2 .. 3 - are rows 8 .. 15 of the whole."""
    for kernel, method in (('mfma4', 'euler'), ('mfma4', 'srk'), ('generic', 'euler')):
        model, flat, coeffs = _problem(4, 17, 64, 3, 4)
        grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
        y0 = (0.5 * torch.randn(16, 64, generator=torch.Generator().manual_seed(3))).to(DEV)
        whole = engine.SolveCall(model, flat, coeffs, grid, y0, method=method, seed=77, kernel=kernel, samples=4).launch().clone()
        shard = engine.SolveCall(model, flat, coeffs[2:4].contiguous(), grid, y0[8:16].contiguous(), method=method, seed=77,
                                 kernel=kernel, samples=4, row_offset=8, global_rows=16).launch().clone()
        assert torch.equal(shard, whole[:, 8:16])
        with pytest.raises(ValueError):
            engine.SolveCall(model, flat, coeffs, grid, y0[:15].contiguous(), samples=4)


def _module(io, no, H, C_, B, seed=3):
    pr = make_problem(seed, io, no, 2, B, H, C_, len(TIMES), times=TIMES)
    m = S.Diffusion_model(C_, H, H, 2, input_option=io, noise_option=no)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.from_numpy(pr['params'][name]))
    m = m.to(DEV).requires_grad_(False)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV))
    return m, torch.from_numpy(pr['y0']).to(DEV)


@pytest.mark.parametrize('io,no,H,fused', [(1, 18, 64, False), (4, 17, 256, False), (4, 17, 128, True), (4, 17, 48, False)])
def test_sdeint_samples_equal_the_hand_replicated_solve(io, no, H, fused):
    """sdeint(options={'samples': 3}) against the caller replicating y0 and the coefficients: the fused addressing where a kernel
    takes it, the replicated fallback elsewhere (the diffusion net at H = 64 on the wave pairs, H = 256, a zero-padded H = 48)."""
    B = 5
    m, y0 = _module(io, no, H, 3, B)
    ts = torch.from_numpy(TS).to(DEV)
    model = engine.recognise(m)[0]
    steps = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV)).N
    assert (engine.forward_path(model, 3 * B, len(TIMES), steps, samples=3) != 'none') == (fused or H == 48)
    got = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 3, 'seed': 19})
    coeffs = m.coeffs
    assert tuple(got.shape) == (len(TS), 3 * B, H) and m.coeffs is coeffs
    m.set_X(coeffs.repeat_interleave(3, 0), m.times)
    ref = S.sdeint(m, y0.repeat_interleave(3, 0), ts, dt=1.0, method='euler', options={'seed': 19})
    m.set_X(coeffs, m.times)
    assert torch.equal(got, ref)
    v = got[-1].reshape(B, 3, H)
    assert (v[:, 0] - v[:, 1]).abs().max() > 1e-4
    ro = torch.tensor([2, 0, 1, 2, 1], device=DEV)
    picked = S.sdeint(m, y0, ts, dt=1.0, method='euler', options={'samples': 3, 'seed': 19, 'row_out': ro})
    assert torch.equal(picked, got[ro.repeat_interleave(3), torch.arange(3 * B, device=DEV)])


def test_wrapper_inference_returns_one_row_per_path():
    B = 6
    m, _ = _module(4, 17, 64, 3, B)
    net = S.NeuralSDE(m, 3, 64, 4).to(DEV).eval().requires_grad_(False)
    final_index = torch.tensor([6, 3, 6, 2, 5, 6], device=DEV)
    times = torch.from_numpy(TIMES).to(DEV)
    with torch.no_grad():
        out = net(times, (m.coeffs,), final_index, options={'samples': 3, 'seed': 5})
        one = net(times, (m.coeffs,), final_index, options={'seed': 5})
    assert tuple(out.shape) == (3 * B, 4) and tuple(one.shape) == (B, 4)
    assert torch.isfinite(out).all()
    v = out.reshape(B, 3, 4)
    assert (v[:, 0] - v[:, 1]).abs().max() > 0


# ---- snsde_sample_stats -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('groups,Sn,width', [(1, 2, 1), (7, 3, 33), (64, 8, 128)])
def test_sample_stats_against_float64(groups, Sn, width):
    """Mean and unbiased variance against float64 of the same float32 inputs, u = 2^-24.

    Mean: the lane adds S terms in order (S - 1 rounded additions, the first into 0 is exact) and divides once (correctly rounded):
    |mean^ - mean| <= (S - 1) u sum|x_s| / S + u |mean| <= S u sum|x_s| / S to first order; the bound asserted, as set by the
    issue, is E_m = (S + 1) u sum|x_s| / S.

    Variance, two passes: d_s = fl(x_s - mean^) has relative error u; the S non-negative terms d_s^2 are accumulated with one fused
    multiply-add each (relative error <= S u on the sum) and the sum is divided by S - 1 (u): a relative factor
    (1 + u)^2 (1 + S u)(1 + u) <= 1 + (S + 3) u + O(u^2) on sum (x_s - mean^)^2.  That sum is EXACTLY
    sum (x_s - mean)^2 + S (mean^ - mean)^2 (the cross term vanishes: sum (x_s - mean) = 0), and |mean^ - mean| <= E_m.  Hence
    |var^ - var| <= (S + 4) u var + (1 + (S + 4) u) S E_m^2 / (S - 1), with S + 4 in place of S + 3 for the second-order terms."""
    u = 2.0 ** -24
    rng = np.random.default_rng(groups + width)
    x = (3.0 * rng.standard_normal((groups, Sn, width)) + 1.0).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    mean, var = S.sample_stats(xd.reshape(groups * Sn, width), Sn)
    mean2, var2 = S.sample_stats(xd.reshape(groups * Sn, width), Sn)
    mean_only, none = S.sample_stats(xd.reshape(groups * Sn, width), Sn, var=False)      # var = NULL
    torch.cuda.synchronize()
    assert tuple(mean.shape) == tuple(var.shape) == (groups, width) and none is None
    assert torch.equal(mean, mean2) and torch.equal(var, var2) and torch.equal(mean, mean_only)
    x64 = x.astype(np.float64)
    m64, v64 = x64.mean(1), x64.var(1, ddof=1)
    e_m = (Sn + 1) * u * np.abs(x64).sum(1) / Sn
    err_m = np.abs(mean.cpu().numpy().astype(np.float64) - m64)
    err_v = np.abs(var.cpu().numpy().astype(np.float64) - v64)
    bound_v = (Sn + 4) * u * v64 + (1 + (Sn + 4) * u) * Sn * e_m ** 2 / (Sn - 1)
    print(f'sample_stats ({groups}, {Sn}, {width}): mean err / bound max {np.max(err_m / e_m):.3f}, var err / bound max {np.max(err_v / np.maximum(bound_v, 1e-300)):.3f}')
    assert (err_m <= e_m).all()
    assert (err_v <= bound_v).all()
    # a (T, B S, H) result folds its leading planes into the groups
    m3, v3 = S.sample_stats(xd.reshape(1, groups * Sn, width).expand(2, -1, -1).contiguous(), Sn)
    assert tuple(m3.shape) == (2, groups, width) and torch.equal(m3[1], mean) and torch.equal(v3[0], var)


def test_sample_stats_of_a_sampled_solve_and_odd_alignment():
    ys = _check(4, 17, 64, 3, 5, 5, kernel='mfma4', expect='lean')
    mean, var = S.sample_stats(ys, 5)
    v = ys.double().reshape(len(TS), 5, 5, 64)
    assert tuple(mean.shape) == (len(TS), 5, 64)
    assert torch.allclose(mean.double(), v.mean(2), rtol=0, atol=1e-5) and torch.allclose(var.double(), v.var(2), rtol=1e-4, atol=1e-9)
    assert (var[-1] > 0).all()      # the paths of an input row part
    # a view that is not 16-byte aligned takes the one-column-per-lane kernel: same numbers
    buf = torch.randn(8 * 3 * 64 + 1, device=DEV)
    a, av = S.sample_stats(buf[1:].reshape(24, 64), 3)
    b, bv = S.sample_stats(buf[1:].clone().reshape(24, 64), 3)
    assert torch.equal(a, b) and torch.equal(av, bv)
    with pytest.raises(ValueError):
        S.sample_stats(buf[1:].reshape(24, 64), 1)
