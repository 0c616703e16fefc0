"""snsde_solve::members on the GPU: M = 3 models of one architecture with different parameters in one fused solve against the
ordinary sdeint of each member run as a shard of the whole (members = 0, its own parameters, row_offset + m Bm, the same
global_rows) - member by member, torch.equal, no tolerance - for every kernel that takes the option.  Every case first asserts, on
the descriptor it launches, that the fused route is taken and which kernel it names, and counts the launches: the loop of M
ordinary solves cannot stand in silently.

Shapes: Bm = 8 rows per member (two 4-row tiles each, so the tile -> member map is not the identity; one case with Bm = 4), nine
irregular knots, eight solver steps of dt = 1 that cross every spline interval, output times between the steps, Philox increments
under a fixed seed."""
import signal

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import engine
from tests.helpers import make_problem

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 0.6, 1.7, 2.2, 3.9, 4.4, 6.0, 6.9, 8.0], np.float32)      # L = 9 knots
TS = np.array([0.0, 2.5, 5.3, 8.0], np.float32)                                  # outputs inside the steps
M, SEED = 3, 41


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('ensemble GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class _launches:
    """Records (members, forward kernel) of every SolveCall launched inside the block, read from the call's own descriptor."""

    def __enter__(self):
        self.seen, self._saved = [], engine.SolveCall.launch
        launch, rec = self._saved, self

        def launch_(call, *a, **k):
            rec.seen.append((int(call.desc.members), engine.forward_kernel(call)))
            return launch(call, *a, **k)
        engine.SolveCall.launch = launch_
        return self

    def __exit__(self, *exc):
        engine.SolveCall.launch = self._saved
        return False


_MEMBERS = {}


def _members(io, no, H, C_, Bm):
    """M modules of one architecture with DIFFERENT random parameters on one control path, and the members' initial states."""
    key = (io, no, H, C_, Bm)
    if key not in _MEMBERS:
        pr = make_problem(300 + H + C_ + Bm, io, no, 2, Bm, H, C_, len(TIMES), times=TIMES)
        coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
        sdes = []
        for m in range(M):
            torch.manual_seed(1000 + 17 * m + H)
            sde = S.Diffusion_model(C_, H, H, 2, input_option=io, noise_option=no).to(DEV).requires_grad_(False)
            sde.set_X(coeffs, times)
            sdes.append(sde)
        y0 = (0.5 * torch.randn(M, Bm, H, generator=torch.Generator().manual_seed(7 + H))).to(DEV)
        _MEMBERS[key] = (sdes, y0, engine.model_struct(C_, H, H, 2, io, no))
    return _MEMBERS[key]


def _check(io, no, H, C_=3, Bm=8, method='euler', kernel='auto', precision='fp32', lean_general=False, exact_order=False,
           row_out=False, row_offset=0, global_rows=None, expect=None, variant=None):
    """The fused ensemble against its members as shards; returns the ensemble's result."""
    sdes, y0, model = _members(io, no, H, C_, Bm)
    ts = torch.from_numpy(TS).to(DEV)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert grid.N == 8
    G = global_rows or M * Bm
    # the route, on the descriptor the launch will carry
    q = dict(method=method, kernel=kernel, precision=precision, global_rows=G, row_offset=row_offset, lean_general=lean_general,
             exact_order=exact_order, members=M)
    assert engine.forward_path(model, M * Bm, len(TIMES), grid.N, **q) != 'none'
    desc = engine.query_descriptor(model, M * Bm, len(TIMES), grid.N, **q)
    assert engine.forward_kernel(desc) == expect, (engine.forward_kernel(desc, keys=True), 'meant', expect)
    if variant is not None:
        assert engine.lean_variant(desc) == variant
    opts = {'seed': SEED, 'kernel': kernel, 'precision': precision, 'exact_order': exact_order}
    if row_out:
        opts['row_out'] = torch.randint(0, len(TS), (Bm,), generator=torch.Generator().manual_seed(3)).to(DEV)
    with _launches() as rec, torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0,
                                options=dict(opts, row_offset=row_offset, global_rows=global_rows, lean_general=lean_general, strict=True))
    assert rec.seen == [(M, expect)], rec.seen      # ONE launch, of the ensemble descriptor, on the kernel meant
    assert tuple(got.shape) == ((M, Bm, H) if row_out else (len(TS), M, Bm, H))
    assert torch.isfinite(got).all()
    with _launches() as ref_rec, torch.no_grad():
        for m in range(M):
            ref = S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0,
                           options=dict(opts, row_offset=row_offset + m * Bm, global_rows=G))
            mine = got[m] if row_out else got[:, m]
            assert torch.equal(mine, ref), (m, float((mine - ref).abs().max()))
    assert ref_rec.seen == [(0, expect)] * M, ref_rec.seen      # (the shards ran the kernel the ensemble ran)
    return got


@pytest.mark.parametrize('method', ['euler', 'milstein'])
@pytest.mark.parametrize('H', [64, 128])
def test_lean_general_kernel(H, method):
    got = _check(4, 17, H, method=method, lean_general=True, expect='lean', variant='general')
    # member 1 against member 0 on the same local rows: a kernel that ignored the member index would repeat member 0's field
    assert (got[-1, 1] - got[-1, 0]).abs().max() > 1e-3 and (got[-1, 2] - got[-1, 1]).abs().max() > 1e-3


def test_members_share_nothing_but_the_control_path():
    """The same initial state and the same Brownian rows for every member (row_offset moves by Bm per member, so this needs the
    zero diffusion of noise_option 0): the members still part, which only their parameters can cause."""
    sdes, y0, model = _members(4, 0, 64, 3, 8)
    ts = torch.from_numpy(TS).to(DEV)
    same = y0[:1].expand(M, -1, -1).contiguous()
    with _launches() as rec, torch.no_grad():
        got = S.sdeint_ensemble(sdes, same, ts, method='euler', dt=1.0, options={'seed': SEED, 'strict': True})
    assert rec.seen == [(M, 'lean')]
    assert torch.equal(got[0, 0], got[0, 1]) and (got[-1, 1] - got[-1, 0]).abs().max() > 1e-3
    with torch.no_grad():
        for m in range(M):
            assert torch.equal(got[:, m], S.sdeint(sdes[m], same[m], ts, method='euler', dt=1.0,
                                                   options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 24}))


def test_lean_specialised_kernel():
    """input_option 4, noise_option 17, Euler at the shape the compile-time specialised instantiation exists for (H = 128, a
    control path of 21 channels); the general instantiation of the same descriptor gives the same bits."""
    spec = _check(4, 17, 128, C_=21, expect='lean', variant='specialised')
    gen = _check(4, 17, 128, C_=21, lean_general=True, expect='lean', variant='general')
    assert torch.equal(spec, gen)


@pytest.mark.parametrize('method', ['euler', 'milstein'])
def test_lean_kernel_with_bf16_operands(method):
    bf = _check(4, 17, 128, method=method, precision='bf16', expect='lean_bf16')
    f32 = _check(4, 17, 128, method=method, expect='lean')
    err = (bf - f32).abs().max()
    assert 0 < err < 0.25      # (another kernel than the f32 one, and still the same solve: states are O(1))


def test_general_kernel_euler_and_srk():
    """kernel = 'mfma4': a diffusion net at H = 64 is the general kernel's under Euler (its net weights come from the member's
    block too); the unfused emb order; the elementwise field under SRK is its SRK variant - pass table shared, stage-time diffusion
    tables per member."""
    _check(1, 18, 64, kernel='mfma4', expect='general_m4')
    _check(4, 17, 128, kernel='mfma4', exact_order=True, expect='general_m4')
    _check(4, 17, 128, kernel='mfma4', method='srk', expect='general_m4')
    _check(4, 17, 64, method='srk', expect='general_m4')
    _check(4, 17, 64, method='milstein', kernel='mfma4', exact_order=True, expect='general_m4')


def test_row_out_offsets_small_members_and_h32():
    _check(4, 17, 64, row_out=True, lean_general=True, expect='lean')
    _check(4, 17, 128, method='srk', row_out=True, expect='general_m4')
    _check(4, 17, 64, row_offset=40, global_rows=96, lean_general=True, expect='lean')      # a shard of a larger problem
    _check(4, 17, 128, method='srk', row_offset=24, global_rows=72, expect='general_m4')
    _check(4, 17, 64, Bm=4, lean_general=True, expect='lean')                               # one tile per member
    _check(4, 17, 32, lean_general=True, expect='lean')
    _check(2, 13, 32, method='milstein', expect='lean')


def test_prepared_blocks_are_reused():
    """SNSDE_FLAG_REUSE_PREPARED / auto_reuse: the second launch skips the prepare launch of all members and gives the same bits."""
    for method, expect in (('euler', 'lean'), ('srk', 'general_m4')):
        sdes, y0, model = _members(4, 17, 64, 3, 8)
        grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
        flat = torch.stack([engine.flatten_params(sde, *engine.recognise(sde)[1:], torch.device(DEV)) for sde in sdes])
        call = engine.SolveCall(model, flat, sdes[0].coeffs, grid, y0.reshape(M * 8, 64).contiguous(), method=method, seed=SEED, members=M)
        assert engine.forward_kernel(call) == expect and int(call.desc.members) == M
        first = call.launch().clone()
        call.workspace_guard = call.workspace.clone()
        again = call.launch(reuse_prepared=True).clone()
        auto = call.launch(auto_reuse=True).clone()
        torch.cuda.synchronize()
        assert torch.equal(call.workspace, call.workspace_guard)      # (nothing was re-prepared)
        assert torch.equal(first, again) and torch.equal(first, auto)
        ts = torch.from_numpy(TS).to(DEV)
        with torch.no_grad():
            assert torch.equal(first.reshape(len(TS), M, 8, 64), S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0, options={'seed': SEED}))


def test_uncovered_plan_loops_and_strict_raises():
    """noise_option 18 at H = 64 under `auto` is the wave pairs' plan: no ensemble kernel, so sdeint_ensemble runs the M ordinary
    solves (each on the wave pairs) and raises under strict."""
    sdes, y0, model = _members(1, 18, 64, 3, 8)
    ts = torch.from_numpy(TS).to(DEV)
    assert engine.forward_path(model, M * 8, len(TIMES), 8, 'euler', members=M, global_rows=M * 8) == 'none'
    with _launches() as rec, torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options={'seed': SEED})
    assert rec.seen == [(0, 'w4')] * M
    with torch.no_grad():
        ref = torch.stack([S.sdeint(sdes[m], y0[m], ts, method='euler', dt=1.0,
                                    options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': M * 8}) for m in range(M)], dim=1)
        assert torch.equal(got, ref)
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options={'seed': SEED, 'strict': True})
        with pytest.raises(ValueError, match='inference only'):
            S.sdeint_ensemble(sdes, y0, ts, method='euler', dt=1.0, options={'seed': SEED, 'save_traj': True})
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble(sdes, y0.clone().requires_grad_(True), ts, method='euler', dt=1.0)


def _wrappers(kind, H=64, C_=3, Bm=8):
    pr = make_problem(77, 4, 17, 2, Bm, H, C_, len(TIMES), times=TIMES)
    models = []
    for m in range(M):
        torch.manual_seed(500 + m)
        func = S.Diffusion_model(C_, H, H, 2, input_option=4, noise_option=17)
        net = kind(func, C_, H, 5).to(DEV)
        for mod in net.linear:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(); mod.running_var.uniform_(0.5, 2.0)
        models.append(net.eval().requires_grad_(False))
    return models, torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)


def test_ensemble_of_classification_wrappers():
    models, coeffs, times = _wrappers(S.NeuralSDE)
    fi = torch.tensor([8, 3, 5, 2, 8, 1, 0, 6], device=DEV)
    ens = S.Ensemble(models).eval()
    with _launches() as rec, torch.no_grad():
        got = ens(times, (coeffs,), fi, options={'seed': SEED})
    assert rec.seen == [(M, 'lean')], rec.seen
    with _launches() as ref_rec, torch.no_grad():
        refs = [net(times, (coeffs,), fi, options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 8 * M}) for m, net in enumerate(models)]
    assert ref_rec.seen == [(0, 'lean')] * M
    assert tuple(got.shape) == (M, 8, 5) and torch.isfinite(got).all()
    assert torch.equal(got, torch.stack(refs))
    assert (got[0] - got[1]).abs().max() > 1e-4


def test_ensemble_of_ists_wrappers_under_their_default_srk():
    models, coeffs, times = _wrappers(S.IstsNeuralSDE)
    ens = S.Ensemble(models).eval()
    with _launches() as rec, torch.no_grad():
        out, z = ens(coeffs, times, options={'seed': SEED})
    assert rec.seen == [(M, 'general_m4')], rec.seen
    with _launches() as ref_rec, torch.no_grad():
        refs = [net(coeffs, times, options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 8 * M}) for m, net in enumerate(models)]
    assert ref_rec.seen == [(0, 'general_m4')] * M
    assert tuple(out.shape) == (M, 8, len(TIMES), 5) and tuple(z.shape) == (M, 8, len(TIMES), 64)
    assert torch.equal(z, torch.stack([r[1] for r in refs]))
    assert torch.equal(out, torch.stack([r[0] for r in refs]))
