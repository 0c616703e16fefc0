"""SNSDE_FLAG_ENSEMBLE_NETS on the GPU (options={'ensemble_nets': True}): M = 3 models with a diffusion net in one fused solve on
the wave pairs (snsde_w4_euler_kernel / snsde_w4_srk_kernel, H = 64) and on the diffusion-net 4-row tiles (snsde_m4n_kernel, H = 16
.. 128) against the ordinary sdeint of each member run as a shard of the whole (members = 0, its own parameters, row_offset + m Bm,
the same global_rows) - member by member, torch.equal, no tolerance.  Every case first asserts, on the descriptor it launches,
which kernel the fused route names, and counts the launches: the loop of M ordinary solves cannot stand in silently.

Shapes: Bm = 8 rows per member (two 4-row tiles: one workgroup of the wave pairs each), Bm = 4 and 12 (an odd number of tiles per
member: the second pair of the member's last workgroup is the surplus one, moved back onto the member's last four rows - not the
batch's, and not the next member's first), nine irregular knots,
eight solver steps of dt = 1 (two Philox blocks of four steps on the pair) that cross every spline interval, output times between
the steps, Philox increments under a fixed seed."""
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


def _members(io, no, H, C_, B, NL=2):
    """M modules of one architecture with DIFFERENT random parameters on one control path of B rows, and the members' initial states."""
    key = (io, no, H, C_, B, NL)
    if key not in _MEMBERS:
        pr = make_problem(300 + H + C_ + B, io, no, NL, B, H, C_, len(TIMES), times=TIMES)
        coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
        sdes = []
        for m in range(M):
            torch.manual_seed(1000 + 17 * m + H)
            sde = S.Diffusion_model(C_, H, H, NL, input_option=io, noise_option=no).to(DEV).requires_grad_(False)
            sde.set_X(coeffs, times)
            sdes.append(sde)
        y0 = (0.5 * torch.randn(M, B, H, generator=torch.Generator().manual_seed(7 + H))).to(DEV)
        _MEMBERS[key] = (sdes, y0, engine.model_struct(C_, H, H, NL, io, no))
    return _MEMBERS[key]


def _check(io, no, H, expect, C_=3, B=8, NL=2, method='euler', kernel='auto', samples=1, row_out=False, row_offset=0, global_rows=None):
    """The fused ensemble against its members as shards; returns the ensemble's result.  B: input rows of a member, samples: paths
    per input row (Bm = B samples rows per member)."""
    sdes, y0, model = _members(io, no, H, C_, B, NL)
    Bm = B * samples
    ts = torch.from_numpy(TS).to(DEV)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    assert grid.N == 8
    G = global_rows or M * Bm
    # the route, on the descriptor the launch will carry
    q = dict(method=method, kernel=kernel, global_rows=G, row_offset=row_offset, members=M, samples=samples if samples > 1 else 0,
             ensemble_samples=samples > 1)
    assert engine.forward_path(model, M * Bm, len(TIMES), grid.N, **q) == 'none'      # (the parent's answer, without the option)
    assert engine.forward_path(model, M * Bm, len(TIMES), grid.N, ensemble_nets=True, **q) != 'none'
    desc = engine.query_descriptor(model, M * Bm, len(TIMES), grid.N, ensemble_nets=True, **q)
    assert engine.forward_kernel(desc) == expect, (engine.forward_kernel(desc, keys=True), 'meant', expect)
    opts = {'seed': SEED, 'kernel': kernel}
    sampled = {'samples': samples} if samples > 1 else {}
    if row_out:
        opts['row_out'] = torch.randint(0, len(TS), (B,), generator=torch.Generator().manual_seed(3)).to(DEV)
    with _launches() as rec, torch.no_grad():
        got = S.sdeint_ensemble(sdes, y0, ts, method=method, dt=1.0,
                                options=dict(opts, row_offset=row_offset, global_rows=global_rows, strict=True, ensemble_nets=True,
                                             **(dict(sampled, ensemble_samples=True) if sampled else {})))
    assert rec.seen == [(M, expect)], rec.seen      # ONE launch, of the ensemble descriptor, on the kernel meant
    assert tuple(got.shape) == ((M, Bm, H) if row_out else (len(TS), M, Bm, H))
    assert torch.isfinite(got).all()
    with _launches() as ref_rec, torch.no_grad():
        for m in range(M):
            ref = S.sdeint(sdes[m], y0[m], ts, method=method, dt=1.0,
                           options=dict(opts, row_offset=row_offset + m * Bm, global_rows=G, **sampled))
            mine = got[m] if row_out else got[:, m]
            assert torch.equal(mine, ref), (m, float((mine - ref).abs().max()))
    assert ref_rec.seen == [(0, expect)] * M, ref_rec.seen      # (the shards ran the kernel the ensemble ran)
    return got


# ---- wave pairs -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method', ['euler', 'srk'])
@pytest.mark.parametrize('io', [1, 3])
@pytest.mark.parametrize('no', [14, 18])
@pytest.mark.parametrize('NL', [1, 2])
def test_wave_pair_instantiations(NL, no, io, method):
    got = _check(io, no, 64, 'w4', NL=NL, method=method)
    # member 1 against member 0 on the same local rows: a kernel that ignored the member would repeat member 0's field
    assert (got[-1, 1] - got[-1, 0]).abs().max() > 1e-3 and (got[-1, 2] - got[-1, 1]).abs().max() > 1e-3


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_wave_pair_gate_and_state_times_net(method):
    _check(5, 19, 64, 'w4', method=method)      # f = tanh(z tanh(y)), raw = q y


@pytest.mark.parametrize('method', ['euler', 'srk'])
@pytest.mark.parametrize('Bm', [4, 12])
def test_wave_pair_odd_number_of_tiles_per_member(Bm, method):
    """Bm / 4 odd: every member's last workgroup has a surplus pair, which solves the member's last four rows a second time with the
    member's parameters (Bm = 4: both pairs of the member's only workgroup solve the same tile).  A surplus pair on the next member's
    rows, or on the batch's last rows, would store another member's solution over them."""
    _check(1, 18, 64, 'w4', B=Bm, method=method)
    _check(3, 14, 64, 'w4', B=Bm, NL=1, method=method, kernel='w4')


def test_wave_pair_row_out_and_shard():
    _check(1, 18, 64, 'w4', row_out=True)
    _check(3, 18, 64, 'w4', method='srk', row_out=True)
    _check(1, 18, 64, 'w4', row_offset=24, global_rows=72)      # the ensemble as a shard of a larger problem
    _check(1, 18, 64, 'w4', method='srk', row_offset=24, global_rows=72)


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_wave_pair_sample_paths(method):
    _check(1, 18, 64, 'w4', B=4, samples=3, method=method)      # Bm = 12 paths per member


# ---- member identity ----------------------------------------------------------------------------------------------------------------

def _flat(sdes):
    return torch.stack([engine.flatten_params(sde, *engine.recognise(sde)[1:], torch.device(DEV)) for sde in sdes])


@pytest.mark.parametrize('case', [(1, 18, 64, 'euler', 'w4'), (1, 18, 64, 'srk', 'w4'), (3, 18, 32, 'srk', 'm4n')])
def test_members_share_nothing_but_the_control_path(case):
    """The same initial state and - through supplied increments, since these fields have no zero diffusion - the same Brownian rows
    for every member: the members still part, which only their parameter blocks can cause, and each equals its own solve."""
    io, no, H, method, expect = case
    Bm = 8
    sdes, y0, model = _members(io, no, H, 3, Bm)
    grid = engine.step_grid(TS, 1.0, TIMES, torch.device(DEV))
    gen = torch.Generator().manual_seed(5)
    dW = torch.randn(grid.N, Bm, H, generator=gen).to(DEV)      # (h = 1: unit variance)
    dU = (0.5 * dW + torch.randn(grid.N, Bm, H, generator=gen).to(DEV) / 12 ** 0.5) if method == 'srk' else None
    same = y0[:1].expand(M, -1, -1).reshape(M * Bm, H).contiguous()
    flat = _flat(sdes)
    rep = lambda x: None if x is None else x.repeat(1, M, 1).contiguous()
    call = engine.SolveCall(model, flat, sdes[0].coeffs, grid, same, dW=rep(dW), dU=rep(dU), method=method, members=M, ensemble_nets=True)
    assert engine.forward_kernel(call) == expect and int(call.desc.members) == M
    got = call.launch().clone().reshape(len(TS), M, Bm, H)
    assert torch.equal(got[0, 0], got[0, 1])
    assert (got[-1, 1] - got[-1, 0]).abs().max() > 1e-3 and (got[-1, 2] - got[-1, 1]).abs().max() > 1e-3
    for m in range(M):
        one = engine.SolveCall(model, flat[m].contiguous(), sdes[0].coeffs, grid, same[:Bm].contiguous(), dW=dW, dU=dU, method=method,
                               row_offset=m * Bm, global_rows=M * Bm)
        assert engine.forward_kernel(one) == expect
        assert torch.equal(got[:, m], one.launch())


# ---- diffusion-net tiles ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H', [16, 32, 128])
def test_m4n_srk_latent_only(H):
    got = _check(3, 18, H, 'm4n', method='srk')
    assert (got[-1, 1] - got[-1, 0]).abs().max() > 1e-3


@pytest.mark.parametrize('samples', [1, 2])
def test_m4n_srk_with_a_control_path(samples):
    _check(4, 18, 32, 'm4n', method='srk', B=8 if samples == 1 else 4, samples=samples)      # the shared coefficients are read


@pytest.mark.parametrize('samples', [1, 2])
def test_m4n_milstein_packs_the_transposed_layers(samples):
    _check(4, 19, 64, 'm4n', method='milstein', B=8 if samples == 1 else 4, samples=samples)


def test_m4n_euler():
    _check(4, 18, 128, 'm4n', kernel='mfma4')           # H = 128 on 4-row tiles
    _check(4, 18, 64, 'm4n', C_=40)                     # the wide control block (five 16-wide k-blocks)
    _check(4, 18, 32, 'm4n', method='srk', B=4)         # one tile per member
    _check(3, 18, 128, 'm4n', method='srk', row_out=True, row_offset=24, global_rows=72)


# ---- wrappers and autograd ----------------------------------------------------------------------------------------------------------

def test_ensemble_of_classification_wrappers_on_the_wave_pairs():
    pr = make_problem(77, 3, 18, 2, 8, 64, 3, len(TIMES), times=TIMES)
    models = []
    for m in range(M):
        torch.manual_seed(500 + m)
        net = S.NeuralSDE(S.Diffusion_model(3, 64, 64, 2, input_option=3, noise_option=18), 3, 64, 5).to(DEV)
        for mod in net.linear:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(); mod.running_var.uniform_(0.5, 2.0)
        models.append(net.eval().requires_grad_(False))
    coeffs, times = torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(TIMES).to(DEV)
    fi = torch.tensor([8, 3, 5, 2, 8, 1, 0, 6], device=DEV)
    ens = S.Ensemble(models).eval()
    with _launches() as rec, torch.no_grad():
        got = ens(times, (coeffs,), fi, options={'seed': SEED, 'ensemble_nets': True})
    assert rec.seen == [(M, 'w4')], rec.seen
    with _launches() as ref_rec, torch.no_grad():
        refs = [net(times, (coeffs,), fi, options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 8 * M}) for m, net in enumerate(models)]
    assert ref_rec.seen == [(0, 'w4')] * M
    assert tuple(got.shape) == (M, 8, 5) and torch.isfinite(got).all()
    assert torch.equal(got, torch.stack(refs))
    assert (got[0] - got[1]).abs().max() > 1e-4


def test_autograd_runs_the_members_own_differentiable_solves():
    """Training stays out of the flag: with ensemble_grad and ensemble_nets under autograd the M differentiable solves run, and
    outputs and dL/dy0 are the members' own."""
    sdes, y0, model = _members(1, 18, 64, 3, 8)
    ts = torch.from_numpy(TS).to(DEV)
    cot = torch.randn(len(TS), M, 8, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    try:
        for sde in sdes:
            sde.requires_grad_(True)
        ya = y0.clone().requires_grad_(True)
        with _launches() as rec:
            got = S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0,
                                    options={'seed': SEED, 'ensemble_grad': True, 'ensemble_nets': True})
        assert [m for m, _ in rec.seen] == [0] * M, rec.seen
        (got * cot).sum().backward()
        mine = [[p.grad.clone() for p in sde.parameters()] for sde in sdes]
        for sde in sdes:
            sde.zero_grad(set_to_none=True)
        yb = y0.clone().requires_grad_(True)
        ref = torch.stack([S.sdeint(sde, yb[m], ts, method='euler', dt=1.0,
                                    options={'seed': SEED, 'row_offset': 8 * m, 'global_rows': 8 * M}) for m, sde in enumerate(sdes)], dim=1)
        (ref * cot).sum().backward()
        assert torch.equal(got, ref) and torch.equal(ya.grad, yb.grad) and ya.grad.abs().max() > 0
        for gm, sde in zip(mine, sdes):
            assert all(torch.equal(a, p.grad) for a, p in zip(gm, sde.parameters()))
        with pytest.raises(NotImplementedError, match='strict'):
            S.sdeint_ensemble(sdes, ya, ts, method='euler', dt=1.0,
                              options={'seed': SEED, 'ensemble_grad': True, 'ensemble_nets': True, 'strict': True})
    finally:
        for sde in sdes:
            sde.zero_grad(set_to_none=True)
            sde.requires_grad_(False)
