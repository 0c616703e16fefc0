"""GPU tests of the drop-in boundary itself (run with -m gpu):

* G6 fixture (tests/golden/dropin.npz, written by tools/check_reference_dropin.py from the REFERENCE's own modules running
  over this package's torchsde / torchcde mirrors): a FOREIGN module — defined here, not stable_neural_sdes_amd's
  Diffusion_model — with the reference's attribute and parameter names is recognised by the engine, solved by the HIP
  path, and reproduces the reference wrappers' outputs;
* NeuralSDE_forecasting end to end on CUDA at the K5 shard size (B=128, H=256, L=50, C=14, Milstein, 50 outputs, loss on the
  decoder of the last 10 states, backward): forward against the numpy fp64 oracle, gradients against fp64 autograd;
* gradients of the fused adjoint against finite differences of the numpy fp64 ORACLE (oracle/sde_oracle.py) for the
  K2 / K4 / K5 model families, so the backward is not only checked against this package's own tensor-op loop;
* the HIP engine under DistributedDataParallel over NCCL (= RCCL), one process per visible GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from oracle import sde_oracle as O
from tests.helpers import assert_parity, draw_dW, grad_close, load, make_problem, param_spec

FD_TOL = 5e-5        # measured <= 4.1e-6 (it was 2e-3 with eps = 1e-5)
GRAD_TOL = {'k5shard': 2e-5, 'pad': 2e-4}      # measured 1.0e-6 / 5.5e-5 (profiles/r05_grad_margins_small.txt); both were 2e-3 .. 3e-3

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _ReplayBM:
    levy_area_approximation = 'space-time'

    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb, return_U=False):
        i, self.n = self.n, self.n + 1
        return (self.dW[i], self.dU[i]) if return_U else self.dW[i]


class ForeignField(torch.nn.Module):
    """A vector field written here from the reference's description (models_sde/neuralsde.py:123-307) for the two options
    the fixture uses — (4, 17) and (6, 17): same attribute names, same parameter names / shapes, tensor-op f and g."""
    sde_type, noise_type = 'ito', 'diagonal'

    def __init__(self, input_channels, hidden_channels, num_hidden_layers, input_option):
        super().__init__()
        H = hidden_channels
        self.input_channels, self.hidden_channels, self.hidden_hidden_channels = input_channels, H, H
        self.num_hidden_layers, self.input_option, self.noise_option = num_hidden_layers, input_option, 17
        self.theta = torch.nn.Parameter(torch.tensor([[1.0]]))
        self.initial_network = torch.nn.Linear(input_channels, H)
        self.linear_in = torch.nn.Linear(H + 2, H)
        self.emb = torch.nn.Linear(2 * H, H)
        self.linears = torch.nn.ModuleList(torch.nn.Linear(H, H) for _ in range(num_hidden_layers - 1))
        self.linear_out = torch.nn.Linear(H, H)
        self.noise_t = torch.nn.Sequential(torch.nn.Linear(2, H), torch.nn.ReLU(), torch.nn.Linear(H, H))

    def set_X(self, coeffs, times):
        self.coeffs, self.times = coeffs, times
        self.X = S.torchcde.CubicSpline(coeffs, times)

    def _tau(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device).expand(y.shape[0], 1)
        return torch.cat([t.sin(), t.cos()], dim=-1)

    def f(self, t, y):
        z = self.emb(torch.cat([self.linear_in(torch.cat([self._tau(t, y), y], dim=-1)),
                                self.initial_network(self.X.evaluate(t))], dim=-1)).relu()
        for lin in self.linears:
            z = lin(z).relu()
        z = self.linear_out(z)
        if self.input_option == 6:
            z = z * y.tanh()
        return z.tanh()

    def g(self, t, y):
        raw = self.noise_t(self._tau(t, y)).relu() * y
        return (self.theta.sigmoid() * torch.nan_to_num(raw)).tanh()


FIX = load('dropin.npz')


def _sd(prefix):
    pre = prefix + '/sd/'
    return {k[len(pre):]: torch.from_numpy(FIX[k].copy()) for k in FIX.files if k.startswith(pre)}


def test_foreign_module_is_recognised_as_a_fast_path_module():
    f = ForeignField(5, 32, 2, 4)
    f.set_X(torch.zeros(3, 8, 20), torch.arange(9.0))
    rec = S.engine.recognise(f)
    assert rec is not None and rec[0].input_option == 4 and rec[0].noise_option == 17


def test_dropin_fixture_classification_wrapper_foreign_field_on_the_hip_path():
    B, H, C, L, NL, io, no, out_ch = (int(v) for v in FIX['cls/dims'])
    model = S.NeuralSDE(ForeignField(C, H, NL, io), C, H, out_ch, initial=True)
    model.load_state_dict(_sd('cls'))                 # the reference wrapper's state_dict, key for key
    model = model.to(DEV).eval()
    times = torch.from_numpy(FIX['cls/times']).to(DEV)
    coeffs = torch.from_numpy(FIX['cls/coeffs']).to(DEV)
    fi = torch.from_numpy(FIX['cls/final_index']).to(DEV)
    with torch.no_grad():
        out = model(times, (coeffs,), fi, bm=_ReplayBM(torch.from_numpy(FIX['cls/dW']).to(DEV)))
        out_strict = model(times, (coeffs,), fi, bm=_ReplayBM(torch.from_numpy(FIX['cls/dW']).to(DEV)),
                           options={'backend': 'hip'})      # raises unless the fused HIP solve takes the call
    np.testing.assert_allclose(out.cpu().numpy(), FIX['cls/out'], rtol=2e-4, atol=2e-5)
    assert torch.equal(out, out_strict)


def test_dropin_fixture_forecasting_wrapper_on_the_hip_path():
    B, H, C, L, NL, io, no, out_ch, out_time = (int(v) for v in FIX['fc/dims'])
    model = S.NeuralSDE_forecasting(ForeignField(C, H, NL, io), C, out_time, H, out_ch, initial=True)
    model.load_state_dict(_sd('fc'))
    model = model.to(DEV).eval()
    coeffs = torch.from_numpy(FIX['fc/coeffs']).to(DEV)
    pieces = tuple(coeffs[..., k * C:(k + 1) * C] for k in range(4))
    with torch.no_grad():
        out = model(torch.from_numpy(FIX['fc/times']).to(DEV), pieces, None,
                    bm=_ReplayBM(torch.from_numpy(FIX['fc/dW']).to(DEV)), options={'backend': 'hip'})
    np.testing.assert_allclose(out.cpu().numpy(), FIX['fc/out'], rtol=2e-4, atol=2e-5)


def test_dropin_fixture_ists_wrapper_default_srk_on_the_hip_path():
    B, H, C, L, NL, io, no, out_ch = (int(v) for v in FIX['ists/dims'])
    model = S.IstsNeuralSDE(ForeignField(C, H, NL, io), C, H, out_ch, initial=True)
    model.load_state_dict(_sd('ists'))
    model = model.to(DEV).eval()
    bm = _ReplayBM(torch.from_numpy(FIX['ists/dW']).to(DEV), torch.from_numpy(FIX['ists/dU']).to(DEV))
    with torch.no_grad():
        out, z = model(torch.from_numpy(FIX['ists/coeffs']).to(DEV), torch.from_numpy(FIX['ists/times']).to(DEV), bm=bm,
                       options={'backend': 'hip'})
    np.testing.assert_allclose(z.cpu().numpy(), FIX['ists/z'], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(out.cpu().numpy(), FIX['ists/out'], rtol=2e-4, atol=2e-5)


def test_integration_md_ctypes_stub_reproduces_sdeint_bit_for_bit():
    """The ctypes stub INTEGRATION.md section 3 prints for a maintainer of neuralsde.py:71-82, exec'd as written, against
    S.torchsde.sdeint on the G6 classification fixture's foreign module (in-kernel Philox, same key): identical bits, Euler
    and Milstein; a bad ts raises ValueError as torchsde does."""
    from tests.test_host_cpu import integration_stub_namespace
    ns = integration_stub_namespace()
    B, H, C, L, NL, io, no, out_ch = (int(v) for v in FIX['cls/dims'])
    field = ForeignField(C, H, NL, io)
    sd = _sd('cls')
    field.load_state_dict({k[len('func.'):]: v for k, v in sd.items() if k.startswith('func.')})
    field = field.to(DEV)
    times = torch.from_numpy(FIX['cls/times']).to(DEV)
    field.set_X(torch.from_numpy(FIX['cls/coeffs']).to(DEV), times)
    y0 = torch.randn(B, H, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    ts = times[[0, L // 2, L - 1]]
    dt = float((times[1:] - times[:-1]).min())
    for code, method in ((0, 'euler'), (1, 'milstein')):
        with torch.no_grad():
            want = S.torchsde.sdeint(field, y0, ts, dt=dt, method=method, options={'seed': 77, 'backend': 'hip'})
        got = ns['sdeint_diffusion_model'](field, y0, ts, dt, seed=77, method=code)
        assert got.shape == want.shape == (3, B, H)
        assert torch.equal(got, want), method
        assert not torch.equal(got[-1], got[0])
    with pytest.raises(ValueError):
        ns['sdeint_diffusion_model'](field, y0, ts.flip(0), dt)


# ---- K5 shard: NeuralSDE_forecasting end to end ------------------------------------------------------------------
def test_forecasting_wrapper_k5_shard_forward_vs_oracle_and_gradients_vs_fp64_autograd():
    B, H, C, L, NL, out_time = 128, 256, 14, 50, 2, 10
    pr = make_problem(55, 4, 17, NL, B, H, C, L, nan_frac=0.3)
    times_h = pr['times']
    dW = draw_dW(55, times_h, 1.0, B, H)
    torch.manual_seed(3)
    field = S.Diffusion_model(C, H, H, NL, input_option=4, noise_option=17)
    field.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    model = S.NeuralSDE_forecasting(field, C, out_time, H, C, initial=True)
    import copy
    model64 = copy.deepcopy(model).double().to(DEV).eval()
    model = model.to(DEV).eval()
    coeffs = torch.from_numpy(pr['coeffs']).to(DEV)
    pieces = tuple(coeffs[..., k * C:(k + 1) * C] for k in range(4))
    times = torch.from_numpy(times_h).to(DEV)
    target = torch.from_numpy(np.random.default_rng(5).standard_normal((B, out_time, C)).astype(np.float32)).to(DEV)

    pred = model(times, pieces, None, method='milstein', bm=_ReplayBM(torch.from_numpy(dW).to(DEV)),
                 options={'backend': 'hip', 'save_traj': True})
    loss = torch.nn.functional.mse_loss(pred, target)
    loss.backward()
    # forward: the states the solve produced against the numpy fp64 oracle on the same increments
    z0 = model.initial_network(field.X.evaluate(times[0])).detach().cpu().numpy()
    ref64, _ = O.solve_diffusion_model(pr['params'], 4, 17, pr['coeffs'], times_h, z0, times_h, 1.0, dW, method='milstein',
                                       dtype=np.float64)
    cpu32, _ = O.solve_diffusion_model(pr['params'], 4, 17, pr['coeffs'], times_h, z0, times_h, 1.0, dW, method='milstein',
                                       dtype=np.float32)
    with torch.no_grad():
        zs = S.sdeint(field, torch.from_numpy(z0).to(DEV), times, dt=1.0, method='milstein',
                      bm=_ReplayBM(torch.from_numpy(dW).to(DEV)), options={'backend': 'hip'})
    assert_parity(zs.cpu().numpy(), ref64, cpu32, what='K5 shard forecasting states')
    # gradients: fp64 autograd through the tensor-op loop of the same wrapper
    pieces64 = tuple(p.double() for p in pieces)
    pred64 = model64(times, pieces64, None, method='milstein', bm=_ReplayBM(torch.from_numpy(dW).double().to(DEV)),
                     options={'backend': 'torch'})
    torch.nn.functional.mse_loss(pred64, target.double()).backward()
    np.testing.assert_allclose(pred.detach().cpu().numpy(), pred64.detach().cpu().numpy(), rtol=1e-3, atol=2e-4)
    ref = dict(model64.named_parameters())
    for name, p in model.named_parameters():
        gref = ref[name].grad
        if gref is None or float(gref.abs().max()) == 0.0:
            continue
        grad_close(p.grad, gref, name, GRAD_TOL['k5shard'], 'k5shard')


# ---- backward against finite differences of the numpy oracle ----------------------------------------------------------
FD_CASES = [
    # io, no, NL, B, H, C, L, method, kernel     (K2 / K4 / K5 model families at sizes the fp64 oracle finishes in seconds)
    (4, 17, 2, 12, 128, 21, 9, 'euler', 'auto'),
    (6, 17, 2, 9, 128, 21, 7, 'euler', 'mfma16'),
    (3, 18, 2, 10, 64, 8, 7, 'euler', 'auto'),
    (4, 17, 2, 8, 256, 14, 6, 'milstein', 'auto'),
    (4, 17, 2, 9, 64, 5, 7, 'srk', 'auto'),             # SRID2: MFMA SRK variant (elementwise diffusion)
    (1, 18, 2, 9, 64, 4, 7, 'srk', 'auto'),             # SRID2 through a diffusion net (torch_ists' neuralsde_1_18 under its default srk)
    (3, 18, 2, 7, 128, 4, 6, 'srk', 'mfma4'),           # README's neuralsde_3_18 at H = 128 (net matrices parked in LDS)
    (3, 18, 2, 8, 64, 4, 6, 'milstein', 'auto'),        # Milstein through a diffusion net (dense dg/dy)
    (5, 15, 1, 8, 32, 4, 6, 'milstein', 'auto'),
    # round 4: per-row output selection (the fused gather of NeuralSDE.forward), SRK with the forward on 16-row
    # tiles (the adjoint walks the same saves on 4-row tiles), a 50-step solve with sparse outputs, more than 9 knots
    (4, 17, 2, 11, 64, 5, 9, 'euler', 'auto', {'row_out': True}),
    (3, 18, 2, 10, 64, 6, 8, 'srk', 'auto', {'row_out': True}),
    (4, 17, 2, 20, 64, 5, 7, 'srk', 'mfma16'),
    (6, 17, 2, 19, 128, 7, 8, 'srk', 'mfma16'),
    (4, 17, 2, 8, 32, 4, 51, 'euler', 'auto', {'ts': [0.0, 25.0, 50.0]}),
    (2, 16, 2, 9, 64, 5, 14, 'milstein', 'auto', {'ts': [0.0, 4.5, 13.0]}),
]


@pytest.mark.parametrize('case', FD_CASES)
def test_fused_backward_vs_finite_differences_of_the_numpy_oracle(case):
    io, no, NL, B, H, C, L, method, kernel = case[:9]
    extra = case[9] if len(case) > 9 else {}
    pr = make_problem(900 + io + no, io, no, NL, B, H, C, L)
    ts = np.asarray(extra['ts'], np.float32) if 'ts' in extra else pr['times']
    dW = draw_dW(900, ts, 1.0, B, H)
    rng = np.random.default_rng(901)
    T = len(ts)
    row_out = rng.integers(0, T, size=B).astype(np.int32) if extra.get('row_out') else None
    if row_out is not None:
        row_out[:2] = (0, T - 1)                 # the initial state and the last output are both somebody's row
    wsum = rng.standard_normal((B, H) if row_out is not None else (T, B, H))
    spec = param_spec(io, no, NL, C, H)
    dU = None
    if method == 'srk':      # space-time Levy integrals on the scale of the increments (h = 1)
        dU = (0.5 * dW + np.sqrt(1.0 / 12) * rng.standard_normal(dW.shape)).astype(np.float32)

    def oracle_loss(params, y0):
        ys, _ = O.solve_diffusion_model(params, io, no, pr['coeffs'], pr['times'], y0, ts, 1.0, dW, method=method, dtype=np.float64, dU=dU)
        if row_out is not None:                  # NeuralSDE.forward's gather (neuralsde.py:115-116): row b reads output row_out[b]
            ys = ys[row_out, np.arange(B)]
        return float((ys * wsum).sum())

    m = S.Diffusion_model(C, H, H, NL, input_option=io, noise_option=no)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pr['params'].items()})
    m = m.to(DEV)
    m.set_X(torch.from_numpy(pr['coeffs']).to(DEV), torch.from_numpy(pr['times']).to(DEV))
    y0 = torch.from_numpy(pr['y0']).to(DEV).requires_grad_(True)
    opts = {'kernel': kernel, 'strict': True}
    if row_out is not None:
        opts['row_out'] = torch.from_numpy(row_out).to(DEV)
    ys = S.sdeint(m, y0, torch.from_numpy(ts).to(DEV),
                  bm=_ReplayBM(torch.from_numpy(dW).to(DEV), None if dU is None else torch.from_numpy(dU).to(DEV)), method=method, dt=1.0,
                  options=opts)
    assert tuple(ys.shape) == tuple(wsum.shape)
    if kernel == 'mfma16' and method == 'srk':       # the configuration under test really is the 16-row-tile SRK forward
        model = S.engine.model_struct(C, H, H, NL, io, no)
        assert S.engine.forward_path(model, B, L, dW.shape[0], method='srk', kernel='mfma16') == 'mfma-srk'
        assert S.engine.backward_mode(model, B, L, S.engine.step_grid(ts, 1.0, pr['times'], DEV), 'srk', 'mfma16') == 1
    (ys * torch.from_numpy(wsum.astype(np.float32)).to(DEV)).sum().backward()
    grads = {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in m.named_parameters() if p.grad is not None}
    gy0 = y0.grad.cpu().numpy().astype(np.float64)

    p64 = {k: np.asarray(v, np.float64) for k, v in pr['params'].items()}
    y64 = pr['y0'].astype(np.float64)
    for trial in range(3):      # random directions over ALL parameters and y0 (a relu kink on the segment would show as an outlier)
        vdir = {n: rng.standard_normal(s) / np.sqrt(np.prod(s)) for n, s in spec}
        vy = rng.standard_normal(y64.shape) / np.sqrt(y64.size)
        eps = 1e-6       # (1e-5 leaves 1e-3 of truncation error in the SRK cases; below 1e-6 nothing changes: profiles/r05_grad_margins.txt)
        up = oracle_loss({k: p64[k] + eps * vdir[k] for k in p64}, y64 + eps * vy)
        dn = oracle_loss({k: p64[k] - eps * vdir[k] for k in p64}, y64 - eps * vy)
        fd = (up - dn) / (2 * eps)
        an = sum(float((grads[k] * vdir[k]).sum()) for k in grads) + float((gy0 * vy).sum())
        if os.environ.get('SNSDE_GRAD_MARGINS'):
            with open(os.environ['SNSDE_GRAD_MARGINS'], 'a') as fh:
                fh.write(f'fd - - - - - {case[:9]} {abs(an - fd) / max(abs(fd), 1.0):.3e} 0\n')
        assert abs(an - fd) <= FD_TOL * max(abs(fd), 1.0), (case, trial, an, fd)


# ---- DistributedDataParallel over NCCL (= RCCL) ----------------------------------------------------------------------------
def test_hip_engine_under_ddp_nccl_matches_the_single_process_full_batch_gradient():
    """One process per visible GPU (world size 1 on a single-GPU box, device_count otherwise): the fused HIP solve inside
    DistributedDataParallel with the parameter arena and a graph-captured step; every rank checks its sharded
    trajectories bit-for-bit against the single-process solve and the all-reduced gradient against the full-batch one."""
    n = max(1, torch.cuda.device_count())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', '29533', os.path.join(ROOT, 'tests', 'ddp_gpu_worker.py')]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f'ddp worker ok world={n}' in r.stdout


def test_training_driver_on_gpu_uses_the_fused_path_and_learns(monkeypatch):
    """train.main (the engine's common_sde.py equivalent; benchmark_classification/common_sde.py:248-298) on cuda: every
    solve of training and evaluation goes through the HIP engine (the tensor-op loop is disabled for the test), the
    training loss falls, the metrics are consistent and the best model is restored."""
    from stable_neural_sdes_amd import train as T
    from tests.test_train_cpu import synthetic_loader
    dev = torch.device('cuda')
    torch.manual_seed(3)
    L, C, H = 12, 4, 32
    times, train = synthetic_loader(256, L, C, 2, 64, seed=1)
    _, val = synthetic_loader(128, L, C, 2, 128, seed=2)
    _, test = synthetic_loader(128, L, C, 2, 128, seed=3)

    def no_loop(*a, **k):
        raise AssertionError('the tensor-op loop ran on a CUDA training step')
    monkeypatch.setattr(S.torchsde, '_sdeint_torch', no_loop)
    factory = T.make_model('neurallnsde', C, 1, H, H, 2, initial=True)
    res = T.main(None, 'neurallnsde', times, train, val, test, dev, factory, 2, 6, 1e-2, dict(method='euler'), 'valloss', log=None,
                 graph_steps=False)      # (eager steps; the default replays them from a graph: next test)
    losses = [h.train_metrics.loss for h in res.history]
    assert len(losses) == 6 and losses[-1] < losses[0], losses
    assert res.train_metrics.dataset_size == 256 and res.val_metrics.confusion.sum() == 128
    assert res.test_metrics.auroc > 0.7, res.test_metrics            # the label is a function of the series' slope
    assert res.memory_usage is not None and res.memory_usage > 0
    assert getattr(res.model.model.func, '_snsde_flat', None) is not None    # the parameter arena was in use


def test_training_driver_with_graph_replayed_steps(monkeypatch):
    """train.main(graph_steps=True): after three eager batches per batch shape the training step is replayed from a CUDA/HIP
    graph (train.GraphedStep) - same recipe, same learning behaviour; the ReduceLROnPlateau change of the rate drops the
    recordings and re-captures."""
    from stable_neural_sdes_amd import train as T
    from tests.test_train_cpu import synthetic_loader
    dev = torch.device('cuda')
    torch.manual_seed(3)
    L, C, H = 12, 4, 32
    times, train = synthetic_loader(288, L, C, 2, 64, seed=1)          # four full batches of 64 and one of 32 per epoch
    _, val = synthetic_loader(128, L, C, 2, 128, seed=2)
    _, test = synthetic_loader(128, L, C, 2, 128, seed=3)
    made = []
    orig = T.GraphedStep

    class Spy(orig):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(T, 'GraphedStep', Spy)
    factory = T.make_model('neurallnsde', C, 1, H, H, 2, initial=True)
    res = T.main(None, 'neurallnsde', times, train, val, test, dev, factory, 2, 8, 1e-2, dict(method='euler'), 'valloss', log=None,
                 )                     # graph_steps=None: replayed wherever eligible (one process, CUDA)
    losses = [h.train_metrics.loss for h in res.history]
    assert len(losses) == 8 and losses[-1] < losses[0], losses
    assert res.test_metrics.auroc > 0.7, res.test_metrics
    gs = made[0]
    assert gs.replays >= 8 * 5 - 2 * (3 + 1) - 8          # everything but the warm-up / capture batches of the two shapes (and re-captures)
    assert all(e['graph'] is not None for e in gs.entries.values()) and len(gs.entries) == 2


def test_graphed_step_falls_back_to_eager_steps_when_the_model_cannot_be_recorded():
    """a model whose step is not capture-safe (a host synchronisation inside forward) trained before graph replay became
    the default and must keep training: GraphedStep gives the recording up, logs why and runs eager steps - with the reference
    loop's per-batch `except AssertionError` (common_sde.py:157-166) around them."""
    from stable_neural_sdes_amd import train as T
    from tests.test_train_cpu import synthetic_loader
    dev = torch.device('cuda')
    torch.manual_seed(5)
    L, C, H = 12, 4, 32
    times, train = synthetic_loader(256, L, C, 2, 64, seed=1)
    _, val = synthetic_loader(64, L, C, 2, 64, seed=2)
    calls = {'n': 0}

    class Syncing(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, *a, **k):
            out = self.inner(*a, **k)
            calls['n'] += 1
            if calls['n'] == 2:
                assert False, 'a failing batch'          # swallowed like the reference does
            float(out.sum().item())                      # host sync: illegal while a stream is capturing
            return out

    def factory():
        model, reg = T.make_model('neurallnsde', C, 1, H, H, 2, initial=True)()
        return Syncing(model), reg
    msgs = []
    res = T.main(None, 'neurallnsde', times, train, val, val, dev, factory, 2, 4, 1e-2, dict(method='euler'), 'valloss', log=msgs.append)
    losses = [h.train_metrics.loss for h in res.history]
    assert len(losses) == 4 and losses[-1] < losses[0], losses
    assert any('cannot be recorded' in m for m in msgs) and any('Caught AssertionError' in m for m in msgs), msgs


PAD_CASES = [
    # io, no, NL, B, H, HH, C, L, ts, dt, method     hidden sizes without an MFMA instantiation: solved zero-padded
    (4, 17, 2, 21, 48, 48, 5, 9, [0, 3.5, 8], 1.0, 'euler'),
    (6, 17, 3, 9, 100, 100, 3, 9, [0, 8], 0.5, 'milstein'),
    (3, 18, 2, 13, 40, 24, 5, 9, [0, 8], 1.0, 'euler'),          # HH != H (latent-only drifts), diffusion net
    (2, 16, 1, 7, 200, 200, 4, 8, [0, 2.5, 7], 1.0, 'srk'),
    (5, 6, 2, 9, 24, 72, 3, 8, [0, 7], 1.0, 'milstein'),         # sigma_diag: the padded state components random-walk, unread
    (1, 13, 4, 11, 96, 80, 3, 8, [0, 7], 1.0, 'euler'),
]


@pytest.mark.parametrize('ci', range(len(PAD_CASES)))
def test_uninstantiated_hidden_sizes_run_zero_padded_on_the_mfma_kernels(ci, monkeypatch):
    """engine.padding_plan: H not in {16, 32, 64, 128, 256} or HH != H used to land on the generic VALU kernels; the
    zero-padded model is exact.  States and gradients vs float64 autograd through the tensor-op loop on replayed increments,
    and the kernel family actually launched must be an MFMA one at the padded width."""
    io, no, NL, B, H, HH, C, L, ts, dt, method = PAD_CASES[ci]
    rng = np.random.default_rng(4000 + ci)
    pr = make_problem(4000 + ci, io, no, NL, B, H, C, L)          # (inputs; the parameters are redrawn below for HH)
    ts = np.asarray(ts, np.float32)
    torch.manual_seed(ci)
    dW = draw_dW(4000 + ci, ts, dt, B, H)
    dU = None
    if method == 'srk':
        g0, g1 = O.step_grid(ts, dt)[:2]
        hh = (g1 - g0).astype(np.float32).reshape(-1, 1, 1)
        dU = (hh * (0.5 * dW + np.sqrt(hh / 12) * rng.standard_normal(dW.shape).astype(np.float32))).astype(np.float32)
    wsum = rng.standard_normal((len(ts), B, H)).astype(np.float32)
    ref_model = S.Diffusion_model(C, H, HH, NL, input_option=io, noise_option=no)
    with torch.no_grad():
        for p in ref_model.parameters():
            p.mul_(1.3)
    state = {k: v.clone() for k, v in ref_model.state_dict().items()}

    def build(dtype, device):
        m = S.Diffusion_model(C, H, HH, NL, input_option=io, noise_option=no)
        m.load_state_dict(state)
        m = m.to(device=device, dtype=dtype)
        m.set_X(torch.from_numpy(pr['coeffs']).to(device=device, dtype=dtype), torch.from_numpy(pr['times']).to(device))
        return m, torch.from_numpy(pr['y0']).to(device=device, dtype=dtype).requires_grad_(True)

    m64, y64 = build(torch.float64, 'cpu')
    want = S.sdeint(m64, y64, torch.from_numpy(ts), method=method, dt=dt, options={'backend': 'torch'},
                    bm=_ReplayBM(torch.from_numpy(dW).double(), None if dU is None else torch.from_numpy(dU).double()))
    (want * torch.from_numpy(wsum).double()).sum().backward()

    launched = []
    real = S.engine.SolveCall

    class Spy(real):
        def __init__(self, model, *a, **k):
            launched.append((model.hidden_channels, model.hidden_hidden_channels))
            super().__init__(model, *a, **k)
    monkeypatch.setattr(S.engine, 'SolveCall', Spy)
    m, y0 = build(torch.float32, DEV)
    got = S.sdeint(m, y0, torch.from_numpy(ts).to(DEV), method=method, dt=dt,
                   bm=_ReplayBM(torch.from_numpy(dW).to(DEV), None if dU is None else torch.from_numpy(dU).to(DEV)))
    (got * torch.from_numpy(wsum).to(DEV)).sum().backward()
    P = next(p for p in (16, 32, 64, 128, 256) if p >= max(H, HH))
    assert launched and all(dims == (P, P) for dims in launched), launched
    assert tuple(got.shape) == (len(ts), B, H)
    scale = max(float(want.detach().abs().max()), 1.0)
    assert float((got.detach().double().cpu() - want.detach()).abs().max()) <= 2e-4 * scale

    def close(g, ref, name):
        grad_close(g, ref, name, GRAD_TOL['pad'], f'pad{ci}')
    close(y0.grad, y64.grad, 'y0')
    ref = dict(m64.named_parameters())
    for name, p in m.named_parameters():
        gr = ref[name].grad
        if gr is None or float(gr.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) < 1e-6, name
            continue
        close(p.grad, gr, name)
    # inference path as well, and Philox increments: the real components of the padded solve = the generic kernel's solve
    with torch.no_grad():
        a = S.sdeint(m, y0.detach(), torch.from_numpy(ts).to(DEV), method=method, dt=dt, options={'seed': 5})
        b = S.sdeint(m, y0.detach(), torch.from_numpy(ts).to(DEV), method=method, dt=dt, options={'seed': 5, 'kernel': 'generic'})
    assert float((a - b).abs().max()) <= 2e-4 * max(float(b.abs().max()), 1.0)


def test_bench_runs_its_rccl_branch_on_one_gpu_and_emits_the_contract_line():
    """`python bench.py --full` with SNSDE_BENCH_FORCE_DIST=1: the process group (nccl = RCCL), the barrier / max-over-ranks timing and
    the K5 gradient all-reduce run at world size 1; the last stdout line is the contract's JSON with roofline objects on the
    headline and on the strong-scaling legs."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SNSDE_BENCH_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29533', HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--full', '--steps', '5', '--warmup', '2', '--no-cpu-baseline'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout.strip().splitlines()[-1]
    assert len(text) < 4096, len(text)                  # the driver keeps a bounded tail of stdout (BENCH_r05: 21 KB line, parsed = null)
    line = json.loads(text)
    assert line['n_gpus'] == 1 and line['steps'] == 5 and line['unit'] == 'row-steps/s' and line['value'] > 1e7
    assert 0.0 < line['roofline']['frac'] < 1.0 and line['roofline']['kernel_ms'] <= line['ms_per_step']
    assert 0.0 < line['summary']['K3_strong']['frac'] < 1.0 and 0.0 < line['summary']['K5_strong_train']['train_frac'] < 1.0
    # the full record (every leg with its own roofline object, timing spreads, provenance) is a file beside the repo copy
    full = json.load(open(os.path.join(root, line['full_record'])))
    assert full['roofline']['traffic_source'] and full['value'] == line['value']
    for leg in ('K3_strong', 'K5_strong_train'):
        assert 0.0 < full['extra'][leg]['roofline']['frac'] < 1.0, leg


def test_plain_bench_run_times_the_given_steps_and_dumps_what_the_last_step_computed(tmp_path):
    """`python bench.py` without --full: the result line carries the contract keys and none of the --full figures, `steps` is the
    number asked for, and --dump-outputs writes the last timed solve's states - the same array whatever the step count (seeded
    inputs, fixed Philox seed) and the one a direct SolveCall on bench.py's inputs returns."""
    import json
    import bench
    dumps = []
    for steps in (3, 7):
        d = tmp_path / f'steps{steps}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', str(steps), '--warmup', '1', '--dump-outputs', str(d)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line['steps'] == steps and line['warmup'] == 1 and line['n_gpus'] == 1 and line['dtype'] == 'f32'
        assert line['unit'] == 'row-steps/s' and line['higher_is_better'] is True and line['value'] > 1e7
        assert abs(line['value'] - bench.B * bench.NSTEP / (line['ms_per_step'] * 1e-3)) <= 1e-6 * line['value']
        assert not {'roofline', 'cpu_baseline', 'summary', 'full_record'} & set(line), sorted(line)
        assert sorted(os.listdir(d)) == ['ys.npy']
        ys = np.load(d / 'ys.npy')
        assert ys.dtype == np.float32 and ys.shape == (2, bench.B, bench.H) and np.isfinite(ys).all()
        dumps.append(ys)
    assert np.array_equal(dumps[0], dumps[1])
    dev = torch.device(DEV)
    pr, _, flat, coeffs, y0 = bench.build_inputs(dev, 0)
    model = S.engine.model_struct(bench.C, bench.H, bench.H, bench.NL, bench.IO, bench.NO)
    grid = S.engine.step_grid(np.array([0.0, float(bench.NSTEP)], np.float32), 1.0, pr['times'], dev)
    ys = S.engine.SolveCall(model, flat, coeffs, grid, y0, method='euler', seed=2024).launch()
    assert np.array_equal(ys.cpu().numpy(), dumps[0])
