"""Resumable solves on the host: snsde_solve_forward_at's exports and validation codes, SolveConfig left alone, and the front
end's extra / extra_solver_state / options['step_offset'] on CPU tensors with a deterministic Brownian stub.  No GPU compute."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stable_neural_sdes_amd as S
from stable_neural_sdes_amd import _lib, engine
from tests.global_rows_cases import KNOTS, STEPS, elementwise_model
from tests.helpers import make_problem

ERR_DIMS, ERR_UNSUPPORTED = -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the descriptor as it was before this entry point existed: the feature adds no field
SOLVE_FIELDS = ('struct_size', 'model', 'batch', 'knots', 'n_steps', 'n_out', 'method', 'kernel', 'flags', 'members', 'row_offset', 'seed',
                'params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'dW', 'ys', 'traj', 'dW_out', 'srk_tab', 'dU', 'dU_out', 'act_save',
                'stage_save', 'seed_dev', 'noise_table', 'row_out', 'z0_weight', 'z0_bias', 'workspace', 'workspace_bytes', 'kl_column1',
                'kl_prior_a', 'kl_prior_b', 'reserved2', 'global_rows', 'samples', 'reserved3')


# ---- C ABI ------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'snsde.h')).read()
    assert re.search(r'^SNSDE_API\s+int\s+snsde_solve_forward_at\(const snsde_solve\* s, int64_t step_offset, void\* hip_stream\);', header, re.M)
    assert 'snsde_solve_forward_at' in _lib.EXPORTS
    L = _lib.lib()
    assert L.snsde_solve_forward_at.argtypes == [C.POINTER(_lib.Solve), C.c_int64, C.c_void_p]
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\bT snsde_solve_forward_at$', dyn, re.M)
    # ... and nothing else about the ABI moved
    assert C.sizeof(_lib.Solve) == 304 and L.snsde_version() == 2
    assert tuple(n for n, _ in _lib.Solve._fields_) == SOLVE_FIELDS


def _solve(model, batch=8, method=0, **kw):
    s = _lib.Solve()
    s.model, s.batch, s.knots, s.n_steps, s.n_out, s.method = model, batch, KNOTS, STEPS, 2, method
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _launch_rc(s, step_offset=None, workspace_bytes=0):
    """The launch validates before it touches a buffer: dummy non-null pointers, an error code back (a descriptor that passes the
    validation stops at SNSDE_ERR_WORKSPACE).  step_offset=None: snsde_solve_forward."""
    s.workspace_bytes = workspace_bytes
    for f in ('params', 'coeffs', 'step_tab', 'out_step', 'out_w', 'y0', 'ys', 'workspace'):
        setattr(s, f, C.c_void_p(4096))
    if step_offset is None:
        return _lib.lib().snsde_solve_forward(C.byref(s), None)
    return _lib.lib().snsde_solve_forward_at(C.byref(s), step_offset, None)


def test_validation_codes():
    model = elementwise_model(32)
    accepted = _launch_rc(_solve(model))      # (a valid descriptor without a workspace: the code behind every check of the offset)
    assert accepted not in (0, ERR_DIMS, ERR_UNSUPPORTED)
    assert _launch_rc(_solve(model), 0) == accepted
    assert _launch_rc(_solve(model), 5) == accepted
    assert _launch_rc(_solve(model), 2 ** 31 - 1 - STEPS) == accepted      # the last global step is INT32_MAX - 1: the largest legal offset
    assert _launch_rc(_solve(model), -1) == ERR_DIMS
    assert _launch_rc(_solve(model), 2 ** 31 - STEPS) == ERR_DIMS
    assert _launch_rc(_solve(model), 2 ** 40) == ERR_DIMS
    assert _launch_rc(_solve(model, act_save=C.c_void_p(4096)), 5) == ERR_UNSUPPORTED
    assert _launch_rc(_solve(model, method=2, srk_tab=C.c_void_p(4096), stage_save=C.c_void_p(4096)), 5) == ERR_UNSUPPORTED
    assert _launch_rc(_solve(model, z0_weight=C.c_void_p(4096), z0_bias=C.c_void_p(4096)), 5) == ERR_UNSUPPORTED
    # offset 0 is snsde_solve_forward: the same answer for a training descriptor
    assert _launch_rc(_solve(model, act_save=C.c_void_p(4096)), 0) == _launch_rc(_solve(model, act_save=C.c_void_p(4096)))
    assert _launch_rc(_solve(model, z0_weight=C.c_void_p(4096), z0_bias=C.c_void_p(4096)), 0) == \
        _launch_rc(_solve(model, z0_weight=C.c_void_p(4096), z0_bias=C.c_void_p(4096)))
    # plain outputs are accepted at an offset
    assert _launch_rc(_solve(model, traj=C.c_void_p(4096), dW_out=C.c_void_p(4096)), 5) == \
        _launch_rc(_solve(model, traj=C.c_void_p(4096), dW_out=C.c_void_p(4096)))


# ---- the offset is a stream coordinate, not a plan input ------------------------------------------------------------------------

def test_solve_config_stays_clean():
    assert 'step_offset' not in engine.SolveConfig._fields
    assert 'step_offset' not in inspect.signature(engine.SolveConfig.of).parameters
    p = inspect.signature(engine.SolveCall.__init__).parameters
    assert p['step_offset'].default == 0 and p['row_offset'].default == 0
    assert not any('OFFSET' in n for n in dir(_lib) if n.startswith('FLAG_'))


@pytest.mark.parametrize('bad', [-1, 2.0, '3', True, 2 ** 31])
def test_step_offset_must_be_a_non_negative_int(bad):
    with pytest.raises(ValueError, match='step_offset'):
        engine.check_step_offset(bad)
    m, pr = _model()
    with pytest.raises(ValueError, match='step_offset'):
        S.sdeint(m, torch.from_numpy(pr['y0']), TS, dt=0.25, method='euler', bm=Stub(), options={'step_offset': bad})
    with pytest.raises(ValueError, match='step_offset'):
        S.sdeint_ensemble([m, m], torch.from_numpy(pr['y0'])[None].repeat(2, 1, 1), TS, dt=0.25, method='euler', bm=Stub(),
                          options={'step_offset': bad})


def test_check_step_offset_bounds_the_last_global_step():
    assert engine.check_step_offset(0) == 0 and engine.check_step_offset(np.int64(7), 3) == 7
    assert engine.check_step_offset(2 ** 31 - 1 - 37, 37) == 2 ** 31 - 1 - 37
    with pytest.raises(ValueError, match='2\\*\\*31'):
        engine.check_step_offset(2 ** 31 - 37, 37)


# ---- front end on CPU tensors ---------------------------------------------------------------------------------------------------

TS = torch.tensor([0.0, 0.75, 2.25, 4.0])


def _model(B=4, H=16, C_=3, L=6, io=4, no=17, seed=5):
    pr = make_problem(seed, io, no, 2, B, H, C_, L, times=np.array([0., 0.7, 1.9, 2.4, 4.1, 5.][:L], np.float32))
    m = S.Diffusion_model(C_, H, H, 2, input_option=io, noise_option=no)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.from_numpy(pr['params'][name]))
    m.requires_grad_(False)
    m.set_X(torch.from_numpy(pr['coeffs']), torch.from_numpy(pr['times']))
    return m, pr


class Stub:
    """A Brownian object whose value depends on (ta, tb) only: re-asking an interval repeats it, so it carries its path across calls."""

    def __init__(self, shape=(4, 16)):
        self.shape, self.asked = shape, []

    def __call__(self, ta, tb=None, return_U=False, **kw):
        ta, tb = float(ta), float(tb)
        self.asked.append((ta, tb))
        gen = torch.Generator().manual_seed(int(round(ta * 4096)) * 1000003 + int(round(tb * 4096)))
        h = torch.tensor(tb - ta, dtype=torch.float32)
        W = torch.randn(self.shape, generator=gen) * h.sqrt()
        if not return_U:
            return W
        return W, h * (0.5 * W + (h / 12).sqrt() * torch.randn(self.shape, generator=gen))


@pytest.mark.parametrize('method', ['euler', 'srk'])
def test_three_chained_calls_equal_the_single_call(method):
    m, pr = _model()
    y0 = torch.from_numpy(pr['y0'])
    whole = S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method=method)
    assert tuple(whole.shape) == (4, 4, 16)
    y, state, steps = y0, None, 0
    for k in range(3):
        ys, state = S.sdeint(m, y, TS[k:k + 2], bm=Stub(), dt=0.25, method=method, extra=True, extra_solver_state=state)
        steps += int(round(float(TS[k + 1] - TS[k]) / 0.25))
        # the state: a 1-tuple of one int64 CPU tensor [steps taken so far, key, keyed]; a bm carries its own path (keyed = 0)
        assert isinstance(state, tuple) and len(state) == 1 and state[0].dtype == torch.int64 and state[0].device.type == 'cpu'
        assert state[0].tolist() == [steps, 0, 0]
        assert torch.equal(ys[0], y) and torch.equal(ys[1], whole[k + 1])
        y = ys[-1]
    assert steps == 16
    # a continuation without extra=True returns the result alone
    last = S.sdeint(m, whole[2], TS[2:], bm=Stub(), dt=0.25, method=method, extra_solver_state=(torch.tensor([9, 0, 0]),))
    assert torch.is_tensor(last) and torch.equal(last[1], whole[3])
    # with a caller's bm the low-level knob is accepted and moves nothing
    assert torch.equal(S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method=method, options={'step_offset': 6}), whole)


def test_extra_returns_the_key_the_solve_drew_from():
    m, pr = _model()
    y0 = torch.from_numpy(pr['y0'])
    ys, state = S.sdeint(m, y0, TS[:2], dt=0.25, method='euler', options={'seed': 11}, extra=True)
    assert state[0].tolist() == [3, 11, 1]
    assert torch.equal(ys, S.sdeint(m, y0, TS[:2], dt=0.25, method='euler', options={'seed': 11}))
    torch.manual_seed(3)
    _, fresh = S.sdeint(m, y0, TS[:2], dt=0.25, method='euler', extra=True)      # no seed given: the call's own draw comes back
    torch.manual_seed(3)
    assert fresh[0].tolist() == [3, int(torch.empty((), dtype=torch.int64).random_().item()), 1]
    _, big = S.sdeint(m, y0, TS[:2], dt=0.25, method='euler', options={'seed': 2 ** 64 - 2, 'step_offset': 0}, extra=True)
    assert big[0].tolist() == [3, -2, 1]      # the key's 64 bits as an int64


def test_refusals():
    m, pr = _model()
    y0 = torch.from_numpy(pr['y0'])
    keyed = (torch.tensor([3, 11, 1]),)
    # a differentiated continuation
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint(m, y0.clone().requires_grad_(True), TS, bm=Stub(), dt=0.25, method='euler', options={'step_offset': 3})
    m.requires_grad_(True)
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', extra_solver_state=(torch.tensor([3, 0, 0]),))
    with pytest.raises(ValueError, match='inference only'):
        S.sdeint_ensemble([m, m], y0[None].repeat(2, 1, 1), TS, bm=Stub(), dt=0.25, method='euler',
                          options={'step_offset': 3, 'ensemble_grad': True})
    m.requires_grad_(False)
    # the tensor-op loop would draw from a torch generator: never a silent continuation on different noise
    for kw in (dict(options={'step_offset': 3}), dict(options={'step_offset': 3, 'seed': 11}), dict(extra_solver_state=keyed),
               dict(options={'step_offset': 3, 'backend': 'torch'}), dict(options={'step_offset': 3, 'samples': 2})):
        with pytest.raises(NotImplementedError, match='fused solve.*caller-supplied `bm`'):
            S.sdeint(m, y0, TS, dt=0.25, method='euler', **kw)
    with pytest.raises(NotImplementedError, match='fused solve.*caller-supplied `bm`'):
        S.sdeint_ensemble([m, m], y0[None].repeat(2, 1, 1), TS, dt=0.25, method='euler', options={'step_offset': 3})
    # a state and options that disagree
    with pytest.raises(ValueError, match="options\\['seed'\\].*disagrees"):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', options={'seed': 12}, extra_solver_state=keyed)
    with pytest.raises(ValueError, match="options\\['step_offset'\\].*disagrees"):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', options={'step_offset': 4}, extra_solver_state=keyed)
    with pytest.raises(ValueError, match='`bm` disagree'):
        S.sdeint(m, y0, TS, bm=Stub(), dt=0.25, method='euler', extra_solver_state=keyed)
    with pytest.raises(ValueError, match='`bm` disagree'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', extra_solver_state=(torch.tensor([3, 0, 0]),))
    # malformed states
    for bad in (torch.tensor([3, 11, 1]), (), (torch.tensor([3, 11]),), (torch.tensor([3., 11., 1.]),), (torch.tensor([-1, 11, 1]),),
                (torch.tensor([3, 11, 2]),), (torch.tensor([3, 11, 1]), torch.tensor([0])), ([3, 11, 1],)):
        with pytest.raises(ValueError, match='malformed'):
            S.sdeint(m, y0, TS, dt=0.25, method='euler', extra_solver_state=bad)
    # a key the host does not know
    with pytest.raises(ValueError, match='device-resident'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', options={'seed': torch.tensor([5])}, extra=True)
    # what stays unimplemented
    with pytest.raises(NotImplementedError, match='logqp'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', logqp=True, extra=True)
    with pytest.raises(NotImplementedError, match='adaptive'):
        S.sdeint(m, y0, TS, dt=0.25, method='euler', adaptive=True, extra=True)
