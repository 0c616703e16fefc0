"""Cases of tests/test_gpu_lean_windows.py and of the generator of its golden fixture (tests/golden/make_lean_windows.py).

The lean forward kernel (csrc/snsde_m4_kernel.h) moved instructions between the operand-read windows of its step loop
(LEAN_GPART_MODE, LEAN_CARRY_MODE): every value is computed by the same operations in the same order, so every output must
reproduce, bit for bit, what the library of the commit BEFORE that change wrote on the same GPU.  The fixture holds those outputs.

Each case is chosen for a boundary the change touches.  Main case: H = 128, two layers, C = 21 (two k-blocks of [X | tau]), B = 5
(a full 4-row tile and a one-row tile), N = 37 steps (two Philox refills, nine spline batches, a multiple of neither 4 nor 16).

run(name) launches one case and returns {array name: numpy array}.  States, trajectory and increments are stored whole; the saved
activations (37 x 3 x 5 x 128 floats per training case, most of the fixture's size otherwise) as one 16-byte SHA-256 prefix per
(step, slot) plane: no less strict than the bytes, and a mismatch still names the step and the layer."""
import hashlib
from collections import namedtuple

import numpy as np

DEV = 'cuda:0'
N, B = 37, 5
SEED = 20261020

# One launch per case as tests/kernel_cases.py describes launches (the forward kernel it is meant to run included), plus what that
# record does not carry: further SolveCall keywords (step_offset, lean_general) and the lean instantiation the launch must report.
Case = namedtuple('Case', 'launch kw variant')


def _c(io=4, H=128, C=21, B_=B, L=N + 1, ts=(0, N), method='euler', kernel='auto', train=False, supplied=False, bf16=False, fwd='lean',
       variant='specialised', **kw):
    from tests.kernel_cases import launch
    return Case(launch('lean windows', io, 17, 2, B_, H, C, L, [float(t) for t in ts], 1.0, method, kernel, train=train, supplied=supplied,
                       bf16=bf16, fwd=fwd), kw, variant)


CASES = {
    # the main case, K2's (4, 17) and the geometric drift (6, 17), inference and training mode
    'main_4_17': _c(), 'main_6_17': _c(io=6),
    'train_4_17': _c(train=True), 'train_6_17': _c(io=6, train=True),
    # output schedules: every step, every 7th step, one output time off the grid (interpolated from yold)
    'every': _c(ts=range(N + 1)), 'seventh': _c(ts=list(range(0, N, 7)) + [N]), 'off_grid': _c(ts=(0, 20.5, N)),
    # a resumed solve: the Philox batches are cut on the global step
    'resumed': _c(step_offset=5),
    # the general instantiation: the same model under SNSDE_FLAG_LEAN_GENERAL, with supplied increments, and with Milstein
    'general': _c(lean_general=True, variant='general'),
    'general_supplied': _c(lean_general=True, supplied=True, variant='general'),
    'general_milstein': _c(method='milstein', kernel='mfma4', lean_general=True, variant='general'),
    'general_train': _c(lean_general=True, train=True, variant='general'),
    # other widths
    'h64': _c(H=64, C=5, kernel='mfma4', variant='general'), 'h32': _c(H=32, C=5, kernel='mfma4', variant='general'),
    # bf16 operands past the step-table refill at step 128: the moved reads of row n + 1 cross it
    'bf16_refill': _c(B_=4, L=131, ts=(0, 130), bf16=True, fwd='lean_bf16', variant=None),
}


def plane_digests(x):
    """(..., B, H) float32 -> (..., 16) uint8: the first 16 bytes of SHA-256 over each (B, H) plane's bytes."""
    x = np.ascontiguousarray(x)
    lead = x.shape[:-2]
    flat = x.reshape((-1,) + x.shape[-2:])
    out = np.stack([np.frombuffer(hashlib.sha256(p.tobytes()).digest()[:16], np.uint8) for p in flat])
    return out.reshape(lead + (16,))


def run(name):
    import torch
    from stable_neural_sdes_amd import engine
    from tests.helpers import assert_kernels, draw_dW, make_problem, param_spec
    case = CASES[name]
    c = case.launch
    pr = make_problem(11, c.io, c.no, c.NL, c.B, c.H, c.C, c.L)
    flat = torch.from_numpy(np.concatenate([pr['params'][n].reshape(-1) for n, _ in param_spec(c.io, c.no, c.NL, c.C, c.H)])).to(DEV)
    model = engine.model_struct(c.C, c.H, c.H, c.NL, c.io, c.no)
    ts = np.array(c.ts, np.float32)
    grid = engine.step_grid(ts, c.dt, pr['times'], torch.device(DEV))
    assert grid.N == int(c.ts[-1]), (name, grid.N)
    dW = torch.from_numpy(draw_dW(3, ts, c.dt, c.B, c.H)).to(DEV) if c.supplied else None
    call = engine.SolveCall(model, flat, torch.from_numpy(pr['coeffs']).to(DEV), grid, torch.from_numpy(pr['y0']).to(DEV), dW=dW,
                            method=c.method, kernel=c.kernel, seed=SEED, row_offset=3, precision='bf16' if c.bf16 else 'fp32',
                            save_traj=c.train, save_dW=c.train, save_act=c.train, **case.kw)
    assert_kernels(call, fwd=c.fwd)
    if case.variant is not None:
        assert engine.lean_variant(call) == case.variant, (name, engine.lean_variant(call))
    ys = call.launch()
    torch.cuda.synchronize()
    out = {'ys': ys.cpu().numpy()}
    if c.train:
        out['traj'] = call.traj.cpu().numpy()
        out['dW_out'] = call.dW_out.cpu().numpy()
        out['act_save_sha'] = plane_digests(call.act_save.cpu().numpy())
    return out
