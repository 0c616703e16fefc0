"""Cases of the GPU tests that are about ONE kernel, each with the forward and the adjoint kernel it is meant to run.

Plain data, importable without a GPU.  The GPU tests (tests/test_gpu_parity.py, tests/test_gpu_w4.py, tests/test_gpu_kernel_census.py)
parametrise over these tables and assert the kernels on the descriptor they launched (engine.forward_kernel / engine.backward_kernel,
the names of _lib.FWD_KERNELS / _lib.REV_KERNELS); tests/test_kernel_census_cpu.py rebuilds every case's descriptor on the host,
asserts that the plan names those kernels, and that the union of the cases covers every kernel and every compiled instantiation of
the two-tile kernels.  A case whose plan moves to another kernel fails there, without a GPU.  STEP_OFFSET_CASES and
POISONED_TRAINING_CASES (tests/test_gpu_step_offset.py, tests/test_gpu_poisoned_allocations.py) are held to their kernels there too.

`fwd` / `rev`: the kernel names; rev = None for a case that runs no backward.  The case tuples of the tests that existed before this
module were moved here unchanged."""
import ctypes as C
from collections import namedtuple

import numpy as np

# One launch of a kernel-specific test, as the census rebuilds it: the model and problem sizes, the output grid, what the launch
# passes (kernel selector, A/B flags, training planes, supplied increments, per-row outputs) and the kernels it is meant to run.
Launch = namedtuple('Launch', 'test io no NL B H C L ts dt method kernel stream_all two_tile train supplied row_out bf16 exact fwd rev')


def launch(test, io, no, NL, B, H, C_, L, ts, dt, method='euler', kernel='auto', stream_all=False, two_tile=False, train=False,
           supplied=True, row_out=False, bf16=False, exact=False, fwd=None, rev=None):
    return Launch(test, io, no, NL, B, H, C_, L, ts, dt, method, kernel, stream_all, two_tile, train, supplied, row_out, bf16, exact, fwd, rev)


def grid_of(L, ts, dt, half_gap=False):
    """(ts, dt) of a case as its test resolves them: ts = None means ts = times = linspace(0, 1, L) with dt = the smallest knot gap
    (half of it for the SRK trajectory cases) unless the case names one."""
    if ts is None:
        ts = np.linspace(0, 1, L).astype(np.float32)
        dt = dt or max(float(np.diff(ts).min()), 1e-3) / (2 if half_gap else 1)
    return np.asarray(ts, np.float32), dt


def n_steps(L, ts, dt):
    from oracle import sde_oracle as O
    ts, dt = grid_of(L, ts, dt)
    return len(O.step_grid(ts, dt)[0]), len(ts)


def descriptor(c):
    """The snsde_solve descriptor of a Launch for the host-only queries: every field the plans read, dummy non-null pointers where
    the launch passes a buffer (no query dereferences them) - what engine.SolveCall fills in for the same arguments."""
    from stable_neural_sdes_amd import _lib, engine
    s = _lib.Solve()
    s.model = engine.model_struct(c.C, c.H, c.H, c.NL, c.io, c.no)
    N, T = n_steps(c.L, c.ts, c.dt)
    s.batch, s.knots, s.n_steps, s.n_out = c.B, c.L, N, T
    s.method = {'euler': _lib.EULER, 'milstein': _lib.MILSTEIN, 'srk': _lib.SRK}[c.method]
    s.kernel = _lib.KERNELS[c.kernel]
    s.flags = (_lib.FLAG_STREAM_ALL if c.stream_all else 0) | (_lib.FLAG_TWO_TILE if c.two_tile else 0)
    s.flags |= (_lib.FLAG_BF16_OPERANDS if c.bf16 else 0) | (_lib.FLAG_EXACT_ORDER if c.exact else 0)
    p = C.c_void_p(256)
    if c.supplied:
        s.dW = p
    if c.row_out:
        s.row_out = p
    if c.train:
        s.traj = s.act_save = p
        if not c.supplied or c.method == 'srk':
            s.dW_out = p
    if c.method == 'srk':
        s.srk_tab = p
        if c.supplied:
            s.dU = p
        if c.train:
            s.dU_out = s.stage_save = p
    return s


def delta_slots(c):
    """Delta planes per pass the adjoint of a training Launch leaves (snsde_save_layout, host-only): 0 where the adjoint sums the
    weight gradients itself or the solve has no MFMA adjoint - no coefficient gradient comes from such a solve's planes."""
    from stable_neural_sdes_amd import _lib
    s = descriptor(c)
    a, p, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().snsde_save_layout(C.byref(s), C.byref(a), C.byref(p), C.byref(d))
    return d.value if rc == 0 else 0


# The instantiation lists of the two-tile kernels, written out once.  (NHID, KUXT, SAVE): hidden layers between the first layer and
# the output layer, 16-wide k-blocks of [X(t) | sin t, cos t], 1 = also compiled in training mode.
M4S2_LIST = ((0, 0, 1), (1, 0, 1), (2, 0, 0), (0, 1, 1), (1, 1, 1), (0, 2, 1), (1, 2, 0))      # csrc/snsde_m4s2_h256.hip: SNSDE_M4S2_LIST
M4T_LIST = ((1, 2, 1), (1, 1, 1))                                                                # csrc/snsde_m4t_h128.hip: SNSDE_M4T_LIST
M4S2_REV_LIST = ((0, 1), (0, 0), (1, 1), (1, 0), (2, 1), (2, 0))                                 # csrc/snsde_m4s2_rev_h256.hip: SNSDE_M4S2_REV_LIST, (NHID, GEO)

TS8, DT8 = [0., 2.5, 6., 8.], 1.0      # the small grid of the two-tile tests: eight steps, one interpolated output

# ---- H = 256, two tiles per wave against the fully streamed kernel (test_gpu_parity.py) --------------------------------------------
# io, no, NL, C, B, method
H256_FWD_CASES = [(4, 17, 2, 14, 37, 'milstein'), (4, 17, 2, 14, 128, 'euler'), (6, 16, 2, 21, 9, 'euler'), (1, 13, 1, 3, 21, 'milstein'),
                  (3, 12, 2, 3, 5, 'euler'), (4, 9, 2, 40, 12, 'euler'), (2, 17, 3, 14, 8, 'euler')]
# (case index, train) where the plan names the two-tile kernel, and where it declines: KUXT = 3 and NHID = 2 with a control block are
# not in SNSDE_M4S2_LIST, (1, 2, 0) is compiled for inference only
H256_FWD_TWO_TILE = [(0, False), (0, True), (1, False), (1, True), (2, False), (3, False), (3, True), (4, False), (4, True)]
H256_FWD_DECLINES = [(2, True), (5, False), (5, True), (6, False), (6, True)]
# io, no, NL, C, B, method, row_out: the adjoint (every case on the two-tile adjoint; forward in training mode)
H256_REV_CASES = [(4, 17, 2, 14, 37, 'milstein', False), (4, 17, 2, 14, 128, 'euler', True), (6, 16, 2, 21, 9, 'euler', False),
                  (1, 13, 1, 3, 21, 'milstein', True), (3, 9, 2, 3, 5, 'euler', False), (5, 3, 1, 4, 12, 'milstein', False)]
H256_REV_FWD = ['lean_two_tile_h256', 'lean_two_tile_h256', 'lean_streamed_h256', 'lean_two_tile_h256', 'lean_two_tile_h256',
                'lean_two_tile_h256']      # (the two-tile arm's forward: (1, 2, 0) is inference only, so case 2 trains on the streamed forward)
H256_CHUNK_CASE = (4, 17, 2, 14, 23, 161)      # io, no, NL, C, B, L: 160 steps, more than one chunk of the step table
# io, no, C, B, method (NL = 2): H = 128 under SNSDE_FLAG_TWO_TILE against the lean kernel
H128_CASES = [(4, 17, 21, 64, 'euler'), (4, 17, 21, 37, 'milstein'), (6, 16, 5, 9, 'euler'), (3, 13, 3, 21, 'milstein')]

# ---- every compiled instantiation of the two-tile kernels at the smallest shapes (test_gpu_kernel_census.py) ------------------------
# (NHID, KUXT) -> io, no, NL, C, method: one model per SNSDE_M4S2_LIST entry; K5's (4, 17) model is the (1, 1) entry
M4S2_MODELS = {(0, 0): (1, 13, 1, 3, 'milstein'), (1, 0): (1, 9, 2, 3, 'euler'), (2, 0): (1, 17, 3, 3, 'euler'),
               (0, 1): (3, 6, 1, 3, 'milstein'), (1, 1): (4, 17, 2, 14, 'euler'), (0, 2): (6, 16, 1, 21, 'euler'),
               (1, 2): (2, 13, 2, 21, 'milstein')}
# (the models are ones whose float32 oracle stays within 3e-6 of the fp64 one on the grid below: at 4 x 9 x 256 outputs assert_parity's
#  99.99 % band allows no outlier at all, so a model that amplifies round-off - (2, 11) under Milstein, raw = t y with t up to 8, puts
#  the float32 ORACLE 5e-4 off and one element outside the band - would test its own dynamics, not the kernel)
M4S2_CASES = [(nhid, kuxt, train) for nhid, kuxt, save in M4S2_LIST for train in ((False, True) if save else (False,))]
M4T_MODELS = {(1, 2): (4, 17, 2, 21, 'euler'), (1, 1): (5, 13, 2, 3, 'milstein')}
M4T_CASES = [(nhid, kuxt, train) for nhid, kuxt, save in M4T_LIST for train in (False, True)]
# (NHID, GEO) -> io, no, NL, C, method, forward kernel of the training-mode launch: one model per SNSDE_M4S2_REV_LIST entry
M4S2_REV_MODELS = {(0, 0): (1, 13, 1, 3, 'milstein', 'lean_two_tile_h256'), (0, 1): (5, 3, 1, 4, 'euler', 'lean_two_tile_h256'),
                   (1, 0): (4, 17, 2, 14, 'euler', 'lean_two_tile_h256'), (1, 1): (6, 16, 2, 5, 'milstein', 'lean_two_tile_h256'),
                   (2, 0): (3, 12, 3, 3, 'euler', 'lean_streamed_h256'), (2, 1): (6, 17, 3, 14, 'milstein', 'lean_streamed_h256')}
CENSUS_B = (3, 9)      # one ragged tile; two tile pairs with a ragged second one

# ---- Euler through a diffusion net: the net kernel (m4n) or the general kernel's 4-row tiles (test_gpu_parity.py) -------------------
# make_plan sends Euler with a net to m4n behind a wide control path (C > 32: five k-blocks) and at H = 128 on 4-row tiles, and keeps
# the general kernel elsewhere
EULER_NET_CASES = [
    # io, no, NL, B, H, C, L     (Euler through a diffusion net on snsde_m4n_kernel.h: wide control paths behind the embedding - the
    (4, 18, 2, 19, 64, 69, 9),   #  sepsis channel count - and H = 128 on 4-row tiles)
    (6, 15, 3, 9, 128, 40, 8),
    (2, 14, 1, 13, 32, 33, 8),
    (1, 18, 2, 21, 128, 5, 9),
    (5, 19, 2, 11, 128, 3, 8),
    (4, 18, 2, 9, 32, 40, 9),    # one case on each side of both terms of the rule at the smallest shapes: C = 40 (> 32: the wide
    (4, 18, 2, 9, 32, 21, 9),    # control path's five k-blocks) against C = 21 behind the embedding at H = 32,
    (3, 15, 1, 9, 128, 3, 9),    # and H = 128 against H = 16 on a latent-only drift
    (3, 15, 1, 9, 16, 3, 9),
]
EULER_NET_FWD = ['m4n'] * 5 + ['m4n', 'general_m4', 'm4n', 'general_m4']      # (the adjoint is the general one on either side)

# ---- SRK / Milstein through the general and the net kernels (test_gpu_parity.py) ------------------------------------------------------
SRK_BWD_CASES = [
    # io, no, NL, B, H, C, L, ts, dt     (MFMA SRK forward + MFMA SRK adjoint + native parameter pass)
    (4, 17, 2, 11, 32, 5, 9, [0, 3.5, 8], 1.0),
    (6, 17, 3, 9, 64, 3, 9, [0, 8], 0.5),
    (2, 16, 1, 9, 16, 2, 12, None, 0.05),
    (1, 0, 2, 7, 32, 3, 8, [0, 7], 1.0),
    (3, 13, 2, 10, 64, 3, 8, [0, 2.5, 7], 1.0),
    (5, 12, 4, 6, 128, 3, 7, [0, 6], 1.0),
    (4, 17, 2, 21, 128, 21, 9, [0, 8], 1.0),
    (2, 3, 2, 9, 32, 3, 8, [0, 7], 1.0),             # closed-form table noise under SRK
    (6, 5, 1, 9, 64, 3, 8, [0, 3, 7], 0.5),
    (3, 11, 2, 9, 16, 3, 8, [0, 7], 1.0),
    (4, 1, 2, 9, 32, 5, 8, [0, 7], 1.0),
    (4, 9, 2, 9, 32, 5, 8, [0, 7], 1.0),             # y-only closed forms under SRK
    (1, 8, 2, 9, 16, 3, 8, [0, 3, 7], 0.5),
    (6, 10, 1, 9, 64, 3, 8, [0, 7], 1.0),
    (4, 17, 2, 9, 256, 14, 8, [0, 3, 7], 1.0),       # H = 256 (streamed weights): the torch_ists default method at the K5 width
    (6, 16, 1, 6, 256, 5, 7, [0, 6], 0.5),
    (4, 17, 2, 9, 64, 40, 8, [0, 3, 7], 1.0),        # wide control path (C > 32) under SRK
    (6, 13, 3, 7, 128, 69, 7, [0, 6], 1.0),
    (1, 18, 2, 9, 16, 3, 8, [0, 7], 0.5),            # SRK through a diffusion net: snsde_m4n_srk_reverse_kernel + weight-gradient
    (3, 15, 3, 8, 16, 4, 8, [0, 7], 1.0),            # jobs over the pass subsets / state planes of the four evaluations
    (1, 14, 1, 17, 32, 3, 9, [0, 2.5, 8], 0.5),
    (3, 18, 2, 33, 64, 5, 12, [0, 2.5, 11], 0.5),
    (5, 19, 2, 21, 64, 5, 9, [0, 8], 1.0),
    (4, 19, 2, 21, 128, 21, 10, [0, 9], 1.0),
    (2, 14, 2, 13, 32, 7, 9, [0, 3.5, 8], 0.5),
    (6, 15, 3, 9, 64, 40, 8, [0, 7], 1.0),
    (1, 18, 2, 37, 128, 5, 9, [0, 8], 1.0),
    (3, 18, 3, 11, 128, 5, 9, [0, 8], 0.5),
    (4, 18, 1, 11, 128, 69, 9, [0, 8], 1.0),
]

MIL_NET_BWD_CASES = [
    # io, no, NL, B, H, C, L, ts, dt     (Milstein through a diffusion net: snsde_m4n_mil_reverse_kernel - tangent + reverse pass
    (1, 18, 2, 9, 16, 3, 8, [0, 7], 0.5),            #  through the net per step - and the second-order weight-gradient jobs)
    (3, 15, 3, 8, 16, 4, 8, [0, 7], 1.0),
    (1, 14, 1, 17, 32, 3, 9, [0, 2.5, 8], 0.5),
    (3, 18, 2, 33, 64, 5, 12, [0, 2.5, 11], 0.5),
    (5, 19, 2, 21, 64, 5, 9, [0, 8], 1.0),
    (2, 14, 2, 13, 32, 7, 9, [0, 3.5, 8], 0.5),
    (6, 15, 3, 9, 64, 40, 8, [0, 7], 1.0),
    (6, 19, 4, 7, 32, 3, 8, [0, 7], 1.0),
    (4, 14, 1, 11, 128, 21, 9, [0, 8], 1.0),         # H = 128, one-layer net: matrices parked in LDS
    (4, 18, 2, 12, 64, 69, 9, [0, 4, 8], 1.0),       # the K4 channel count
]

SRK_CASES = [
    # io, no, NL, B, H, C, L, ts, dt
    (6, 17, 2, 19, 32, 5, 9, [0, 2.5, 8], 0.5),      # torch_ists / tutorial GSDE-SRK flavour
    (4, 17, 2, 37, 128, 21, 13, [0, 12], 1.0),
    (2, 16, 1, 9, 16, 2, 12, None, None),            # ts = times = linspace(0,1,12): interpolated outputs
    (1, 18, 2, 8, 24, 3, 8, [0, 7], 0.5),
    (3, 15, 3, 8, 16, 4, 8, [0, 7], 1.0),
    (0, 5, 2, 8, 12, 3, 8, [0, 7], 1.0),
    (5, 8, 2, 8, 10, 3, 8, [0, 3.5, 7], 0.25),
    (1, 0, 2, 5, 8, 3, 8, [0, 7], 1.0),
    (1, 12, 1, 9, 64, 3, 8, [0, 2.5, 7], 1.0),       # MFMA SRK variant: every drift family, H = 16 .. 128, NL 1 .. 4
    (3, 13, 3, 21, 32, 3, 9, [0, 8], 0.5),
    (5, 17, 2, 13, 16, 3, 8, [0, 7], 1.0),
    (4, 16, 4, 9, 64, 21, 9, [0, 4, 8], 1.0),
    (2, 0, 2, 7, 128, 32, 8, [0, 7], 1.0),
    (4, 6, 2, 9, 32, 5, 8, [0, 7], 1.0),
    (1, 2, 2, 9, 64, 3, 8, [0, 3, 7], 0.5),
    (2, 9, 2, 9, 32, 3, 8, [0, 7], 1.0),
    (5, 7, 2, 9, 16, 3, 8, [0, 7], 0.5),
    (4, 17, 2, 9, 256, 14, 9, [0, 3.5, 8], 1.0),     # H = 256 on the MFMA SRK variant (weights streamed)
    (1, 13, 1, 5, 256, 3, 8, [0, 7], 0.5),
    (0, 17, 2, 9, 64, 5, 8, [0, 7], 1.0),            # y-free drift and wide control paths on the MFMA SRK variant
    (0, 4, 1, 6, 128, 21, 8, [0, 3, 7], 0.5),
    (4, 17, 2, 9, 64, 40, 9, [0, 8], 1.0),
    (6, 16, 3, 7, 128, 69, 8, [0, 7], 1.0),
    (2, 12, 1, 9, 32, 33, 8, [0, 2.5, 7], 0.5),
    (1, 18, 2, 9, 16, 3, 8, [0, 7], 0.5),            # diffusion nets on the MFMA net kernels (snsde_m4n_kernel.h): H = 16 .. 128,
    (1, 14, 1, 17, 32, 3, 9, [0, 2.5, 8], 0.5),      # one- and two-layer nets, raw = net and net * y, every drift family
    (3, 18, 2, 33, 64, 5, 12, [0, 2.5, 11], 0.5),
    (5, 19, 2, 21, 64, 5, 9, [0, 8], 1.0),
    (4, 19, 2, 21, 128, 21, 10, [0, 9], 1.0),
    (2, 14, 2, 13, 32, 7, 9, [0, 3.5, 8], 0.5),
    (6, 15, 3, 9, 64, 40, 8, [0, 7], 1.0),
    (1, 18, 2, 37, 128, 5, 9, [0, 8], 1.0),          # H = 128: net matrices parked in the waves' LDS slices
    (3, 18, 3, 11, 128, 5, 9, [0, 8], 0.5),
    (4, 18, 1, 11, 128, 69, 9, [0, 8], 1.0),         # wide control path (C = 69) with a net
    (6, 19, 4, 7, 32, 3, 8, [0, 7], 1.0),
]

# ---- the wave-pair kernels at H = 64 (test_gpu_w4.py) -------------------------------------------------------------------------------
W4_CASES = [
    # io, no, NL, B, C, L, ts, dt
    (3, 18, 2, 37, 5, 9, [0, 3.5, 8], 1.0),          # BASELINE config 4's model; ragged last tile, an interpolated output
    (1, 14, 1, 9, 3, 8, [0, 7], 0.5),                # one-layer drift, one-layer net, no time features in the drift
    (5, 19, 2, 21, 3, 9, [0, 8], 1.0),               # geometric drift, raw = net * y
    (3, 15, 1, 13, 4, 8, [0, 2.5, 7], 1.0),
    (1, 18, 2, 64, 3, 12, None, None),               # every knot an output, linspace grid
    (5, 14, 2, 8, 3, 8, [0, 7], 1.0),
]

W4_BWD = [
    # io, no, NL, B, C, L, ts, dt
    (3, 18, 2, 21, 5, 9, [0, 3.5, 8], 1.0),
    (1, 14, 1, 9, 3, 8, [0, 7], 0.5),
    (5, 19, 2, 13, 3, 9, [0, 8], 1.0),
    (3, 15, 2, 11, 4, 8, [0, 2.5, 7], 1.0),
    (1, 18, 1, 10, 3, 8, [0, 7], 1.0),
]

W4_SRK_CASES = [
    # io, no, NL, B, C, L, ts, dt
    (3, 18, 2, 37, 5, 9, [0, 3.5, 8], 1.0),          # the README's neuralsde_3_18 under torch_ists' default method
    (1, 18, 2, 9, 3, 8, [0, 7], 0.5),
    (5, 19, 2, 21, 3, 9, [0, 8], 1.0),
    (3, 15, 1, 13, 4, 8, [0, 2.5, 7], 1.0),
    (1, 14, 2, 16, 3, 12, None, None),
]

W4_SRK_BWD = [
    (3, 18, 2, 21, 5, 9, [0, 3.5, 8], 1.0),
    (1, 14, 1, 9, 3, 8, [0, 7], 0.5),
    (5, 19, 2, 13, 3, 9, [0, 8], 1.0),
    (3, 15, 2, 11, 4, 8, [0, 2.5, 7], 1.0),
    (1, 18, 1, 10, 3, 8, [0, 7], 1.0),
]



# ---- what the tables above are meant to run ------------------------------------------------------------------------------------------
# test_srk_backward_on_the_mfma_path: SRK_BWD_CASES x kernel.  The elementwise diffusions (rows 0 .. 17) run the general kernel's SRK
# variant and its adjoint, the diffusion nets (18 ..) the net kernel and snsde_m4n_srk_reverse_kernel - except, under 'auto', the two
# H = 64 rows with a latent-only drift, which the wave-pair kernels take (tests/test_gpu_w4.py is about those)
SRK_BWD_FIRST_NET, SRK_BWD_AUTO_W4 = 18, (21, 22)


def srk_bwd_kernels(ci, kernel):
    if kernel == 'auto' and ci in SRK_BWD_AUTO_W4:
        return 'w4', 'w4_fused'
    return ('general_m4', 'general_srk') if ci < SRK_BWD_FIRST_NET else ('m4n', 'm4n_srk')


MIL_NET_KERNELS = ('m4n', 'm4n_milstein')      # test_milstein_backward_through_a_diffusion_net_on_the_mfma_path: every row
# test_srk_diffusion_nets_take_the_mfma_net_kernels: the net rows of SRK_CASES at instantiated sizes; 'auto' takes the wave pair
# for the two H = 64 rows with a latent-only drift
SRK_NET_ROWS = [i for i, c in enumerate(SRK_CASES) if c[1] in (14, 15, 18, 19) and c[4] in (16, 32, 64, 128)]
SRK_NET_AUTO_W4 = (26, 27)
# tests/test_gpu_w4.py: kernel selector -> (forward, adjoint) at H = 64 with a diffusion net
W4_KERNELS = {'euler': {'w4': ('w4', 'w4_fused'), 'auto': ('w4', 'w4_fused'), 'mfma4': ('general_m4', 'general'), 'generic': ('generic', 'generic')},
              'srk': {'w4': ('w4', 'w4_fused'), 'auto': ('w4', 'w4_fused'), 'mfma4': ('m4n', 'm4n_srk'), 'generic': ('generic_srk', 'generic')}}
# test_long_solves_cross_the_step_table_chunks: H, method -> kernels under 'mfma4' (300 steps, B = 9)
LONG_CASES = [(32, 'euler'), (64, 'milstein'), (128, 'euler'), (256, 'milstein'), (256, 'euler')]
LONG_KERNELS = {32: ('lean', 'general'), 64: ('lean', 'general'), 128: ('lean', 'general'), 256: ('lean_two_tile_h256', 'two_tile_h256')}
# the K-shaped full-size tests (BASELINE.json): name -> io, no, NL, B, H, C, L, method, {kernel selector: forward kernel}
K_SHAPES = {
    'K2': (4, 17, 2, 1024, 128, 21, 101, 'euler', {'auto': 'lean', 'mfma16': 'general_m16', 'mfma4': 'lean', 'mfma4x': 'general_m4'}),      # ('x': the unfused emb order, which the lean kernel does not carry)
    'K3': (6, 17, 2, 512, 128, 21, 201, 'euler', {'mfma4': 'lean', 'mfma16': 'general_m16', 'generic': 'generic'}),
    'K3 4096': (6, 17, 2, 4096, 128, 21, 201, 'euler', {'auto': 'general_m16'}),
    'K4': (3, 18, 2, 2048, 64, 69, 72, 'euler', {'auto': 'w4', 'w4': 'w4', 'mfma4': 'general_m4', 'mfma16': 'general_m16', 'generic': 'generic'}),
    'K4 srk': (3, 18, 2, 2048, 64, 69, 72, 'srk', {'auto': 'w4', 'mfma4': 'm4n'}),
    'K5': (4, 17, 2, 128, 256, 14, 50, 'milstein', {'mfma4': 'lean_two_tile_h256', 'mfma16': 'general_m16', 'generic': 'generic'}),
    'K5 1024': (4, 17, 2, 1024, 256, 14, 50, 'milstein', {'auto': 'lean_two_tile_h256'}),
}
# routes at the edges of the table: no kernel (test_mfma_unsupported_configuration_is_refused_not_silently_rerouted), the bf16 lean
# kernel (tests/test_gpu_bf16.py: inference only, no adjoint), the generic adjoints (GEN_BWD_CASES rows 0 and 10)
EDGE_LAUNCHES = [
    launch('unsupported: net on a y-free drift, wide control', 0, 18, 2, 8, 64, 40, 5, [0, 4], 1.0, kernel='mfma', fwd='none'),
    launch('unsupported: H not instantiated', 4, 17, 2, 8, 48, 3, 5, [0, 4], 1.0, kernel='mfma16', fwd='none'),
    launch('unsupported: auto takes the generic kernel', 4, 17, 2, 8, 48, 3, 5, [0, 4], 1.0, fwd='generic'),
    launch('bf16 K2', 4, 17, 2, 1024, 128, 21, 101, [0, 100], 1.0, supplied=False, bf16=True, fwd='lean_bf16', rev='none'),
    launch('generic backward euler', 4, 17, 2, 11, 24, 5, 9, [0, 3, 8], 1.0, kernel='generic', train=True, fwd='generic', rev='generic'),
    launch('generic backward srk', 4, 17, 2, 11, 24, 5, 9, [0, 3.5, 8], 1.0, 'srk', kernel='generic', train=True, fwd='generic_srk', rev='generic'),
]

# ---- resumable solves (tests/test_gpu_step_offset.py), moved here unchanged: every forward kernel once, Philox-driven, inference ----
# 37 steps of dt = 0.25 over knots 0 .. 10; outputs 1 and 2 are interpolated inside steps 10 and 24
STEP_OFFSET_TS, STEP_OFFSET_DT, STEP_OFFSET_L = [0.0, 2.6, 6.1, 9.25], 0.25, 11
# One Philox-driven inference launch per forward kernel at its smallest shapes: test, io, no, NL, B, H, C, L, ts, dt, method, kernel
STEP_OFFSET_CASES = [
    launch('lean specialised', 4, 17, 2, 8, 128, 21, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, supplied=False, fwd='lean'),
    launch('lean general', 4, 17, 2, 8, 32, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='mfma4', supplied=False, fwd='lean'),
    launch('lean general milstein', 6, 16, 2, 8, 32, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'milstein', 'mfma4', supplied=False, fwd='lean'),
    launch('lean bf16', 4, 17, 2, 8, 64, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, supplied=False, bf16=True, fwd='lean_bf16'),
    launch('two tiles h128', 4, 17, 2, 8, 128, 21, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='mfma4', two_tile=True, supplied=False, fwd='lean_two_tile_h128'),
    launch('two tiles h256', 4, 17, 2, 8, 256, 14, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='mfma4', supplied=False, fwd='lean_two_tile_h256'),
    launch('streamed h256', 4, 17, 2, 8, 256, 14, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='mfma4', stream_all=True, supplied=False, fwd='lean_streamed_h256'),
    launch('general m4 euler', 4, 17, 2, 8, 32, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='mfma4', exact=True, supplied=False, fwd='general_m4'),
    launch('general m4 srk', 6, 17, 2, 8, 32, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'srk', 'mfma4', supplied=False, fwd='general_m4'),
    launch('general m16 euler', 4, 17, 2, 32, 32, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='mfma16', supplied=False, fwd='general_m16'),
    launch('m4n srk', 1, 18, 2, 8, 16, 3, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'srk', 'mfma4', supplied=False, fwd='m4n'),
    launch('m4n milstein', 1, 18, 2, 8, 32, 3, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'milstein', supplied=False, fwd='m4n'),
    launch('m4n euler', 4, 18, 2, 8, 32, 40, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, supplied=False, fwd='m4n'),
    launch('w4 euler', 3, 18, 2, 8, 64, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='w4', supplied=False, fwd='w4'),
    launch('w4 srk', 3, 18, 2, 8, 64, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'srk', 'w4', supplied=False, fwd='w4'),
    launch('generic euler', 4, 17, 2, 8, 24, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, kernel='generic', supplied=False, fwd='generic'),
    launch('generic milstein net', 3, 18, 2, 8, 24, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'milstein', 'generic', supplied=False, fwd='generic'),
    launch('generic srk', 4, 17, 2, 8, 24, 5, STEP_OFFSET_L, STEP_OFFSET_TS, STEP_OFFSET_DT, 'srk', 'generic', supplied=False, fwd='generic_srk'),
]

# ---- the solve chain under poisoned allocations (tests/test_gpu_poisoned_allocations.py) ---------------------------------------------
# Forward, inference: STEP_OFFSET_CASES above (every forward kernel once).  Training: one Philox-driven case per adjoint kernel - of
# each family above the row with the fewest B x H among those with an explicit output grid, every M4S2_REV_MODELS entry at B = 3, the
# generic rows of EDGE_LAUNCHES and one lean / general row (the long-solve model of LONG_CASES at H = 32 on the small grid).
# tests/test_kernel_census_cpu.py holds every row to the kernels it names and the table to every adjoint kernel.
def _poisoned_training():
    out = []

    def add(test, *a, **k):
        out.append(launch(test, *a, train=True, supplied=False, **k))

    io, no, NL, B, C_, L, ts, dt = W4_BWD[1]
    add('w4 fused', io, no, NL, B, 64, C_, L, ts, dt, 'euler', 'w4', fwd='w4', rev='w4_fused')
    add('general srk', *SRK_BWD_CASES[9], 'srk', 'mfma4', fwd='general_m4', rev='general_srk')
    add('m4n srk', *SRK_BWD_CASES[SRK_BWD_FIRST_NET], 'srk', 'mfma4', fwd='m4n', rev='m4n_srk')
    add('m4n milstein', *MIL_NET_BWD_CASES[0], 'milstein', 'auto', fwd=MIL_NET_KERNELS[0], rev=MIL_NET_KERNELS[1])
    for (nhid, geo), (io, no, NL, C_, method, fwd) in M4S2_REV_MODELS.items():
        add(f'two tile h256 {(nhid, geo)}', io, no, NL, CENSUS_B[0], 256, C_, 9, TS8, DT8, method, 'mfma4', fwd=fwd, rev='two_tile_h256')
    out.extend(c._replace(supplied=False) for c in EDGE_LAUNCHES if c.rev == 'generic')
    add('lean / general', 4, 17, 2, 9, 32, 5, 9, TS8, DT8, 'euler', 'mfma4', fwd='lean', rev='general')
    return out


POISONED_TRAINING_CASES = _poisoned_training()


def census():
    """Every launch of the kernel-specific GPU tests, with the kernels it is meant to run (rev = None: the launch has no backward)."""
    out = []

    def add(test, *a, **k):
        out.append(launch(test, *a, **k))

    two, streamed = ('lean_two_tile_h256', 'two_tile_h256'), ('lean_streamed_h256', 'general')
    for table, planned in ((H256_FWD_TWO_TILE, two[0]), (H256_FWD_DECLINES, streamed[0])):
        for ci, train in table:
            io, no, NL, C_, B, method = H256_FWD_CASES[ci]
            for supplied in (False, True):
                for all_ in (True, False):
                    add(f'h256 forward case {ci} train={train}', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', stream_all=all_, train=train,
                        supplied=supplied, fwd=streamed[0] if all_ else planned)
    for ci, (io, no, NL, C_, B, method, ro) in enumerate(H256_REV_CASES):
        for supplied in (False, True):
            add(f'h256 adjoint case {ci}', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', train=True, supplied=supplied, row_out=ro,
                fwd=H256_REV_FWD[ci], rev=two[1])
            add(f'h256 adjoint case {ci}', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', stream_all=True, train=True, supplied=supplied,
                row_out=ro, fwd=streamed[0], rev=streamed[1])
    io, no, NL, C_, B, L = H256_CHUNK_CASE
    for all_ in (True, False):
        add('h256 chunks', io, no, NL, B, 256, C_, L, [0., 77.5, 160.], 1.0, 'milstein', 'mfma4', stream_all=all_, train=True, supplied=False,
            fwd=(streamed if all_ else two)[0], rev=(streamed if all_ else two)[1])
    for ci, (io, no, C_, B, method) in enumerate(H128_CASES):
        for train in (False, True):
            for supplied in (False, True):
                for tt in (False, True):
                    add(f'h128 case {ci}', io, no, 2, B, 128, C_, 9, TS8, DT8, method, 'mfma4', two_tile=tt, train=train, supplied=supplied,
                        fwd='lean_two_tile_h128' if tt else 'lean')
    for nhid, kuxt, train in M4S2_CASES:
        io, no, NL, C_, method = M4S2_MODELS[(nhid, kuxt)]
        for B in CENSUS_B:
            for supplied in (False, True):
                for all_ in (True, False):
                    add(f'm4s2 {(nhid, kuxt, train)}', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', stream_all=all_, train=train,
                        supplied=supplied, fwd=(streamed if all_ else two)[0])
    for nhid, kuxt, train in M4T_CASES:
        io, no, NL, C_, method = M4T_MODELS[(nhid, kuxt)]
        for B in CENSUS_B:
            for supplied in (False, True):
                for tt in (False, True):
                    add(f'm4t {(nhid, kuxt, train)}', io, no, NL, B, 128, C_, 9, TS8, DT8, method, 'mfma4', two_tile=tt, train=train,
                        supplied=supplied, fwd='lean_two_tile_h128' if tt else 'lean')
    for (nhid, geo), (io, no, NL, C_, method, fwd) in M4S2_REV_MODELS.items():
        for B in CENSUS_B:
            add(f'm4s2 rev {(nhid, geo)} autograd', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', train=True, fwd=fwd, rev=two[1])
            for ro in (False, True):
                add(f'm4s2 rev {(nhid, geo)}', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', train=True, supplied=False, row_out=ro,
                    fwd=fwd, rev=two[1])
                add(f'm4s2 rev {(nhid, geo)}', io, no, NL, B, 256, C_, 9, TS8, DT8, method, 'mfma4', stream_all=True, train=True, supplied=False,
                    row_out=ro, fwd=streamed[0], rev=streamed[1])
    for ci, (io, no, NL, B, H, C_, L) in enumerate(EULER_NET_CASES):
        add(f'euler net {ci}', io, no, NL, B, H, C_, L, [0, 2.5, L - 1], 0.5, fwd=EULER_NET_FWD[ci])
        add(f'euler net {ci}', io, no, NL, B, H, C_, L, [0, 2.5, L - 1], 0.5, train=True, fwd=EULER_NET_FWD[ci], rev='general')
    for ci in SRK_NET_ROWS:
        add(f'srk net row {ci}', *SRK_CASES[ci], 'srk', 'auto', fwd='w4' if ci in SRK_NET_AUTO_W4 else 'm4n')
        add(f'srk net row {ci}', *SRK_CASES[ci], 'srk', 'mfma4', fwd='m4n')
    for ci, case in enumerate(SRK_BWD_CASES):
        for kernel in ('mfma4', 'auto'):
            fwd, rev = srk_bwd_kernels(ci, kernel)
            add(f'srk backward {ci} {kernel}', *case, 'srk', kernel, train=True, fwd=fwd, rev=rev)
    for ci, case in enumerate(MIL_NET_BWD_CASES):
        add(f'milstein net backward {ci}', *case, 'milstein', 'auto', train=True, fwd=MIL_NET_KERNELS[0], rev=MIL_NET_KERNELS[1])
    for method, fwd_cases, bwd_cases in (('euler', W4_CASES, W4_BWD), ('srk', W4_SRK_CASES, W4_SRK_BWD)):
        for ci, (io, no, NL, B, C_, L, ts, dt) in enumerate(fwd_cases):
            for kernel in ('w4', 'mfma4', 'generic'):
                add(f'w4 {method} forward {ci} {kernel}', io, no, NL, B, 64, C_, L, ts, dt, method, kernel, fwd=W4_KERNELS[method][kernel][0])
        for ci, (io, no, NL, B, C_, L, ts, dt) in enumerate(bwd_cases):
            for kernel in ('w4', 'auto', 'mfma4'):
                fwd, rev = W4_KERNELS[method][kernel]
                add(f'w4 {method} backward {ci} {kernel}', io, no, NL, B, 64, C_, L, ts, dt, method, kernel, train=True, fwd=fwd, rev=rev)
    for H, method in LONG_CASES:
        fwd, rev = LONG_KERNELS[H]
        add(f'long solve H={H}', 4, 17, 2, 9, H, 5, 9, [0.0, 3.1, 8.0], 8.0 / 300, method, 'mfma4', fwd=fwd)
        add(f'long solve H={H}', 4, 17, 2, 9, H, 5, 9, [0.0, 3.1, 8.0], 8.0 / 300, method, 'mfma4', train=True, fwd=fwd, rev=rev)
    for name, (io, no, NL, B, H, C_, L, method, kernels) in K_SHAPES.items():
        for kernel, fwd in kernels.items():
            ts = [1, 30, 72] if name.startswith('K4') else ([0, L - 1] if name[:2] in ('K2', 'K3') else list(range(L)))
            add(f'{name} {kernel}', io, no, NL, B, H, C_, L, ts, 1.0, method, kernel.rstrip('x'), exact=kernel.endswith('x'), fwd=fwd)
    return out + EDGE_LAUNCHES
