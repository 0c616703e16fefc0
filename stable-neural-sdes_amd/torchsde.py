"""``sdeint`` with the call contract of torchsde 0.2.5 at the reference's four call sites
(benchmark_classification/models_sde/neuralsde.py:71-82, benchmark_forecasting/...:71-82,145-156,
torch-ists/.../nsde_model.py:63-74):

    sdeint(sde=func, y0=z0, ts=ts, dt=dt, method='euler', options={'dt': dt})  ->  (T, B, H)

Dispatch, in the order ``sdeint`` asks (the first route that takes the call solves it)
  1. sampled (_sdeint_samples): options={'samples': S > 1}, every backend.  It expands y0 / row_out to S paths per input row
     and either hands the fused route the coefficients in place (a kernel that maps paths to rows) or replicates them and
     calls ``sdeint`` again without the option.
  2. fused (_sdeint_hip): ``sde`` honours the Diffusion_model contract (engine.recognise) under the default drift /
     diffusion names and ``y0`` is a CUDA tensor (backend 'auto'), or backend='hip'.  ONE fused HIP solve (libsnsde.so);
     with gradients the fused adjoint (_FusedSolve).  If the library is missing this raises.  A valid request that no kernel
     covers, or a gradient no fused adjoint returns, takes the tensor-op loop on the same device (one warning per
     configuration) unless options={'strict': True}; a refused shard, a bf16 refusal and a sampled solve that the query
     accepted are errors either way.
  3. padded (_sdeint_padded), from inside the fused route: fp32, kernel 'auto', no save_traj / recompute / samples and a hidden
     size without an MFMA instantiation (engine.padding_plan): the zero-padded model on the MFMA kernels, exactly.
  4. composed (_sdeint_composed): default names, not a Diffusion_model, backend 'auto', CUDA: a tutorial-style field that
     fields.compose maps onto the lean kernel and verifies.  None (not such a field, not covered) passes the call on.
  5. latent (_sdeint_latent): other names (torch-ists' f_aug / g_aug), backend 'auto', CUDA: the latent dynamics on the fused
     kernels, the KL accumulator in the solve or as one batched quadrature.  Falls back to the loop itself.
  6. tensor-op loop (_sdeint_torch): everything else (backend='torch', CPU tensors = the reference's CPU plumbing
     configuration, arbitrary ``sde.f/g``): the same fixed-step scheme written with tensor ops, calling ``sde.f`` / ``sde.g``
     once per step.

Fixed-step semantics (restated from torchsde 0.2.5; its source is not in the
reference tree): time accumulates in float32 by repeated ``curr_t + dt`` clamped to ``ts[-1]``;
outputs are linearly interpolated between the two solver states bracketing each ``ts[k]``;
Euler ``y + f*h + g*dW``; Milstein adds ``0.5 * g * dg/dy * (dW^2 - h)`` (Ito, diagonal noise).

Of torchsde's other keywords, ``extra=True`` / ``extra_solver_state`` are implemented (resumable solves: ``sdeint``'s docstring);
``adaptive=True`` and ``logqp=True`` raise NotImplementedError.
"""
import collections
import os
import warnings

import numpy as np
import torch

from . import engine
from .controldiffeq import _HostTimes

METHODS = ('euler', 'milstein', 'srk')


class BrownianIncrements:
    """Minimal Brownian-motion object: ``bm(ta, tb)`` ~ N(0, (tb - ta) I) of shape (B, H).

    Increments over disjoint intervals are independent draws from one generator; unlike
    torchsde.BrownianInterval it does not support re-querying overlapping intervals (the fixed-step
    solvers never do)."""

    def __init__(self, t0=0.0, t1=1.0, size=None, dtype=torch.float32, device=None, entropy=None, **kwargs):
        self.shape = tuple(size)
        self.dtype, self.device = dtype, device
        self.generator = torch.Generator(device=device if device is not None else 'cpu')
        self.generator.manual_seed(int(entropy) if entropy is not None else int(torch.empty((), dtype=torch.int64).random_().item()))

    levy_area_approximation = 'space-time'

    def __call__(self, ta, tb=None, return_U=False, **kwargs):
        h = (torch.as_tensor(tb, dtype=self.dtype) - torch.as_tensor(ta, dtype=self.dtype))
        z = torch.randn(self.shape, dtype=self.dtype, device=self.device, generator=self.generator)
        h = h.to(z.device)
        W = z * h.sqrt()
        if not return_U:
            return W
        xi = torch.randn(self.shape, dtype=self.dtype, device=self.device, generator=self.generator)
        return W, h * (0.5 * W + (h / 12).sqrt() * xi)     # U = int_ta^tb (W_s - W_ta) ds


BrownianInterval = BrownianIncrements      # torchsde.BrownianInterval(t0, t1, size, dtype, device, entropy, ...) call sites


class BaseSDE(torch.nn.Module):
    """torchsde.BaseSDE: an nn.Module that records its noise / SDE type (torch-ists .../NSDE/latent_sde.py:31 subclasses
    ``torchsde.SDEIto``)."""

    def __init__(self, noise_type, sde_type):
        super().__init__()
        if noise_type not in ('diagonal', 'scalar', 'additive', 'general'):
            raise ValueError(f"Expected noise type in ('diagonal', 'scalar', 'additive', 'general'), but found {noise_type}")
        if sde_type not in ('ito', 'stratonovich'):
            raise ValueError(f"Expected sde type in ('ito', 'stratonovich'), but found {sde_type}")
        self.noise_type = noise_type
        self.sde_type = sde_type


class SDEIto(BaseSDE):
    def __init__(self, noise_type):
        super().__init__(noise_type=noise_type, sde_type='ito')


class SDEStratonovich(BaseSDE):
    def __init__(self, noise_type):
        super().__init__(noise_type=noise_type, sde_type='stratonovich')


def _as_ts(ts, y0):
    if not torch.is_tensor(ts):
        if not isinstance(ts, (tuple, list)) or not all(isinstance(t, (float, int)) for t in ts):
            raise ValueError("Evaluation times `ts` must be a 1-D Tensor or list/tuple of floats.")
        ts = torch.tensor(ts, dtype=y0.dtype, device=y0.device)
    if ts.dim() != 1 or ts.numel() < 2:
        raise ValueError("Evaluation times `ts` must be a 1-D Tensor with at least two entries.")
    return ts


def _fresh_seed():
    # drawn from torch's CPU generator: reproducible under torch.manual_seed, no device sync
    return int(torch.empty((), dtype=torch.int64).random_().item())


_CAPTURE_SEEDS = {}
_UNFUSED_WARNED = set()


def _coeffs_need_grad(sde):
    """The control path's packed coefficients take part in this differentiation."""
    coeffs = getattr(sde, 'coeffs', None)
    return torch.is_grad_enabled() and torch.is_tensor(coeffs) and coeffs.requires_grad


class _NoCoeffGradient(Exception):
    """Raised before the launch by a fused solve that cannot return dL/d coeffs (its adjoint leaves no delta planes)."""


def _unfused_coeff_grad(sde, what, options):
    """The fallback rule for dL/d coeffs: a configuration whose fused backward does not produce it takes the tensor-op loop on
    the same device (one warning per configuration); options={'strict': True} raises instead.  Never a silent None."""
    if options.get('strict', False):
        raise NotImplementedError(f"sdeint: no fused gradient with respect to the control path's coefficients for {what}; "
                                  "drop options['strict'] (or pass options={'backend': 'torch'}) to differentiate through the "
                                  "tensor-op loop")
    key = ('coeffs', what)
    if key not in _UNFUSED_WARNED:
        _UNFUSED_WARNED.add(key)
        warnings.warn(f"sdeint: no fused gradient with respect to the control path's coefficients for {what}; "
                      "differentiating through the unfused tensor-op loop (slow).")


def _dev_key(device):
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def _capture_seed(device):
    """Device-resident Philox key for solves recorded into a hipGraph: the increment is part of the graph, so every
    replay integrates against fresh Brownian increments (a host-drawn seed would be frozen into the recording)."""
    state = _CAPTURE_SEEDS.get(_dev_key(device))
    if state is None:
        raise RuntimeError("sdeint without options['seed'] inside a CUDA graph capture: call "
                           "stable_neural_sdes_amd.torchsde.prepare_graph_capture(device) before capturing")
    state.add_(1)
    return state


def prepare_graph_capture(device):
    """Allocate the device-resident seed used by solves that are recorded into a CUDA/HIP graph (call once, outside
    the capture).  The key is drawn from torch's CPU generator, so torch.manual_seed makes replays reproducible."""
    key = _dev_key(device)
    if key not in _CAPTURE_SEEDS:
        _CAPTURE_SEEDS[key] = torch.tensor([_fresh_seed() & 0x3FFFFFFFFFFFFFFF], dtype=torch.int64,
                                           device=torch.device('cuda', key))
    return _CAPTURE_SEEDS[key]


def _philox_key(options, device):
    """The Philox key of a solve whose kernels draw the increments: options['seed'] (an int; a device tensor as it is), else a
    device-resident key that a recording advances itself (fresh noise per replay), else a fresh host draw."""
    seed = options.get('seed')
    if seed is None:      # (only a CUDA device records: the capture query needs one)
        capturing = torch.device(device).type == 'cuda' and torch.cuda.is_current_stream_capturing()
        return _capture_seed(device) if capturing else _fresh_seed()
    return seed if torch.is_tensor(seed) else int(seed)


def _row_offset(options, rows):
    """The global row of this call's first row (Philox counters use the global row): options['row_offset'], where None is "not
    given"; else, one process per GPU (DDP), rank * rows - ranks that seed identically must not integrate against identical
    Brownian paths, and shard r of equal-sized shards starts at row r * rows; else 0.  Always an int."""
    given = options.get('row_offset')
    if given is not None:
        return engine.check_row_offset(given, rows)      # rows row_offset .. row_offset + rows - 1 inside [0, 2**32): ValueError otherwise
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return engine.check_row_offset(dist.get_rank() * int(rows), rows)
    return 0


def _device_row_out(options, device):
    """options['row_out'] (per-row output selection fused into the solve: the result is (B, H)) as the kernels read it."""
    row_out = options.get('row_out')
    return None if row_out is None else row_out.to(device=device, dtype=torch.int32).contiguous()


def _recompute_steps(options):
    """Steps per chunk of recompute mode: options['recompute'], else the process-wide environment variable; 0 = off."""
    return max(int(options.get('recompute', os.environ.get('SNSDE_RECOMPUTE_STEPS', 0)) or 0), 0)


def _default_names(names):
    """names={'drift': 'f', 'diffusion': 'g'} is the default mapping: such a call may still take a fused route."""
    return names is None or (names.get('drift', 'f') == 'f' and names.get('diffusion', 'g') == 'g'
                             and not (set(names) - {'drift', 'diffusion'}))


def _differentiated(sde, y0, params=None):
    """This solve is differentiated: grad is enabled and y0, a parameter or the control path's coefficients require it.
    params: the module's parameters where the caller has them listed already (engine.param_index spares the walk)."""
    params = getattr(sde, 'parameters', tuple)() if params is None else params      # (a generator: nothing is walked yet)
    return torch.is_grad_enabled() and (y0.requires_grad or any(p.requires_grad for p in params) or _coeffs_need_grad(sde))


_NO_GENERATOR_CONTINUATION = ("sdeint: options['step_offset'] != 0 (a continued Brownian path) needs the fused solve, whose kernels draw "
                              "the Philox increments of the global steps, or a caller-supplied `bm`, which carries the path itself; {what} "
                              "would draw from a torch generator and continue on different noise")


def _continued_without_path(options, bm, what):
    """A route that draws its increments from a torch generator cannot continue a path: NotImplementedError for step_offset != 0
    without a caller's `bm` (never a silent continuation on different noise)."""
    if bm is None and int(options.get('step_offset') or 0) != 0:
        raise NotImplementedError(_NO_GENERATOR_CONTINUATION.format(what=what))


def _seed_bits(seed):
    """A Philox key as the int64 whose 64 bits it is (what the solver state stores; SolveCall masks it back)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >= (1 << 63) else s


def _read_solver_state(state):
    """(steps taken so far, key bits, keyed) of an `extra_solver_state`; ValueError if it is not what `extra=True` returned."""
    ok = (isinstance(state, (tuple, list)) and len(state) == 1 and torch.is_tensor(state[0]) and state[0].dtype == torch.int64
          and state[0].device.type == 'cpu' and tuple(state[0].shape) == (3,))
    if ok:
        taken, key, keyed = (int(v) for v in state[0].tolist())
        ok = taken >= 0 and keyed in (0, 1)
    if not ok:
        raise ValueError("extra_solver_state is malformed: expected the 1-tuple sdeint(..., extra=True) returned, one int64 CPU tensor "
                         "[steps taken so far, Philox key, keyed]")
    return taken, key, keyed


def sdeint(sde, y0, ts, bm=None, method=None, dt=1e-3, adaptive=False, rtol=1e-5, atol=1e-4, dt_min=1e-5,
           options=None, names=None, logqp=False, extra=False, extra_solver_state=None, **unused_kwargs):
    """torchsde.sdeint's call contract (module docstring).  Resumable solves, torchsde's keywords:

    ``extra=True`` returns ``(ys, state)``; ``extra_solver_state=state`` continues the SAME Brownian path from ``ys[-1]``: the
    next call's ``y0``.  ``state`` is a 1-tuple holding one int64 CPU tensor [steps taken so far, Philox key, keyed] (opaque to
    callers): keyed = 1 - the kernels drew from that key (options['seed'], or the fresh draw of the first call, returned instead
    of discarded); keyed = 0 - a ``bm`` was supplied and carries the path.  A continued call runs with
    options['step_offset'] = steps taken so far and the stored key: local step i draws the normals of global step
    step_offset + i (include/snsde.h: snsde_solve_forward_at).  The pieces equal the single call over the concatenated ``ts`` bit
    for bit exactly when every cut time is a step boundary of the single call's grid; otherwise the single call interpolates across
    the cut while the pieces land on it, as in torchsde.  Between the pieces ``sde.set_X`` may be called with a longer coefficient
    tensor and longer ``times`` (streaming: the causal Hermite path keeps the coefficients of its existing intervals).
    Inference only by default: a differentiated call with step_offset != 0 is a ValueError.  options={'resume_grad': True} opts in
    to training through continued solves (SNSDE_FLAG_RESUME_GRAD): ``extra=True``, ``extra_solver_state`` and step_offset != 0 are
    then legal on a differentiated call, the fused node hands the offset to the forward launch and to its backward call
    (snsde_solve_backward_at / snsde_backward_with_gradients_at: the adjoints that regenerate Philox increments draw those of the
    global steps), and with piece j's ``y0`` being piece j-1's ``ys[-1]`` inside the autograd graph the states equal the uncut
    differentiable solve bit for bit, dL/dy0 follows the same adjoint recursion and the parameter and coefficient gradients are the
    pieces' gradients summed by autograd (truncated back-propagation: detach ``y0`` between the pieces).  It goes with
    samples + sample_grad, row_offset / global_rows, a control path that requires grad and precision='bf16' + bf16_grad; it does
    not take recompute (the option or SNSDE_RECOMPUTE_STEPS) or z0_linear on a continued piece (ValueError), and ``sdeint_ensemble``
    stays inference only.  The routes that are autograd through tensor ops anyway (CPU tensors, backend='torch' with a ``bm``)
    simply stop refusing.  A route that would draw from a torch generator
    (the tensor-op loop without ``bm``, the latent route, the "no kernel covers it" fallback) raises NotImplementedError for
    step_offset != 0.  options={'step_offset': n0} is the same knob without the state (with a ``bm`` it has no effect on the
    increments).  A device-tensor seed (graph capture) with ``extra=True`` is a ValueError: the host does not know the key."""
    if unused_kwargs:
        warnings.warn(f"Unexpected arguments {unused_kwargs}")
    if adaptive:
        raise NotImplementedError("adaptive stepping is not implemented; the reference only uses fixed dt")
    if logqp:
        raise NotImplementedError("logqp is not implemented")
    if not extra and extra_solver_state is None:
        return _sdeint(sde, y0, ts, bm, method, dt, options, names)
    options = dict(options or {})
    keyed = 1 if bm is None else 0
    if extra_solver_state is not None:
        taken, key, was_keyed = _read_solver_state(extra_solver_state)
        if was_keyed != keyed:
            raise ValueError("extra_solver_state and `bm` disagree: " +
                             ("the state continues a path the kernels drew from a Philox key, this call supplies a `bm`" if was_keyed else
                              "the state continues the path of a supplied `bm`, this call has none"))
        if options.get('step_offset') is not None and options['step_offset'] != taken:
            raise ValueError(f"options['step_offset']={options['step_offset']!r} disagrees with extra_solver_state "
                             f"({taken} steps taken so far)")
        seed = options.get('seed')
        if keyed and seed is not None and (torch.is_tensor(seed) or _seed_bits(seed) != key):
            raise ValueError(f"options['seed']={seed!r} disagrees with the Philox key of extra_solver_state")
        options['step_offset'] = taken
        if keyed:
            options['seed'] = key
    else:
        taken = engine.check_step_offset(options.get('step_offset') or 0)
    if keyed:
        seed = options.get('seed')
        capturing = torch.is_tensor(y0) and y0.is_cuda and torch.cuda.is_current_stream_capturing()
        if torch.is_tensor(seed) or (seed is None and capturing):
            raise ValueError("extra=True / extra_solver_state with a device-resident Philox key (a tensor seed, graph capture): the host "
                             "does not know the key a continuation would need; pass an int options['seed']")
        if seed is None:
            options['seed'] = _fresh_seed()      # (the call's own fresh draw, made here so that the state can return it)
    ys = _sdeint(sde, y0, ts, bm, method, dt, options, names)
    if not extra:
        return ys
    steps = engine.grid_steps(_HostTimes.get(_as_ts(ts, y0)), float(dt))
    return ys, (torch.tensor([taken + steps, _seed_bits(options['seed']) if keyed else 0, keyed], dtype=torch.int64),)


def _sdeint(sde, y0, ts, bm, method, dt, options, names):
    if not torch.is_tensor(y0) or y0.dim() != 2:
        raise ValueError("`y0` must be a 2-dimensional tensor of shape (batch, channels).")
    ts = _as_ts(ts, y0)
    options = dict(options or {})
    if method is None:
        method = 'srk'   # torchsde's default for Ito / diagonal noise
    if method not in METHODS:
        raise ValueError(f"Expected method in {METHODS}, but found {method}.")
    if not (float(dt) > 0):
        raise ValueError("`dt` must be positive.")
    backend = options.get('backend', 'auto')
    if backend not in ('auto', 'hip', 'torch'):
        raise ValueError("options['backend'] must be 'auto', 'hip' or 'torch'")
    # options={'step_offset': n0}: this call's first step is global step n0 of its Brownian path (a continued solve; inference).
    # Checked for every backend; from here on an int that every route finds in `options`
    step_offset = options['step_offset'] = engine.check_step_offset(options.get('step_offset') or 0)
    # options={'resume_grad': True}: a continued solve may be differentiated (opt-in; sdeint's docstring).  Checked for every backend
    resume_grad = engine.check_resume_grad(options['resume_grad']) if 'resume_grad' in options else False
    if step_offset and not resume_grad and _differentiated(sde, y0):
        raise ValueError(f"step_offset={step_offset} is inference only: y0, the control path or a parameter requires grad (use "
                         "torch.no_grad() or requires_grad_(False)); a continued solve has no backward")
    if resume_grad and _differentiated(sde, y0):
        for name, bad in (("recompute (options['recompute'] or SNSDE_RECOMPUTE_STEPS in the environment)", _recompute_steps(options) > 0),
                          ('z0_linear on a continued piece (it starts from the state handed over, not from X(ts[0]))',
                           step_offset != 0 and 'z0_linear' in options)):
            if bad:
                raise ValueError(f"resume_grad=True (training through continued solves) does not take {name}")
    # options={'samples': S}: S Brownian paths per input row (inference; _sdeint_samples).  Checked for every backend; 1 = no option
    # options={'sample_grad': True}: such a solve may be differentiated (opt-in: its training planes are per path).  No effect on 1
    samples = engine.check_samples(options.pop('samples')) if 'samples' in options else 1
    sample_grad = engine.check_sample_grad(options.pop('sample_grad')) if 'sample_grad' in options else False
    # options={'precision': 'bf16', 'bf16_grad': True}: the bf16-operand solve may be differentiated (opt-in, straight-through gradient;
    # _bf16_grad_conflicts).  Checked for every backend, before anything is routed
    bf16_grad = engine.check_bf16_grad(options['bf16_grad']) if 'bf16_grad' in options else False
    if bf16_grad:
        _bf16_grad_conflicts(sde, y0, options, backend, samples)
    # options={'row_offset': r}: the global row of this call's first row (of its first path under `samples`).  The Philox counter holds the
    # global row in 32 bits: rows outside [0, 2**32) are a ValueError, for every backend (engine.check_row_offset, include/snsde.h)
    if options.get('row_offset') is not None:
        engine.check_row_offset(options['row_offset'], y0.shape[0] * samples)
    if samples > 1:
        return _sdeint_samples(sde, y0, ts, bm, method, float(dt), options, names, samples, sample_grad)
    if backend != 'torch':      # (the tensor-op loop has no tiles to plan: it accepts the option and ignores it)
        engine.resolve_global_rows(options.get('global_rows'), y0.shape[0], options.get('row_offset') or 0)      # ValueError if malformed

    default_names = _default_names(names)
    rec = engine.recognise(sde) if default_names else None
    # options={'precision': 'bf16'}: inference on the bf16-operand kernel (engine.check_bf16), or a ValueError - never fp32 instead
    precision = options.get('precision', 'fp32')
    engine.precision_flags(precision)
    if precision == 'bf16':
        if backend == 'torch':
            raise ValueError("precision='bf16' is a HIP kernel option; backend='torch' has no bf16 solve")
        if _differentiated(sde, y0) and not bf16_grad:
            raise ValueError("precision='bf16' is inference only: y0, the control path or a parameter requires grad (use torch.no_grad(), "
                             "requires_grad_(False) or precision='fp32'; options={'bf16_grad': True} opts in to training through it)")
        if rec is None:
            raise ValueError("precision='bf16' needs an sde honouring the Diffusion_model contract (the fused HIP solve)")
        if not y0.is_cuda:
            raise ValueError("precision='bf16' needs CUDA (ROCm) tensors")
    want_hip = backend == 'hip' or (backend == 'auto' and rec is not None and y0.is_cuda)
    if 'z0_linear' in options and not (want_hip and rec is not None and y0.is_cuda):
        y0 = _materialise_z0(sde, y0, ts, options.pop('z0_linear'))      # only the fused solve evaluates the initial state itself
    if want_hip:
        if rec is None:
            raise ValueError("options['backend']='hip' needs an sde honouring the Diffusion_model contract")
        if not y0.is_cuda:
            raise ValueError("the HIP engine needs CUDA (ROCm) tensors")
        return _sdeint_hip(sde, rec, y0, ts, bm, method, float(dt), options)
    if default_names and rec is None and backend == 'auto' and y0.is_cuda:
        ys = _sdeint_composed(sde, y0, ts, bm, method, float(dt), options)     # tutorial-style fields (fields.py)
        if ys is not None:
            return ys
    if not default_names and rec is None and backend == 'auto' and y0.is_cuda:
        return _sdeint_latent(sde, y0, ts, bm, method, float(dt), options, names)    # LatentSDE-shaped modules (falls back itself)
    return _sdeint_torch(sde, y0, ts, bm, method, float(dt), options, names)


def _bf16_grad_conflicts(sde, y0, options, backend, samples):
    """options={'bf16_grad': True} (training through the bf16-operand forward, SNSDE_FLAG_BF16_GRAD): ValueError for everything the
    option does not go with - it is the bf16 kernel and the fused adjoint behind it or nothing, never an fp32 stand-in."""
    if options.get('precision', 'fp32') != 'bf16':
        raise ValueError("bf16_grad=True differentiates a precision='bf16' solve: pass options={'precision': 'bf16', 'bf16_grad': True}")
    for name, bad in (('samples > 1', samples > 1),
                      ("recompute (options['recompute'] or SNSDE_RECOMPUTE_STEPS in the environment)", _recompute_steps(options) > 0),
                      ("param_pass='torch'", options.get('param_pass', 'hip') == 'torch'), ("backend='torch'", backend == 'torch'),
                      ('a control path that requires grad (dL/dcoeffs has no bf16 form yet)', _coeffs_need_grad(sde)),
                      ('CPU tensors', not y0.is_cuda)):
        if bad:
            raise ValueError(f"bf16_grad=True (training through the bf16-operand solve) does not take {name}")


def _sdeint_samples(sde, y0, ts, bm, method, dt, options, names, S, sample_grad=False):
    """options={'samples': S}, S > 1: S Brownian paths per input row in one solve, for a predictive mean / variance / ensemble
    (engine.sample_stats).  The control path stays (B, L-1, 4C); y0 (B, H) - or already (B S, H) - and a row_out of length B are
    expanded path-major (path b S + s), the result is (T, B S, H) ((B S, H) with row_out) and path p draws the Philox stream of
    global row row_offset + p.  Inference only unless options={'sample_grad': True}.  Where a kernel maps paths to input rows
    (engine.forward_path(..., samples=S)) the coefficients are read in place; everywhere else (other kernel families, the composed /
    latent / tensor-op routes, CPU) they are replicated with repeat_interleave and the ordinary solve runs with the same seed and
    offsets: the same result either way.
    sample_grad: the solve is differentiable - gradients arrive at the caller's y0 (a (B, H) one: summed over the paths by the
    expansion's own backward), parameters and (B, L-1, 4C) coefficients.  Where the library plans the sampled adjoint
    (engine.backward_mode(..., samples=S, sample_grad=True) == 1) the fused node runs on the coefficients in place and
    dL/d coeffs comes out of snsde_coeff_gradients already summed over the paths; everywhere else the coefficients are
    replicated and the ordinary differentiable solve runs (autograd sums over the paths) - the fused solve again, no warning.
    param_pass='torch' (the library-GEMM cross-check of the native pass) has no sampled form: ValueError."""
    needs_grad = _differentiated(sde, y0)
    if needs_grad and not sample_grad:
        raise ValueError(f"samples={S} is inference only: y0, the control path or a parameter requires grad (use torch.no_grad() or "
                         "requires_grad_(False), or opt in to training through the sample paths with options={'sample_grad': True})")
    if sample_grad:
        for name, bad in (('recompute', bool(options.get('recompute'))), ('save_traj', bool(options.get('save_traj', False))),
                          ("precision='bf16'", options.get('precision', 'fp32') == 'bf16'),
                          ("param_pass='torch'", options.get('param_pass', 'hip') == 'torch')):
            if bad:
                raise ValueError(f"sample_grad=True (training through samples={S} paths per input row) does not take {name}")
    if options.get('save_traj', False) or options.get('recompute'):
        raise ValueError(f"samples={S} is inference only: save_traj / recompute are training options")
    backend = options.get('backend', 'auto')
    if 'z0_linear' in options:
        y0 = _materialise_z0(sde, y0, ts, options.pop('z0_linear'))      # (per input row, before the expansion)
    coeffs = getattr(sde, 'coeffs', None)
    control = torch.is_tensor(coeffs) and coeffs.dim() == 3 and hasattr(sde, 'set_X')
    B = int(coeffs.shape[0]) if control else int(y0.shape[0])
    if y0.shape[0] == B:
        y0 = y0.repeat_interleave(S, dim=0)
    elif y0.shape[0] != B * S:
        raise ValueError(f"samples={S}: y0 has {y0.shape[0]} rows, expected {B} (one per input row) or {B * S} (one per path)")
    row_out = options.get('row_out')
    if row_out is not None:
        if row_out.numel() == B:
            row_out = row_out.repeat_interleave(S)
        elif row_out.numel() != B * S:
            raise ValueError(f"samples={S}: row_out has {row_out.numel()} entries, expected {B} or {B * S}")
        options['row_out'] = row_out
    row_offset = options['row_offset'] = _row_offset(options, B * S)      # (counted in paths)
    if row_offset % S:
        raise ValueError(f"samples={S}: row_offset={row_offset} must be a multiple of samples (whole groups of paths per shard)")
    if backend != 'torch':
        options['global_rows'] = engine.resolve_global_rows(options.get('global_rows'), B * S, row_offset)
        if options['global_rows'] % S:
            raise ValueError(f"samples={S}: global_rows={options['global_rows']} must be a multiple of samples")
    rec = engine.recognise(sde) if _default_names(names) and control else None
    if rec is not None and y0.is_cuda and backend != 'torch':
        model = rec[0]
        grid = engine.step_grid(_HostTimes.get(ts), dt, _HostTimes.get(sde.times), y0.device)
        kernel, precision, L = options.get('kernel', 'auto'), options.get('precision', 'fp32'), int(coeffs.shape[1]) + 1
        engine.precision_flags(precision)
        # (a hidden size the fused route zero-pads runs padded in the replicated solve: take that route, for the same result)
        padded = precision == 'fp32' and kernel == 'auto' and engine.padding_plan(model, B * S, L, grid.N, method) is not None
        # (options['recompute'] was refused above; its process-wide equivalent, which the ordinary solve honours, is left: recompute
        #  mode re-runs the forward chunk by chunk on one coefficient row per path, so such a process trains on the replicated route)
        eng = dict(method=method, kernel=kernel, exact_order=bool(options.get('exact_order', False)), global_rows=int(options['global_rows']),
                   samples=S)      # (the engine's options of this solve: what both queries are asked with)
        if needs_grad:      # the sampled adjoint route (mode 1 with delta planes), or the replicated differentiable solve below
            fused = not padded and not _recompute_steps(options) and engine.backward_mode(model, B * S, L, grid, sample_grad=True, **eng) == 1
        else:
            fused = not padded and engine.forward_path(model, B * S, L, grid.N, precision=precision, row_offset=row_offset, **eng) != 'none'
        if fused:
            try:
                return _sdeint_hip(sde, rec, y0, ts, bm, method, dt, dict(options, samples=S, sample_grad=needs_grad))
            except engine._lib.SnsdeError as exc:
                # the query named a kernel and the launch still found none: the replicated solve, unless the caller's Brownian
                # object has been queried already (a stateful one would not repeat its increments) or the caller is strict
                if not exc.no_kernel or bm is not None or options.get('strict', False) or needs_grad:
                    raise
    saved = (coeffs, sde.times) if control else None
    if control:
        sde.set_X(coeffs.repeat_interleave(S, dim=0), sde.times)
    try:
        return sdeint(sde, y0, ts, bm=bm, method=method, dt=dt, options=options, names=names)
    finally:
        if control:
            sde.set_X(*saved)


def _same_model(a, b):
    return all(getattr(a, f) == getattr(b, f) for f, _ in engine._lib.Model._fields_)


def _same_control(a, b):
    """Two members hold the same control path: set_X with the same tensors (the same storage, shape and version)."""
    for name in ('coeffs', 'times'):
        x, y = getattr(a, name, None), getattr(b, name, None)
        if not (torch.is_tensor(x) and torch.is_tensor(y)):
            return False
        if x is not y and (x.data_ptr() != y.data_ptr() or tuple(x.shape) != tuple(y.shape) or tuple(x.stride()) != tuple(y.stride())
                           or x.dtype != y.dtype):
            return False
    return True


def sdeint_ensemble(sdes, y0, ts, bm=None, method=None, dt=1e-3, options=None):
    """M models of one architecture on one batch in ONE fused solve (include/snsde.h: snsde_solve.members; inference unless
    options={'ensemble_grad': True}): deep-ensemble
    prediction, the seed models of one configuration on a test set, the points of a sweep.

    sdes: a sequence of M modules honouring the Diffusion_model contract with equal model structs, all holding the same control
    path (set_X with the same tensors); y0 (M, B, H).  Returns (T, M, B, H), or (M, B, H) with options['row_out'] of length B.
    Options: seed, row_offset, global_rows, kernel, precision ('bf16' allowed), exact_order, row_out, strict, backend
    (and lean_general, the A/B switch).  Member m's rows are rows row_offset + m B .. of the whole problem: the result equals, bit
    for bit, M ordinary sdeint calls with options row_offset + m B and global_rows (the caller's, else M B).

    Where the library plans it - CUDA float32, no `bm`, B % 4 == 0, engine.forward_path(..., members=M) != 'none' - that is one
    launch over M B rows with the members' parameter blocks stacked and the control path shared; everywhere else (another kernel,
    composed or latent fields, members of different architecture, backend='torch', CPU, a supplied `bm`) exactly those M calls run,
    without a warning: the same result either way.  options={'strict': True} raises NotImplementedError instead of looping.
    ValueError: a solve that would be differentiated (grad enabled and y0, a member's parameter or the coefficients require it)
    without the opt-in below, samples > 1, save_traj, recompute, z0_linear.

    options={'ensemble_grad': True} (SNSDE_FLAG_ENSEMBLE_GRAD) opts in to training: under autograd the result is differentiable
    with respect to y0 (M, B, H), every member's parameters and the shared coefficients.  Where the library plans the ensemble
    adjoint (engine.backward_mode(..., members=M, ensemble_grad=True) == 1: the lean / general 4-row-tile kernels, elementwise
    diffusions, H <= 128) one autograd node runs ONE fused training forward and ONE snsde_backward_with_gradients for all members;
    member m's outputs and gradients equal, bit for bit, its own differentiable sdeint at row_offset + m B with the same global_rows.
    Everywhere else (CPU, backend='torch', a supplied bm, an uncovered plan, B % 4 != 0, different architectures, coefficients that
    require grad) exactly those M differentiable sdeint calls run and are stacked - autograd then sums coeffs.grad over the members;
    options={'strict': True} raises NotImplementedError instead.  ValueError together with ensemble_grad: samples > 1, save_traj,
    recompute (the option or SNSDE_RECOMPUTE_STEPS), z0_linear, sample_grad, bf16_grad, precision='bf16' under autograd,
    param_pass='torch'.

    options={'samples': S, 'ensemble_samples': True} (SNSDE_FLAG_ENSEMBLE_SAMPLES) opts in to S Brownian paths per input row for
    every member: y0 is (M, B, H) - expanded path-major, path b S + s, as sdeint's `samples` does - or already (M, B S, H), a
    row_out has length B or B S, the control path stays (B, L-1, 4C) and the result is (T, M, B S, H); engine.ensemble_stats turns
    it into the predictive mean and the within- / between-member variance.  Member m's rows equal, bit for bit, its own sampled
    sdeint (options samples=S, row_offset + m B S, the same global_rows).  Under autograd it needs ensemble_grad=True and
    sample_grad=True as well (ValueError otherwise); where engine.backward_mode(..., members=M, samples=S, ensemble_samples=True,
    ensemble_grad=True, sample_grad=True) == 1 the one fused node runs.  The loop route - taken in the same cases as above, with
    (B S) % 4 != 0 in place of B % 4 != 0 - runs those M sampled sdeint calls (with sample_grad under autograd): the same result.
    Without ensemble_samples, samples > 1 raises ValueError; sample_grad without samples > 1 and ensemble_samples stays a conflict.

    options={'ensemble_nets': True} (SNSDE_FLAG_ENSEMBLE_NETS) opts in to the fused solve on the kernels of the diffusion nets
    (noise_option 14 / 15 / 18 / 19): the wave pairs at H = 64 (Euler, SRK) and the diffusion-net 4-row tiles (SRK, Milstein, Euler
    at H = 128 or with a wide control path).  Without it those plans keep the loop of M calls (engine.forward_path(..., members=M)
    == 'none'); with it engine.forward_path(..., members=M, ensemble_nets=True) decides, and the contract is the one above, bit for
    bit, `samples` with ensemble_samples included.  Inference only: under autograd (with ensemble_grad) such an ensemble runs the M
    differentiable sdeint calls, as every plan without a fused adjoint does.  A bool, ValueError otherwise; no effect elsewhere.

    options={'ensemble_nets': True, 'ensemble_grad': True, 'ensemble_nets_grad': True} (SNSDE_FLAG_ENSEMBLE_NETS_GRAD) opts in to
    training through such an ensemble on the wave pairs (H = 64, Euler / SRK): where engine.backward_mode(..., members=M,
    ensemble_grad=True, ensemble_nets=True, ensemble_nets_grad=True) == 1 the one fused node runs - one training forward and one
    snsde_backward_with_gradients for all members, block m of the gradient to member m's parameters, bit for bit the member's own
    differentiable sdeint at row_offset + m B.  Everywhere else (the diffusion-net 4-row tiles, `samples`, coefficients that require
    grad, ...) the M differentiable calls run as above and `strict` raises.  ensemble_nets_grad without ensemble_nets and
    ensemble_grad raises ValueError (it names the missing option); a bool, ValueError otherwise."""
    sdes = list(sdes)
    M = len(sdes)
    if M < 1:
        raise ValueError("sdeint_ensemble needs at least one member")
    if not torch.is_tensor(y0) or y0.dim() != 3 or y0.shape[0] != M:
        raise ValueError(f"`y0` must be a 3-dimensional tensor of shape (members, batch, channels) = ({M}, B, H).")
    options = dict(options or {})
    if method is None:
        method = 'srk'
    if method not in METHODS:
        raise ValueError(f"Expected method in {METHODS}, but found {method}.")
    if not (float(dt) > 0):
        raise ValueError("`dt` must be positive.")
    backend = options.get('backend', 'auto')
    if backend not in ('auto', 'hip', 'torch'):
        raise ValueError("options['backend'] must be 'auto', 'hip' or 'torch'")
    S = engine.check_samples(options.pop('samples')) if 'samples' in options else 1
    ensemble_samples = engine.check_ensemble_samples(options.pop('ensemble_samples')) if 'ensemble_samples' in options else False
    if S > 1 and not ensemble_samples:
        raise ValueError("sdeint_ensemble does not take samples > 1 (sample paths of an ensemble are not built) without the opt-in "
                         "options={'ensemble_samples': True}")
    ensemble_samples = ensemble_samples and S > 1      # (no effect on one path per row)
    ensemble_grad = engine.check_ensemble_grad(options.pop('ensemble_grad')) if 'ensemble_grad' in options else False
    ensemble_nets = engine.check_ensemble_nets(options.pop('ensemble_nets')) if 'ensemble_nets' in options else False
    ensemble_nets_grad = engine.check_ensemble_nets_grad(options.pop('ensemble_nets_grad')) if 'ensemble_nets_grad' in options else False
    if ensemble_nets_grad:
        missing = [n for n, on in (('ensemble_nets', ensemble_nets), ('ensemble_grad', ensemble_grad)) if not on]
        if missing:
            raise ValueError("ensemble_nets_grad=True (training through an ensemble on the wave-pair kernels) also needs "
                             + " and ".join(f"options={{'{n}': True}}" for n in missing))
    if ensemble_samples:      # (sample_grad is this route's own option then; everywhere else it stays the conflict it was)
        sample_grad = engine.check_sample_grad(options.pop('sample_grad')) if 'sample_grad' in options else False
    else:
        sample_grad = False
    needs_grad = any(_differentiated(sde, y0) for sde in sdes)
    if ensemble_grad:
        for name, bad in (('save_traj', bool(options.get('save_traj', False))),
                          ("recompute (options['recompute'] or SNSDE_RECOMPUTE_STEPS in the environment)", _recompute_steps(options) > 0),
                          ('z0_linear', 'z0_linear' in options), ('sample_grad', bool(options.get('sample_grad', False))),
                          ('bf16_grad', bool(options.get('bf16_grad', False))),
                          ("precision='bf16' under autograd", needs_grad and options.get('precision', 'fp32') == 'bf16'),
                          ("param_pass='torch'", options.get('param_pass', 'hip') == 'torch')):
            if bad:
                raise ValueError(f"ensemble_grad=True (training through an ensemble of {M} members) does not take {name}")
    for name, bad in (('save_traj', bool(options.get('save_traj', False))), ('recompute', _recompute_steps(options) > 0),
                      ('z0_linear', 'z0_linear' in options), ('sample_grad', bool(options.get('sample_grad', False))),
                      ('bf16_grad', bool(options.get('bf16_grad', False)))):
        if bad:
            raise ValueError(f"sdeint_ensemble is inference only: it does not take {name}")
    if needs_grad and not ensemble_grad:
        raise ValueError("sdeint_ensemble is inference only: y0, the control path or a member's parameter requires grad (use "
                         "torch.no_grad() or requires_grad_(False)); training through an ensemble is not built")
    if needs_grad and ensemble_samples and not sample_grad:
        raise ValueError(f"samples={S} paths per input row of an ensemble are inference only: y0, the control path or a member's parameter "
                         "requires grad (opt in to training through them with options={'ensemble_grad': True, 'sample_grad': True})")
    needs_grad = needs_grad and ensemble_grad
    ts = _as_ts(ts, y0)
    B = int(y0.shape[1])
    if ensemble_samples:
        # y0 (M, B, H) - one row per input row, expanded path-major like _sdeint_samples does - or already (M, B S, H); a row_out of
        # length B likewise.  From here on B counts the PATHS of a member
        c0 = getattr(sdes[0], 'coeffs', None)
        rows_in = int(c0.shape[0]) if torch.is_tensor(c0) and c0.dim() == 3 else B
        if B == rows_in:
            y0 = y0.repeat_interleave(S, dim=1)
        elif B != rows_in * S:
            raise ValueError(f"samples={S}: y0 has {B} rows per member, expected {rows_in} (one per input row) or {rows_in * S} (one per path)")
        B = rows_in * S
        if options.get('row_out') is not None:
            ro = options['row_out']
            if ro.numel() == rows_in:
                options['row_out'] = ro.repeat_interleave(S)
            elif ro.numel() != B:
                raise ValueError(f"samples={S}: row_out has {ro.numel()} entries, expected {rows_in} or {B}")
    row_offset = _row_offset(options, M * B)
    global_rows = engine.resolve_global_rows(options.get('global_rows'), M * B, row_offset) or M * B
    # options={'step_offset': n0}: a continued solve (sdeint's docstring) - handed to the fused call and to the loop of M solves alike
    step_offset = options['step_offset'] = engine.check_step_offset(options.get('step_offset') or 0)
    if step_offset and needs_grad:
        raise ValueError(f"step_offset={step_offset} is inference only: y0, the control path or a member's parameter requires grad; a "
                         "continued solve has no backward")
    if ensemble_samples and (row_offset % S or global_rows % S):
        raise ValueError(f"samples={S}: row_offset={row_offset} and global_rows={global_rows} must be multiples of samples (whole groups "
                         "of paths per shard)")
    options['seed'] = _philox_key(options, y0.device) if bm is None else options.get('seed')      # (one key for every member)
    strict = bool(options.get('strict', False))
    row_out = options.get('row_out')
    if row_out is not None and row_out.numel() != B:
        raise ValueError(f"row_out has {row_out.numel()} entries, expected {B} (one per row of a member)")

    def loop(why):
        if strict:
            raise NotImplementedError(f"sdeint_ensemble: no fused solve of these {M} members ({why}); drop options['strict'] to run "
                                      "them as M sdeint calls")
        opts = {k: v for k, v in options.items() if k not in ('strict', 'lean_general') and v is not None}
        if ensemble_samples:      # the M sampled solves (differentiable ones under sample_grad), each a shard of the whole
            opts['samples'] = S
            if needs_grad:
                opts['sample_grad'] = True
        outs = [sdeint(sde, y0[m], ts, bm=bm, method=method, dt=dt,
                       options=dict(opts, row_offset=row_offset + m * B, global_rows=global_rows)) for m, sde in enumerate(sdes)]
        return torch.stack(outs, dim=0 if row_out is not None else 1)

    if backend == 'torch' or not y0.is_cuda:
        return loop("the tensor-op loop has no fused form" if backend == 'torch' else 'CPU tensors')
    if bm is not None:
        return loop('a supplied Brownian object is queried per member')
    if M == 1 or B % 4:
        return loop('one member' if M == 1 else f'{B} rows per member are not a whole number of 4-row tiles')
    recs = [engine.recognise(sde) for sde in sdes]
    if any(r is None for r in recs):
        return loop('a member does not honour the Diffusion_model contract')
    model, layout, numel = recs[0]
    if not all(_same_model(model, r[0]) for r in recs[1:]):
        return loop('members of different architecture')
    if not all(_same_control(sdes[0], sde) for sde in sdes[1:]):
        return loop('members hold different control paths')
    if needs_grad and _coeffs_need_grad(sdes[0]):
        return loop('the control path requires grad (dL/dcoeffs of an ensemble is the sum of the members\' own)')
    coeffs = sdes[0].coeffs
    if coeffs.dim() != 3 or coeffs.shape[0] != B // S:
        raise ValueError("sde.coeffs must have shape (batch, len(times) - 1, 4 * input_channels)")
    dev = y0.device
    kernel, precision = options.get('kernel', 'auto'), options.get('precision', 'fp32')
    engine.precision_flags(precision)
    exact_order, lean_general = bool(options.get('exact_order', False)), bool(options.get('lean_general', False))
    L = int(coeffs.shape[1]) + 1
    grid = engine.step_grid(_HostTimes.get(ts), dt, _HostTimes.get(sdes[0].times), dev)
    # the engine's options of this solve, built once: the path query, the mode query and the launch all take them
    eng = dict(method=method, kernel=kernel, precision=precision, exact_order=exact_order, lean_general=lean_general, global_rows=global_rows,
               members=M, samples=S if ensemble_samples else 0, ensemble_samples=ensemble_samples, ensemble_nets=ensemble_nets)
    if engine.forward_path(model, M * B, L, grid.N, row_offset=row_offset, **eng) == 'none':
        return loop('the plan arrives at a kernel that does not map rows to members')
    if needs_grad:
        # the ensemble adjoint route (mode 1 with delta planes for every member), or the M differentiable solves
        # (the training solve: fp32, with its opt-ins and without lean_general, which neither the mode query nor the node passes)
        train = dict(eng, ensemble_grad=True, sample_grad=ensemble_samples, ensemble_nets_grad=ensemble_nets_grad)
        del train['lean_general']
        if precision != 'fp32' or engine.backward_mode(model, M * B, L, grid, **train) != 1:
            return loop('no fused adjoint plans this ensemble')
        pidxs = [engine.param_index(sde, r[1]) for sde, r in zip(sdes, recs)]
        counts = [len(p.params) for p in pidxs]
        eopt = _EnsembleOptions(engine=train, param_pass=options.get('param_pass', 'hip'), row_offset=row_offset, seed=options['seed'],
                                row_out=None if row_out is None else _device_row_out(options, dev).repeat(M))
        ys = _FusedEnsembleSolve.apply(sdes, recs, coeffs.detach().to(device=dev, dtype=torch.float32).contiguous(), grid, method, eopt,
                                       counts, y0, *[p for pi in pidxs for p in pi.params])
        return ys.reshape(M, B, -1) if row_out is not None else ys.reshape(grid.T, M, B, -1)
    flat = torch.stack([engine.flatten_params(sde, r[1], r[2], dev) for sde, r in zip(sdes, recs)])      # (M, numel)
    coeffs = coeffs.detach().to(device=dev, dtype=torch.float32).contiguous()
    y0c = y0.detach().to(torch.float32).reshape(M * B, -1).contiguous()
    rows = None if row_out is None else _device_row_out(options, dev).repeat(M)
    call = engine.SolveCall(model, flat, coeffs, grid, y0c, seed=options['seed'], row_offset=row_offset, row_out=rows, step_offset=step_offset,
                            **eng)
    try:
        ys = call.launch()
    except engine._lib.SnsdeError as exc:
        if not exc.no_kernel:
            raise
        return loop(f'the launch was refused ({exc})')
    ys = ys.reshape(M, B, -1) if row_out is not None else ys.reshape(grid.T, M, B, -1)
    return ys.to(y0.dtype)


# What the fused ensemble node reads from `options`, resolved once by sdeint_ensemble: `engine`, the engine's options of the training
# solve (the keywords its mode query was asked with and its SolveCall takes), and what is no engine configuration
_EnsembleOptions = collections.namedtuple('_EnsembleOptions', ('engine', 'param_pass', 'row_offset', 'seed', 'row_out'))


class _FusedEnsembleSolve(torch.autograd.Function):
    """Differentiable fused solve of M members (options={'ensemble_grad': True}, mode 1 only): forward = ONE training-mode solve
    with members = M (engine.SolveCall(..., **opt.engine): ensemble_grad=True), backward = ONE snsde_backward_with_gradients (param_pass='split':
    the two C calls) whose (M, numel) gradient is handed to each member's parameters block by block.  The increment-keeping rule is
    _FusedSolve.forward's (keep_dw)."""

    NO_GRAD_INPUTS = 7      # sdes .. counts; y0 and the members' parameters follow

    @staticmethod
    def forward(ctx, sdes, recs, coeffs, grid, method, opt, counts, y0, *params):
        model, layout, numel = recs[0]
        M, B = int(y0.shape[0]), int(y0.shape[1])
        dev = y0.device
        flat = torch.stack([engine.flatten_params(sde, r[1], r[2], dev) for sde, r in zip(sdes, recs)])      # (M, numel)
        y0c = y0.detach().to(torch.float32).reshape(M * B, -1).contiguous()
        keep_dw = not (method in ('euler', 'milstein') and not torch.is_tensor(opt.seed) and opt.param_pass in ('hip', 'split')
                       and os.environ.get('SNSDE_KEEP_INCREMENTS') != '1')
        call = engine.SolveCall(model, flat, coeffs, grid, y0c, seed=opt.seed, row_offset=opt.row_offset, save_traj=True, save_dW=keep_dw,
                                save_act=True, row_out=opt.row_out, **opt.engine)
        ys = call.launch()
        ctx.call, ctx.sdes, ctx.layouts, ctx.counts = call, sdes, [r[1] for r in recs], counts
        ctx.param_pass, ctx.y0_shape, ctx.y0_dtype = opt.param_pass, tuple(y0.shape), y0.dtype
        return ys.to(y0.dtype) if y0.dtype != ys.dtype else ys.detach()

    @staticmethod
    def backward(ctx, grad_ys):
        call = ctx.call
        grad_ys = grad_ys.to(torch.float32).contiguous()
        if ctx.param_pass == 'split':      # the two C calls one after the other, every a_n written
            adj, delta = engine.solve_backward(call, grad_ys, save_delta=True, adj0_only=False)
            flat = engine.param_gradients(call, adj, delta)
        else:
            adj, flat = engine.backward_with_gradients(call, grad_ys, adj0_only=True)
        grads = []
        for m, (sde, layout) in enumerate(zip(ctx.sdes, ctx.layouts)):
            grads.extend(engine.param_index(sde, layout).grads_from_flat(flat[m]))
        return (None,) * _FusedEnsembleSolve.NO_GRAD_INPUTS + (adj[0].reshape(ctx.y0_shape).to(ctx.y0_dtype),) + tuple(grads)


def sdeint_adjoint(sde, y0, ts, bm=None, method=None, adjoint_method=None, adjoint_adaptive=False, adjoint_rtol=1e-5,
                   adjoint_atol=1e-4, adjoint_options=None, adjoint_params=None, names=None, **kwargs):
    """torchsde.sdeint_adjoint's call contract (in-tree user: torch-ists .../NSDE/latent_sde.py:134-141).  Gradients come
    from the adjoint of the DISCRETE scheme: for a Diffusion_model on CUDA the fused HIP adjoint kernels
    (snsde_solve_backward + snsde_param_gradients: no autograd graph over the steps, memory O(N B H) of saved states
    rather than ~25 autograd nodes per step), otherwise autograd through the tensor-op loop.  torchsde integrates the
    continuous adjoint SDE backwards instead; the two agree to the discretisation error of the forward scheme.  The
    adjoint_* solver options have no counterpart here: they are accepted for signature compatibility and a non-default value
    is reported once per process."""
    given = [n for n, v, d in (('adjoint_method', adjoint_method, None), ('adjoint_adaptive', adjoint_adaptive, False),
                               ('adjoint_rtol', adjoint_rtol, 1e-5), ('adjoint_atol', adjoint_atol, 1e-4),
                               ('adjoint_options', adjoint_options, None), ('adjoint_params', adjoint_params, None)) if v != d]
    if given and 'sdeint_adjoint' not in _UNFUSED_WARNED:
        _UNFUSED_WARNED.add('sdeint_adjoint')
        warnings.warn(f"sdeint_adjoint: {', '.join(given)} ignored - gradients are the adjoint of the DISCRETE scheme "
                      "(fused HIP adjoint kernels for a Diffusion_model on CUDA, autograd through the step loop otherwise), "
                      "not torchsde's continuous stochastic adjoint; both agree to the forward scheme's discretisation error.")
    return sdeint(sde, y0, ts, bm=bm, method=method, names=names, **kwargs)


# the resampling step and the genealogy trace under this module's name too (what a `import torchsde` user of sdeint_filter reaches for)
sample_resample, filter_paths, filter_particles = engine.sample_resample, engine.filter_paths, engine.filter_particles

FilterResult = collections.namedtuple('FilterResult', 'ys log_weight ancestor ess logz')


def sdeint_filter(sde, y0, ts, log_likelihood, bm=None, method=None, dt=None, options=None, threshold=0.5, stratified=False,
                  generator=None, differentiable=False):
    """Bootstrap particle filter of an SDE state-space model on the sample paths of a solve: options={'samples': S} (required)
    paths per input row are advanced from one observation time to the next, weighed by the observation and resampled.  For
    k = 1 .. T-1:
      1. ``sdeint`` over [ts[k-1], ts[k]]: the first piece with ``extra=True``, the later ones with ``extra_solver_state`` - the
         SAME Brownian streams at the global step count, so slot p keeps slot p's stream and two children of one ancestor
         diverge on independent noise;
      2. ``inc = log_likelihood(k, y_k)``: y_k (B S, H) is the state at ts[k], inc (B, S) the log-likelihood of observation k per
         path (for example ``sample_loglik(readout(y_k), S, obs[k], stats=True)[1]``);
      3. ``engine.sample_resample(y_k, S, log_weight, inc, None, threshold, stratified, generator)``;
      4. the resampled state is the next piece's ``y0``.
    Returns FilterResult(ys (T, B S, H): the states BEFORE each resampling; log_weight (T, B, S): the carried weights after each
    step; ancestor (T, B, S) int32; ess (T, B); logz (T, B)).  Entry 0 is the start: zero weights, the identity, ess = S,
    logz = 0.  logsumexp(log_weight[k]) - log S = logz[k] = log p(y_1..k) (the running estimate of the log marginal likelihood);
    ``engine.filter_paths(ys, ancestor, S)`` traces the surviving trajectories; the particles after the last resampling are
    ys[-1] gathered by ancestor[-1].  log_weight[k] belongs to the particles AFTER step k's resampling, ys[k] gathered by
    ancestor[k]: ``engine.filter_particles(ys, ancestor, S)`` is that set for every k, and
    ``engine.sample_stats(engine.filter_particles(r.ys, r.ancestor, S), S, log_weight=r.log_weight)`` the filtered mean and
    variance of all T times in one launch (``sample_crps`` and ``sample_quantiles`` take ``log_weight=`` likewise).  dt=None reads options['dt'], else sdeint's default.  Inference only by default (the loop runs under no_grad); a route that cannot
    continue a Brownian path raises in ``sdeint`` (its docstring), and ensembles are not driven here (``sample_resample`` itself
    serves them).
    differentiable=True trains through the filter: the loop runs with autograd enabled, every piece is solved with
    options sample_grad and resume_grad (``sdeint``'s docstring: the fused adjoint of a continued, sampled solve), ``inc`` keeps its
    graph and the resampling is ``sample_resample(..., differentiable=True)``, whose backward holds the ancestors fixed.  logz,
    log_weight and ys then carry gradients to the model's parameters, y0, the control path and whatever ``log_likelihood`` closes
    over; ancestor and ess carry none.  ``-r.logz[-1].mean()`` is the FIVO loss (Maddison et al. 2017) - its gradient drops the
    score-function term of the resampling decisions, the estimator that paper trains with.  The forward values equal those of
    the default call bit for bit under the same seed and ``generator``."""
    options = dict(options or {})
    if 'samples' not in options:
        raise ValueError("sdeint_filter needs options={'samples': S}: the particles per input row")
    S = engine.check_samples(options['samples'])
    if not callable(log_likelihood):
        raise ValueError("log_likelihood must be callable: log_likelihood(k, y_k) -> (B, S) log-likelihood of observation k per path")
    if not torch.is_tensor(y0) or y0.dim() != 2:
        raise ValueError("`y0` must be a 2-dimensional tensor of shape (batch, channels).")
    ts = _as_ts(ts, y0)
    if dt is None:
        dt = options.get('dt', 1e-3)
    coeffs = getattr(sde, 'coeffs', None)
    control = torch.is_tensor(coeffs) and coeffs.dim() == 3 and hasattr(sde, 'set_X')
    T = int(ts.numel())
    ys, state, y, logw = [], None, y0, None
    weights, ancestors, esss, logzs = [], [], [], []
    differentiable = bool(differentiable)
    if differentiable:
        options.update(sample_grad=True, resume_grad=True)
    with torch.enable_grad() if differentiable else torch.no_grad():
        for k in range(1, T):
            # (without a control path nothing tells an expanded y0 from a batch of B S rows: the later pieces hand their rows over as they are)
            opts = options if k == 1 or control else {o: v for o, v in options.items() if o != 'samples'}
            piece, state = sdeint(sde, y, ts[k - 1:k + 1], bm=bm, method=method, dt=dt, options=opts, extra=True, extra_solver_state=state)
            if k == 1:
                B = int(piece.shape[1]) // S
                logw = torch.zeros((B, S), device=piece.device, dtype=piece.dtype)
                ys.append(piece[0])
                weights.append(logw)
                ancestors.append(torch.arange(S, device=piece.device, dtype=torch.int32).expand(B, S).contiguous())
                esss.append(torch.full((B,), float(S), device=piece.device, dtype=piece.dtype))
                logzs.append(torch.zeros((B,), device=piece.device, dtype=piece.dtype))
            yk = piece[1]
            inc = log_likelihood(k, yk)
            if not torch.is_tensor(inc) or tuple(inc.shape) != (B, S):
                raise ValueError(f"log_likelihood({k}, y_k) must return a tensor of shape {(B, S)} (one log-likelihood per input row and "
                                 f"path), got {tuple(inc.shape) if torch.is_tensor(inc) else type(inc).__name__}")
            inc = (inc if differentiable else inc.detach()).to(device=logw.device, dtype=logw.dtype)
            r = engine.sample_resample(yk, S, logw, inc, None, threshold, stratified, generator, differentiable=differentiable)
            ys.append(yk)
            weights.append(r.log_weight)
            ancestors.append(r.ancestor)
            esss.append(r.ess)
            logzs.append(r.logz)
            y, logw = r.state, r.log_weight
    return FilterResult(torch.stack(ys), torch.stack(weights), torch.stack(ancestors), torch.stack(esss), torch.stack(logzs))


def _materialise_z0(sde, y0, ts, lin):
    """lin = options['z0_linear'] = the wrapper's `initial_network`: y0 is a placeholder and the solve starts from
    initial_network(X(ts[0])) (NeuralSDE._prepare_initial_state, neuralsde.py:63-69).  Evaluated here with tensor ops for
    every path but the no-grad fused solve, which computes it inside its prepare launch."""
    return lin(sde.X.evaluate(ts[0])).to(y0.dtype)


def _z0_fusable(lin, sde, y0):
    w, b = lin.weight, lin.bias
    return (b is not None and w.is_cuda and w.dtype == torch.float32 and b.dtype == torch.float32 and w.is_contiguous()
            and tuple(w.shape) == (y0.shape[1], sde.input_channels) and not torch.is_grad_enabled())


class _DrawnIncrements:
    """bm(ta, tb[, return_U]) over increments that were already drawn from the caller's Brownian object, in call order: a
    fallback from the fused path to the tensor-op loop must not query a stateful `bm` a second time."""

    def __init__(self, dW, dU=None):
        self.dW, self.dU, self.n = dW, dU, 0

    def __call__(self, ta, tb=None, return_U=False, **kwargs):
        i, self.n = self.n, self.n + 1
        return (self.dW[i], self.dU[i]) if return_U else self.dW[i]


# What a fused solve reads from `options`, resolved once by _sdeint_hip: _FusedSolve.forward and _sdeint_padded take this record
# and the backward mode decided beside it, never the dict.  `engine`: the engine's options of the solve - the keywords the mode
# query is asked with and SolveCall takes (method, kernel, precision, exact_order, global_rows, samples, sample_grad, bf16_grad);
# the rest is no engine configuration, but for lean_general, which only the sampled node passes on
# step_offset: of a differentiated solve only under options['resume_grad'] (sdeint has refused the others)
_FusedOptions = collections.namedtuple('_FusedOptions', (
    'engine', 'save_traj', 'strict', 'param_pass', 'recompute', 'lean_general', 'row_offset', 'row_out', 'seed', 'step_offset'))


def _sdeint_hip(sde, rec, y0, ts, bm, method, dt, options):
    model, layout, numel = rec
    dev = y0.device
    z0_lin = None
    if 'z0_linear' in options:
        z0_lin = options['z0_linear']
        if not (_z0_fusable(z0_lin, sde, y0) and bm is None and options.get('kernel', 'auto') == 'auto'
                and not options.get('save_traj', False)):
            y0, z0_lin = _materialise_z0(sde, y0, ts, z0_lin), None
    pidx = engine.param_index(sde, layout)
    coeff_grad = _coeffs_need_grad(sde)      # dL/d coeffs wanted: the adjoint's delta planes give it (engine.coeff_gradients)
    needs_grad = _differentiated(sde, y0, pidx.params)
    coeffs = coeffs_src = sde.coeffs
    # (samples > 1: from _sdeint_samples only - a kernel that takes it, no padding; sample_grad: a training solve the library plans)
    samples = int(options.get('samples', 1))
    if coeffs.dim() != 3 or coeffs.shape[0] * samples != y0.shape[0]:
        raise ValueError("sde.coeffs must have shape (batch, len(times) - 1, 4 * input_channels)")
    coeffs = coeffs.detach().to(device=dev, dtype=torch.float32).contiguous()
    y0c = y0.detach().to(torch.float32).contiguous()
    B, L = y0c.shape[0], coeffs.shape[1] + 1
    times_host = _HostTimes.get(sde.times)
    grid = engine.step_grid(_HostTimes.get(ts), dt, times_host, dev)
    # (without `bm` the kernels draw Philox increments: nothing to draw here)
    dW, dU = _draw_increments(bm, grid, y0, method, dtype=torch.float32, philox=True, host_times=True)

    step_offset = int(options.get('step_offset') or 0)      # (a continued solve: inference, or training under resume_grad)

    def loop():      # the tensor-op loop on the same device, on the increments already drawn (and on y0 as it is by then)
        if dW is None:
            _continued_without_path(options, None, 'the tensor-op loop this configuration falls back to (no kernel covers it)')
        return _sdeint_torch(sde, y0, ts, bm if dW is None else _DrawnIncrements(dW, dU), method, dt, options, None)
    row_offset = _row_offset(options, B)
    # options={'global_rows': N | 'world'}: the rows of the whole problem this batch is a shard of - the library then plans its
    # kernels as for N rows on one device, and the shards reproduce the unsharded solve bit for bit (opt-in; default: the local batch)
    kernel, precision = options.get('kernel', 'auto'), options.get('precision', 'fp32')
    global_rows = engine.resolve_global_rows(options.get('global_rows'), B, row_offset)
    bf16_grad = bool(options.get('bf16_grad', False)) and precision == 'bf16'
    eng = dict(method=method, kernel=kernel, precision=precision, exact_order=bool(options.get('exact_order', False)), global_rows=global_rows,
               samples=samples, sample_grad=bool(options.get('sample_grad', False)), bf16_grad=bf16_grad)
    opt = _FusedOptions(
        engine=eng, seed=_philox_key(options, dev), save_traj=bool(options.get('save_traj', False)),
        strict=bool(options.get('strict', False)), param_pass=options.get('param_pass', 'hip'), recompute=_recompute_steps(options),
        lean_general=bool(options.get('lean_general', False)), row_offset=row_offset, row_out=_device_row_out(options, dev),
        step_offset=step_offset)
    if precision == 'bf16':
        if needs_grad and not bf16_grad:      # (a z0_linear that requires grad was materialised above: y0 then does)
            raise ValueError("precision='bf16' is inference only: y0 or a parameter requires grad")
        if opt.save_traj and not (needs_grad and bf16_grad):
            raise ValueError("precision='bf16' is inference only: save_traj is a training output")
        engine.check_bf16(model, B, L, grid.N, method, kernel)
        # training (bf16_grad): the bf16 kernel with the fused MFMA adjoint behind it, or an error - whatever `strict` says, the
        # tensor-op loop cannot round operands and no f32 kernel stands in
        if needs_grad and engine.backward_mode(model, B, L, grid, **eng) != 1:      # (bf16_grad: one path per row, _bf16_grad_conflicts)
            raise ValueError(f"bf16_grad=True does not cover this configuration (hidden_channels={model.hidden_channels}, "
                             f"num_hidden_layers={model.num_hidden_layers}, input_option={model.input_option}, "
                             f"noise_option={model.noise_option}, method={method!r}, kernel={kernel!r}): no fused adjoint plans "
                             "this bf16-operand solve")
    if engine.shard_refused(model, B, L, grid.N, method, kernel, global_rows=global_rows, row_offset=row_offset):
        # the kernel planned for the whole problem cannot run this shard (a wave-pair plan, fewer than four rows): an error with or
        # without `strict` - another kernel or the tensor-op loop would not reproduce the unsharded solve
        raise engine._lib.SnsdeError(engine._lib.SNSDE_ERR_UNSUPPORTED,
                                     f"global_rows={global_rows}: the kernel planned for the whole problem cannot run this "
                                     f"{B}-row shard")
    # (options['recompute'] alone, not _recompute_steps: its process-wide equivalent moves no model off the padded solve, which
    #  never recomputes)
    if precision == 'fp32' and kernel == 'auto' and not opt.save_traj and not options.get('recompute') and samples == 1:
        pad = engine.padding_plan(model, B, L, grid.N, method)
        if pad is not None and coeff_grad:      # (the padded solve's autograd node has no coefficient gradient: the fallback rule)
            _unfused_coeff_grad(sde, f"hidden_channels={model.hidden_channels} (a zero-padded solve)", options)
            return loop()
        # a hidden size without MFMA instantiation: solve the zero-padded model (exact) - in training, where its adjoint is the MFMA one
        if pad is not None and (not needs_grad or engine.backward_mode(pad[0], B, L, grid, method, global_rows=global_rows) == 1):
            if z0_lin is not None:
                y0, z0_lin = _materialise_z0(sde, y0, ts, z0_lin), None
            return _sdeint_padded(sde, rec, pad, coeffs, grid, y0, dW, dU, method, opt, needs_grad, step_offset)
    if needs_grad:
        mode = engine.backward_mode(model, B, L, grid, **eng)
        if samples > 1 and mode != 1:      # (_sdeint_samples asked the same query: the sampled node is mode 1 or not built at all)
            raise engine._lib.SnsdeError(engine._lib.SNSDE_ERR_UNSUPPORTED, f"samples={samples}: no fused adjoint plans this sampled solve")
        if mode == 0 and opt.strict:
            raise NotImplementedError(
                "the fused backward covers 'euler', 'srk' and 'milstein' for every noise_option (Milstein: all but 7, "
                "sqrt(y), whose derivative is not finite at the clipped values), within the LDS budget of the generic "
                "adjoint kernels; pass options={'backend': 'torch'} to differentiate this configuration through the "
                "tensor-op loop")
        if mode == 0:
            # no fused adjoint for this configuration (Milstein with sqrt(y); shapes beyond the generic adjoint's LDS budget):
            # differentiate through the unfused tensor-op loop on the same device rather than fail the
            # reference's training loop; options={'strict': True} raises instead
            key = (sde.input_option, sde.noise_option, method)
            if key not in _UNFUSED_WARNED:
                _UNFUSED_WARNED.add(key)
                warnings.warn(f"sdeint: no fused backward for input_option={key[0]}, noise_option={key[1]}, method={method!r}; "
                              "differentiating through the unfused tensor-op loop (slow).")
            return loop()
        if coeff_grad and mode == 1 and method != 'srk' and samples == 1 and opt.recompute > 0:
            what = "options['recompute']"
        else:
            try:      # (_NoCoeffGradient: only where dL/d coeffs is wanted)
                return _FusedSolve.apply(sde, rec, coeffs, grid, times_host, (dW, dU), method, opt, mode,
                                         coeffs_src if coeff_grad else None, y0, *pidx.params)
            except _NoCoeffGradient:
                what = (f"input_option={sde.input_option}, noise_option={sde.noise_option}, method={method!r}, "
                        f"hidden_channels={model.hidden_channels} at {B} rows (an adjoint that sums the weight gradients itself)")
        _unfused_coeff_grad(sde, what, options)
        return loop()
    flat = engine.flatten_params(sde, layout, numel, dev)
    call = engine.SolveCall(model, flat, coeffs, grid, y0c, dW=dW, seed=opt.seed, row_offset=opt.row_offset, save_traj=opt.save_traj, dU=dU,
                            row_out=opt.row_out, step_offset=step_offset,
                            z0_linear=None if z0_lin is None else (z0_lin.weight.detach(), z0_lin.bias.detach().contiguous()),
                            **dict(eng, sample_grad=False, bf16_grad=False))      # (inference: the training opt-ins stay off)
    try:
        ys = call.launch()
    except engine._lib.SnsdeError as exc:
        if samples > 1:              # (the path query accepted this solve: a refusal now is an error, not another route)
            raise
        if precision == 'bf16':      # (checked above; a refusal here is not answered with an fp32 solve either)
            raise ValueError(f"precision='bf16': the solve was refused ({exc})") from exc
        # a valid request no kernel covers (Milstein with noise_option 7, sqrt(y)): same behaviour as the gradient path, the
        # unfused tensor-op loop, unless strict
        # (SNSDE_ERR_LDS: a hidden size whose per-tile buffers exceed the LDS budget of the only kernel family that covers
        # the request — the generic Milstein kernel for the diffusion nets above H ~ 460 — is the same situation)
        if not exc.no_kernel or opt.strict:
            raise
        if z0_lin is not None:
            y0 = _materialise_z0(sde, y0, ts, z0_lin)
        return loop()
    if opt.save_traj:
        sde.last_trajectory = call.traj
    return ys.to(y0.dtype)


def _sdeint_composed(sde, y0, ts, bm, method, dt, options):
    """Fused solve of a tutorial-style field (tutorial/*.ipynb cell 7; fields.compose): no-grad calls only, the lean
    4-row-tile kernel with the variant switches.  None = not such a field / not covered: the caller takes the generic
    stepper."""
    from . import fields
    needs_grad = _differentiated(sde, y0)      # (a solve whose coefficients require grad returns below)
    field = fields.compose(sde)
    coeffs = getattr(sde, 'coeffs', None)
    if field is None or not torch.is_tensor(coeffs) or coeffs.dim() != 3 or coeffs.shape[0] != y0.shape[0]:
        return None
    if _coeffs_need_grad(sde):      # (composed fields return no coefficient gradient: the fallback rule)
        _unfused_coeff_grad(sde, "a composed (tutorial-style) field", options)
        return None
    dev = y0.device
    if torch.cuda.is_current_stream_capturing() and (bm is not None or field.verified.get(str(dev)) is not True):
        return None      # graph capture: solves (training ones too) of a mapping that was verified before the capture (a warm-up solve)
    coeffs = coeffs.detach().to(device=dev, dtype=torch.float32).contiguous()
    times_host = _HostTimes.get(sde.times)
    if not fields.verify(field, coeffs, times_host, dev):
        return None
    grid = engine.step_grid(_HostTimes.get(ts), dt, times_host, dev)
    # (the ODE field has no diffusion: nothing to draw; without `bm` the kernels draw Philox increments)
    dW, dU = _draw_increments(None if field.parts.get('ode', False) else bm, grid, y0, method, dtype=torch.float32, philox=True,
                              host_times=True)
    tab_times = engine.noise_table_times(grid, method)
    seed = _philox_key(options, dev)
    row_offset = _row_offset(options, y0.shape[0])
    # (these fields run on 4-row tiles at every batch size: the option is checked and handed down, it moves no choice today)
    global_rows = engine.resolve_global_rows(options.get('global_rows'), y0.shape[0], row_offset)
    row_out = _device_row_out(options, dev)
    if needs_grad:
        # training: the composition and the module's own g stay in the autograd graph; the solve between them is the fused
        # forward + adjoint + weight-gradient pass (flat-block and table gradients flow back through those graphs)
        if engine.backward_mode(field.model, int(y0.shape[0]), coeffs.shape[1] + 1, grid, method, table=field.tabulated,
                                global_rows=global_rows) != 1:
            return None
        flat = field.flat(dev, grad=True)
        tab = field.noise_table(tab_times, dev, grad=True) if field.tabulated else None
        return _ComposedSolve.apply(field.model, coeffs, grid, dW, method, seed, row_offset, row_out, y0, flat, tab, dU, None,
                                    global_rows, int(options.get('step_offset') or 0))      # (an offset here: sdeint's resume_grad opt-in)
    # options={'trust_versions': True}: the cached composed block / table are keyed on the parameters' addresses and version
    # counters alone (no content fingerprint = no device->host read per solve); in-place edits through `.data` are then the
    # caller's to avoid
    field.trust_versions = bool(options.get('trust_versions', False))
    flat, tab = field.inference_inputs(tab_times, dev)
    call = engine.SolveCall(field.model, flat, coeffs, grid, y0.detach().to(torch.float32).contiguous(), dW=dW, dU=dU,
                            method=method, seed=seed, row_offset=row_offset, row_out=row_out, noise_table=tab,
                            global_rows=global_rows, step_offset=int(options.get('step_offset') or 0))
    try:
        return call.launch().to(y0.dtype)
    except engine._lib.SnsdeError as exc:
        if not exc.no_kernel:
            raise
        return None


def _draw_increments(bm, grid, y0, method, seed=None, dtype=None, philox=False, scalar=False, host_times=False):
    """Every increment of a solve up front, (N, B, H) I_k (and I_k0 for SRK, which asks `bm` with return_U=True as torchsde does),
    on y0's device in `dtype` (default: y0's).  The only code that queries a caller's Brownian object: once per step, in step
    order, at the grid's times - host tensors with host_times, else on y0's device.  Without `bm`: (None, None) under `philox`
    (the kernels draw the increments), else a torch generator seeded with `seed` (an int; otherwise a fresh seed); `scalar`:
    that draw is (N, B, 1), torchsde's scalar noise."""
    if bm is None and philox:
        return None, None
    dev, dtype = y0.device, y0.dtype if dtype is None else dtype
    t0s, t1s = torch.from_numpy(grid.t0), torch.from_numpy(grid.t1)
    if not host_times or bm is None:
        t0s, t1s = t0s.to(dev), t1s.to(dev)
    if bm is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed) if seed is not None and not torch.is_tensor(seed) else _fresh_seed())
        hcol = (t1s - t0s).to(dtype).reshape(-1, *([1] * y0.dim()))
        wshape = (grid.N, y0.shape[0], 1) if scalar else (grid.N,) + tuple(y0.shape)
        dW = torch.randn(wshape, dtype=dtype, device=dev, generator=gen) * hcol.sqrt()
        dU = None
        if method == 'srk':      # I_k0 = h (I_k / 2 + sqrt(h / 12) xi): the space-time Levy integral
            xi = torch.randn((grid.N,) + tuple(y0.shape), dtype=dtype, device=dev, generator=gen)
            dU = hcol * (0.5 * dW + (hcol / 12).sqrt() * xi)
        return dW, dU
    drawn = [bm(t0s[n], t1s[n], **({'return_U': True} if method == 'srk' else {})) for n in range(grid.N)]
    stack = lambda parts: torch.stack([p.to(device=dev, dtype=dtype) for p in parts])
    return (stack([d[0] for d in drawn]), stack([d[1] for d in drawn])) if method == 'srk' else (stack(drawn), None)


def _sdeint_latent(sde, y0, ts, bm, method, dt, options, names):
    """torch-ists' LatentSDE through names={'drift': 'f_aug', 'diffusion': 'g_aug'} (latent_sde.py:60-89, 134-141): the state
    is [latent | KL accumulator] and the accumulator never feeds back, so the solve splits into
      * the LATENT dynamics - posterior-drift MLP of [sin t, cos t, y], constant shared diffusion - on the fused kernels
        (fields.compose_latent: forward, adjoint and weight gradients as for the tutorial fields), returning every state, and
      * the accumulator = the scheme's own update of the last channel, evaluated for ALL steps at once: one batched call of the
        module's f_aug / g_aug (the same `_srk_step` / Euler update the tensor-op loop runs) on the (N B) states of the solve.
    Autograd joins the two: the batched step's graph gives d/d parameters and the cotangents of every state, which enter the
    fused adjoint as output gradients.  N sequential launches of ~25-100 kernels become one solve + one batched step.
    Falls back to the tensor-op loop (same increments) for anything it does not recognise."""
    from . import fields
    _continued_without_path(options, bm, 'the latent route')
    field = None
    if y0.dim() == 2 and y0.shape[1] >= 2 and not torch.cuda.is_current_stream_capturing() and 'row_out' not in options:
        field = fields.compose_latent(sde, names, int(y0.shape[1]))
    if field is None:
        return _sdeint_torch(sde, y0, ts, bm, method, dt, options, names)
    dev, B = y0.device, int(y0.shape[0])
    Hl, P = field.parts['latent'], field.model.hidden_channels
    ts_host = _HostTimes.get(ts)
    times_host = np.array([ts_host[0], ts_host[-1]], dtype=np.float32)
    grid = engine.step_grid(ts_host, dt, times_host, dev)
    # Increments: the caller's `bm` or, with options['seed'], the generator stream the tensor-op loop draws (same results on both
    # paths) are drawn up front; an unseeded call of the in-solve accumulator path lets the kernels draw Philox increments
    # (no (N, B, H) tensors of normals at all) and only draws here if it has to fall back
    acc = field.parts.get('acc')
    # (a learnable prior / diffusion - any tensor h() or g() can reach that requires grad - keeps the split solve below, whose
    #  quadrature goes through the module's own f_aug and carries that gradient; the in-solve constants are plain floats)
    in_solve = (acc is not None and P > Hl and os.environ.get('SNSDE_LATENT_SPLIT') != '1' and
                not (torch.is_grad_enabled() and any(t.requires_grad for t in field.parts.get('prior_leaves', ()))))
    philox = in_solve and bm is None and options.get('seed') is None
    drawn = []

    def increments():
        if not drawn:
            drawn.append(_draw_increments(bm, grid, y0, method, seed=options.get('seed')))
        return drawn[0]
    dW, dU = (None, None) if philox else increments()

    def fallback():
        return _sdeint_torch(sde, y0, ts, _DrawnIncrements(*increments()), method, dt, options, names)
    view = field.sde
    cache = field.__dict__.setdefault('_dummy_control', {})
    key = (B, str(dev))
    if key not in cache:        # the field has no control path: one zero channel on the knots [ts[0], ts[-1]]
        cache.clear()
        cache[key] = torch.zeros(B, 1, 4, device=dev, dtype=torch.float32)
    coeffs = cache[key]
    view.coeffs, view.times = coeffs, torch.from_numpy(times_host).to(dev)
    try:
        if not fields.verify(field, coeffs, times_host, dev):
            return fallback()
    except RuntimeError:
        return fallback()
    needs_grad = _differentiated(sde, y0)      # (a latent module has no control path: y0 and the parameters)
    widen = lambda t: None if t is None else torch.nn.functional.pad(t[..., :Hl].to(torch.float32), (0, P - Hl)).contiguous()
    # (1) the accumulator INSIDE the solve (snsde.h: kl_column1): column Hl of the padded state integrates the KL rate with the
    #     scheme's own drift weights, the adjoint kernels carry its cotangent back into the drift net - one solve over the
    #     caller's grid, no quadrature launches.  Needs the module's prior drift in the form fields.compose_latent recognised,
    #     a diffusion without gradient (the reference's sigma is a buffer) and a spare padded column.
    if in_solve:
        kl = (Hl, acc[0], acc[1])
        key = _fresh_seed() if philox else 0
        tt = engine.noise_table_times(grid, method)
        y0a = torch.nn.functional.pad(y0[:, :Hl + 1], (0, P - Hl - 1))
        try:
            if needs_grad:
                tab = field.noise_table(tt, dev, grad=True)
                if not tab.requires_grad and engine.backward_mode(field.model, B, 2, grid, method, table=True, kl_column=Hl) == 1:
                    Y = _ComposedSolve.apply(field.model, coeffs, grid, widen(dW), method, key, 0, None, y0a, field.flat(dev, grad=True),
                                             tab.detach(), widen(dU), kl)
                    return Y[:, :, :Hl + 1].to(y0.dtype)
            else:
                flat, tab = field.inference_inputs(tt, dev)
                call = engine.SolveCall(field.model, flat, coeffs, grid, y0a.detach().to(torch.float32).contiguous(), dW=widen(dW),
                                        dU=widen(dU), method=method, seed=key, noise_table=tab, kl_column=kl)
                return call.launch()[:, :, :Hl + 1].to(y0.dtype)
        except engine._lib.SnsdeError as exc:
            if not exc.no_kernel:      # (no kernel for this shape: the split solve below)
                raise
    # (2) the split solve: latent dynamics fused, the accumulator as one batched quadrature over every state
    dW, dU = increments()
    full = engine.every_step_grid(grid)
    tab_times = engine.noise_table_times(full, method)
    y0p = torch.nn.functional.pad(y0[:, :Hl], (0, P - Hl))
    if needs_grad:
        if engine.backward_mode(field.model, B, 2, full, method, table=True) != 1:
            return fallback()
        flat = field.flat(dev, grad=True)
        # grad=True = no cache key, i.e. no host read-back.  The reference's sigma is a buffer (no gradient); a module whose diffusion
        # is learnable keeps the table in the autograd graph, and _ComposedSolve returns dL/d table like it does for the tutorial fields
        tab = field.noise_table(tab_times, dev, grad=True)
        if not tab.requires_grad:
            tab = tab.detach()
        try:
            Y = _ComposedSolve.apply(field.model, coeffs, full, widen(dW), method, 0, 0, None, y0p, flat, tab, widen(dU))
        except engine._lib.SnsdeError as exc:
            if not exc.no_kernel:      # no kernel / LDS budget: the tensor-op loop on the increments already drawn
                raise
            return fallback()
    else:
        flat, tab = field.inference_inputs(tab_times, dev)
        call = engine.SolveCall(field.model, flat, coeffs, full, y0p.detach().to(torch.float32).contiguous(), dW=widen(dW),
                                dU=widen(dU), method=method, seed=0, noise_table=tab)
        try:
            Y = call.launch()
        except engine._lib.SnsdeError as exc:
            if not exc.no_kernel:
                raise
            return fallback()
    N = grid.N
    lat = Y[:, :, :Hl].to(y0.dtype)                               # (N + 1, B, Hl)
    f_aug, g_aug = _call(sde, names, 'drift', 'f'), _call(sde, names, 'diffusion', 'g')
    t_rows = full.d_t0.to(y0.dtype).reshape(N, 1, 1).expand(N, B, 1).reshape(N * B, 1)
    h_rows = torch.from_numpy(grid.t1 - grid.t0).to(device=dev, dtype=y0.dtype).reshape(N, 1, 1).expand(N, B, 1).reshape(N * B, 1)
    ya = torch.cat([lat[:-1], torch.zeros(N, B, 1, device=dev, dtype=y0.dtype)], dim=-1).reshape(N * B, Hl + 1)
    try:
        if method == 'srk':
            inc = _srk_step(f_aug, g_aug, t_rows, h_rows, ya, dW.reshape(N * B, -1), dU.reshape(N * B, -1))[:, -1]
        else:            # Euler; Milstein's correction g dg/dy vanishes for the constant diffusion (checked by the probe's g)
            inc = f_aug(t_rows, ya)[:, -1] * h_rows[:, 0] + g_aug(t_rows, ya)[:, -1] * dW.reshape(N * B, -1)[:, -1]
    except (RuntimeError, ValueError, TypeError, IndexError):
        return fallback()
    acc = torch.cat([y0[:, Hl].unsqueeze(0), y0[:, Hl].unsqueeze(0) + torch.cumsum(inc.reshape(N, B), dim=0)], dim=0)
    aug = torch.cat([lat, acc.unsqueeze(-1)], dim=-1)             # (N + 1, B, Hl + 1): every state of the augmented solve
    idx = torch.from_numpy(grid.out_step.astype(np.int64)).to(dev)
    w = torch.from_numpy(grid.out_w).to(device=dev, dtype=y0.dtype)
    if bool((grid.out_w[:, 0] == 0).all()):
        outs = aug.index_select(0, idx + 1)
    else:          # outputs inside a step: torchsde's linear interpolation between the step's end states
        outs = w[:, 0].reshape(-1, 1, 1) * aug.index_select(0, idx) + w[:, 1].reshape(-1, 1, 1) * aug.index_select(0, idx + 1)
    return torch.cat([y0.unsqueeze(0).to(aug.dtype), outs], dim=0)


def _sdeint_padded(sde, rec, pad, coeffs, grid, y0, dW, dU, method, opt, needs_grad, step_offset=0):
    """Solve the zero-padded model (engine.padding_plan) on the MFMA kernels and drop the padded state components.  opt: the
    _FusedOptions of _sdeint_hip, which has also checked that a training solve of the padded model has the MFMA adjoint."""
    model, layout, _ = rec
    model_p, layout_p, _, P = pad
    H, dev = model.hidden_channels, y0.device
    flat = engine.padded_flat(sde, layout, layout_p, H, P, dev, needs_grad)
    widen = lambda t: None if t is None else torch.nn.functional.pad(t, (0, P - H)).contiguous()
    if needs_grad:
        ys = _ComposedSolve.apply(model_p, coeffs, grid, widen(dW), method, opt.seed, opt.row_offset, opt.row_out,
                                  torch.nn.functional.pad(y0, (0, P - H)), flat, None, widen(dU), None, opt.engine['global_rows'], step_offset)
    else:
        call = engine.SolveCall(model_p, flat, coeffs, grid, widen(y0.detach().to(torch.float32)), dW=widen(dW), method=method,
                                seed=opt.seed, row_offset=opt.row_offset, dU=widen(dU), row_out=opt.row_out,
                                global_rows=opt.engine['global_rows'], step_offset=step_offset)
        ys = call.launch().to(y0.dtype)
    return ys[..., :H]


class _ComposedSolve(torch.autograd.Function):
    """Differentiable fused solve of a composed (tutorial-style) field: inputs are the composed parameter block and the
    time-only diffusion table, both produced by ordinary torch ops from the module's parameters, so autograd carries the
    gradients this node returns (dL/dy0, dL/d block, dL/d table) on to the module."""

    @staticmethod
    def forward(ctx, model, coeffs, grid, dW, method, seed, row_offset, row_out, y0, flat, tab, dU=None, kl_column=None, global_rows=0,
                step_offset=0):
        y0c = y0.detach().to(torch.float32).contiguous()
        call = engine.SolveCall(model, flat.detach().contiguous(), coeffs, grid, y0c, dW=dW, method=method, seed=seed,
                                row_offset=row_offset, row_out=row_out, dU=dU,
                                noise_table=None if tab is None else tab.detach().contiguous(),
                                save_traj=True, save_dW=True, save_act=True, kl_column=kl_column, global_rows=global_rows,
                                step_offset=step_offset, resume_grad=step_offset != 0)      # (an offset: sdeint's resume_grad opt-in)
        ys = call.launch()
        ctx.call, ctx.y0_dtype, ctx.has_tab = call, y0.dtype, tab is not None
        return ys.to(y0.dtype) if y0.dtype != ys.dtype else ys.detach()

    @staticmethod
    def backward(ctx, grad_ys):
        call = ctx.call
        out = engine.backward_with_gradients(call, grad_ys.to(torch.float32).contiguous(), adj0_only=engine.adj0_suffices(call),
                                             want_table_grad=ctx.has_tab)
        adj, gflat, gtab = out if ctx.has_tab else (out + (None,))
        return (None,) * 8 + (adj[0].to(ctx.y0_dtype), gflat, gtab, None, None, None, None)


class _FusedSolve(torch.autograd.Function):
    """Differentiable fused solve.  forward = the HIP solve in training mode (keeps every state, the increments used
    and, on the MFMA path, the per-pass activations); backward = the HIP adjoint recursion (snsde_solve_backward) for
    dL/dy0 and every adjoint a_n, then the parameter gradients: mode 1 (MFMA path) the native split-R weight-gradient
    pass (snsde_param_gradients), mode 2 (generic adjoint kernels) ONE batched evaluation of the step function over
    all (step, row) pairs whose autograd yields them.  This replaces autograd through the ~25 x N nodes of the
    unrolled loop (benchmark_classification/common_sde.py:158-160)."""

    # forward's leading inputs that take no gradient (sde .. mode); coeffs_src, y0 and the parameters follow in this order
    NO_GRAD_INPUTS = 9

    @staticmethod
    def forward(ctx, sde, rec, coeffs, grid, times_host, increments, method, opt, mode, coeffs_src, y0, *params):
        # opt, mode: the _FusedOptions and engine.backward_mode (1 or 2) that _sdeint_hip resolved - nothing is decided again here
        # coeffs_src: the caller's coefficient tensor when dL/d coeffs is wanted (a differentiable input; the kernels read
        # `coeffs`, its detached float32 copy), else None - such a solve launches and allocates nothing beyond the parameter pass
        model, layout, numel = rec
        dW, dU = increments
        flat = engine.flatten_params(sde, layout, numel, y0.device)
        y0c = y0.detach().to(torch.float32).contiguous()
        eng = opt.engine
        samples = eng['samples'] if eng['sample_grad'] else 1      # (sampled training: _sdeint_samples)
        # recompute mode (_recompute_steps: options={'recompute': steps per chunk} or the environment): keep states and increments only,
        # re-run the forward kernel chunk by chunk inside backward (engine.backward_recompute)
        ctx.recompute = 0
        if mode == 1 and method != 'srk' and samples == 1:      # (a sampled node never recomputes: _sdeint_samples routes around it)
            ctx.recompute = opt.recompute
            if ctx.recompute >= grid.N:      # one chunk = the whole solve: the saved-activation mode with a second forward on top
                ctx.recompute = 0            # (and the parent's states / increments kept beside the chunk's: MORE memory, K5 N = 49)
        # mode 2: the generic adjoint prepares its own weights, so the forward takes whatever kernel is fastest
        save_act = mode == 1 and not ctx.recompute
        # the increments are kept only where the backward cannot get them otherwise: the MFMA Euler / Milstein adjoint reads
        # supplied ones in place and REGENERATES Philox ones (host key) - one (N, B, H) store and load less per step
        nets = model.noise_option in (14, 15, 18, 19)
        keep_dw = not (save_act and method in ('euler', 'milstein') and not (nets and method == 'milstein')
                       and not torch.is_tensor(opt.seed) and opt.param_pass in ('hip', 'split')
                       and os.environ.get('SNSDE_KEEP_INCREMENTS') != '1')
        call = engine.SolveCall(model, flat, coeffs, grid, y0c, dW=dW, seed=opt.seed, row_offset=opt.row_offset, save_traj=True,
                                save_dW=keep_dw, save_act=save_act, row_out=opt.row_out, dU=dU,
                                step_offset=opt.step_offset, resume_grad=opt.step_offset != 0,      # (a continued piece: resume_grad)
                                lean_general=samples > 1 and opt.lean_general,      # (the sampled route's A/B switch)
                                **dict(eng, samples=samples, sample_grad=samples > 1))   # (bf16 reaches here under bf16_grad, mode 1, only)
        ctx.coeffs_dtype = None if coeffs_src is None else coeffs_src.dtype
        if coeffs_src is not None and mode == 1 and call.act_save is not None and call.delta_slots == 0:
            raise _NoCoeffGradient()      # (before the launch: _sdeint_hip applies the fallback rule)
        ctx.mode, ctx.method = mode, method
        ctx.param_pass = opt.param_pass
        ctx.layout = (layout, numel)
        ys = call.launch()
        ctx.call, ctx.sde, ctx.grid, ctx.times_host = call, sde, grid, times_host
        ctx.y0_dtype = y0.dtype
        # a NEW tensor object for the output: returning call.ys itself would give it this node as grad_fn, and the node
        # holds the call: a reference cycle that keeps every saved tensor of the solve alive until the cyclic collector runs
        return ys.to(y0.dtype) if y0.dtype != ys.dtype else ys.detach()

    @staticmethod
    def backward(ctx, grad_ys):
        call, sde, grid = ctx.call, ctx.sde, ctx.grid
        lead = (None,) * _FusedSolve.NO_GRAD_INPUTS
        want_c = ctx.coeffs_dtype is not None and ctx.needs_input_grad[len(lead)]      # dL/d coeffs: only where autograd asks for it
        gcoeffs, grad_ys = None, grad_ys.to(torch.float32).contiguous()
        if ctx.mode == 1 and ctx.recompute:
            g0, flat = engine.backward_recompute(call, grad_ys, ctx.recompute)
            grads = engine.param_index(sde, ctx.layout[0]).grads_from_flat(flat)
            return lead + (None, g0.to(ctx.y0_dtype)) + tuple(grads)
        if ctx.mode == 1:     # MFMA adjoint kernel + native weight-gradient pass on the saved activations / deltas
            if ctx.param_pass == 'torch':     # library-GEMM cross-check of the native pass
                adj, delta = engine.solve_backward(call, grad_ys, save_delta=True, adj0_only=False)
                grads = _parameter_gradients_gemm(sde, call, grid, adj, delta, method=ctx.method, want_coeffs=want_c)
                if want_c:
                    grads, gcoeffs = grads
            else:
                if ctx.param_pass == 'split':     # the two C calls one after the other (what the fused call must reproduce bit for bit)
                    adj, delta = engine.solve_backward(call, grad_ys, save_delta=True, adj0_only=engine.adj0_suffices(call))
                    flat = engine.param_gradients(call, adj, delta)
                elif want_c:
                    adj, flat, delta = engine.backward_with_gradients(call, grad_ys, adj0_only=engine.adj0_suffices(call), return_delta=True)
                else:
                    adj, flat = engine.backward_with_gradients(call, grad_ys, adj0_only=engine.adj0_suffices(call))
                grads = engine.param_index(sde, ctx.layout[0]).grads_from_flat(flat)
                if want_c:      # the native pass over the same delta planes (snsde_coeff_gradients)
                    gcoeffs = engine.coeff_gradients(call, adj, delta)
        else:                 # generic adjoint kernels (any dims; Euler / Milstein / SRK) + batched autograd parameter pass
            adj = engine.solve_backward(call, grad_ys)
            grads = _parameter_gradients(sde, call, grid, adj, method=ctx.method, want_coeffs=want_c)
            if want_c:
                grads, gcoeffs = grads
        if gcoeffs is not None and gcoeffs.dtype != ctx.coeffs_dtype:
            gcoeffs = gcoeffs.to(ctx.coeffs_dtype)
        return lead + (gcoeffs, adj[0].to(ctx.y0_dtype)) + tuple(grads)


def _spline_piece(coeffs, idx, frac):
    """X(t) of n (step, interval) pairs for every row, (n, B, C): coeffs (B, L - 1, 4C) packed (a, b, 2c, 3d), idx (n,) the
    interval of each time and frac (n, 1, 1) its offset into it.  The operation order is the kernels' (cross-checked bit for bit)."""
    Cn = coeffs.shape[-1] // 4
    rows = coeffs[:, idx, :].permute(1, 0, 2)
    a_, b_, c2, d3 = (rows[..., k * Cn:(k + 1) * Cn] for k in range(4))
    return a_ + (b_ + (0.5 * c2 + d3 * frac / 3) * frac) * frac


@torch.no_grad()
def _parameter_gradients_gemm(sde, call, grid, adj, delta, method='euler', want_coeffs=False):
    """Parameter gradients from the tensors the two kernels left in HBM, as plain library GEMMs:
        d layer.weight = sum_{step,row} delta_layer^T . layer_input,   d layer.bias = sum delta_layer
    (delta from the adjoint kernel, layer inputs from the forward's act_save / trajectory), plus the elementwise
    diffusion-side reductions for theta and the time-only noise MLP.  Same result as `_parameter_gradients`
    (kept as the autograd cross-check) at a fraction of the memory traffic."""
    P = dict(sde.named_parameters())
    io, no = sde.input_option, sde.noise_option
    if no not in (0, 12, 13, 16, 17):
        raise NotImplementedError("the library-GEMM cross-check pass covers noise_option 0/12/13/16/17 only; use param_pass='hip'")
    N, B, H = call.dW_out.shape
    dev = adj.device
    NB = N * B
    slots = call.act_save.shape[1]
    nhid = slots - 2
    act = call.act_save          # (N, slots, B, H): z0, hidden.., zout
    grads = {k: None for k in P}
    t0 = torch.from_numpy(grid.step_tab[:, 0].copy()).to(dev)
    hh = torch.from_numpy(grid.step_tab[:, 1].copy()).to(dev)
    Y = call.traj[:-1]
    # ---- drift side -----------------------------------------------------------------------------------
    def wgrad(d3, x3):
        # sum_{n,b} d[n,b,:]^T x[n,b,:] as a batched GEMM over the steps (K = B per batch entry) + a small sum:
        # ~5x faster than one (H x N*B)(N*B x K) GEMM, whose reduction dimension is 1e5 long
        return torch.bmm(d3.transpose(1, 2), x3).sum(0)

    d_out = delta[:, 0]
    grads['linear_out.weight'] = wgrad(d_out, act[:, nhid])
    grads['linear_out.bias'] = d_out.sum((0, 1))
    for l in range(nhid):
        d_l = delta[:, nhid - l]
        grads[f'linears.{l}.weight'] = wgrad(d_l, act[:, l])
        grads[f'linears.{l}.bias'] = d_l.sum((0, 1))
    d0 = delta[:, nhid + 1]                           # (N, B, H) w.r.t. the pre-activation of z0
    if io in (3, 4, 5, 6):
        tau = torch.stack([t0.sin(), t0.cos()], dim=-1).unsqueeze(1).expand(N, B, 2)
        yin = torch.cat([tau, Y], dim=-1)
    else:
        yin = Y
    idx = torch.from_numpy(grid.step_tab[:, 5].copy().view('int32').astype('int64')).to(dev)      # each step's spline interval
    frac = torch.from_numpy(grid.step_tab[:, 4].copy()).to(dev).view(N, 1, 1)                      # ... and its offset into it
    if io in (2, 4, 6):
        Xraw = _spline_piece(call.keep[1], idx, frac)                                   # (N, B, C)
        yy = torch.baddbmm(P['linear_in.bias'], yin, P['linear_in.weight'].t().expand(N, -1, -1))
        Xt = torch.baddbmm(P['initial_network.bias'], Xraw, P['initial_network.weight'].t().expand(N, -1, -1))
        grads['emb.weight'] = torch.cat([wgrad(d0, yy), wgrad(d0, Xt)], dim=1)
        grads['emb.bias'] = d0.sum((0, 1))
        dcat = torch.matmul(d0, P['emb.weight'])
        d_in, d_x = dcat[..., :H], dcat[..., H:]
        grads['initial_network.weight'] = wgrad(d_x, Xraw)
        grads['initial_network.bias'] = d_x.sum((0, 1))
    else:
        d_in = d0
    grads['linear_in.weight'] = wgrad(d_in, yin)
    grads['linear_in.bias'] = d_in.sum((0, 1))
    # ---- diffusion side: g = tanh(sigmoid(theta) * nan_to_num(raw)), raw = s_n (no 12,16) or s_n * y (13,17) ----
    if no in (12, 13, 16, 17):
        sig = P['theta'].sigmoid()
        with torch.enable_grad():
            tn = torch.cat([t0.sin().unsqueeze(-1), t0.cos().unsqueeze(-1)], dim=-1)      # (N, 2)
            net = sde.noise_t
            s_n = net(tn)
            if no >= 16:
                s_n = s_n.relu()
        sd = s_n.detach().unsqueeze(1)                                                  # (N, 1, H)
        raw = sd * Y if no in (13, 17) else sd.expand(N, B, H)
        finite = torch.isfinite(raw)
        rc = torch.nan_to_num(raw)
        g = (sig * rc).tanh()
        du = adj[1:] * call.dW_out * (1 - g * g)
        dtheta = (du * rc).sum()
        ds = du * sig * finite
        ds = (ds * Y).sum(1) if no in (13, 17) else ds.sum(1)                           # (N, H)
        if method == 'milstein' and no in (13, 17):
            # + a . d/dc [1/2 (dW^2 - h) g g'],  g' = (1 - g^2) c,  c = sigmoid(theta) s_n   (zero for y-independent g)
            c = sig * sd
            q = call.dW_out * call.dW_out - hh.view(N, 1, 1)
            ex = adj[1:] * (1 - g * g) * (0.5 * q) * ((1 - 3 * g * g) * c * Y + g) * finite
            dtheta = dtheta + (ex * sd).sum()
            ds = ds + (ex * sig).sum(1)
        grads['theta'] = (dtheta * sig * (1 - sig)).reshape(1, 1)
        net_params = [p for p in net.parameters()]
        gs = torch.autograd.grad(s_n, net_params, grad_outputs=ds)
        for (name, _), gval in zip(net.named_parameters(), gs):
            grads['noise_t.' + name] = gval
    else:   # no == 0: theta receives no gradient (g == 0)
        grads['theta'] = torch.zeros_like(P['theta'])
    out = [grads[k] if grads[k] is not None else torch.zeros_like(P[k]) for k in P]
    if not want_coeffs:
        return out
    # dL/d coeffs from the same delta plane (the cross-check of snsde_coeff_gradients): v = dL/dX(t_n) through initial_network,
    # spread over the four coefficient blocks of step n's interval with the weights (1, r, r^2 / 2, r^3 / 3)
    coeffs = call.keep[1]
    gc = torch.zeros_like(coeffs)
    if io in (0, 2, 4, 6):
        Cn = coeffs.shape[-1] // 4
        v = torch.matmul(d_x if io != 0 else d0, P['initial_network.weight'])                 # (N, B, C)
        r = frac.view(N)
        phi = torch.stack([torch.ones_like(r), r, 0.5 * r * r, r * r * r / 3], dim=-1)          # (N, 4)
        contrib = (phi.view(N, 1, 4, 1) * v.unsqueeze(2)).reshape(N, B, 4 * Cn)
        gc.index_add_(1, idx, contrib.permute(1, 0, 2).contiguous())
    return out, gc


def _parameter_gradients(sde, call, grid, adj, max_rows=1 << 19, method='euler', want_coeffs=False):
    """sum over steps n and rows of  a_{n+1} . d(f(t_n, y_n) h_n + g(t_n, y_n) dW_n)/d theta  with y_n, a_{n+1}, dW_n
    constants: one batched forward of the vector field over (step, row) pairs + autograd (library GEMMs)."""
    from . import modules
    params = list(sde.parameters())
    P = dict(sde.named_parameters())
    io, no = sde.input_option, sde.noise_option
    N, B, H = call.dW_out.shape
    dev = adj.device
    t0 = torch.from_numpy(grid.step_tab[:, 0].copy()).to(dev)
    hh = torch.from_numpy(grid.step_tab[:, 1].copy()).to(dev)
    idx = torch.from_numpy(grid.step_tab[:, 5].copy().view('int32').astype('int64')).to(dev)
    frac = torch.from_numpy(grid.step_tab[:, 4].copy()).to(dev)
    coeffs = call.keep[1]
    Cn = coeffs.shape[-1] // 4
    uses_x = io in (0, 2, 4, 6)
    total = [torch.zeros_like(p) for p in params]
    if want_coeffs:      # the coefficients as one more leaf of the batched evaluation: dL/d coeffs comes out of the same autograd pass
        coeffs = coeffs.detach().requires_grad_(True)
        params = params + [coeffs]
        total.append(torch.zeros_like(coeffs))
    steps_per_chunk = max(1, max_rows // B)
    with torch.enable_grad():
        for lo in range(0, N, steps_per_chunk):
            hi = min(N, lo + steps_per_chunk)
            n = hi - lo
            Y = call.traj[lo:hi].reshape(n * B, H)
            A = adj[lo + 1:hi + 1].reshape(n * B, H)
            DW = call.dW_out[lo:hi].reshape(n * B, H)
            col = t0[lo:hi].repeat_interleave(B).unsqueeze(-1)
            hcol = hh[lo:hi].repeat_interleave(B).unsqueeze(-1)
            tau = torch.cat([col.sin(), col.cos()], dim=-1)
            Xraw = None
            if uses_x:
                Xraw = _spline_piece(coeffs, idx[lo:hi], frac[lo:hi].view(n, 1, 1)).reshape(n * B, Cn)
            f = None if method == 'srk' else modules.drift_rows(P, io, tau, Y, Xraw)
            if method == 'srk':
                surrogate = (A * _srk_rows(P, io, no, grid, lo, hi, B, Y, DW, call.dU_out[lo:hi].reshape(n * B, H), coeffs,
                                           hcol)).sum()
            elif method == 'milstein' and no in (14, 15, 18, 19):
                # diffusion net: torchsde's Milstein term is the VJP of g with cotangent g (dW^2 - h) (dense dg/dy)
                Yg = Y.detach().requires_grad_(True)
                g = modules.diffusion_rows(P, no, col, tau, Yg)
                gdg, = torch.autograd.grad(g, Yg, grad_outputs=g * (DW * DW - hcol), create_graph=True)
                surrogate = (A * (f * hcol + g * DW + 0.5 * gdg)).sum()
            elif method == 'milstein':   # + 1/2 g dg/dy (dW^2 - h); g is elementwise in y for the other options
                Yg = Y.detach().requires_grad_(True)
                g = modules.diffusion_rows(P, no, col, tau, Yg)
                if g.requires_grad and g.grad_fn is not None:
                    dg, = torch.autograd.grad(g.sum(), Yg, create_graph=True, allow_unused=True)
                else:
                    dg = None
                dg = torch.zeros_like(Yg) if dg is None else dg       # diffusion independent of y: no Milstein term
                surrogate = (A * (f * hcol + g * DW + 0.5 * g * dg * (DW * DW - hcol))).sum()
            else:
                g = modules.diffusion_rows(P, no, col, tau, Y)
                surrogate = (A * (f * hcol + g * DW)).sum()
            gs = torch.autograd.grad(surrogate, params, allow_unused=True)
            for acc, gpart in zip(total, gs):
                if gpart is not None:
                    acc.add_(gpart)
    if want_coeffs:
        return total[:-1], total[-1]
    return total


def _srk_rows(P, io, no, grid, lo, hi, B, Y, I_k, I_k0, coeffs, hcol):
    """One SRID2 step of every (step, row) pair of steps lo..hi-1 as a differentiable function of the parameters
    (states, increments constant): the stage times / spline intervals come from the solver's stage table."""
    from . import modules
    tab = engine.srk_table(grid)[lo:hi]   # (n, 4, stride): t, sin t, cos t, frac, interval index
    n = hi - lo
    Cn = coeffs.shape[-1] // 4
    uses_x = io in (0, 2, 4, 6)

    def at(slot):
        t = tab[:, slot, 0].to(Y.dtype).repeat_interleave(B).unsqueeze(-1)
        tau = torch.stack([tab[:, slot, 1], tab[:, slot, 2]], dim=-1).to(Y.dtype).repeat_interleave(B, dim=0)
        Xraw = None
        if uses_x:
            idx = tab[:, slot, 4].contiguous().view(torch.int32).to(torch.int64)
            Xraw = _spline_piece(coeffs, idx, tab[:, slot, 3].to(Y.dtype).view(n, 1, 1)).reshape(n * B, Cn)
        return t, tau, Xraw

    slots_f = (0, 3, 2, 0)      # C0 = 0, 1, 1/2, 0  -> stage-table slots (0, 1/4, 1/2, 1)
    slots_g = (0, 1, 3, 1)      # C1 = 0, 1/4, 1, 1/4

    def f(stage, y):
        t, tau, Xraw = at(slots_f[stage])
        return modules.drift_rows(P, io, tau, y, Xraw)

    def g(stage, y):
        t, tau, _ = at(slots_g[stage])
        return modules.diffusion_rows(P, no, t, tau, y)

    T = _SRK
    h = hcol
    rdt = h.sqrt()
    I_kk = (I_k * I_k - h) / 2
    I_kkk = (I_k ** 3 - 3 * h * I_k) / 6
    fs, gs = [], []
    y1 = Y
    for s in range(4):
        H0, H1 = Y, Y
        for j in range(s):
            H0 = H0 + T['A0'][s][j] * fs[j] * h + T['B0'][s][j] * gs[j] * I_k0 / h
            H1 = H1 + T['A1'][s][j] * fs[j] * h + T['B1'][s][j] * gs[j] * rdt
        fs.append(f(s, H0) if T['alpha'][s] != 0.0 or any(T['A0'][k][s] != 0.0 or T['A1'][k][s] != 0.0 for k in range(s + 1, 4))
                  else torch.zeros_like(Y))
        gs.append(g(s, H1))
        gw = T['beta1'][s] * I_k + T['beta2'][s] * I_kk / rdt + T['beta3'][s] * I_k0 / h + T['beta4'][s] * I_kkk / h
        y1 = y1 + T['alpha'][s] * fs[s] * h + gw * gs[s]
    return y1


def _call(sde, names, key, default):
    return getattr(sde, (names or {}).get(key, default))


# Roessler's SRI2W1 (SIAM J. Numer. Anal. 48(3), 2010) = torchsde 0.2.5 `tableaus/srid2.py`, the scheme behind method='srk' for
# diagonal noise; the same numbers as csrc/snsde_internal.h (SRK_B1_*, srk_w*) and, independently transcribed, oracle/sde_oracle.py
_SRK = dict(C0=(0.0, 1.0, 0.5, 0.0), C1=(0.0, 0.25, 1.0, 0.25),
            A0=((), (1.0,), (0.25, 0.25), (0.0, 0.0, 0.0)), A1=((), (0.25,), (1.0, 0.0), (0.0, 0.0, 0.25)),
            B0=((), (0.0,), (1.0, 0.5), (0.0, 0.0, 0.0)), B1=((), (-0.5,), (1.0, 0.0), (2.0, -1.0, 0.5)),
            alpha=(1 / 6, 1 / 6, 2 / 3, 0.0), beta1=(-1.0, 4 / 3, 2 / 3, 0.0), beta2=(1.0, -4 / 3, 1 / 3, 0.0),
            beta3=(2.0, -4 / 3, -2 / 3, 0.0), beta4=(-2.0, 5 / 3, -2 / 3, 1.0))


def _srk_step(f, g, t0, h, y, I_k, I_k0):
    """One SRID2 step.  Terms whose tableau coefficient is zero are not formed (x + 0 * z = x exactly for finite z: same values,
    a third of the tensor ops), nor is the drift of the last stage, which no later term reads (alpha[3] = 0)."""
    T = _SRK
    rdt = h.sqrt()
    I_kk = (I_k * I_k - h) / 2
    I_kkk = (I_k ** 3 - 3 * h * I_k) / 6
    fs, gs = [], []
    y1 = y
    for s in range(4):
        H0, H1 = y, y
        for j in range(s):
            if T['A0'][s][j] != 0.0:
                H0 = H0 + T['A0'][s][j] * fs[j] * h
            if T['B0'][s][j] != 0.0:
                H0 = H0 + T['B0'][s][j] * gs[j] * I_k0 / h
            if T['A1'][s][j] != 0.0:
                H1 = H1 + T['A1'][s][j] * fs[j] * h
            if T['B1'][s][j] != 0.0:
                H1 = H1 + T['B1'][s][j] * gs[j] * rdt
        need_f = T['alpha'][s] != 0.0 or any(T['A0'][r][s] != 0.0 or T['A1'][r][s] != 0.0 for r in range(s + 1, 4))
        fs.append(f(t0 + T['C0'][s] * h, H0) if need_f else None)
        gs.append(g(t0 + T['C1'][s] * h, H1))
        gw = None
        for coef, term in ((T['beta1'][s], lambda c: c * I_k), (T['beta2'][s], lambda c: c * I_kk / rdt),
                           (T['beta3'][s], lambda c: c * I_k0 / h), (T['beta4'][s], lambda c: c * I_kkk / h)):
            if coef != 0.0:        # (same expression forms as the unskipped sum: bit-identical values)
                gw = term(coef) if gw is None else gw + term(coef)
        if T['alpha'][s] != 0.0:
            y1 = y1 + T['alpha'][s] * fs[s] * h
        if gw is not None:
            y1 = y1 + gw * gs[s]
    return y1


def _sdeint_torch(sde, y0, ts, bm, method, dt, options, names):
    """Unfused scheme on tensor ops (arbitrary sde, CPU plumbing, autograd)."""
    _continued_without_path(options, bm, 'the tensor-op loop')
    f = _call(sde, names, 'drift', 'f')
    g = _call(sde, names, 'diffusion', 'g')
    noise_type = getattr(sde, 'noise_type', 'diagonal')
    if noise_type == 'scalar':
        # torchsde's scalar noise: g is (B, H, 1), one Brownian motion per row, g_prod = g[..., 0] * I with I (B, 1)
        # (the tutorial's Neural ODE notebook solves an ODE this way, g = 0).  Euler only: the higher-order schemes need
        # the dense Jacobian-vector product of g there.
        if method != 'euler':
            raise NotImplementedError("scalar noise: only method='euler' is implemented")
        g_scalar = g
        g = lambda t, y: g_scalar(t, y).squeeze(-1)
    elif noise_type != 'diagonal':
        raise NotImplementedError("only diagonal (and, under Euler, scalar) noise is implemented")
    if getattr(sde, 'sde_type', 'ito') != 'ito':
        raise NotImplementedError("only Ito SDEs are implemented")
    ts_host = _HostTimes.get(ts)
    grid = engine.StepGrid(ts_host, dt, np.array([0.0, 1.0], dtype=np.float32), None)
    t0s = torch.from_numpy(grid.t0).to(y0.device)
    w = torch.from_numpy(grid.out_w).to(device=y0.device, dtype=y0.dtype)
    hs = (torch.from_numpy(grid.t1).to(y0.device) - t0s).to(y0.dtype)
    dW_all, dU_all = _draw_increments(bm, grid, y0, method, seed=options.get('seed'), scalar=noise_type == 'scalar')
    needs_grad = _differentiated(sde, y0)
    if (y0.is_cuda and not needs_grad and method in ('euler', 'srk') and options.get('graph', True)
            and not torch.cuda.is_current_stream_capturing()):
        ys = _graphed_steps(f, g, y0, grid, t0s, hs, w, dW_all, dU_all, method)
        if ys is not None:
            return _select_rows(ys, options)
    y = y0
    ys = [y0]
    k = 0
    for n in range(grid.N):
        t0, h = t0s[n], hs[n]
        prev = y
        I = dW_all[n]
        if method == 'srk':
            y = _srk_step(f, g, t0, h, y, I, dU_all[n])
        elif method == 'euler':
            y = y + f(t0, y) * h + g(t0, y) * I
        else:
            v = I * I - h
            # g * dg/dy * v for diagonal noise; when differentiating, the cotangent keeps its dependence on y so that
            # autograd through this loop is the exact gradient of the discrete scheme (what the fused adjoint computes)
            # (the state, not y0 alone: it also carries a graph from a tensor that f / g close over without declaring a parameter)
            diff = needs_grad or (torch.is_grad_enabled() and y.requires_grad)
            with torch.enable_grad():
                yy = y if y.requires_grad else y.detach().requires_grad_(True)
                gv = g(t0, yy)
                if gv.requires_grad:
                    gdg, = torch.autograd.grad(gv, yy, grad_outputs=(gv if diff else gv.detach()) * v, allow_unused=True,
                                               create_graph=diff)
                else:            # a diffusion that depends on neither the state nor a parameter (a constant buffer): no correction
                    gdg = None
            gv = gv if diff else gv.detach()
            gdg = torch.zeros_like(y) if gdg is None else gdg
            y = y + f(t0, y) * h + gv * I + 0.5 * gdg
        while k < grid.T - 1 and grid.out_step[k] == n:
            ys.append(y if grid.out_w[k, 0] == 0 else w[k, 0] * prev + w[k, 1] * y)
            k += 1
    return _select_rows(torch.stack(ys, dim=0), options)


def _select_rows(ys, options):
    row_out = (options or {}).get('row_out')
    if row_out is not None:     # same contract as the fused path: each row's own output state, (B, H)
        idx = row_out.to(device=ys.device, dtype=torch.int64).reshape(1, -1, 1).expand(1, ys.shape[1], ys.shape[2])
        ys = ys.gather(0, idx).squeeze(0)
    return ys


def _graphed_steps(f, g, y0, grid, t0s, hs, w, dW_all, dU_all, method):
    """Generic-`sde` stepper for CUDA tensors without gradients: ONE solver step of the user's f / g —
    time, step size and increments picked from device arrays by an in-graph step counter, state updated in place — is
    recorded into a hipGraph inside this call and replayed N times, so a step costs one graph launch instead of the
    ~25-100 kernel launches of the tensor-op loop.  The graph lives only for this call (every tensor the user's module
    touches is alive and fixed meanwhile).  Returns None — the caller then runs the eager loop — when the step cannot be
    recorded (a device->host sync or data-dependent control flow inside f / g)."""
    dev = y0.device
    y_buf = y0.detach().clone()
    prev_buf = y_buf.clone()
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

    def step():
        t = t0s.index_select(0, cnt).squeeze(0)
        h = hs.index_select(0, cnt).squeeze(0)
        I = dW_all.index_select(0, cnt).squeeze(0)
        prev_buf.copy_(y_buf)
        if method == 'euler':
            y_new = y_buf + f(t, y_buf) * h + g(t, y_buf) * I
        else:
            y_new = _srk_step(f, g, t, h, y_buf, I, dU_all.index_select(0, cnt).squeeze(0))
        y_buf.copy_(y_new)
        cnt.add_(1)

    prev_mode = torch.cuda.get_sync_debug_mode()
    try:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            torch.cuda.set_sync_debug_mode('error')        # a sync inside f / g means the step cannot be recorded
            step()                                          # torch's capture recipe: one eager run on a side stream
            torch.cuda.set_sync_debug_mode(prev_mode)
        torch.cuda.current_stream(dev).wait_stream(side)
        y_buf.copy_(y0); cnt.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            step()
    except Exception as exc:
        torch.cuda.set_sync_debug_mode(prev_mode)
        torch.cuda.synchronize(dev)
        if os.environ.get('SNSDE_DEBUG_GRAPH') == '1':
            warnings.warn(f'generic-sde step not recorded: {type(exc).__name__}: {exc}')
        return None
    ys = torch.empty((grid.T,) + tuple(y0.shape), dtype=y0.dtype, device=dev)
    ys[0].copy_(y0)
    k = 0
    with torch.no_grad():
        for n in range(grid.N):
            graph.replay()
            while k < grid.T - 1 and grid.out_step[k] == n:
                if grid.out_w[k, 0] == 0:
                    ys[k + 1].copy_(y_buf)
                else:
                    ys[k + 1].copy_(w[k, 0] * prev_buf + w[k, 1] * y_buf)
                k += 1
    return ys
