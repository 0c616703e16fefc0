"""nn.Module API of the reference's SDE models with identical constructor signatures, attribute names
and state_dict keys/shapes, so checkpoints and the ``common_sde.py`` training loop carry over:

  Diffusion_model          models_sde/neuralsde.py:123-307 (three numerically identical copies in the
                           reference: benchmark_classification, benchmark_forecasting, torch_ists)
  NeuralSDE                benchmark_classification/models_sde/neuralsde.py:51-120
  NeuralSDE_forecasting    benchmark_forecasting/models_sde/neuralsde.py:123-186
  IstsNeuralSDE            torch-ists/torch_ists/diff_module/NSDE/nsde_model.py:46-84

``NeuralSDE*.forward`` reach the integrator through ``torchsde.sdeint`` exactly like the reference;
with this package's ``torchsde`` that is the fused HIP solve for CUDA tensors.  ``Diffusion_model.f/g``
exist for the generic tensor-op loop (CPU plumbing, autograd) and for probing; on CUDA float32
tensors under no_grad they run through the HIP vector-field kernel.
"""
import torch
from torch import nn

from . import engine
from . import torchcde as _torchcde
from . import torchsde as _torchsde
from .controldiffeq import _HostTimes

PROPOSAL_METHOD_CONTRACT = {"lsde": (2, 16), "lnsde": (4, 17), "gsde": (6, 17)}

_TIME_IN = (3, 4, 5, 6)      # linear_in sees [sin t, cos t, y]
_CONTROL_EMB = (2, 4, 6)     # emb(cat[yy, Xt])
_GEOMETRIC = (5, 6)          # z * tanh(y)


def prepare_sde_solver_kwargs(times, kwargs, *, default_method, respect_euler_grid):
    """dt = max(min gap of `times`, 1e-3); default method; options['dt'] (neuralsde.py:30-48)."""
    kwargs = dict(kwargs)
    host = _HostTimes.get(times)
    dt = max(float((host[1:] - host[:-1]).min()), 1e-3)
    kwargs.setdefault('method', default_method)
    if kwargs['method'] in ('srk', 'euler'):
        options = kwargs.setdefault('options', {})
        grid_given = 'step_size' in options or 'grid_constructor' in options
        if 'dt' not in options and (kwargs['method'] == 'srk' or not respect_euler_grid or not grid_given):
            options['dt'] = dt
    return kwargs, dt


_prepare_sde_solver_kwargs = prepare_sde_solver_kwargs


def _lin(P, name, x):
    return torch.nn.functional.linear(x, P[name + '.weight'], P[name + '.bias'])


def drift_rows(P, io, tau, y, Xraw):
    """Drift f of Diffusion_model for rows with their own time features `tau` (rows, 2) and control value
    `Xraw` (rows, C): the reference's f (neuralsde.py:295-302) written over a name->tensor dict so it serves the
    module, foreign modules honouring the same parameter names, and the batched parameter-gradient pass."""
    Xt = _lin(P, 'initial_network', Xraw) if io in (0,) + _CONTROL_EMB else None
    if io == 0:
        z = Xt
    else:
        z = _lin(P, 'linear_in', torch.cat([tau, y], dim=-1) if io in _TIME_IN else y)
        if io in _CONTROL_EMB:
            z = _lin(P, 'emb', torch.cat([z, Xt], dim=-1))
    z = z.relu()
    i = 0
    while f'linears.{i}.weight' in P:
        z = _lin(P, f'linears.{i}', z).relu()
        i += 1
    z = _lin(P, 'linear_out', z)
    if io in _GEOMETRIC:
        z = z * y.tanh()
    return z.tanh()


def raw_diffusion_rows(P, no, col, tau, y):
    """Un-clipped diffusion (neuralsde.py:233-288) for rows with time column `col` (rows,1) / features `tau`."""
    if no == 0:
        return torch.zeros_like(y)
    if no <= 6:
        scale = (P['sigma'] if no <= 3 else P['sigma_diag']).exp().expand_as(y)
        kind = (no - 1) % 3
        return scale if kind == 0 else (scale * col if kind == 1 else scale * y)
    if no == 7:
        return y.sqrt()
    if no == 8:
        return y ** 3
    if no == 9:
        return y.sigmoid()
    if no == 10:
        return y.relu()
    if no == 11:
        return col * y
    time_only = no in (12, 13, 16, 17)
    x = tau if time_only else torch.cat([tau, y], dim=-1)
    name = 'noise_t' if time_only else 'noise_y'
    if name + '.0.weight' in P:
        out = _lin(P, name + '.2', _lin(P, name + '.0', x).relu())
    else:
        out = _lin(P, name, x)
    if no >= 16:
        out = out.relu()
    return out * y if no % 2 == 1 else out


def diffusion_rows(P, no, col, tau, y):
    return (P['theta'].sigmoid() * torch.nan_to_num(raw_diffusion_rows(P, no, col, tau, y))).tanh()


class Diffusion_model(nn.Module):
    def __init__(self, input_channels, hidden_channels, hidden_hidden_channels, num_hidden_layers, theta=1.0,
                 sigma=1.0, input_option=0, noise_option=0):
        super().__init__()
        if input_option not in range(7):
            raise ValueError(f"Unknown input_option {input_option}.")
        if noise_option not in range(20):
            raise ValueError(f"Unknown noise_option {noise_option}.")
        self.sde_type = "ito"
        self.noise_type = "diagonal"
        self.input_option = input_option
        self.noise_option = noise_option
        self.input_channels = input_channels
        self.hidden_channels = hidden_channels
        H, HH = hidden_channels, hidden_hidden_channels
        # creation order = the reference's, so a given torch.manual_seed yields the same initialisation
        self.initial_network = nn.Linear(input_channels, H)
        self.linear_in = nn.Linear(H + 2 if input_option in _TIME_IN else H, HH)
        if input_option in _CONTROL_EMB:
            self.emb = nn.Linear(2 * H, H)
        self.linears = nn.ModuleList(nn.Linear(HH, HH) for _ in range(num_hidden_layers - 1))
        self.linear_out = nn.Linear(HH, H)
        self.theta = nn.Parameter(torch.tensor([[theta]]))
        if noise_option in (1, 2, 3):
            self.sigma = nn.Parameter(torch.tensor([sigma]))
        if noise_option in (4, 5, 6):
            self.sigma_diag = nn.Parameter(torch.tensor([sigma] * H))
        if noise_option in (12, 13):
            self.noise_t = nn.Linear(2, H)
        if noise_option in (14, 15):
            self.noise_y = nn.Linear(H + 2, H)
        if noise_option in (16, 17):
            self.noise_t = nn.Sequential(nn.Linear(2, H), nn.ReLU(), nn.Linear(H, H))
        if noise_option in (18, 19):
            self.noise_y = nn.Sequential(nn.Linear(H + 2, H), nn.ReLU(), nn.Linear(H, H))

    # -- control path ------------------------------------------------------------------------------
    def set_X(self, coeffs, times):
        self.coeffs = coeffs
        self.times = times
        self.X = _torchcde.CubicSpline(self.coeffs, self.times)

    # -- vector field --------------------------------------------------------------------------------
    def _fused_ok(self, t, y):
        """The HIP vector-field probe serves CUDA float32 states under no_grad, one scalar time for all rows, and a module
        the engine recognises (NL - 1 <= 8 hidden `linears`); everything else takes the tensor-op formulas below."""
        return (y.is_cuda and y.dtype == torch.float32 and not torch.is_grad_enabled()
                and hasattr(self, 'coeffs') and self.coeffs.is_cuda
                and (not torch.is_tensor(t) or t.numel() == 1) and engine.recognise(self) is not None)

    def _fused_fg(self, t, y, which):
        # f and g of one (t, y) come out of the same launch: a solver step that asks for both evaluates once.  Each half is
        # handed out once per launch - asking for the same half again re-evaluates, so a caller that edits parameters
        # through `.data` (no version bump) between two f(t, y) calls, finite differences say, never sees the old value.
        # The entry keeps `y` itself: the other half is handed out only to a call with the SAME tensor object at the same
        # version (an address-keyed entry could be hit by a new temporary that the caching allocator placed at a freed
        # temporary's address: f(t, y + d) followed by g(t, y - d)), and holding the reference keeps that address taken.
        key = (float(t), y._version, tuple(y.shape), self.coeffs.data_ptr(), self.coeffs._version,
               tuple(p._version for p in self.parameters()))
        hit = getattr(self, '_fg_cache', None)
        if hit is not None and hit[3] is y and hit[0] == key and which not in hit[2]:
            hit[2].add(which)
            out = hit[1]
            if len(hit[2]) == 2:
                object.__setattr__(self, '_fg_cache', None)     # both halves handed out: drop the references
            return out
        model, layout, numel = engine.recognise(self)
        flat = engine.flatten_params(self, layout, numel, y.device)
        coeffs = self.coeffs.detach().to(torch.float32).contiguous()
        out = engine.eval_fg(model, flat, coeffs, _HostTimes.get(self.times), float(t), y.contiguous())
        object.__setattr__(self, '_fg_cache', (key, out, {which}, y))
        return out

    @staticmethod
    def _tau(t, y):
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        col = t.expand(y.shape[0], 1) if t.dim() == 0 else t.reshape(y.shape[0], 1)
        return col, torch.cat([col.sin(), col.cos()], dim=-1)

    def _drift(self, t, y):
        io = self.input_option
        Xraw = self.X.evaluate(t) if io in (0,) + _CONTROL_EMB else None
        return drift_rows(dict(self.named_parameters()), io, self._tau(t, y)[1], y, Xraw)

    def _raw_diffusion(self, t, y):
        col, tau = self._tau(t, y)
        return raw_diffusion_rows(dict(self.named_parameters()), self.noise_option, col, tau, y)

    def f(self, t, y):
        if self._fused_ok(t, y):
            return self._fused_fg(t, y, 0)[0]
        return self._drift(t, y)

    def g(self, t, y):
        if self._fused_ok(t, y):
            return self._fused_fg(t, y, 1)[1]
        return (self.theta.sigmoid() * torch.nan_to_num(self._raw_diffusion(t, y))).tanh()


class _SDEHead(nn.Module):
    default_method = 'euler'
    respect_euler_grid = False

    def _prepare_initial_state(self, times, z0):
        if z0 is None:
            assert self.initial, "Was not expecting to be given no value of z0."
            return self.initial_network(self.func.X.evaluate(times[0]))
        assert not self.initial, "Was expecting to be given a value of z0."
        return z0

    def _initial_state(self, times, z0, kwargs):
        """(z0, kwargs).  Inference on the fused path: z0 is an uninitialised placeholder and options['z0_linear'] hands the
        solve `initial_network`, which evaluates initial_network(X(times[0])) inside its prepare launch (no spline-evaluate
        and addmm launches of its own); everything else: `_prepare_initial_state` (neuralsde.py:63-69).  Under grad - training
        through sample paths included (options={'samples': S, 'sample_grad': True}) - z0 is materialised here with tensor ops, one
        row per INPUT row; sdeint expands it to one row per path, so autograd sums its gradient over the paths.  Training through
        bf16 operands (options={'precision': 'bf16', 'bf16_grad': True}) likewise: the options pass through to sdeint untouched and
        z0 = initial_network(X(t0)) is an fp32 tensor op outside the solve, as in fp32 training."""
        func = self.func
        if (z0 is None and self.initial and not torch.is_grad_enabled() and getattr(func, 'coeffs', None) is not None
                and func.coeffs.is_cuda and self.initial_network.weight.is_cuda
                and self.initial_network.weight.dtype == torch.float32 and engine.recognise(func) is not None):
            kwargs = dict(kwargs)
            kwargs['options'] = dict(kwargs.get('options') or {}, z0_linear=self.initial_network)
            z0 = torch.empty(func.coeffs.shape[0], self.initial_network.out_features, device=func.coeffs.device,
                             dtype=torch.float32)
            return z0, kwargs
        return self._prepare_initial_state(times, z0), kwargs

    def _readout(self, z):
        """self.linear(z); one fused launch (snsde_readout_head) for inference on CUDA float32 when the head has the
        wrappers' structure and is in evaluation mode."""
        if z.is_cuda and z.dtype == torch.float32 and not torch.is_grad_enabled():
            layers = engine.head_layers(self.linear)
            if layers is not None and layers[1].weight.is_cuda and layers[1].weight.dtype == torch.float32:
                return engine.readout_head(z, layers)
        return self.linear(z)

    def _solve_sde_path(self, times, ts, z0, kwargs):
        kwargs, dt = prepare_sde_solver_kwargs(times, kwargs, default_method=self.default_method,
                                               respect_euler_grid=self.respect_euler_grid)
        return _torchsde.sdeint(sde=self.func, y0=z0, ts=ts, dt=dt, **kwargs)


class NeuralSDE(_SDEHead):
    """Classification head: solve to each row's own final time, read out with an MLP."""

    def __init__(self, func, input_channels, hidden_channels, output_channels, initial=True):
        super().__init__()
        self.func = func
        self.initial = initial
        self.initial_network = nn.Linear(input_channels, hidden_channels)
        self.linear = nn.Sequential(nn.Linear(hidden_channels, hidden_channels), nn.BatchNorm1d(hidden_channels),
                                    nn.ReLU(), nn.Dropout(0.1), nn.Linear(hidden_channels, output_channels))

    @staticmethod
    def output_times(times, final_index):
        """ts = [times[0]] + times[unique(final_index) minus {0, L-1}] + [times[-1]] and the per-row index
        into it (neuralsde.py:91-103)."""
        uniq, inverse = final_index.unique(sorted=True, return_inverse=True)
        has_first = bool(uniq[0] == 0)
        if has_first:
            uniq = uniq[1:]
        row_slot = inverse if has_first else inverse + 1
        if uniq.numel() > 0 and bool(uniq[-1] == len(times) - 1):
            uniq = uniq[:-1]
        ts = torch.cat([times[:1], times[uniq], times[-1:]])
        return ts, row_slot

    def forward(self, times, coeffs, final_index, z0=None, stream=False, **kwargs):
        self.func.set_X(*coeffs, times)
        z0, kwargs = self._initial_state(times, z0, kwargs)
        if stream:
            return self.linear(self._solve_sde_path(times, times, z0, kwargs).movedim(0, -2))
        if z0.is_cuda and engine.recognise(self.func) is not None:
            # Fused solve: output grid = every knot, and each row's own state is selected INSIDE the solve
            # (options['row_out']; ys comes back as (B, H)).  The step grid depends only on ts[0], dt and ts[-1], and
            # each output is the interpolation of the two solver states around it, so the selected states are
            # bit-identical to solving on the reference's `unique(final_index)` grid and gathering
            # (neuralsde.py:91-116) — without its two device->host syncs and without the (T, B, H) round trip.
            kwargs = dict(kwargs)
            kwargs['options'] = dict(kwargs.get('options') or {}, row_out=final_index)
            return self._readout(self._solve_sde_path(times, times, z0, kwargs))
        ts, row_slot = self.output_times(times, final_index)
        z_t = self._solve_sde_path(times, ts, z0, kwargs)
        if row_slot.numel() != z_t.shape[1]:      # options={'samples': S}: S paths per row, path-major
            row_slot = row_slot.repeat_interleave(z_t.shape[1] // row_slot.numel())
        idx = row_slot.reshape(1, -1, 1).expand(1, z_t.shape[1], z_t.shape[2])
        z = z_t.gather(0, idx).squeeze(0)
        return self._readout(z)


class NeuralSDE_forecasting(_SDEHead):
    """Forecasting head: the four natural-spline tensors are concatenated, every knot is an output time and
    the last ``output_time`` states are decoded."""

    def __init__(self, func, input_channels, output_time, hidden_channels, output_channels, initial=True):
        super().__init__()
        self.func = func
        self.initial = initial
        self.output_time = output_time
        self.initial_network = nn.Linear(input_channels, hidden_channels)
        self.linear = nn.Sequential(nn.Linear(hidden_channels, hidden_channels), nn.ReLU(),
                                    nn.Linear(hidden_channels, output_channels))

    def forward(self, times, coeffs, final_index, z0=None, stream=False, **kwargs):
        self.func.set_X(torch.cat(coeffs, dim=-1), times)
        z0, kwargs = self._initial_state(times, z0, kwargs)
        z = self._solve_sde_path(times, times, z0, kwargs).movedim(0, -2)
        return self._readout(z[:, z.shape[1] - self.output_time:, :])


class IstsNeuralSDE(_SDEHead):
    """torch_ists flavour: ``forward(coeffs, times)`` -> (readout, latent path); default method srk."""
    default_method = 'srk'
    respect_euler_grid = True

    def __init__(self, func, input_channels, hidden_channels, output_channels, initial=True):
        super().__init__()
        self.func = func
        self.initial = initial
        self.initial_network = nn.Linear(input_channels, hidden_channels)
        self.linear = nn.Sequential(nn.Tanh(), nn.Linear(hidden_channels, hidden_channels), nn.ReLU(),
                                    nn.Linear(hidden_channels, output_channels))

    def forward(self, coeffs, times, **kwargs):
        self.func.set_X(coeffs, times)
        if self.initial:
            z0, kwargs = self._initial_state(times, None, kwargs)
        else:
            z0 = self.initial_network(torch.zeros_like(self.func.X.evaluate(times[0])))
        z = self._solve_sde_path(times, times, z0, kwargs).permute(1, 0, 2)
        return self._readout(z), z


class Ensemble(nn.Module):
    """M wrappers of one class (NeuralSDE, NeuralSDE_forecasting or IstsNeuralSDE) and one architecture evaluated on one batch
    together: the call signature is the wrapper's own, every result gains a leading axis of size M.

    Each member's initial state is its own (its `initial_network` on the shared control path, or the caller's z0[m]), ONE
    torchsde.sdeint_ensemble runs over the members' `func` - a single fused solve where the library plans it, the M ordinary solves
    otherwise - and each member's own readout follows.  Inference: in eval() and under no_grad the output equals calling the M
    wrappers one after the other with options={'seed': s, 'row_offset': m B, 'global_rows': M B}, bit for bit (member m's rows are
    rows m B .. of an M B-row problem).  Training through an ensemble is an opt-in, options={'ensemble_grad': True}
    (torchsde.sdeint_ensemble): in train() with gradients required each member's initial state is the differentiable tensor-op form
    (`_prepare_initial_state`: `_initial_state` never hands `initial_network` to the solve under grad), the readouts stay the
    members' own, and outputs and every member's parameter gradients equal the M wrapper calls in training mode with the options
    above.  Without the opt-in sdeint_ensemble raises under autograd.
    options={'samples': S, 'ensemble_samples': True} (with 'ensemble_grad' and 'sample_grad' under autograd) pass through to
    sdeint_ensemble: S Brownian paths per input row for every member.  Each member's initial state stays one row per input row
    (the solve expands it), the readouts return one row per path as the wrappers do for `samples`, and every output is
    (M, B S, ..) - equal to the M wrapper calls with options={'samples': S, 'row_offset': m B S, 'global_rows': M B S}.
    options={'ensemble_nets': True} passes through unchanged as well: members whose field has a diffusion net (noise_option 14 / 15 /
    18 / 19) then take the fused solve on the wave-pair / diffusion-net kernels in eval(); in train() under autograd (with
    'ensemble_grad') they run the M differentiable solves, as without the option - unless 'ensemble_nets_grad': True is passed as
    well: members on the wave pairs (H = 64, Euler / SRK) then train through one fused forward and one fused backward per step."""

    KINDS = ()      # (the three wrapper classes: filled below, once they are all defined)

    def __init__(self, models):
        super().__init__()
        models = list(models)
        if not models or type(models[0]) not in self.KINDS or any(type(m) is not type(models[0]) for m in models):
            raise ValueError("Ensemble takes one or more wrappers of ONE class: NeuralSDE, NeuralSDE_forecasting or IstsNeuralSDE")
        first = models[0]
        for m in models[1:]:
            if (m.initial != first.initial or m.initial_network.weight.shape != first.initial_network.weight.shape
                    or getattr(m, 'output_time', None) != getattr(first, 'output_time', None)):
                raise ValueError("the members of an Ensemble have one architecture (same channels, same `initial`, same output_time)")
        self.models = nn.ModuleList(models)

    def __len__(self):
        return len(self.models)

    def _member_z0(self, m, times, z0, kwargs, dt):
        """Member m's initial state, with the bits the member's own call would start from: where that call hands its
        `initial_network` to the fused solve (_SDEHead._initial_state, and the solve takes it: torchsde._sdeint_hip), the library's
        stand-alone form of the same launch (engine.initial_state); everywhere else `_prepare_initial_state`."""
        func, lin = m.func, m.initial_network
        state, kw = m._initial_state(times, z0, {'options': kwargs.get('options')})
        opts = kw.get('options') or {}
        if 'z0_linear' not in opts:
            return state
        method, kernel = kwargs['method'], opts.get('kernel', 'auto')
        coeffs = func.coeffs
        fused = (opts.get('backend', 'auto') != 'torch' and kwargs.get('bm') is None and kernel == 'auto' and lin.bias is not None
                 and lin.weight.is_contiguous() and lin.bias.dtype == torch.float32 and coeffs.dim() == 3
                 and tuple(lin.weight.shape) == (func.hidden_channels, func.input_channels))
        if int(opts.get('samples') or 1) > 1:      # (sample paths: the member's own call materialises z0 with tensor ops, torchsde._sdeint_samples)
            fused = False
        if fused:
            grid = engine.step_grid(_HostTimes.get(times), dt, _HostTimes.get(func.times), coeffs.device)
            # (a hidden size the member's solve zero-pads starts from the tensor-op state: torchsde._sdeint_hip)
            fused = not (opts.get('precision', 'fp32') == 'fp32' and
                         engine.padding_plan(engine.recognise(func)[0], int(coeffs.shape[0]), int(coeffs.shape[1]) + 1, grid.N, method) is not None)
        if not fused:
            return m._prepare_initial_state(times, None)
        return engine.initial_state(lin.weight.detach(), lin.bias.detach().contiguous(),
                                    coeffs.detach().to(torch.float32).contiguous(), grid)

    def _solve(self, times, ts, z0, kwargs, row_out=None, zero_state=False):
        """(T, M, B, H) - (M, B, H) with row_out - of the members' fields from their own initial states."""
        head = self.models[0]
        kwargs, dt = prepare_sde_solver_kwargs(times, kwargs, default_method=head.default_method,
                                               respect_euler_grid=head.respect_euler_grid)
        extra = set(kwargs) - {'method', 'options', 'bm', 'dt'}
        if extra:
            raise ValueError(f"Ensemble does not take the solver arguments {sorted(extra)}")
        if zero_state:      # (IstsNeuralSDE with initial=False: nsde_model.py's zero control value)
            z0s = [m.initial_network(torch.zeros_like(m.func.X.evaluate(times[0]))) for m in self.models]
        else:
            z0s = [self._member_z0(m, times, None if z0 is None else z0[i], kwargs, dt) for i, m in enumerate(self.models)]
        options = dict(kwargs.get('options') or {})
        if row_out is not None:
            options['row_out'] = row_out
        return _torchsde.sdeint_ensemble([m.func for m in self.models], torch.stack(z0s), ts, bm=kwargs.get('bm'),
                                         method=kwargs['method'], dt=kwargs.get('dt', dt), options=options)

    def forward(self, *args, **kwargs):
        kind = type(self.models[0])
        if kind is IstsNeuralSDE:
            return self._forward_ists(*args, **kwargs)
        return self._forward_benchmark(kind is NeuralSDE_forecasting, *args, **kwargs)

    def _forward_benchmark(self, forecasting, times, coeffs, final_index, z0=None, stream=False, **kwargs):
        models = self.models
        control = (torch.cat(coeffs, dim=-1),) if forecasting else tuple(coeffs)      # (one control path, the same tensors for all)
        for m in models:
            m.func.set_X(*control, times)
        if forecasting:
            ys = self._solve(times, times, z0, kwargs)
            zs = [ys[:, i].contiguous().movedim(0, -2) for i in range(len(models))]
            return torch.stack([m._readout(z[:, z.shape[1] - m.output_time:, :]) for m, z in zip(models, zs)])
        if stream:
            ys = self._solve(times, times, z0, kwargs)
            return torch.stack([m.linear(ys[:, i].contiguous().movedim(0, -2)) for i, m in enumerate(models)])
        if control[0].is_cuda and all(engine.recognise(m.func) is not None for m in models):
            ys = self._solve(times, times, z0, kwargs, row_out=final_index)      # each row's own state, selected inside the solve
            return torch.stack([m._readout(ys[i]) for i, m in enumerate(models)])
        ts, row_slot = NeuralSDE.output_times(times, final_index)
        ys = self._solve(times, ts, z0, kwargs)
        if row_slot.numel() != ys.shape[2]:      # options={'samples': S, 'ensemble_samples': True}: S paths per row, path-major
            row_slot = row_slot.repeat_interleave(ys.shape[2] // row_slot.numel())
        idx = row_slot.reshape(1, -1, 1).expand(1, ys.shape[2], ys.shape[3])
        return torch.stack([m._readout(ys[:, i].gather(0, idx).squeeze(0)) for i, m in enumerate(models)])

    def _forward_ists(self, coeffs, times, **kwargs):
        models = self.models
        for m in models:
            m.func.set_X(coeffs, times)
        ys = self._solve(times, times, None, kwargs, zero_state=not models[0].initial)
        zs = [ys[:, i].contiguous().permute(1, 0, 2) for i in range(len(models))]
        return torch.stack([m._readout(z) for m, z in zip(models, zs)]), torch.stack(zs)


Ensemble.KINDS = (NeuralSDE, NeuralSDE_forecasting, IstsNeuralSDE)


def make_sde_model(name, input_channels, output_channels, hidden_channels, hidden_hidden_channels,
                   num_hidden_layers, initial=True):
    """The five SDE entries of ``common_sde.make_model`` (benchmark_classification/common_sde.py:301-342)."""
    options = {'staticsde': (1, 0), 'naivesde': (1, 18), 'neurallsde': (2, 16), 'neurallnsde': (4, 17),
               'neuralgsde': (6, 17)}
    if name not in options:
        raise ValueError(f"Unrecognised SDE model name {name}. Valid names are {sorted(options)}.")
    io, no = options[name]
    field = Diffusion_model(input_channels, hidden_channels, hidden_hidden_channels, num_hidden_layers,
                            input_option=io, noise_option=no)
    model = NeuralSDE(func=field, input_channels=input_channels, hidden_channels=hidden_channels,
                      output_channels=output_channels, initial=initial)
    return model, field
