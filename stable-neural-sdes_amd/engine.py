"""Host plumbing around the C ABI: model recognition, flat parameter block, time grid, launch.

PyTorch is used only for device memory and streams; all arithmetic of the hot path runs in
libsnsde.so (HIP).  Nothing here falls back to CPU math.
"""
import os
import ctypes as C
import collections
import functools
import math
import struct
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

_GRID_CACHE = OrderedDict()
_GRID_CACHE_MAX = 16


def model_struct(input_channels, hidden_channels, hidden_hidden_channels, num_hidden_layers, input_option,
                 noise_option, activation=0, drift_output=0, diffusion_output=0, time_feature=0):
    """snsde_model; the four trailing switches (include/snsde.h SNSDE_ACT_* ...) are 0 for the reference's models."""
    return _lib.Model(int(input_channels), int(hidden_channels), int(hidden_hidden_channels),
                      int(num_hidden_layers), int(input_option), int(noise_option), int(activation),
                      int(drift_output), int(diffusion_output), int(time_feature))


def recognise(sde):
    """Fast-path contract: an object exposing the reference Diffusion_model's attributes
    (models_sde/neuralsde.py:123-184) and exactly its parameter names/shapes.  Returns
    (Model struct, layout, numel) or None."""
    need = ('input_option', 'noise_option', 'hidden_channels', 'input_channels', 'coeffs', 'times')
    if not all(hasattr(sde, a) for a in need) or not hasattr(sde, 'named_parameters'):
        return None
    cached = getattr(sde, '_snsde_rec', None)     # (key, result): parameter names/shapes are fixed after construction
    key = (sde.input_option, sde.noise_option, sde.hidden_channels, sde.input_channels, len(sde._parameters),
           len(sde._modules))
    if cached is not None and cached[0] == key:
        return cached[1]
    result = _recognise(sde)
    try:
        object.__setattr__(sde, '_snsde_rec', (key, result))
    except Exception:
        pass
    return result


class ParamIndex:
    """The module's parameters resolved ONCE: in named_parameters() order (what autograd.Function.apply receives and backward
    returns) and in the C ABI's layout order, with the per-parameter (offset, numel, shape) of the flat block.  A training step
    walked named_parameters() six times (~25 us each: half of the host time of sdeint() on the K2 step, which is host-bound);
    the cached lists are validated by identity against the owning submodules' _parameters dicts (~2 us), so a re-assigned
    parameter (module.weight = nn.Parameter(...)) or a replaced layer rebuilds them."""

    def __init__(self, sde, layout):
        named = list(sde.named_parameters())
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        by_name = dict(named)
        self.layout_params = [by_name[name] for name, _, _ in layout]
        offs = {name: (off, shape) for name, off, shape in layout}
        self.sizes = [by_name[name].numel() for name, _, _ in layout]              # split sizes of the flat block (layout order)
        order = {name: i for i, (name, _, _) in enumerate(layout)}
        self.to_layout = [order[n] for n in self.names]                             # named order -> index in the layout
        self.shapes = [tuple(offs[n][1]) for n in self.names]
        self.owners = []
        for n in self.names:
            mod, parts = sde, n.split('.')
            for q in parts[:-1]:
                mod = mod._modules[q]
            self.owners.append((mod._parameters, parts[-1]))
        self.all_f32 = all(p.dtype == torch.float32 for p in self.params)
        self.layout_obj, self.layout_key = layout, tuple(layout)      # (name, offset, shape) triples: compared by VALUE when the object differs
        # the module tree the lists were read from: every (parent's _modules dict, name, child) edge and, per module, the sizes of
        # its _parameters / _modules dicts - a replaced submodule (whose old _parameters dict still holds the old tensors), an
        # added or a removed parameter / submodule all show here without walking named_modules() again (25 us per walk)
        mods = list(sde.modules())
        self.edges = [(m._modules, k, c) for m in mods for k, c in m._modules.items()]
        self.sizes_seen = [(m._parameters, len(m._parameters), m._modules, len(m._modules)) for m in mods]
        self.n_params = sum(len(m._parameters) for m in mods)

    def valid(self, sde, layout):
        if self.layout_obj is not layout and self.layout_key != tuple(layout):
            return False
        for d, k, child in self.edges:
            if d.get(k) is not child:
                return False
        for pd, npar, md, nmod in self.sizes_seen:
            if len(pd) != npar or len(md) != nmod:
                return False
        for (d, k), p in zip(self.owners, self.params):
            if d.get(k) is not p:
                return False
        return True

    # the index rides in the module's __dict__ but must not travel with copies of it: deepcopy / pickle / torch.save
    # carry nothing, the copy is indexed afresh
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())

    def grads_from_flat(self, flat):
        """Per-parameter views of a flat gradient in the C ABI's layout, in named_parameters() order."""
        pieces = flat.split(self.sizes)
        out = []
        for i, shape, p in zip(self.to_layout, self.shapes, self.params):
            g = pieces[i].view(shape)
            out.append(g if p.dtype == torch.float32 else g.to(p.dtype))
        return out


def param_index(sde, layout):
    idx = sde.__dict__.get('_snsde_pidx') if hasattr(sde, '__dict__') else None
    if idx is None or not idx.valid(sde, layout):
        idx = ParamIndex(sde, layout)
        try:
            sde.__dict__['_snsde_pidx'] = idx
        except Exception:
            pass
    return idx


def _recognise(sde):
    if getattr(sde, 'sde_type', 'ito') != 'ito' or getattr(sde, 'noise_type', 'diagonal') != 'diagonal':
        return None
    params = dict(sde.named_parameters())
    lin = params.get('linear_in.weight')
    out = params.get('linear_out.weight')
    if lin is None or out is None:
        return None
    n_hidden = sum(1 for k in params if k.startswith('linears.') and k.endswith('.weight'))
    m = model_struct(sde.input_channels, sde.hidden_channels, lin.shape[0], n_hidden + 1, sde.input_option,
                     sde.noise_option)
    try:
        layout, numel = _lib.param_layout(m)
    except _lib.SnsdeError:
        return None
    if set(params) != {n for n, _, _ in layout}:
        return None
    for name, _, shape in layout:
        if tuple(params[name].shape) != tuple(shape):
            return None
    return m, layout, numel


_MFMA_SIZES = (16, 32, 64, 128, 256)
_PAD_CACHE = {}


PRECISIONS = ('fp32', 'bf16')


def precision_flags(precision, bf16_grad=False):
    """SNSDE_FLAG_* bits of an operand precision ('fp32': none; 'bf16': SNSDE_FLAG_BF16_OPERANDS, with bf16_grad also
    SNSDE_FLAG_BF16_GRAD - the flag means nothing without bf16 operands)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    if precision != 'bf16':
        return 0
    return _lib.FLAG_BF16_OPERANDS | (_lib.FLAG_BF16_GRAD if bf16_grad else 0)


def resolve_global_rows(global_rows, batch, row_offset=0):
    """The `global_rows` of a descriptor (include/snsde.h) from what a caller passed: None / 0 = this call is the whole problem;
    'world' = world_size x the local batch under an initialised process group (equal shards), else the local batch; an integer =
    the rows of the whole problem, at least row_offset + batch (ValueError otherwise)."""
    if global_rows is None or (not isinstance(global_rows, str) and int(global_rows) == 0):
        return 0
    if isinstance(global_rows, str):
        if global_rows != 'world':
            raise ValueError(f"global_rows must be an integer or 'world', got {global_rows!r}")
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        return world * int(batch)
    g = int(global_rows)
    if g < int(row_offset) + int(batch) or int(row_offset) < 0:
        raise ValueError(f"global_rows={g} is smaller than row_offset + batch = {int(row_offset)} + {int(batch)}: it is the row count "
                         "of the WHOLE problem this solve is a batch shard of")
    return g


def check_samples(samples):
    """The `samples` option (Brownian paths per input row): an int >= 1, ValueError otherwise (bool is not an int here)."""
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise ValueError(f"samples must be an integer >= 1 (Brownian paths per input row), got {samples!r}")
    return samples


def _check_bool_option(name, value, what):
    """An opt-in switch of a solve: a bool, ValueError otherwise."""
    if not isinstance(value, bool):
        raise ValueError(f"{name} must be a bool ({what}), got {value!r}")
    return value


# the opt-ins as sdeint / sdeint_ensemble check them (SNSDE_FLAG_SAMPLE_GRAD, _BF16_GRAD, _ENSEMBLE_GRAD, _ENSEMBLE_SAMPLES,
# _ENSEMBLE_NETS, _ENSEMBLE_NETS_GRAD - the last meaningful together with ensemble_nets and ensemble_grad)
check_sample_grad = functools.partial(_check_bool_option, 'sample_grad', what='differentiate a solve of `samples` paths per input row')
check_resume_grad = functools.partial(_check_bool_option, 'resume_grad', what='differentiate a continued solve, step_offset != 0')
check_bf16_grad = functools.partial(_check_bool_option, 'bf16_grad', what="differentiate a precision='bf16' solve")
check_ensemble_grad = functools.partial(_check_bool_option, 'ensemble_grad', what='differentiate a solve of `members` models')
check_ensemble_samples = functools.partial(_check_bool_option, 'ensemble_samples',
                                           what='`samples` paths per input row for each of `members` models')
check_ensemble_nets = functools.partial(_check_bool_option, 'ensemble_nets', what='`members` models on the diffusion-net kernels in one solve')
check_ensemble_nets_grad = functools.partial(_check_bool_option, 'ensemble_nets_grad',
                                             what='differentiate `members` models on the wave-pair kernels')

_METHODS = {'euler': _lib.EULER, 'milstein': _lib.MILSTEIN, 'srk': _lib.SRK}
# The one place where an option name meets its SNSDE_FLAG_* bit (the two bf16 bits: precision_flags; SNSDE_FLAG_REUSE_PREPARED is
# no configuration: SolveCall.launch sets it per launch).  Not in the table, on purpose: SNSDE_FLAG_RESUME_GRAD (_lib.RESUME_GRAD,
# option 'resume_grad').  Like step_offset, which it goes with, it belongs to the launch: no plan and no size query reads it, so it
# is no field of SolveConfig (whose fields key the memos of those queries) - SolveCall(..., resume_grad=True) sets the bit beside the
# record's flags, and it is the one descriptor flag that is neither here nor in precision_flags nor set per launch
_FLAG_TABLE = (('exact_order', _lib.FLAG_EXACT_ORDER), ('stream_all', _lib.FLAG_STREAM_ALL), ('two_tile', _lib.FLAG_TWO_TILE),
               ('lean_general', _lib.FLAG_LEAN_GENERAL), ('sample_grad', _lib.FLAG_SAMPLE_GRAD), ('ensemble_grad', _lib.FLAG_ENSEMBLE_GRAD),
               ('ensemble_samples', _lib.FLAG_ENSEMBLE_SAMPLES), ('ensemble_nets', _lib.FLAG_ENSEMBLE_NETS),
               ('ensemble_nets_grad', _lib.FLAG_ENSEMBLE_NETS_GRAD))
_PRESENT = C.c_void_p(16)      # a pointer of which a host-side query reads the presence only
_MODEL_INTS = struct.Struct(f'{len(_lib.Model._fields_)}i')


def _option_flags(is_set):
    """The SNSDE_FLAG_* bits of the _FLAG_TABLE switches that `is_set(name)` holds for."""
    return sum(bit for name, bit in _FLAG_TABLE if is_set(name))


class SolveConfig(collections.namedtuple('SolveConfig', (
        'model', 'batch', 'knots', 'n_steps', 'n_out', 'method', 'kernel', 'precision', 'exact_order', 'stream_all', 'two_tile', 'lean_general',
        'sample_grad', 'bf16_grad', 'ensemble_grad', 'ensemble_samples', 'ensemble_nets', 'ensemble_nets_grad', 'samples', 'members',
        'global_rows', 'dW', 'noise_table', 'row_out', 'seed_dev', 'training', 'kl_column'))):
    """Everything the library's plan reads of a solve, and nothing else: hashable, so it is also the key of every memo of a
    host-side query.  model: the ten integers of _lib.Model; samples / members: 0, or > 1; dW .. training: the presence of what the
    plan looks at (supplied increments, the noise table, the per-row output selection, a device-resident seed, the training planes).
    Built by `SolveConfig.of`, which normalises (`replace` goes through it again).  Not in it: row_offset (no plan reads it, and the
    members of an ensemble's loop route would each get an entry of their own) and the value of the seed."""
    __slots__ = ()

    @classmethod
    def of(cls, model, batch, knots, n_steps, n_out=2, method='euler', kernel='auto', precision='fp32', exact_order=False,
           stream_all=False, two_tile=False, lean_general=False, sample_grad=False, bf16_grad=False, ensemble_grad=False,
           ensemble_samples=False, ensemble_nets=False, ensemble_nets_grad=False, samples=0, members=0, global_rows=0, dW=False,
           noise_table=False, row_out=False, seed_dev=False, training=False, kl_column=None):
        """The normalised record: samples / members are 0 unless > 1, and an opt-in that means nothing without its carrier is
        dropped (sample_grad: samples > 1; the ensemble_*: members > 1, ensemble_samples also samples > 1; bf16_grad:
        precision='bf16').  KeyError for an unknown method or kernel, ValueError for an unknown precision."""
        _METHODS[method], _lib.KERNELS[kernel], precision in PRECISIONS or precision_flags(precision)
        samples, members = int(samples or 0), int(members or 0)
        sampled, ensemble = samples > 1, members > 1
        if not isinstance(model, tuple):
            model = _MODEL_INTS.unpack(model)
        return cls(model, batch, knots, n_steps, n_out, method, kernel, precision, bool(exact_order), bool(stream_all), bool(two_tile),
                   bool(lean_general), sampled and bool(sample_grad), precision == 'bf16' and bool(bf16_grad), ensemble and bool(ensemble_grad),
                   ensemble and sampled and bool(ensemble_samples), ensemble and bool(ensemble_nets), ensemble and bool(ensemble_nets_grad),
                   samples if sampled else 0, members if ensemble else 0, int(global_rows), bool(dW), bool(noise_table), bool(row_out),
                   bool(seed_dev), bool(training), None if kl_column is None else int(kl_column))

    def replace(self, **changes):
        """This record with `changes`, normalised again."""
        return SolveConfig.of(**dict(self._asdict(), **changes))

    @property
    def flags(self):
        """The descriptor's flags: precision_flags and the _FLAG_TABLE bits of the switches."""
        return precision_flags(self.precision, self.bf16_grad) | _option_flags(self.__getattribute__)


def _describe(config, row_offset=0, planes=True):
    """The _lib.Solve of a SolveConfig: every configuration field, and _PRESENT in each pointer whose presence the plan reads.
    The one place a plan descriptor is made - a query asks with it as it is, SolveCall then writes its buffers over the
    placeholders.  row_offset: written where the caller has one (no plan reads it).  planes=False leaves the training planes
    null (SolveCall asks for its save layout before it has allocated them)."""
    s = _lib.Solve()
    s.model = _lib.Model(*config.model)
    s.batch, s.knots, s.n_steps, s.n_out = config.batch, config.knots, config.n_steps, config.n_out
    s.method, s.kernel, s.flags = _METHODS[config.method], _lib.KERNELS[config.kernel], config.flags
    s.row_offset, s.global_rows, s.samples, s.members = int(row_offset), config.global_rows, config.samples, config.members
    if config.training and planes:
        s.traj = s.act_save = _PRESENT
    if config.dW:
        s.dW = _PRESENT
    if config.noise_table:
        s.noise_table = _PRESENT
    if config.row_out:
        s.row_out = _PRESENT
    if config.seed_dev:
        s.seed_dev = _PRESENT
    if config.kl_column is not None:
        s.kl_column1 = config.kl_column + 1
    return s


def query_descriptor(model, batch, knots, n_steps, method='euler', kernel='auto', table=False, precision='fp32', global_rows=0,
                     row_offset=0, samples=0, lean_general=False, exact_order=False, sample_grad=False, training=False, bf16_grad=False,
                     members=0, ensemble_grad=False, ensemble_samples=False, ensemble_nets=False, ensemble_nets_grad=False):
    """The _lib.Solve descriptor of a solve that has not been allocated, as the host-side queries of the library read it (no
    device pointer is real): what forward_path asks about, and what forward_kernel / _lib.lib().snsde_workspace_bytes take."""
    return _describe(SolveConfig.of(model, batch, knots, n_steps, 2, method, kernel, precision, exact_order=exact_order,
                                    lean_general=lean_general, sample_grad=sample_grad, bf16_grad=bf16_grad, ensemble_grad=ensemble_grad,
                                    ensemble_samples=ensemble_samples, ensemble_nets=ensemble_nets, ensemble_nets_grad=ensemble_nets_grad,
                                    samples=samples, members=members, global_rows=global_rows, noise_table=table, training=training),
                     row_offset)


def forward_path(model, batch, knots, n_steps, method='euler', kernel='auto', table=False, precision='fp32', global_rows=0,
                 row_offset=0, samples=0, lean_general=False, exact_order=False, sample_grad=False, training=False, bf16_grad=False,
                 members=0, ensemble_grad=False, ensemble_samples=False, ensemble_nets=False, ensemble_nets_grad=False):
    """Name of the kernel family a forward solve of this shape takes (_lib.PATHS; host-side query).  global_rows: the rows of the
    whole problem this solve is a batch shard of (the planner then chooses as for that many rows on one device); 0: none.
    samples: Brownian paths per input row (include/snsde.h; `batch` then counts paths); 'none' where the kernel the plan arrives
    at does not map paths to input rows.  sample_grad: SNSDE_FLAG_SAMPLE_GRAD; training: the solve writes its training planes
    (a sampled solve has them under sample_grad only, on the kernels the sampled adjoint route covers; a bf16 solve under bf16_grad
    only: SNSDE_FLAG_BF16_GRAD).  members: models of one architecture in the call (include/snsde.h; `batch` then counts the rows
    of all members); 'none' where the plan arrives at a kernel that does not map rows to members.  ensemble_grad:
    SNSDE_FLAG_ENSEMBLE_GRAD - an ensemble has training planes under it only, on the kernels the ensemble adjoint route covers.
    ensemble_samples: SNSDE_FLAG_ENSEMBLE_SAMPLES - members > 1 together with samples > 1 ('none' without it).
    ensemble_nets: SNSDE_FLAG_ENSEMBLE_NETS - members > 1 on the wave pairs ('w4') and the diffusion-net tiles ('none' without it).
    ensemble_nets_grad: SNSDE_FLAG_ENSEMBLE_NETS_GRAD - with ensemble_nets and ensemble_grad, training planes of an ensemble on 'w4'."""
    return _lib.PATHS[_lib.lib().snsde_forward_path(C.byref(query_descriptor(**locals())))]


def shard_refused(model, batch, knots, n_steps, method='euler', kernel='auto', table=False, global_rows=0, row_offset=0):
    """True when the kernel planned for the whole problem (global_rows) cannot run this shard - a wave-pair plan and fewer than four
    rows - although the whole problem has a kernel: such a solve is an error, never another kernel or the tensor-op loop."""
    if not global_rows or forward_path(model, batch, knots, n_steps, method, kernel, table, global_rows=global_rows,
                                       row_offset=row_offset) != 'none':
        return False
    return forward_path(model, min(int(global_rows), 2 ** 31 - 1), knots, n_steps, method, kernel, table) != 'none'


def check_bf16(model, batch, knots, n_steps, method='euler', kernel='auto'):
    """Raise ValueError unless the bf16-operand kernel takes this inference solve (there is no fp32 stand-in for it)."""
    if method == 'srk':
        raise ValueError("precision='bf16' covers Euler and Milstein only, not SRK")
    if forward_path(model, batch, knots, n_steps, method, kernel, precision='bf16') != 'lean-bf16':
        raise ValueError(f"precision='bf16' does not cover this configuration (hidden_channels={model.hidden_channels}, "
                         f"num_hidden_layers={model.num_hidden_layers}, input_option={model.input_option}, "
                         f"noise_option={model.noise_option}, method={method!r}, kernel={kernel!r}): it runs the lean 4-row-tile "
                         "kernel at H = 64 / 128 on the reference's Diffusion_model fields only")


def padding_plan(model, batch, knots, n_steps, method):
    """Hidden sizes the MFMA kernels are not instantiated for (H not in 16 / 32 / 64 / 128 / 256, or a hidden width HH != H)
    would land on the generic VALU kernels (~13x slower).  Zero-padding the model to the next instantiated size P is exact:
    padded hidden units have zero weights and biases (relu(0) = 0), padded state components have zero output weights
    (tanh(0) = 0 drift) and are read by nothing (zero first-layer / diffusion-net columns), so the real components evolve
    exactly as in the unpadded model and the padded ones are dropped from the outputs.
    Returns (padded model struct, its layout, numel, P) when that moves the solve onto an MFMA kernel, else None."""
    H, HH = model.hidden_channels, model.hidden_hidden_channels
    if H in _MFMA_SIZES and HH == H:
        return None
    if model.activation or model.drift_output or model.diffusion_output or model.time_feature:
        return None      # field variants: the padded block below is the reference Diffusion_model's, not theirs
    key = (model.input_channels, H, HH, model.num_hidden_layers, model.input_option, model.noise_option, int(batch), int(knots),
           int(n_steps), method)
    if key not in _PAD_CACHE:
        plan = None
        P = next((p for p in _MFMA_SIZES if p >= max(H, HH)), None)
        if P is not None and model.activation == 0 and forward_path(model, batch, knots, n_steps, method) in ('generic', 'generic-srk'):
            mp = model_struct(model.input_channels, P, P, model.num_hidden_layers, model.input_option, model.noise_option)
            try:
                layout_p, numel_p = _lib.param_layout(mp)
                if forward_path(mp, batch, knots, n_steps, method) not in ('none', 'generic', 'generic-srk'):
                    plan = (mp, layout_p, numel_p, P)
            except _lib.SnsdeError:
                plan = None
        _PAD_CACHE[key] = plan
    return _PAD_CACHE[key]


def padded_flat(sde, layout, layout_p, H, P, device, grad):
    """The padded model's parameter block from the module's parameters (torch ops: differentiable when grad).  Every tensor
    sits in the top-left corner of its padded shape, except emb.weight whose two H-wide column blocks (yy | X_t) go to
    columns [0, H) and [P, P + H)."""
    params = dict(sde.named_parameters())
    pieces = []
    with torch.set_grad_enabled(grad):
        for (name, _, shape), (name_p, _, shape_p) in zip(layout, layout_p):
            assert name == name_p
            w = params[name].to(device=device, dtype=torch.float32)
            if not grad:
                w = w.detach()
            if tuple(shape) == tuple(shape_p):
                z = w
            else:
                z = w.new_zeros(tuple(shape_p))
                if name == 'emb.weight':
                    z[:shape[0], :H] = w[:, :H]
                    z[:shape[0], P:P + H] = w[:, H:]
                elif w.dim() == 2:
                    z[:shape[0], :shape[1]] = w
                else:
                    z[:shape[0]] = w
            pieces.append(z.reshape(-1))
        return torch.cat(pieces)


def flatten_params(sde, layout, numel, device):
    """One float32 device buffer in the C ABI's layout (state_dict order).

    The first call concatenates the parameters and (when they are float32 tensors on `device`) re-points every
    `param.data` at its slice of that buffer, so later calls — including after in-place optimizer steps, which now
    write straight into the buffer — return it without launching anything.  Anything that re-allocates a parameter
    (`.to()`, `.double()`, a new nn.Parameter) is detected by the address check and triggers a fresh flatten."""
    plist = param_index(sde, layout).layout_params
    arena = getattr(sde, '_snsde_flat', None)
    if arena is not None and arena.device == device:
        base = arena.data_ptr()
        if all(p.data_ptr() == base + 4 * off and p.dtype == torch.float32 for p, (_, off, _) in zip(plist, layout)):
            return arena
    flat = torch.cat([p.detach().reshape(-1).to(device=device, dtype=torch.float32) for p in plist])
    assert flat.numel() == numel
    if all(p.dtype == torch.float32 and p.device == device for p in plist) and os.environ.get('SNSDE_NO_PARAM_ARENA') != '1':
        with torch.no_grad():
            for p, (_, off, shape) in zip(plist, layout):
                p.data = flat[off:off + p.numel()].view(shape)
        try:
            object.__setattr__(sde, '_snsde_flat', flat)
        except Exception:
            pass
    return flat


class StepGrid:
    """Host + device copy of the fixed-step grid (snsde_grid_build)."""

    def __init__(self, ts_host, dt, times_host, device):
        L = _lib.lib()
        ts32 = np.ascontiguousarray(ts_host, dtype=np.float32)
        times32 = np.ascontiguousarray(times_host, dtype=np.float32)
        if ts32.ndim != 1 or ts32.shape[0] < 2:
            raise ValueError('`ts` must be a 1-D sequence of at least two times.')
        n = C.c_int32()
        rc = L.snsde_grid_count(ts32.ctypes.data, ts32.shape[0], float(dt), C.byref(n))
        if rc == -7:
            raise ValueError('Evaluation times `ts` must be strictly increasing and `dt` positive '
                             '(and large enough to advance float32 time).')
        _lib.check(rc, 'snsde_grid_count')
        self.N = n.value
        self.T = ts32.shape[0]
        self.step_tab = np.zeros((self.N, _lib.SNSDE_STEP_STRIDE), dtype=np.float32)
        self.out_step = np.zeros(self.T - 1, dtype=np.int32)
        self.out_w = np.zeros((self.T - 1, 2), dtype=np.float32)
        _lib.check(L.snsde_grid_build(ts32.ctypes.data, self.T, float(dt), times32.ctypes.data, times32.shape[0],
                                      self.N, self.step_tab.ctypes.data, self.out_step.ctypes.data,
                                      self.out_w.ctypes.data), 'snsde_grid_build')
        self._times32 = times32
        self._d_srk = None
        self.t0 = self.step_tab[:, 0].copy()
        self.t1 = self.step_tab[:, 7].copy()
        self.device = device
        if device is not None and device.type == 'cuda':
            self.d_step_tab = torch.from_numpy(self.step_tab).to(device)
            self.d_t0 = torch.from_numpy(self.t0).to(device)
            self.d_out_step = torch.from_numpy(self.out_step).to(device)
            self.d_out_w = torch.from_numpy(self.out_w).to(device)


def grid_steps(ts_host, dt):
    """The number of solver steps of the fixed-step grid over `ts_host` (snsde_grid_count; host only)."""
    ts32 = np.ascontiguousarray(ts_host, dtype=np.float32)
    n = C.c_int32()
    _lib.check(_lib.lib().snsde_grid_count(ts32.ctypes.data, ts32.shape[0], float(dt), C.byref(n)), 'snsde_grid_count')
    return n.value


def sub_grid(grid, n0, n1):
    """The solver steps n0 .. n1-1 of `grid` as a StepGrid of their own: the SAME step rows (times, step sizes, spline
    intervals), the parent's outputs that fall inside, and one more output at the end of the last step.  Returns
    (sub grid, ks) with ks = the parent's output numbers (k + 1) of the sub grid's outputs 1 .. len(ks); its last output
    (the state after step n1 - 1) is the chunk's hand-over to the steps behind it."""
    g = StepGrid.__new__(StepGrid)
    K = n1 - n0
    tab = grid.step_tab[n0:n1].copy()
    ks = [k for k in range(grid.T - 1) if n0 <= grid.out_step[k] < n1]
    out_step = np.array([grid.out_step[k] - n0 for k in ks] + [K - 1], dtype=np.int32)
    out_w = np.array([grid.out_w[k] for k in ks] + [(0.0, 1.0)], dtype=np.float32).reshape(-1, 2)
    nout = np.zeros(K, dtype=np.int32)
    first = np.zeros(K, dtype=np.int32)
    for j, st in enumerate(out_step):
        if nout[st] == 0:
            first[st] = j
        nout[st] += 1
    tab[:, 8] = nout.view(np.float32)
    tab[:, 9] = first.view(np.float32)
    g.N, g.T = K, len(out_step) + 1
    g.step_tab, g.out_step, g.out_w = tab, out_step, out_w
    g._times32, g._d_srk = grid._times32, None
    g.t0, g.t1 = tab[:, 0].copy(), tab[:, 7].copy()
    g.device = grid.device
    g.d_step_tab = torch.from_numpy(tab).to(grid.device)
    g.d_t0 = torch.from_numpy(g.t0).to(grid.device)
    g.d_out_step = torch.from_numpy(out_step).to(grid.device)
    g.d_out_w = torch.from_numpy(out_w).to(grid.device)
    return g, [k + 1 for k in ks]


def every_step_grid(grid):
    """`grid`'s solver steps with an output after EVERY step (T = N + 1, no interpolation): the solve then returns the whole
    trajectory as its result, so a caller can attach cotangents to any state (torchsde._sdeint_latent: the KL path integral of
    a latent SDE is a quadrature over all of them).  Memoised on the grid."""
    g = grid.__dict__.get('_every_step')
    if g is not None:
        return g
    g = StepGrid.__new__(StepGrid)
    N = grid.N
    tab = grid.step_tab.copy()
    tab[:, 8] = np.ones(N, dtype=np.int32).view(np.float32)
    tab[:, 9] = np.arange(N, dtype=np.int32).view(np.float32)
    g.N, g.T = N, N + 1
    g.step_tab = tab
    g.out_step = np.arange(N, dtype=np.int32)
    g.out_w = np.tile(np.array([[0.0, 1.0]], dtype=np.float32), (N, 1))
    g._times32, g._d_srk = grid._times32, None
    g.t0, g.t1 = tab[:, 0].copy(), tab[:, 7].copy()
    g.device = grid.device
    if grid.device is not None and grid.device.type == 'cuda':
        g.d_step_tab = torch.from_numpy(tab).to(grid.device)
        g.d_t0 = torch.from_numpy(g.t0).to(grid.device)
        g.d_out_step = torch.from_numpy(g.out_step).to(grid.device)
        g.d_out_w = torch.from_numpy(g.out_w).to(grid.device)
    grid.__dict__['_every_step'] = g
    return g


def chunk_plan(grid, chunk):
    """[(n0, n1, sub grid, parent output numbers)] for the recompute-mode backward (memoised on the grid)."""
    cache = grid.__dict__.setdefault('_chunks', {})
    if chunk not in cache:
        cache[chunk] = [(n0, min(n0 + chunk, grid.N)) + sub_grid(grid, n0, min(n0 + chunk, grid.N))
                        for n0 in range(0, grid.N, chunk)]
    return cache[chunk]


def backward_recompute(call, grad_ys, chunk, stream=None):
    """Recompute-mode backward of a solve that kept only its states and increments (SolveCall with save_traj / save_dW,
    no save_act): the steps are revisited in chunks of `chunk`, last chunk first; each chunk re-runs the forward kernel
    from its saved first state with the saved increments (bit-identical states, now with the per-step activations), then
    the adjoint kernel and the weight-gradient pass on those.  Peak extra memory = one chunk's activations and deltas
    (2 x chunk x NSAVE x B x H floats) instead of N x NSAVE x B x H for the whole solve; the chunk buffers are written
    and read back within microseconds, i.e. out of the 256 MB last-level cache rather than HBM.
    Returns (dL/dy0 (B, H), flat parameter gradient)."""
    grid, N = call.grid, call.grid.N
    model, flat, coeffs = call.model, call.keep[0], call.keep[1]
    method = {_lib.EULER: 'euler', _lib.MILSTEIN: 'milstein'}[call.desc.method]
    B, H = call.traj.shape[1:]
    dev = call.traj.device
    per_row = call.keep[6] is not None          # grad_ys is (B, H): row b's gradient belongs to output row_out[b]
    row_out = call.keep[6]
    carry = torch.zeros((B, H), device=dev, dtype=torch.float32)
    total = None
    for n0, n1, sub, ks in reversed(chunk_plan(grid, chunk)):
        g = torch.zeros((sub.T, B, H), device=dev, dtype=torch.float32)
        for j, k in enumerate(ks):                # the parent's outputs inside the chunk
            if per_row:
                g[j + 1] = torch.where((row_out == k).unsqueeze(1), grad_ys, g[j + 1])
            else:
                g[j + 1] = grad_ys[k]
        g[sub.T - 1] += carry                     # everything behind the chunk acts on its last state
        # the chunk reads the parent's increments in place (no second copy: the adjoint takes `dW` where there is no `dW_out`), and
        # its adjoint + weight-gradient pass are one C call
        c = SolveCall(model, flat, coeffs, sub, call.traj[n0], dW=call.dW_out[n0:n1], method=method, kernel='auto',
                      save_traj=True, save_dW=False, save_act=True, exact_order=call.config.exact_order,
                      global_rows=call.config.global_rows)
        c.launch(stream)
        adj, part = backward_with_gradients(c, g, stream=stream, adj0_only=adj0_suffices(c))
        total = part if total is None else total.add_(part)
        carry = adj[0].clone()
        # drop this chunk's activations / deltas / workspaces BEFORE the next chunk allocates its own: the caching allocator then
        # hands the same blocks out again, and the peak is ONE chunk's buffers (two chunks were alive at once before: 50 steps per
        # chunk at K2 peaked above the saved-activation mode)
        c.keep_bwd = c.keep_pg = None
        del c, adj, part, g
    if per_row:
        g0 = torch.where((row_out == 0).unsqueeze(1), grad_ys, torch.zeros_like(grad_ys))
    else:
        g0 = grad_ys[0]
    return carry + g0, total


def srk_table(grid):
    """Device (N, 4, SNSDE_SRK_STRIDE) stage-time table of a StepGrid (built on first use)."""
    if grid._d_srk is None:
        tab = np.zeros((grid.N, 4, _lib.SNSDE_SRK_STRIDE), dtype=np.float32)
        _lib.check(_lib.lib().snsde_grid_srk_build(grid.step_tab.ctypes.data, grid.N, grid._times32.ctypes.data,
                                                   grid._times32.shape[0], tab.ctypes.data), 'snsde_grid_srk_build')
        grid.srk_host = tab
        grid._d_srk = torch.from_numpy(tab).to(grid.device)
    return grid._d_srk


def srk_stage_times(grid):
    """Device (4 N,) tensor of the SRID2 stage times t0 + {0, 1/4, 1/2, 1} h of every step (column 0 of the stage table)."""
    if getattr(grid, '_d_srk_times', None) is None:
        grid._d_srk_times = srk_table(grid)[:, :, 0].reshape(-1).contiguous()
    return grid._d_srk_times


def noise_table_times(grid, method):
    """Device tensor of the times a time-only diffusion factor is tabulated at: the step times; SRK: every step's four stage times."""
    return srk_stage_times(grid) if method == 'srk' else grid.d_t0


def step_grid(ts_host, dt, times_host, device):
    key = (np.asarray(ts_host, dtype=np.float32).tobytes(), float(dt),
           np.asarray(times_host, dtype=np.float32).tobytes(), str(device))
    g = _GRID_CACHE.get(key)
    if g is None:
        g = StepGrid(ts_host, dt, times_host, device)
        _GRID_CACHE[key] = g
        if len(_GRID_CACHE) > _GRID_CACHE_MAX:
            _GRID_CACHE.popitem(last=False)
    else:
        _GRID_CACHE.move_to_end(key)
    return g


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _check_f32(name, t, shape=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f'{name} must be a contiguous float32 CUDA tensor')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {tuple(shape)}')


def check_step_offset(step_offset, n_steps=0):
    """`step_offset` of a resumed solve as a non-negative int whose last global step, step_offset + n_steps, fits 31 bits (the
    Philox counter word and the library's check); ValueError otherwise."""
    if isinstance(step_offset, bool) or not isinstance(step_offset, (int, np.integer)) or int(step_offset) < 0:
        raise ValueError(f'step_offset={step_offset!r}: the global index of this solve\'s first step, a non-negative int')
    if int(step_offset) + int(n_steps) > 2 ** 31 - 1:
        raise ValueError(f'step_offset={step_offset!r}: step_offset + n_steps = {int(step_offset) + int(n_steps)} exceeds 2**31 - 1')
    return int(step_offset)


def check_row_offset(row_offset, batch):
    """`row_offset` of a solve of `batch` rows as an int with 0 <= row_offset and row_offset + batch <= 2**32 (the first Philox counter
    word is the global row, 32 bits: the library refuses rows beyond it instead of re-drawing the paths of rows 0 ..); ValueError
    otherwise.  Independent of global_rows."""
    r = int(row_offset)
    if r < 0 or r + int(batch) > 2 ** 32:
        raise ValueError(f'row_offset={row_offset!r}: the global rows row_offset .. row_offset + batch - 1 = {r} .. {r + int(batch) - 1} of a '
                         'solve must lie in [0, 2**32) (the Philox counter holds the global row in 32 bits)')
    return r


class SolveCall:
    """A fully prepared solve: owns references to every device buffer named in the descriptor so the
    launch itself is one C call that only enqueues kernels (hipGraph-capturable).
    stream_all / two_tile: the A/B switches of include/snsde.h (SNSDE_FLAG_STREAM_ALL: H = 256 on the fully streamed sixteen-wave
    kernels instead of the two-tile ones; SNSDE_FLAG_TWO_TILE: H = 128 on the four-wave two-tile kernel) - same results bit for bit."""

    def __init__(self, model, flat_params, coeffs, grid, y0, dW=None, method='euler', seed=0, row_offset=0,
                 kernel='auto', save_traj=False, save_dW=False, exact_order=False, save_act=False, dU=None, row_out=None,
                 noise_table=None, z0_linear=None, kl_column=None, stream_all=False, two_tile=False, precision='fp32',
                 lean_general=False, global_rows=0, samples=0, sample_grad=False, bf16_grad=False, members=0, ensemble_grad=False,
                 ensemble_samples=False, ensemble_nets=False, ensemble_nets_grad=False, step_offset=0, resume_grad=False):
        B, H = y0.shape
        C_ = model.input_channels
        L = coeffs.shape[1] + 1
        dev = y0.device
        # samples = S > 1: y0, dW, dU, row_out, the result and (sample_grad: training) every saved plane are per PATH (B rows), coeffs
        # per input row (B / S rows)
        S = int(samples) if samples else 1
        if S < 1 or B % S:
            raise ValueError(f'samples={samples!r}: the {B} rows of y0 are paths, a whole number of groups of `samples` per input row')
        if S > 1 and (((save_traj or save_dW or save_act) and not sample_grad) or z0_linear is not None):
            raise ValueError('samples > 1 is inference only: no saved trajectory, increments or activations, and y0 is the caller\'s')
        # members = M > 1 (a model ensemble; inference unless ensemble_grad opts in, SNSDE_FLAG_ENSEMBLE_GRAD): flat_params is (M, numel), y0 / dW / dU / row_out and the result hold the rows
        # of all members, member-major (B = M Bm rows), coeffs is the members' shared control path (Bm rows)
        M = int(members) if members else 1
        if M < 1 or B % M or (M > 1 and (B // M) % 4):
            raise ValueError(f'members={members!r}: the {B} rows of y0 are those of all members, each a whole number of 4-row tiles')
        # members and samples together (SNSDE_FLAG_ENSEMBLE_SAMPLES): row m Bm + b S + s, coeffs (Bm / S rows) shared by all members
        if M > 1 and S > 1 and ensemble_samples and (B // M) % S:
            raise ValueError(f'members={members!r}, samples={samples!r}: the {B // M} rows of a member are a whole number of groups of `samples` paths')
        if M > 1 and ((S > 1 and not ensemble_samples) or ((save_traj or save_dW or save_act) and not ensemble_grad) or z0_linear is not None or noise_table is not None
                      or kl_column is not None):
            raise ValueError('members > 1 is inference only: no samples (without ensemble_samples), saved planes, fused initial network, supplied noise table or '
                             'accumulator column')
        _check_f32('y0', y0, (B, model.hidden_channels))
        _check_f32('coeffs', coeffs, (B // S // M, L - 1, 4 * C_))
        _check_f32('params', flat_params)
        if M > 1 and tuple(flat_params.shape) != (M, _lib.param_layout(model)[1]):
            raise ValueError(f'params has shape {tuple(flat_params.shape)}, expected (members, numel) = {(M, _lib.param_layout(model)[1])}')
        if dW is not None:
            _check_f32('dW', dW, (grid.N, B, H))
        self.model, self.grid = model, grid
        # step_offset = n0 (resumable solves, snsde_solve_forward_at): local step i draws the normals of global step n0 + i.  A stream
        # coordinate like row_offset and seed - kept on the call, not in SolveConfig: no plan and no size query reads it
        self.step_offset = check_step_offset(step_offset, grid.N)
        row_offset = check_row_offset(row_offset, B)
        # resume_grad (SNSDE_FLAG_RESUME_GRAD): a continued solve may keep its training planes; the backward calls then take the offset
        if self.step_offset and ((save_act and not resume_grad) or z0_linear is not None):
            raise ValueError('step_offset != 0 is inference only: a continued solve has no backward (no saved activations) and starts '
                             'from the caller\'s state (no fused initial network)')
        if dU is not None:
            _check_f32('dU', dU, (grid.N, B, H))
        if row_out is not None:
            if row_out.dtype != torch.int32 or not row_out.is_cuda or not row_out.is_contiguous() or tuple(row_out.shape) != (B,):
                raise ValueError('row_out must be a contiguous int32 CUDA tensor of shape (batch,)')
        if noise_table is not None:      # the time-only diffusion factor per step (SRK: at the step's four stage times)
            _check_f32('noise_table', noise_table, (4 * grid.N if method == 'srk' else grid.N, H))
        if z0_linear is not None:     # (weight (H, C), bias (H)): y0 is then an output, filled by the solve's prepare launch
            _check_f32('z0 weight', z0_linear[0], (H, C_))
            _check_f32('z0 bias', z0_linear[1], (H,))
        self.keep = (flat_params, coeffs, y0, dW, grid, dU, row_out, noise_table, z0_linear)
        # per-row output selection: one state per row instead of one plane per output time
        self.ys = torch.empty((B, H) if row_out is not None else (grid.T, B, H), device=dev, dtype=torch.float32)
        self.traj = torch.empty((grid.N + 1, B, H), device=dev, dtype=torch.float32) if save_traj else None
        self.dW_out = torch.empty((grid.N, B, H), device=dev, dtype=torch.float32) if save_dW else None
        self.act_save = self.stage_save = None
        # the record normalises: an opt-in without its carrier (samples > 1, members > 1, precision='bf16') has no effect.  (kernel
        #  selector, flags and the kind of Philox key go in BEFORE the layout / workspace queries below: which adjoint a solve gets - and
        #  with it whether it needs delta planes at all - depends on them, on the supplied increments, the noise table, the accumulator
        #  column and the per-row output selection.)  global_rows: rows of the whole problem this solve is a batch shard of (0: it is the
        #  whole problem) - what the library plans its kernels from
        cfg = SolveConfig.of(model, B, L, grid.N, grid.T, method, kernel, precision, exact_order, stream_all, two_tile, lean_general,
                             sample_grad, bf16_grad, ensemble_grad, ensemble_samples, ensemble_nets, ensemble_nets_grad, S, M,
                             resolve_global_rows(global_rows, B, row_offset), dW is not None, noise_table is not None, row_out is not None,
                             torch.is_tensor(seed), bool(save_traj or save_dW or save_act), None if kl_column is None else kl_column[0])
        # host-side queries of the library (save layout, workspace sizes) depend on the configuration only: memoised by the record
        self.config = self.cfg_key = cfg
        s = _describe(cfg, row_offset, planes=False)
        if resume_grad:      # (no plan input: set beside the record's flags, after the record has keyed the memos)
            s.flags |= _lib.RESUME_GRAD
        self.base_flags, self.members = s.flags, M
        if torch.is_tensor(seed):     # device-resident key: re-read by every launch / graph replay
            if seed.dtype != torch.int64 or not seed.is_cuda or seed.numel() != 1:
                raise ValueError('a tensor seed must be a one-element int64 CUDA tensor')
            self.keep = self.keep + (seed,)
            s.seed_dev = _ptr(seed)
        else:
            s.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        s.dW, s.row_out, s.noise_table = _ptr(dW), _ptr(row_out), _ptr(noise_table)
        if kl_column is not None:     # (column, a, b): path-integral accumulator column with the linear prior drift a y + b (snsde.h)
            s.kl_prior_a, s.kl_prior_b = float(kl_column[1]), float(kl_column[2])
        self.delta_slots = 0          # (delta planes of the adjoint: snsde_save_layout, solves with save_act)
        if save_act:
            lay = _SIZE_CACHE.get(('layout', cfg))
            if lay is None:
                slots, planes, dslots = C.c_int32(), C.c_int32(), C.c_int32()
                _lib.check(_lib.lib().snsde_save_layout(C.byref(s), C.byref(slots), C.byref(planes), C.byref(dslots)), 'snsde_save_layout')
                lay = _SIZE_CACHE[('layout', cfg)] = (slots.value, planes.value, dslots.value)
            nslots, nplanes, self.delta_slots = lay
            passes = 3 * grid.N if method == 'srk' else grid.N      # SRK: three drift passes per step
            self.act_save = torch.empty((passes, nslots, B, H), device=dev, dtype=torch.float32)
            if method == 'srk':
                shape = (passes + 1, B, H) if nplanes == 1 else (passes + 1, nplanes, B, H)
                self.stage_save = torch.empty(shape, device=dev, dtype=torch.float32)
        if method == 'srk':
            s.srk_tab = _ptr(srk_table(grid))
            s.dU = _ptr(dU)
            self.dU_out = torch.empty((grid.N, B, H), device=dev, dtype=torch.float32) if save_dW else None
            s.dU_out = _ptr(self.dU_out)
        s.params, s.coeffs = _ptr(flat_params), _ptr(coeffs)
        s.step_tab, s.out_step, s.out_w = _ptr(grid.d_step_tab), _ptr(grid.d_out_step), _ptr(grid.d_out_w)
        s.y0, s.ys = _ptr(y0), _ptr(self.ys)
        s.traj, s.dW_out = _ptr(self.traj), _ptr(self.dW_out)
        s.act_save = _ptr(self.act_save)
        s.stage_save = _ptr(self.stage_save)
        if z0_linear is not None:
            s.z0_weight, s.z0_bias = _ptr(z0_linear[0]), _ptr(z0_linear[1])
        nbytes = _SIZE_CACHE.get(('fwd', cfg))
        if nbytes is None:
            nbytes = _SIZE_CACHE[('fwd', cfg)] = int(_lib.lib().snsde_workspace_bytes(C.byref(s)))
        self.workspace = torch.empty(max(nbytes, 256), device=dev, dtype=torch.uint8)
        s.workspace = _ptr(self.workspace)
        s.workspace_bytes = self.workspace.numel()
        self.desc = s

    def _prepared_key(self):
        """What the prepared workspace (packed weights, folded products, time tables) was built from: address and version counter
        of the parameter block (+ the supplied noise table).  In-place writes to those tensors bump the counter; writes through an
        alias with its own counter (`tensor.data`, the per-parameter views of the arena) do not - callers that update parameters
        that way build a new SolveCall per solve (torchsde.sdeint does) or pass auto_reuse=False."""
        flat, table = self.keep[0], self.keep[7]
        return (flat.data_ptr(), flat._version, None if table is None else (table.data_ptr(), table._version))

    def launch(self, stream=None, reuse_prepared=False, auto_reuse=False):
        """Enqueue the solve.  reuse_prepared=True skips weight packing / time tables (legal while the parameter block and grid are
        unchanged since the previous launch of this call).  auto_reuse=True (opt-in: evaluation epochs over frozen parameters) lets
        the call set the flag itself from the second launch on while the parameter block's version counter has not moved - the
        counter does NOT see writes through an alias (`p.data`, the per-parameter views of the arena an optimizer steps on), so a
        call that lives across optimizer steps must not use it.  The prepare launch is ~8 us of a 200 us K2 solve."""
        stream = torch.cuda.current_stream(self.ys.device) if stream is None else stream
        capturing = torch.cuda.is_current_stream_capturing()
        key = self._prepared_key()
        if auto_reuse and not reuse_prepared and not capturing and getattr(self, '_prep_key', None) == key:
            reuse_prepared = True
        self.desc.flags = self.base_flags | (_lib.FLAG_REUSE_PREPARED if reuse_prepared else 0)
        _lib.check(_lib.lib().snsde_solve_forward_at(C.byref(self.desc), C.c_int64(self.step_offset), C.c_void_p(stream.cuda_stream)),
                   'snsde_solve_forward_at')
        if not capturing:             # a recorded prepare launch has not run: it prepared nothing an eager launch could reuse
            self._prep_key = key
        return self.ys


def lean_variant(call):
    """Which instantiation of the lean kernel the forward of a SolveCall (or a _lib.Solve descriptor) launches: 'general' (the field's options tested at run time),
    'specialised' (compiled for exactly those options, csrc/snsde_m4_kernel.h: CfgSpec) or 'none' (another kernel)."""
    return _lib.LEAN_VARIANTS[_lib.lib().snsde_lean_variant(C.byref(_desc(call)))]


def _desc(call_or_desc):
    return call_or_desc.desc if hasattr(call_or_desc, 'desc') else call_or_desc


def forward_kernel(call_or_desc, keys=False, ensemble_nets=False, ensemble_nets_grad=False):
    """Name of the exact kernel the forward of a SolveCall (or a _lib.Solve descriptor) launches (_lib.FWD_KERNELS: the
    enumerators of csrc/snsde_mfma_kernels.h FwdKernel, 'generic', 'generic_srk' or 'none'); forward_path folds several of them into
    one family.  keys=True: (name, NHID, KUXT) - the plan's keys of the two-tile kernels' instantiation lists, -1 off the MFMA routes.
    ensemble_nets=True / ensemble_nets_grad=True: the answer for the descriptor with SNSDE_FLAG_ENSEMBLE_NETS /
    SNSDE_FLAG_ENSEMBLE_NETS_GRAD set (a copy; the descriptor is left alone)."""
    nhid, kuxt = C.c_int32(), C.c_int32()
    desc = _desc(call_or_desc)
    if ensemble_nets or ensemble_nets_grad:
        desc = type(desc).from_buffer_copy(desc)
        desc.flags |= _option_flags(dict(ensemble_nets=ensemble_nets, ensemble_nets_grad=ensemble_nets_grad).get)
    name = _lib.FWD_KERNELS[_lib.lib().snsde_forward_kernel(C.byref(desc), C.byref(nhid), C.byref(kuxt))]
    return (name, nhid.value, kuxt.value) if keys else name


def backward_kernel(call_or_desc):
    """Name of the exact adjoint kernel of a SolveCall (or a _lib.Solve descriptor): _lib.REV_KERNELS - the enumerators of
    csrc/snsde_mfma_kernels.h RevKernel where backward_supported is 1, 'generic' where it is 2, 'none' where it is 0."""
    return _lib.REV_KERNELS[_lib.lib().snsde_backward_kernel(C.byref(_desc(call_or_desc)))]


def backward_supported(call):
    """0 = no fused backward; 1 = MFMA adjoint kernel (needs save_act); 2 = generic adjoint kernel (forward must run
    on the generic kernel; needs traj + dW_out only)."""
    return int(_lib.lib().snsde_backward_supported(C.byref(call.desc)))


class _BoundedCache(dict):
    """Memo of host-side library queries per configuration; one entry per distinct (batch, knots, steps, outputs, ...) a process
    solves - dropped wholesale past `cap` entries (ragged last batches of many lengths must not grow it without bound)."""
    cap = 4096

    def __setitem__(self, k, v):
        if len(self) >= self.cap:
            self.clear()
        super().__setitem__(k, v)


_MODE_CACHE = _BoundedCache()
_SIZE_CACHE = _BoundedCache()      # host-side size queries of the library per configuration (SolveCall.config)


def backward_mode(model, batch, knots, grid, method, kernel='auto', exact_order=False, table=False, kl_column=None, global_rows=0,
                  samples=0, sample_grad=False, precision='fp32', bf16_grad=False, members=0, ensemble_grad=False,
                  ensemble_samples=False, ensemble_nets=False, ensemble_nets_grad=False):
    """backward_supported for a solve that has not been allocated yet (memoised per configuration); table: the solve
    supplies a noise_table; global_rows: the rows of the whole problem the solve is a batch shard of (0: none); samples: paths
    per input row (`batch` counts paths) - 0 without sample_grad (SNSDE_FLAG_SAMPLE_GRAD).  precision='bf16': 0, or under bf16_grad
    (SNSDE_FLAG_BF16_GRAD) 1 where the bf16 lean kernel runs the forward and the general MFMA adjoint its backward.  members: models
    in the call (`batch` counts the rows of all of them) - 0 without ensemble_grad (SNSDE_FLAG_ENSEMBLE_GRAD), 1 or 0 with it.  members and
    samples together: 0 unless ensemble_samples (SNSDE_FLAG_ENSEMBLE_SAMPLES), ensemble_grad and sample_grad are all set.
    ensemble_nets / ensemble_nets_grad (SNSDE_FLAG_ENSEMBLE_NETS / SNSDE_FLAG_ENSEMBLE_NETS_GRAD): with ensemble_grad, 1 where the
    ensemble runs on the wave pairs and each member's adjoint is the fused wave-pair adjoint; without all three, as above."""
    # (no lean_general and no training planes: neither moves the adjoint's plan; no row_offset: the caller has checked global_rows
    #  against it)
    cfg = SolveConfig.of(model, batch, knots, grid.N, grid.T, method, kernel, precision, exact_order=exact_order, sample_grad=sample_grad,
                         bf16_grad=bf16_grad, ensemble_grad=ensemble_grad, ensemble_samples=ensemble_samples, ensemble_nets=ensemble_nets,
                         ensemble_nets_grad=ensemble_nets_grad, samples=samples, members=members, global_rows=global_rows,
                         noise_table=table, kl_column=kl_column)
    hit = _MODE_CACHE.get(cfg)
    if hit is None:
        hit = _MODE_CACHE[cfg] = int(_lib.lib().snsde_backward_supported(C.byref(_describe(cfg))))
    return hit


def adj0_suffices(call):
    """The MFMA adjoint + native weight-gradient pass of this solve never read the intermediate adjoints from memory (all but
    Milstein through a diffusion net, whose second-order weight-gradient jobs do)."""
    return not (call.desc.method == _lib.MILSTEIN and call.model.noise_option in (14, 15, 18, 19))


def _backward_setup(call, adj=None, delta=None, adj0_only=False, want_delta=False, want_table_grad=False, want_grad=False):
    """What the three backward entry points share: the _lib.Backward bound to the solve's descriptor (with its base flags) and the
    buffers it names.  Returns (descriptor, adj, delta, table gradient, parameter gradient):
      adj    the caller's, else (N + 1, B, H) - (1, B, H) under adj0_only (BWD_ADJ0_ONLY)
      delta  the caller's, else under want_delta the (passes, delta slots, B, H) planes of snsde_save_layout - None at 0 slots (the
             adjoint of such a solve sums the weight gradients itself, include/snsde.h)
      table gradient (want_table_grad: solves with a supplied noise_table)  zeros (N, H); SRK: one row per stage time, (4 N, H)
      parameter gradient (want_grad)  numel floats; an ensemble: (M, numel)"""
    dev = call.traj.device
    b = _lib.Backward()
    b.fwd = call.desc
    b.fwd.flags = call.base_flags
    if adj is None:
        adj = torch.empty_like(call.traj[:1]) if adj0_only else torch.empty_like(call.traj)
        b.flags = _lib.BWD_ADJ0_ONLY if adj0_only else 0
    if delta is None and want_delta and call.delta_slots != 0:
        passes, _, B, H = call.act_save.shape
        delta = torch.empty((passes, call.delta_slots, B, H), device=dev, dtype=torch.float32)
    b.adj, b.delta_save = _ptr(adj), _ptr(delta)
    tab_grad = grad = None
    if want_table_grad:
        rows = call.grid.N * (4 if call.config.method == 'srk' else 1)
        tab_grad = torch.zeros((rows, call.model.hidden_channels), device=dev, dtype=torch.float32)
        b.grad_noise_table = _ptr(tab_grad)
    if want_grad:
        flat = call.keep[0]
        grad = torch.empty(tuple(flat.shape) if call.members > 1 else flat.numel(), device=dev, dtype=torch.float32)
    return b, adj, delta, tab_grad, grad


def solve_backward(call, grad_ys, stream=None, save_delta=False, adj0_only=False):
    """Adjoint recursion over a finished training-mode solve (SolveCall with save_traj/save_dW/save_act):
    returns adj (N+1, B, H), adj[n] = dL/dy_n; adj[0] is the gradient w.r.t. y0.  adj0_only (MFMA adjoint kernels, mode 1,
    not Milstein through a diffusion net): adj is (1, B, H) - the intermediate adjoints stay on chip."""
    if call.traj is None:
        raise ValueError('backward needs a solve run with save_traj (and save_act on the MFMA path)')
    _check_f32('grad_ys', grad_ys, tuple(call.ys.shape))
    b, adj, delta, _, _ = _backward_setup(call, adj0_only=adj0_only, want_delta=save_delta and call.act_save is not None)
    b.grad_ys = _ptr(grad_ys)
    nbytes = _lib.lib().snsde_backward_workspace_bytes(C.byref(b))
    ws = torch.empty(max(nbytes, 256), device=adj.device, dtype=torch.uint8)
    b.workspace, b.workspace_bytes = _ptr(ws), ws.numel()
    stream = torch.cuda.current_stream(adj.device) if stream is None else stream
    if call.step_offset:      # a continued solve (resume_grad): the adjoint regenerates the increments of the global steps
        _lib.check(_lib.lib().snsde_solve_backward_at(C.byref(b), C.c_int64(call.step_offset), C.c_void_p(stream.cuda_stream)),
                   'snsde_solve_backward_at')
    else:
        _lib.check(_lib.lib().snsde_solve_backward(C.byref(b), C.c_void_p(stream.cuda_stream)), 'snsde_solve_backward')
    call.keep_bwd = (ws, grad_ys)
    call.bwd_desc = b
    return (adj, delta) if save_delta else adj


def param_gradients(call, adj, delta, stream=None, want_table_grad=False):
    """Flat parameter gradient (the C ABI's layout) of a finished MFMA-path solve + adjoint: snsde_param_gradients
    (split-R MFMA weight-gradient GEMMs, diffusion reductions, first-layer algebra), all on the device.
    want_table_grad (solves with a supplied noise_table): returns (grad, dL/d noise_table (N, H); SRK: (4 N, H))."""
    b, _, _, tab_grad, grad = _backward_setup(call, adj=adj, delta=delta, want_table_grad=want_table_grad, want_grad=True)
    bws = call.keep_bwd[0]          # the adjoint's workspace: holds its per-workgroup diffusion-side sums
    b.workspace, b.workspace_bytes = _ptr(bws), bws.numel()
    L = _lib.lib()
    nbytes = L.snsde_param_gradients_workspace_bytes(C.byref(b))
    if nbytes == 0:
        raise NotImplementedError('snsde_param_gradients covers the MFMA-path configurations only')
    ws = torch.empty(nbytes, device=adj.device, dtype=torch.uint8)
    stream = torch.cuda.current_stream(adj.device) if stream is None else stream
    _lib.check(L.snsde_param_gradients(C.byref(b), _ptr(grad), _ptr(ws), ws.numel(), C.c_void_p(stream.cuda_stream)),
               'snsde_param_gradients')
    call.keep_pg = (ws, adj, delta, tab_grad)
    return (grad, tab_grad) if want_table_grad else grad


def backward_with_gradients(call, grad_ys, stream=None, adj0_only=True, want_table_grad=False, return_delta=False):
    """solve_backward + param_gradients as ONE C call (snsde_backward_with_gradients; mode 1 solves): same results, one
    host -> library transition.  Returns (adj, flat gradient[, dL/d noise_table]); return_delta appends the delta planes the
    adjoint left (None where the solve has none) - what coeff_gradients reads."""
    if call.traj is None or call.act_save is None:
        raise ValueError('backward needs a solve run with save_traj and save_act')
    _check_f32('grad_ys', grad_ys, tuple(call.ys.shape))
    dev = call.traj.device
    b, adj, delta, tab_grad, grad = _backward_setup(call, adj0_only=adj0_only, want_delta=True, want_table_grad=want_table_grad, want_grad=True)
    b.grad_ys = _ptr(grad_ys)
    L = _lib.lib()
    key = ('bwd', adj0_only, want_table_grad, call.config)
    sizes = _SIZE_CACHE.get(key)
    if sizes is None:
        b.workspace, b.workspace_bytes = C.c_void_p(16), 1 << 40      # (only its presence matters to the size queries)
        sizes = _SIZE_CACHE[key] = (max(int(L.snsde_backward_workspace_bytes(C.byref(b))), 256),
                                    int(L.snsde_param_gradients_workspace_bytes(C.byref(b))))
    if sizes[1] == 0:
        raise NotImplementedError('snsde_backward_with_gradients covers the MFMA-path configurations only')
    ws = torch.empty(sizes[0], device=dev, dtype=torch.uint8)
    b.workspace, b.workspace_bytes = _ptr(ws), ws.numel()
    pws = torch.empty(sizes[1], device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    if call.step_offset:      # a continued solve (resume_grad): the adjoint regenerates the increments of the global steps
        _lib.check(L.snsde_backward_with_gradients_at(C.byref(b), _ptr(grad), _ptr(pws), pws.numel(), C.c_int64(call.step_offset),
                                                      C.c_void_p(stream.cuda_stream)), 'snsde_backward_with_gradients_at')
    else:
        _lib.check(L.snsde_backward_with_gradients(C.byref(b), _ptr(grad), _ptr(pws), pws.numel(), C.c_void_p(stream.cuda_stream)),
                   'snsde_backward_with_gradients')
    call.keep_bwd = (ws, grad_ys)
    call.keep_pg = (pws, adj, delta, tab_grad)
    call.bwd_desc = b
    out = (adj, grad, tab_grad) if want_table_grad else (adj, grad)
    return out + (delta,) if return_delta else out


def coeff_gradients(call, adj, delta, stream=None):
    """dL/d coeffs (B, L-1, 4C; a sampled solve: one row per INPUT row, the sum over its paths) of a finished mode-1 solve + adjoint (solve_backward with save_delta, or backward_with_gradients
    with return_delta): snsde_coeff_gradients on the delta planes, enqueue-only.  `adj` is the adjoint call's result (kept
    alive with the planes).  SnsdeError -4 for a solve without delta planes (call.delta_slots == 0) and every other
    configuration the entry point does not cover (include/snsde.h)."""
    b = getattr(call, 'bwd_desc', None)
    if b is None:
        raise ValueError('coeff_gradients needs the adjoint of this solve first (solve_backward / backward_with_gradients)')
    b.delta_save = _ptr(delta)
    coeffs = call.keep[1]
    L = _lib.lib()
    key = ('cgrad', call.config)
    nbytes = _SIZE_CACHE.get(key)
    if nbytes is None:
        nbytes = _SIZE_CACHE[key] = int(L.snsde_coeff_gradients_workspace_bytes(C.byref(b)))
    ws = torch.empty(max(nbytes, 256), device=coeffs.device, dtype=torch.uint8)
    grad = torch.empty_like(coeffs)
    stream = torch.cuda.current_stream(coeffs.device) if stream is None else stream
    _lib.check(L.snsde_coeff_gradients(C.byref(b), _ptr(grad), _ptr(ws), ws.numel(), C.c_void_p(stream.cuda_stream)),
               'snsde_coeff_gradients')
    call.keep_cg = (ws, adj, delta)
    return grad


def initial_state(weight, bias, coeffs, grid):
    """weight . X(ts[0]) + bias, (B, H), through the device code a fused z0_linear solve starts from (snsde_initial_state): the
    same bits as that solve's own initial state, which the tensor-op form `linear(X.evaluate(ts[0]))` only approximates.  weight
    (H, C), bias (H), coeffs (B, L-1, 4C): contiguous float32 CUDA tensors; grid: the solve's StepGrid."""
    H, C_ = weight.shape
    B, L = coeffs.shape[0], coeffs.shape[1] + 1
    _check_f32('z0 weight', weight, (H, C_))
    _check_f32('z0 bias', bias, (H,))
    _check_f32('coeffs', coeffs, (B, L - 1, 4 * C_))
    y0 = torch.empty((B, H), device=coeffs.device, dtype=torch.float32)
    s = _lib.Solve()
    s.model.hidden_channels, s.model.input_channels = H, C_
    s.batch, s.knots = B, L
    s.coeffs, s.step_tab, s.y0 = _ptr(coeffs), _ptr(grid.d_step_tab), _ptr(y0)
    s.z0_weight, s.z0_bias = _ptr(weight), _ptr(bias)
    stream = torch.cuda.current_stream(coeffs.device)
    _lib.check(_lib.lib().snsde_initial_state(C.byref(s), C.c_void_p(stream.cuda_stream)), 'snsde_initial_state')
    return y0


def eval_fg(model, flat_params, coeffs, times_host, t, y, kernel='auto'):
    """f(t, y), g(t, y) through the solver's device code (snsde_eval_fg)."""
    B, H = y.shape
    L = coeffs.shape[1] + 1
    dev = y.device
    t = float(np.float32(t))
    # one-row step table for time t (h is irrelevant here); nextafter keeps ts increasing
    ts = np.array([t, np.nextafter(np.float32(t), np.float32(np.inf)) + np.float32(1.0)], dtype=np.float32)
    g = StepGrid(ts, 2.0 + abs(t), times_host, dev)
    s = _lib.Solve()
    s.model = model
    s.batch, s.knots, s.n_steps, s.n_out = B, L, 1, 2
    s.kernel = _lib.KERNELS[kernel]
    s.params, s.coeffs = _ptr(flat_params), _ptr(coeffs)
    nbytes = _lib.lib().snsde_workspace_bytes(C.byref(s))
    ws = torch.empty(max(nbytes, 256), device=dev, dtype=torch.uint8)
    s.workspace, s.workspace_bytes = _ptr(ws), ws.numel()
    f = torch.empty_like(y)
    gg = torch.empty_like(y)
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().snsde_eval_fg(C.byref(s), _ptr(g.d_step_tab), _ptr(y), _ptr(f), _ptr(gg),
                                        C.c_void_p(stream.cuda_stream)), 'snsde_eval_fg')
    return f, gg


def head_layers(seq):
    """(input_tanh, linear1, batchnorm or None, linear2) when `seq` is one of the wrappers' readout heads in a state the
    fused head reproduces - [Tanh,] Linear, [BatchNorm1d on running statistics,] ReLU, [Dropout in eval mode,] Linear - else
    None (benchmark_classification/models_sde/neuralsde.py:59-61; benchmark_forecasting/...:153-155; torch_ists nsde_model)."""
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else None
    if not mods:
        return None
    tanh = isinstance(mods[0], torch.nn.Tanh)
    if tanh:
        mods = mods[1:]
    if len(mods) < 3 or not isinstance(mods[0], torch.nn.Linear) or not isinstance(mods[-1], torch.nn.Linear):
        return None
    lin1, lin2, mid = mods[0], mods[-1], mods[1:-1]
    bn = None
    if isinstance(mid[0], torch.nn.BatchNorm1d):
        bn, mid = mid[0], mid[1:]
        if bn.training or bn.running_mean is None:
            return None
    if not mid or not isinstance(mid[0], torch.nn.ReLU):
        return None
    for m in mid[1:]:
        if not (isinstance(m, torch.nn.Dropout) and (not m.training or m.p == 0.0)):
            return None
    if lin2.in_features != lin1.out_features or (bn is not None and bn.num_features != lin1.out_features):
        return None
    if lin1.out_features > 128 or lin1.in_features > 256:
        # wider heads: the library GEMM chain is faster (measured 27 vs 42 us at 1280 x 256 x 256 x 14; the kernel itself
        # takes hidden sizes up to 512)
        return None
    return tanh, lin1, bn, lin2


def readout_head(x, layers, stream=None):
    """out = linear2(relu(bn(linear1(act(x))))) over the last dimension of x in ONE launch (snsde_readout_head); inference
    only - the caller checks torch.is_grad_enabled().  `layers` = (input_tanh, linear1, batchnorm or None, linear2)."""
    tanh, lin1, bn, lin2 = layers
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    _check_f32('head input', x2, (x2.shape[0], lin1.in_features))
    out = torch.empty((x2.shape[0], lin2.out_features), device=x.device, dtype=torch.float32)
    h = _lib.Head()
    h.rows, h.in_features, h.hidden, h.out_features = x2.shape[0], lin1.in_features, lin1.out_features, lin2.out_features
    h.input_tanh = 1 if tanh else 0
    keep = [x2, lin1.weight.detach().contiguous(), lin2.weight.detach().contiguous()]
    h.x, h.w1, h.w2, h.out = _ptr(x2), _ptr(keep[1]), _ptr(keep[2]), _ptr(out)
    h.b1 = _ptr(None if lin1.bias is None else lin1.bias.detach())
    h.b2 = _ptr(None if lin2.bias is None else lin2.bias.detach())
    if bn is not None:
        h.bn_eps = float(bn.eps)
        h.bn_mean, h.bn_var = _ptr(bn.running_mean), _ptr(bn.running_var)
        h.bn_weight = _ptr(None if bn.weight is None else bn.weight.detach())
        h.bn_bias = _ptr(None if bn.bias is None else bn.bias.detach())
    stream = torch.cuda.current_stream(x.device) if stream is None else stream
    _lib.check(_lib.lib().snsde_readout_head(C.byref(h), C.c_void_p(stream.cuda_stream)), 'snsde_readout_head')
    return out.reshape(*lead, lin2.out_features)


def sample_stats(ys, samples, var=True, log_weight=None):
    """Mean and unbiased variance over the sample axis of a sampled solve's result (sdeint options={'samples': S}): ys is
    (..., B S, H) with path index b S + s; returns (mean, var), each (..., B, H) (var None when var=False).  CUDA float32 input:
    one launch of snsde_sample_stats (one lane per output element walks its S samples in order, twice: deterministic) - inside an
    autograd node whose backward is snsde_sample_stats_backward when the input requires grad; other tensors: the same two passes
    in torch, which autograd differentiates.
    log_weight (..., B, S) - a particle filter's log-weights, `FilterResult.log_weight` against `filter_particles` of its states -
    makes them the weighted mean sum w_n x_n and the reliability-weights unbiased variance sum w_n (x_n - mean)^2 / D',
    D' = sum w_n (1 - w_n), w = softmax(log_weight): see `sample_stats_weighted_tensor_ops` for the definitions (dead samples,
    unusable weight sets; a single live sample gives var = 0 / 0 = NaN).  The weights carry no gradient."""
    if log_weight is not None:
        return _sample_stats_weighted(ys, samples, var, log_weight)
    S = check_samples(samples)
    if ys.dim() < 2 or ys.shape[-2] % S:
        raise ValueError(f'ys has shape {tuple(ys.shape)}: its second-to-last axis must hold a whole number of groups of {S} paths')
    if var and S < 2:
        raise ValueError('the unbiased variance needs samples >= 2')
    W = ys.shape[-1]
    out_shape = tuple(ys.shape[:-2]) + (ys.shape[-2] // S, W)
    if ys.is_cuda and ys.dtype == torch.float32 and ys.numel() > 0 and ys.requires_grad and torch.is_grad_enabled():
        mean, vout = _SampleStats.apply(ys, S, bool(var))      # (the kernels below inside one autograd node)
        return mean, (vout if var else None)
    if not (ys.is_cuda and ys.dtype == torch.float32) or ys.numel() == 0:
        v = ys.reshape(out_shape[:-1] + (S, W))
        mean = v.sum(dim=-2) / S
        return mean, ((v - mean.unsqueeze(-2)).square().sum(dim=-2) / (S - 1) if var else None)
    ys = ys.contiguous()
    mean = torch.empty(out_shape, device=ys.device, dtype=torch.float32)
    vout = torch.empty(out_shape, device=ys.device, dtype=torch.float32) if var else None
    _lib.check(_lib.lib().snsde_sample_stats(_ptr(ys), ys.numel() // (S * W), S, W, _ptr(mean), _ptr(vout),
                                             C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)), 'snsde_sample_stats')
    return mean, vout


def sample_stats_backward(grad_mean, grad_var, ys, mean, samples):
    """dL/d ys of `sample_stats` from dL/d mean and dL/d var (None: no variance term): one launch of snsde_sample_stats_backward.
    ys (..., B S, H), mean / grad_mean / grad_var (..., B, H): contiguous float32 CUDA tensors."""
    S, W = int(samples), ys.shape[-1]
    _check_f32('ys', ys)
    _check_f32('grad_mean', grad_mean, tuple(ys.shape[:-2]) + (ys.shape[-2] // S, W))
    if grad_var is not None:
        _check_f32('grad_var', grad_var, tuple(grad_mean.shape))
        _check_f32('mean', mean, tuple(grad_mean.shape))
    out = torch.empty_like(ys)
    _lib.check(_lib.lib().snsde_sample_stats_backward(_ptr(grad_mean), _ptr(grad_var), _ptr(ys), _ptr(mean if grad_var is not None else None),
                                                      ys.numel() // (S * W), S, W, _ptr(out),
                                                      C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_stats_backward')
    return out


class _SampleStats(torch.autograd.Function):
    """sample_stats of a CUDA float32 tensor that requires grad: the forward kernel, and snsde_sample_stats_backward as its backward."""

    @staticmethod
    def forward(ctx, ys, S, var):
        ysc = ys.detach().contiguous()
        with torch.no_grad():
            mean, vout = sample_stats(ysc, S, var)
        ctx.S, ctx.var = S, var
        ctx.save_for_backward(ysc, mean)
        if not var:
            vout = mean.new_empty(0)
            ctx.mark_non_differentiable(vout)
        return mean, vout

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mean, grad_var):
        ys, mean = ctx.saved_tensors
        gm = torch.zeros_like(mean) if grad_mean is None else grad_mean.to(torch.float32).contiguous()
        gv = grad_var.to(torch.float32).contiguous() if ctx.var and grad_var is not None else None
        return sample_stats_backward(gm, gv, ys, mean, ctx.S), None, None


def ensemble_stats(ys, members, samples, within=True, between=True):
    """Predictive mean and the two parts of the predictive variance of a sampled ensemble solve (sdeint_ensemble with
    options={'samples': S, 'ensemble_samples': True}): ys is (..., M, B S, W) - the (T, M, B S, H) result, or a stacked (M, B S, out)
    readout - with path index b S + s inside a member.  Returns (mean, within, between), each (..., B, W):
        mean_m, var_m   member m's mean and unbiased variance over its S paths (sample_stats of member m: the same bits)
        mean            their mean over the members
        within          the mean of var_m: the aleatoric part, the spread of the noise (None when within=False)
        between         the unbiased variance of mean_m over the members: the epistemic part (None when between=False)
    and within + between is the law-of-total-variance estimate.  CUDA float32 input: one launch of snsde_ensemble_stats (one lane
    per output element walks members and samples in order: deterministic) - inside an autograd node whose backward is
    snsde_ensemble_stats_backward when the input requires grad; other tensors: the same sums in torch."""
    S = check_samples(samples)
    if isinstance(members, bool) or not isinstance(members, int) or members < 1:
        raise ValueError(f'members must be an integer >= 1 (models of the ensemble), got {members!r}')
    M = members
    if ys.dim() < 3 or ys.shape[-3] != M or ys.shape[-2] % S:
        raise ValueError(f'ys has shape {tuple(ys.shape)}: expected (..., members, rows, width) with members = {M} and a whole number '
                         f'of groups of {S} paths per member')
    if within and S < 2:
        raise ValueError('the within-member variance needs samples >= 2')
    if between and M < 2:
        raise ValueError('the between-member variance needs members >= 2')
    W, G = ys.shape[-1], ys.shape[-2] // S
    lead = tuple(ys.shape[:-3])
    out_shape = lead + (G, W)
    native = ys.is_cuda and ys.dtype == torch.float32 and ys.numel() > 0
    if native and ys.requires_grad and torch.is_grad_enabled():
        mean, wout, bout = _EnsembleStats.apply(ys, M, S, bool(within), bool(between))      # (the kernels below inside one autograd node)
        return mean, (wout if within else None), (bout if between else None)
    if not native:
        v = ys.reshape(lead + (M, G, S, W))
        mm = v.sum(dim=-2) / S
        mean = mm.sum(dim=-3) / M
        wout = ((v - mm.unsqueeze(-2)).square().sum(dim=-2) / (S - 1)).sum(dim=-3) / M if within else None
        bout = (mm - mean.unsqueeze(-3)).square().sum(dim=-3) / (M - 1) if between else None
        return mean, wout, bout
    ys = ys.contiguous()
    outer = ys.numel() // (M * G * S * W)
    mean = torch.empty(out_shape, device=ys.device, dtype=torch.float32)
    wout = torch.empty(out_shape, device=ys.device, dtype=torch.float32) if within else None
    bout = torch.empty(out_shape, device=ys.device, dtype=torch.float32) if between else None
    _lib.check(_lib.lib().snsde_ensemble_stats(_ptr(ys), outer, M, G, S, W, _ptr(mean), _ptr(wout), _ptr(bout),
                                               C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)), 'snsde_ensemble_stats')
    return mean, wout, bout


def ensemble_stats_backward(grad_mean, grad_within, grad_between, ys, members, samples):
    """dL/d ys of `ensemble_stats` from dL/d mean, dL/d within and dL/d between (None: no such term): one launch of
    snsde_ensemble_stats_backward.  ys (..., M, B S, W), the gradients (..., B, W): contiguous float32 CUDA tensors."""
    M, S, W = int(members), int(samples), ys.shape[-1]
    _check_f32('ys', ys)
    G = ys.shape[-2] // S
    shape = tuple(ys.shape[:-3]) + (G, W)
    for name, g in (('grad_mean', grad_mean), ('grad_within', grad_within), ('grad_between', grad_between)):
        if g is not None:
            _check_f32(name, g, shape)
    out = torch.empty_like(ys)
    _lib.check(_lib.lib().snsde_ensemble_stats_backward(_ptr(grad_mean), _ptr(grad_within), _ptr(grad_between), _ptr(ys),
                                                        ys.numel() // (M * G * S * W), M, G, S, W, _ptr(out),
                                                        C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_ensemble_stats_backward')
    return out


class _EnsembleStats(torch.autograd.Function):
    """ensemble_stats of a CUDA float32 tensor that requires grad: the forward kernel, and snsde_ensemble_stats_backward as its backward."""

    @staticmethod
    def forward(ctx, ys, M, S, within, between):
        ysc = ys.detach().contiguous()
        with torch.no_grad():
            mean, wout, bout = ensemble_stats(ysc, M, S, within, between)
        ctx.M, ctx.S, ctx.within, ctx.between = M, S, within, between
        ctx.save_for_backward(ysc)
        if not within:
            wout = mean.new_empty(0)
            ctx.mark_non_differentiable(wout)
        if not between:
            bout = mean.new_empty(0)
            ctx.mark_non_differentiable(bout)
        return mean, wout, bout

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mean, grad_within, grad_between):
        ys, = ctx.saved_tensors
        gm = None if grad_mean is None else grad_mean.to(torch.float32).contiguous()
        gw = grad_within.to(torch.float32).contiguous() if ctx.within and grad_within is not None else None
        gb = grad_between.to(torch.float32).contiguous() if ctx.between and grad_between is not None else None
        return ensemble_stats_backward(gm, gw, gb, ys, ctx.M, ctx.S), None, None, None, None


SCORE_MAX_POOLED = 256      # pooled samples N = members * samples the score kernels stage in LDS (csrc/snsde_sample_set.h: MAX_N)
SCORE_MAX_QUANTILES = 8     # quantile levels per launch (they travel in the kernel's argument struct)


def _score_dims(ys, samples, members):
    """(S, M, lead, G, W) of a result scored over its sample paths: ys (..., B S, W) for members = 1, (..., M, B S, W) otherwise."""
    S = check_samples(samples)
    if isinstance(members, bool) or not isinstance(members, int) or members < 1:
        raise ValueError(f'members must be an integer >= 1 (models of the ensemble), got {members!r}')
    M = members
    if M == 1:
        if ys.dim() < 2 or ys.shape[-2] % S:
            raise ValueError(f'ys has shape {tuple(ys.shape)}: its second-to-last axis must hold a whole number of groups of {S} paths')
        lead = tuple(ys.shape[:-2])
    else:
        if ys.dim() < 3 or ys.shape[-3] != M or ys.shape[-2] % S:
            raise ValueError(f'ys has shape {tuple(ys.shape)}: expected (..., members, rows, width) with members = {M} and a whole '
                             f'number of groups of {S} paths per member')
        lead = tuple(ys.shape[:-3])
    return S, M, lead, ys.shape[-2] // S, ys.shape[-1]


def _pooled(ys, S, M, lead, G, W):
    """The pooled sample sets as a tensor (..., G, N, W), n = m S + s (a view where members = 1)."""
    if M == 1:
        return ys.reshape(lead + (G, S, W))
    return ys.reshape(lead + (M, G, S, W)).movedim(-4, -3).reshape(lead + (G, M * S, W))


def _score_native(ys, N, *others):
    return (ys.is_cuda and ys.dtype == torch.float32 and ys.numel() > 0 and N <= SCORE_MAX_POOLED
            and all(o.is_cuda and o.dtype == torch.float32 and o.device == ys.device for o in others))


def _outer(lead):
    n = 1
    for e in lead:
        n *= e
    return n


def sample_crps(ys, samples, target, fair=True, members=1, rank=False, log_weight=None):
    """Continuous ranked probability score of the sample paths of a solve against an observation.  ys is (..., B S, W) - a
    sampled solve's result, path index b S + s - or, with members = M > 1, (..., M, B S, W): the paths of all members are pooled
    into one sample set x_n, n = m S + s, N = M S (the predictive mixture whose variance `ensemble_stats` splits).  target y is
    (..., B, W).  With d_n = x_n - y, the strict counts c_n = #{x_j < x_n} - #{x_j > x_n} and D = N - 1 (fair: the unbiased
    estimator, N >= 2) or D = N,
        crps = sum |d_n| / N - sum c_n d_n / (N D)        (= mean |x - y| - sum_ij |x_i - x_j| / (2 N D))
    of shape (..., B, W); with rank=True returns (crps, rank, ties), rank = #{x_n < y} and ties = #{x_n == y} as float32 (for the
    PIT / rank histogram; no gradient).  Differentiable in ys and target, sign(0) = 0.  The comparisons are IEEE (a NaN sample
    counts in no c_n, in neither rank nor ties) and NaN / +-Inf flow through the formula as written, in the one element whose
    set holds them: a diverged path turns its own score into NaN and no other.
    CUDA float32 inputs with N <= 256: one launch of snsde_sample_crps (the (N, 64-column) slab of a group staged in LDS, no
    (.., S, S, ..) intermediate, deterministic, capturable) - inside an autograd node whose backward is snsde_sample_crps_backward
    when an input requires grad.  Other tensors: the same definitions in tensor ops, the counts from a sort.
    log_weight (..., B, N), one log-weight per pooled path n = m S + s, scores the weighted sample set: with w = softmax(log_weight),
    C_n = sum_j w_j [x_j < x_n] - sum_j w_j [x_j > x_n] and D = D' = sum w_n (1 - w_n) (fair) or 1,
        crps = sum w_n |d_n| - sum w_n C_n d_n / D        (= E_w |X - y| - sum_ij w_i w_j |x_i - x_j| / (2 D))
    and rank / ties become the weighted PIT pieces sum w_n [x_n < y], sum w_n [x_n == y] in [0, 1]: see
    `sample_crps_weighted_tensor_ops`.  The weights carry no gradient."""
    if log_weight is not None:
        return _sample_crps_weighted(ys, samples, target, fair, members, rank, log_weight)
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N, out_shape = M * S, lead + (G, W)
    if tuple(target.shape) != out_shape:
        raise ValueError(f'target has shape {tuple(target.shape)}, expected {out_shape} (one observation per input row and column)')
    if fair and N < 2:
        raise ValueError('the fair (unbiased) score needs at least 2 pooled samples')
    fair, rank = bool(fair), bool(rank)
    if _score_native(ys, N, target):
        if (ys.requires_grad or target.requires_grad) and torch.is_grad_enabled():
            crps, rk, ti = _SampleCRPS.apply(ys, target, S, M, fair, rank)
        else:
            crps, rk, ti = _sample_crps_launch(ys.contiguous(), target.contiguous(), S, M, fair, rank)
        return (crps, rk, ti) if rank else crps
    return sample_crps_tensor_ops(ys, S, target, fair, M, rank)


def sample_crps_tensor_ops(ys, samples, target, fair=True, members=1, rank=False):
    """`sample_crps` stated in tensor ops (any device and dtype; autograd differentiates it): the strict counts c_n come from a
    sort of each column, so there is no (.., N, N, ..) intermediate.  What `sample_crps` runs off the kernels' domain."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    x = _pooled(ys, S, M, lead, G, W)
    D = N - 1 if fair else N
    d = x - target.unsqueeze(-2)
    with torch.no_grad():      # (integers: no gradient)
        xt = x.transpose(-1, -2).contiguous()
        xs = torch.sort(xt, dim=-1).values
        c = (torch.searchsorted(xs, xt, right=False) + torch.searchsorted(xs, xt, right=True) - N).transpose(-1, -2).to(d.dtype)
    crps = d.abs().sum(dim=-2) / N - (c * d).sum(dim=-2) / (N * D)
    if not rank:
        return crps
    with torch.no_grad():
        return crps, (d < 0).sum(dim=-2).to(torch.float32), (d == 0).sum(dim=-2).to(torch.float32)


def _sample_crps_launch(ys, target, S, M, fair, rank):
    G, W = ys.shape[-2] // S, ys.shape[-1]
    crps = torch.empty_like(target)
    rk = torch.empty_like(target) if rank else None
    ti = torch.empty_like(target) if rank else None
    _lib.check(_lib.lib().snsde_sample_crps(_ptr(ys), _ptr(target), ys.numel() // (M * G * S * W), M, G, S, W, int(fair), _ptr(crps),
                                            _ptr(rk), _ptr(ti), C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_crps')
    return crps, rk, ti


def sample_crps_backward(grad_crps, ys, target, samples, fair=True, members=1, grad_target=True):
    """(dL/d ys, dL/d target) of `sample_crps` from dL/d crps: one launch of snsde_sample_crps_backward (dL/d target None when
    grad_target=False).  Contiguous float32 CUDA tensors, ys (..., B S, W) or (..., M, B S, W), the others (..., B, W)."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    _check_f32('ys', ys)
    _check_f32('target', target, lead + (G, W))
    _check_f32('grad_crps', grad_crps, lead + (G, W))
    gys = torch.empty_like(ys)
    gt = torch.empty_like(target) if grad_target else None
    _lib.check(_lib.lib().snsde_sample_crps_backward(_ptr(grad_crps), _ptr(ys), _ptr(target), _outer(lead), M, G, S, W, int(bool(fair)),
                                                     _ptr(gys), _ptr(gt), C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_crps_backward')
    return gys, gt


class _SampleCRPS(torch.autograd.Function):
    """sample_crps of CUDA float32 tensors of which one requires grad: the forward kernel, and snsde_sample_crps_backward as its backward."""

    @staticmethod
    def forward(ctx, ys, target, S, M, fair, rank):
        ysc, tc = ys.detach().contiguous(), target.detach().contiguous()
        crps, rk, ti = _sample_crps_launch(ysc, tc, S, M, fair, rank)
        ctx.S, ctx.M, ctx.fair = S, M, fair
        ctx.save_for_backward(ysc, tc)
        if not rank:
            rk, ti = crps.new_empty(0), crps.new_empty(0)
        ctx.mark_non_differentiable(rk, ti)
        return crps, rk, ti

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_crps, grad_rank, grad_ties):
        ys, target = ctx.saved_tensors
        g = torch.zeros_like(target) if grad_crps is None else grad_crps.to(torch.float32).contiguous()
        gys, gt = sample_crps_backward(g, ys, target, ctx.S, ctx.fair, ctx.M, grad_target=ctx.needs_input_grad[1])
        return (gys if ctx.needs_input_grad[0] else None), gt, None, None, None, None


_CDIST_MAX_PLANE = 2 ** 23     # distances per torch.cdist call of `sample_energy_tensor_ops`


def _energy_dims(ys, samples, target, fair, members, path):
    """(S, M, lead, G, W, N, result shape) of an energy score; the shape errors of `sample_energy`."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    if tuple(target.shape) != lead + (G, W):
        raise ValueError(f'target has shape {tuple(target.shape)}, expected {lead + (G, W)} (one observed vector per input row)')
    if fair and N < 2:
        raise ValueError('the fair (unbiased) score needs at least 2 pooled samples')
    return S, M, lead, G, W, N, ((G,) if path else lead + (G,))


def sample_energy(ys, samples, target, fair=True, members=1, path=False, log_weight=None, mask=None):
    """Energy score of the sample paths of a solve against an observation: the multivariate generalisation of the CRPS, which
    also sees the dependence between the components of the vector.  ys, samples, members and target (..., B, W) as for
    `sample_crps`; the pooled samples x_n of an input row are vectors: of the W components of the last axis (path=False: the
    result is (..., B)), or of ALL leading axes by W (path=True: the whole path as one vector, the result is (B,); ys is
    addressed in place, never permuted).  With D = N - 1 (fair: the unbiased estimator, N >= 2) or D = N,
        energy = sum_n ||x_n - y|| / N - sum_{n<j} ||x_n - x_j|| / (N D)
    every distance from differences (never a Gram matrix).  Differentiable in ys and target, d||d|| = d / ||d|| and 0 at d = 0.
    CUDA float32 inputs with N <= 256: one launch of snsde_sample_energy (no (.., N, N) intermediate, deterministic, capturable)
    - inside an autograd node whose backward is snsde_sample_energy_backward when an input requires grad.  Other tensors:
    `sample_energy_tensor_ops`.
    log_weight (..., B, N) - under path (B, N): one log-weight per pooled path of a score - scores the weighted sample set: with
    w = softmax(log_weight) and D = D' = sum w_n (1 - w_n) (fair) or 1,
        energy = sum_n w_n ||x_n - y|| - sum_{n<j} w_n w_j ||x_n - x_j|| / D
    with the dead samples and unusable weight sets of `normalised_weights`; the weights carry no gradient.  mask marks the
    observed coordinates of a target with gaps: a tensor of the shape of target (bool, or a number: observed where != 0 - a
    fractional value does not weigh), or 'nan' for "a NaN target is a gap".  Every norm is then taken over the observed
    coordinates only; an unobserved one is selected out, never multiplied: NaN / Inf there in ys or target reaches nothing, and
    the gradients there are exact zeros.  A score with nothing observed is 0.  mask=None is the call as it always was: a NaN
    target poisons its score.  Either argument routes CUDA float32 inputs with N <= 256 to snsde_sample_energy_weighted / _backward
    and everything else to `sample_energy_weighted_tensor_ops`.  A particle filter's result r scores as
        sample_energy(filter_particles(r.ys, r.ancestor, S), S, target, log_weight=r.log_weight)"""
    if log_weight is not None or mask is not None:
        return _sample_energy_weighted(ys, samples, target, fair, members, path, log_weight, mask)
    fair, path = bool(fair), bool(path)
    S, M, lead, G, W, N, out_shape = _energy_dims(ys, samples, target, fair, members, path)
    if _score_native(ys, N, target):
        if (ys.requires_grad or target.requires_grad) and torch.is_grad_enabled():
            return _SampleEnergy.apply(ys, target, S, M, fair, path)
        return _sample_energy_launch(ys.contiguous(), target.contiguous(), S, M, fair, path)
    return sample_energy_tensor_ops(ys, S, target, fair, M, path)


def sample_energy_tensor_ops(ys, samples, target, fair=True, members=1, path=False):
    """`sample_energy` stated in tensor ops (any device and dtype; autograd differentiates it): torch.linalg.vector_norm of the
    differences to the observation and torch.cdist in its direct-difference mode - an (.., N, N) plane, no (.., N, N, V) tensor.
    What `sample_energy` runs off the kernels' domain, and the baseline the kernels are timed against."""
    fair, path = bool(fair), bool(path)
    S, M, lead, G, W, N, out_shape = _energy_dims(ys, samples, target, fair, members, path)
    if ys.numel() == 0:
        return ys.new_zeros(out_shape)
    x, y = _pooled(ys, S, M, lead, G, W), target                        # (..., G, N, W), (..., G, W)
    if path:      # every leading axis joins the vector: (G, N, outer W)
        O = _outer(lead)
        x = x.reshape(O, G, N, W).permute(1, 2, 0, 3).reshape(G, N, O * W)
        y = y.reshape(O, G, W).permute(1, 0, 2).reshape(G, O * W)
    D = N - 1 if fair else N
    a = torch.linalg.vector_norm(x - y.unsqueeze(-2), dim=-1).sum(dim=-1) / N
    # torch.cdist's direct kernel launches one 256-thread block per distance and HIP bounds a grid at 2^32 threads: 2^23
    # distances per call (the groups are independent, so the slices change no value)
    flat = x.reshape((-1, N, x.shape[-1]))
    step = max(1, _CDIST_MAX_PLANE // (N * N))
    sums = [torch.cdist(flat[i:i + step], flat[i:i + step], compute_mode='donot_use_mm_for_euclid_dist').sum(dim=(-2, -1))
            for i in range(0, flat.shape[0], step)]
    b = (sums[0] if len(sums) == 1 else torch.cat(sums)).reshape(a.shape) / (2 * N * D)
    return a - b


def _sample_energy_launch(ys, target, S, M, fair, path):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    energy = torch.empty((G,) if path else lead + (G,), device=ys.device, dtype=torch.float32)
    _lib.check(_lib.lib().snsde_sample_energy(_ptr(ys), _ptr(target), _outer(lead), M, G, S, W, int(fair), int(path), _ptr(energy),
                                              C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)), 'snsde_sample_energy')
    return energy


def sample_energy_backward(grad_energy, ys, target, samples, fair=True, members=1, path=False, grad_target=True):
    """(dL/d ys, dL/d target) of `sample_energy` from dL/d energy: one launch of snsde_sample_energy_backward (dL/d target None
    when grad_target=False).  Contiguous float32 CUDA tensors, ys (..., B S, W) or (..., M, B S, W), target (..., B, W), grad_energy
    (..., B) or, under path, (B,)."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    _check_f32('ys', ys)
    _check_f32('target', target, lead + (G, W))
    _check_f32('grad_energy', grad_energy, (G,) if path else lead + (G,))
    gys = torch.empty_like(ys)
    gt = torch.empty_like(target) if grad_target else None
    _lib.check(_lib.lib().snsde_sample_energy_backward(_ptr(grad_energy), _ptr(ys), _ptr(target), _outer(lead), M, G, S, W, int(bool(fair)),
                                                       int(bool(path)), _ptr(gys), _ptr(gt),
                                                       C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_energy_backward')
    return gys, gt


class _SampleEnergy(torch.autograd.Function):
    """sample_energy of CUDA float32 tensors of which one requires grad: the forward kernel, and snsde_sample_energy_backward as its backward."""

    @staticmethod
    def forward(ctx, ys, target, S, M, fair, path):
        ysc, tc = ys.detach().contiguous(), target.detach().contiguous()
        ctx.S, ctx.M, ctx.fair, ctx.path = S, M, fair, path
        ctx.save_for_backward(ysc, tc)
        return _sample_energy_launch(ysc, tc, S, M, fair, path)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_energy):
        ys, target = ctx.saved_tensors
        gys, gt = sample_energy_backward(grad_energy.to(torch.float32).contiguous(), ys, target, ctx.S, ctx.fair, ctx.M, ctx.path,
                                         grad_target=ctx.needs_input_grad[1])
        return (gys if ctx.needs_input_grad[0] else None), gt, None, None, None, None


def _loglik_args(ys, samples, target, mask, std, members, log_weight):
    """(S, M, lead, G, W, N, mask, logvar, inv_var) of a masked likelihood; the argument errors of `sample_loglik`.  mask=None is
    ~isnan(target) as float32; a bool mask becomes float32.  logvar = 2 log(std) and inv_var = exp(-logvar) in double."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    if tuple(target.shape) != lead + (G, W):
        raise ValueError(f'target has shape {tuple(target.shape)}, expected {lead + (G, W)} (one observed vector per input row)')
    if mask is None:
        mask = (~torch.isnan(target)).to(torch.float32)
    elif tuple(mask.shape) != lead + (G, W):
        raise ValueError(f'mask has shape {tuple(mask.shape)}, expected {lead + (G, W)} (the shape of target)')
    elif not mask.dtype.is_floating_point:
        mask = mask.to(torch.float32)
    if isinstance(std, bool) or not isinstance(std, (int, float, np.integer, np.floating)) or not math.isfinite(std) or std <= 0:
        raise ValueError(f'std must be a finite number > 0 (the standard deviation of the observation noise), got {std!r}')
    if log_weight is not None and tuple(log_weight.shape) != (G, N):
        raise ValueError(f'log_weight has shape {tuple(log_weight.shape)}, expected {(G, N)} (one log importance weight per input '
                         f'row and pooled sample)')
    logvar = 2.0 * math.log(float(std))
    return S, M, lead, G, W, N, mask, logvar, math.exp(-logvar)


def sample_loglik(ys, samples, target, mask=None, std=0.1, members=1, log_weight=None, norm=False, stats=False, log_std=None):
    """Masked Gaussian log-likelihood of the sample paths of a solve against a partially observed target, and its
    importance-weighted (IWAE) bound: the objective that trains options={'samples': S} on data with gaps.  ys is
    (..., B S, W) or (..., M, B S, W) as for `sample_energy(path=True)`: the pooled samples x_n (n = m S + s, N = M S) of an
    input row are vectors of ALL leading axes by W, component v, addressed in place.  target y and mask m are (..., B, W); an
    element is observed where m_v != 0, and mask=None means ~isnan(target) as float32.  std > 0 is the scalar standard deviation
    of the observation noise, logvar = 2 log(std) (in double).
        logpx[b, n] = sum_{v observed} m_v (-1/2) (log 2 pi + logvar + (y_v - x_nv)^2 / var)                  (B, N)
        count[b]    = sum_{v observed} m_v                                                                    (B,)
        norm=True:    logpx[b, .] / count[b] where count[b] > 0, and 0 where count[b] == 0 (the reference's args.norm would give
                      0 / 0 there: a deliberate difference)
        bound[b]    = logsumexp_n(logpx[b, n] + log_weight[b, n]) - log N                                     (B,)
        sqerr[b]    = sum_{v observed} m_v (y_v - mean_n x_nv)^2      (the numerator of the masked MSE of the sample mean: divide
                      by count; a metric, no gradient - like rank in `sample_crps`)
    log_weight (B, N) is an optional log importance weight: -kl_coef * kl of the reference's objective, or the per-path KL
    column of the latent route; None is 0.  Returns bound, or (bound, logpx, count, sqerr) with stats=True.
    Select, never multiply: an element with m_v == 0 is never read into a sum - it contributes an exact +0 and receives an
    exact-zero gradient, whatever target or ys hold there.  NaN-marked targets (the convention of torchcde and of
    natural_cubic_spline_coeffs) are accepted as they are; the reference multiplies by the mask and needs them zero-filled.
    Fractional mask values act as weights.  A NaN in an observed element of path n makes logpx[b, n], bound[b] and sqerr[b] NaN
    and touches no other row.  Differentiable in ys, target and log_weight; not in mask or a float std.
    CUDA float32 inputs with N <= 256: one launch of snsde_sample_loglik (the slab read once, no intermediate, deterministic,
    capturable) - inside an autograd node whose backward is snsde_sample_loglik_backward when an input requires grad.  Other
    tensors: `sample_loglik_tensor_ops`.
    Noise per channel or per entry, learned or known.  std may be a tensor instead, or log_std = log(std) may be given - the
    parametrisation of a learnable parameter; exactly one of them describes the noise, so log_std together with a std other than
    the default float is a ValueError.  With W = ys.shape[-1] the tensor is (W,): per channel, component v = o W + w of the vector
    uses entry w; or the shape of target (..., B, W): per entry, a known error bar for every measurement; a 0-dim tensor is the
    (W,) vector of that one value.  With ls_v the log-std of component v of row b,
        logpx[b, n] = sum_{v observed} m_v (-1/2) (log 2 pi + 2 ls_v + (y_v - x_nv)^2 exp(-2 ls_v))
    and count, norm, bound, sqerr, log_weight and members as above.  The call is differentiable in the noise tensor too:
    d logpx[b, n] / d ls_v = m_v ((y_v - x_nv)^2 exp(-2 ls_v) - 1); a tensor std enters as std.log() in tensor ops, so autograd
    chains through it.  Select, never multiply covers the noise: at an unobserved element ls_v is never read into a sum - NaN
    or Inf there reaches no value and no gradient - and its own gradient is an exact +0; a NaN ls_v at an observed element makes
    the logpx and bound of the rows that observe it NaN and no other.  A tensor std must be > 0: that is checked for a CPU
    tensor, where the check costs no device synchronisation, and NOT for a CUDA tensor - a std <= 0 there gives NaN (or, at 0,
    infinite) results in the rows that observe it, like any NaN ls_v.  log_std is never checked.
    CUDA float32 tensors on one device with N <= 256 run snsde_sample_loglik_noise, and snsde_sample_loglik_noise_backward
    (followed, for a per-channel tensor, by snsde_sample_loglik_noise_reduce: a fixed-order column sum) as the backward; everything
    else `sample_loglik_tensor_ops`.  A float std with log_std=None is the scalar call above: its code path, kernel and bits."""
    norm, stats = bool(norm), bool(stats)
    if log_std is not None or isinstance(std, torch.Tensor):
        return _sample_loglik_noise(ys, samples, target, mask, std, members, log_weight, norm, stats, log_std)
    S, M, lead, G, W, N, mask, logvar, inv_var = _loglik_args(ys, samples, target, mask, std, members, log_weight)
    others = (target, mask) if log_weight is None else (target, mask, log_weight)
    if _score_native(ys, N, *others):
        if any(t.requires_grad for t in (ys,) + others) and torch.is_grad_enabled():
            out = _SampleLoglik.apply(ys, target, mask, log_weight, S, M, logvar, inv_var, norm)
        else:
            out = _sample_loglik_launch(ys.contiguous(), target.contiguous(), mask.contiguous(),
                                        None if log_weight is None else log_weight.contiguous(), S, M, logvar, inv_var, norm)
        return out if stats else out[0]
    return sample_loglik_tensor_ops(ys, S, target, mask, std, M, log_weight, norm, stats)


def sample_loglik_tensor_ops(ys, samples, target, mask=None, std=0.1, members=1, log_weight=None, norm=False, stats=False,
                             log_std=None):
    """`sample_loglik` stated in tensor ops (any device and dtype; autograd differentiates it): torch.where on the mask selects
    the observed residuals - never a product with the mask - so NaN and Inf at unobserved positions reach neither a value nor a
    gradient; a tensor std / log_std is selected the same way.  What `sample_loglik` runs off the kernels' domain, and the
    baseline the kernels are timed against."""
    norm, stats = bool(norm), bool(stats)
    noise = log_std is not None or isinstance(std, torch.Tensor)
    if noise:
        ls, entry = _loglik_noise_arg(std, log_std, target)
        std = LOGLIK_DEFAULT_STD
    S, M, lead, G, W, N, mask, logvar, inv_var = _loglik_args(ys, samples, target, mask, std, members, log_weight)
    O = _outer(lead)
    x = _pooled(ys, S, M, lead, G, W).reshape(O, G, N, W).permute(1, 2, 0, 3).reshape(G, N, O * W)      # (G, N, V)
    y = target.to(x.dtype).reshape(O, G, W).permute(1, 0, 2).reshape(G, 1, O * W)
    m = mask.detach().to(x.dtype).reshape(O, G, W).permute(1, 0, 2).reshape(G, 1, O * W)
    obs = m != 0
    d = torch.where(obs, y - x, x.new_zeros(()))                                  # (G, N, V): exact zeros where unobserved
    if noise:
        lsv = ls.to(x.dtype)
        lsv = lsv.reshape(O, G, W).permute(1, 0, 2).reshape(G, 1, O * W) if entry else lsv.expand(O, W).reshape(1, 1, O * W)
        lsv = torch.where(obs, lsv, x.new_zeros(()))                              # (G, 1, V): selected like the residuals
        logpx = (-0.5 * m * ((math.log(2.0 * math.pi) + 2.0 * lsv) + d * d * torch.exp(-2.0 * lsv))).sum(dim=-1)
    else:
        logpx = (-0.5 * m * ((math.log(2.0 * math.pi) + logvar) + d * d * inv_var)).sum(dim=-1)
    count = m.sum(dim=-1)                                                         # (G, 1)
    if norm:
        some = count > 0
        logpx = torch.where(some, logpx / torch.where(some, count, torch.ones_like(count)), logpx.new_zeros(()))
    a = logpx if log_weight is None else logpx + log_weight.to(x.dtype)
    bound = torch.logsumexp(a, dim=-1) - math.log(N)
    if not stats:
        return bound
    with torch.no_grad():      # (a metric)
        e = d.mean(dim=1)
        sqerr = (m[:, 0] * e * e).sum(dim=-1)
    return bound, logpx, count[:, 0], sqerr


def _sample_loglik_launch(ys, target, mask, logw, S, M, logvar, inv_var, norm):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    N = M * S
    logpx = torch.empty((G, N), device=ys.device, dtype=torch.float32)
    count, bound, sqerr = (torch.empty((G,), device=ys.device, dtype=torch.float32) for _ in range(3))
    _lib.check(_lib.lib().snsde_sample_loglik(_ptr(ys), _ptr(target), _ptr(mask), _ptr(logw), _outer(lead), M, G, S, W, logvar, inv_var,
                                              int(norm), _ptr(logpx), _ptr(count), _ptr(bound), _ptr(sqerr),
                                              C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)), 'snsde_sample_loglik')
    return bound, logpx, count, sqerr


def sample_loglik_backward(grad_logpx, grad_bound, ys, target, mask, logpx, count, samples, std=0.1, members=1, log_weight=None,
                           norm=False, grad_target=True, grad_log_weight=True):
    """(dL/d ys, dL/d target, dL/d log_weight) of `sample_loglik` from dL/d logpx (B, N) and dL/d bound (B,) - either may be None -
    and the forward's logpx and count: one launch of snsde_sample_loglik_backward.  dL/d target is None when grad_target=False,
    dL/d log_weight when grad_log_weight=False.  Contiguous float32 CUDA tensors, shapes as for `sample_loglik`."""
    S, M, lead, G, W, N, mask, logvar, inv_var = _loglik_args(ys, samples, target, mask, std, members, log_weight)
    _check_f32('ys', ys)
    _check_f32('target', target)
    _check_f32('mask', mask)
    _check_f32('logpx', logpx, (G, N))
    _check_f32('count', count, (G,))
    for name, t, shape in (('grad_logpx', grad_logpx, (G, N)), ('grad_bound', grad_bound, (G,)), ('log_weight', log_weight, (G, N))):
        if t is not None:
            _check_f32(name, t, shape)
    return _sample_loglik_backward_launch(grad_logpx, grad_bound, ys, target, mask, log_weight, logpx, count, S, M, logvar, inv_var,
                                          bool(norm), grad_target, grad_log_weight)


def _sample_loglik_backward_launch(grad_logpx, grad_bound, ys, target, mask, logw, logpx, count, S, M, logvar, inv_var, norm,
                                   grad_target, grad_logw):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    gys = torch.empty_like(ys)
    gt = torch.empty_like(target) if grad_target else None
    glw = torch.empty_like(logpx) if grad_logw else None
    _lib.check(_lib.lib().snsde_sample_loglik_backward(_ptr(grad_logpx), _ptr(grad_bound), _ptr(ys), _ptr(target), _ptr(mask), _ptr(logw),
                                                       _ptr(logpx), _ptr(count), _outer(lead), M, G, S, W, logvar, inv_var, int(norm),
                                                       _ptr(gys), _ptr(gt), _ptr(glw),
                                                       C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_loglik_backward')
    return gys, gt, glw


class _SampleLoglik(torch.autograd.Function):
    """sample_loglik of CUDA float32 tensors of which one requires grad: the forward kernel, and snsde_sample_loglik_backward as its
    backward (from the saved logpx and count).  count and sqerr carry no gradient; mask receives none."""

    @staticmethod
    def forward(ctx, ys, target, mask, logw, S, M, logvar, inv_var, norm):
        ysc, tc, mc = ys.detach().contiguous(), target.detach().contiguous(), mask.detach().contiguous()
        lw = None if logw is None else logw.detach().contiguous()
        bound, logpx, count, sqerr = _sample_loglik_launch(ysc, tc, mc, lw, S, M, logvar, inv_var, norm)
        ctx.S, ctx.M, ctx.logvar, ctx.inv_var, ctx.norm, ctx.has_logw = S, M, logvar, inv_var, norm, lw is not None
        ctx.save_for_backward(ysc, tc, mc, logpx, count, *(() if lw is None else (lw,)))
        ctx.mark_non_differentiable(count, sqerr)
        ctx.set_materialize_grads(False)
        return bound, logpx, count, sqerr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_bound, grad_logpx, grad_count, grad_sqerr):
        ys, target, mask, logpx, count = ctx.saved_tensors[:5]
        lw = ctx.saved_tensors[5] if ctx.has_logw else None
        gb = None if grad_bound is None else grad_bound.to(torch.float32).contiguous()
        gl = None if grad_logpx is None else grad_logpx.to(torch.float32).contiguous()
        gys, gt, glw = _sample_loglik_backward_launch(gl, gb, ys, target, mask, lw, logpx, count, ctx.S, ctx.M, ctx.logvar, ctx.inv_var,
                                                      ctx.norm, ctx.needs_input_grad[1], ctx.has_logw and ctx.needs_input_grad[3])
        return (gys if ctx.needs_input_grad[0] else None), gt, None, glw, None, None, None, None, None


LOGLIK_DEFAULT_STD = 0.1      # sample_loglik's std when the noise is a tensor (log_std, or a tensor std)


def _loglik_noise_arg(std, log_std, target):
    """(log_std, entry) of a tensor noise: log_std as a tensor of shape (W,) (entry False: per channel) or target's (entry True);
    the argument errors of the noise.  A 0-dim tensor is expanded to (W,)."""
    if log_std is not None:
        if isinstance(std, torch.Tensor) or isinstance(std, bool) or std != LOGLIK_DEFAULT_STD:
            raise ValueError(f'std and log_std both describe the observation noise: give one of them (std is {std!r} with log_std set)')
        if not isinstance(log_std, torch.Tensor) or not log_std.dtype.is_floating_point:
            raise ValueError(f'log_std must be a floating-point tensor (the log standard deviation of the observation noise), got '
                             f'{log_std!r}')
        ls = log_std
    else:
        if not std.dtype.is_floating_point:
            raise ValueError(f'a tensor std must be floating point, got {std.dtype}')
        if not std.is_cuda and not bool((std > 0).all()):      # (free on the host; a CUDA tensor is not read back)
            raise ValueError('a tensor std must be > 0 everywhere (the standard deviation of the observation noise)')
        ls = std.log()
    if target.dim() < 2:
        raise ValueError(f'target has shape {tuple(target.shape)}, expected (..., B, W)')
    W = target.shape[-1]
    if ls.dim() == 0:
        return ls.expand(W), False
    if tuple(ls.shape) == (W,):
        return ls, False
    if tuple(ls.shape) == tuple(target.shape):
        return ls, True
    raise ValueError(f'the noise tensor has shape {tuple(ls.shape)}, expected {(W,)} (per channel) or {tuple(target.shape)} (per '
                     f'entry: the shape of target)')


def _sample_loglik_noise(ys, samples, target, mask, std, members, log_weight, norm, stats, log_std):
    """`sample_loglik` with a tensor noise: the kernels' route or the tensor-op statement."""
    ls, entry = _loglik_noise_arg(std, log_std, target)
    S, M, lead, G, W, N, mask, _, _ = _loglik_args(ys, samples, target, mask, LOGLIK_DEFAULT_STD, members, log_weight)
    others = (target, mask, ls) if log_weight is None else (target, mask, ls, log_weight)
    if _score_native(ys, N, *others):
        if any(t.requires_grad for t in (ys,) + others) and torch.is_grad_enabled():
            out = _SampleLoglikNoise.apply(ys, target, mask, log_weight, ls, S, M, entry, norm)
        else:
            out = _sample_loglik_noise_launch(ys.contiguous(), target.contiguous(), mask.contiguous(),
                                              None if log_weight is None else log_weight.contiguous(), ls.contiguous(), S, M, entry, norm)
        return out if stats else out[0]
    return sample_loglik_tensor_ops(ys, S, target, mask, LOGLIK_DEFAULT_STD, M, log_weight, norm, stats, log_std=ls)


def _sample_loglik_noise_launch(ys, target, mask, logw, ls, S, M, entry, norm):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    N = M * S
    logpx = torch.empty((G, N), device=ys.device, dtype=torch.float32)
    count, bound, sqerr = (torch.empty((G,), device=ys.device, dtype=torch.float32) for _ in range(3))
    _lib.check(_lib.lib().snsde_sample_loglik_noise(_ptr(ys), _ptr(target), _ptr(mask), _ptr(logw), _ptr(ls), _outer(lead), M, G, S, W,
                                                    _lib.NOISE_ENTRY if entry else _lib.NOISE_CHANNEL, int(norm), _ptr(logpx), _ptr(count),
                                                    _ptr(bound), _ptr(sqerr), C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_loglik_noise')
    return bound, logpx, count, sqerr


def sample_loglik_noise_reduce(grad_entry):
    """The (W,) column sum of a per-entry gradient plane (..., B, W) in the fixed order of snsde_sample_loglik_noise_reduce: the
    rows in blocks of 64, each block ascending, then the blocks ascending.  A contiguous float32 CUDA tensor; the partial sums are
    allocated here (torch.empty), not by the library."""
    _check_f32('grad_entry', grad_entry)
    W = grad_entry.shape[-1]
    rows = grad_entry.numel() // W
    parts = -(-rows // _lib.LOGLIK_NOISE_REDUCE_ROWS)
    partial = torch.empty((parts, W), device=grad_entry.device, dtype=torch.float32) if parts > 1 else None
    out = torch.empty((W,), device=grad_entry.device, dtype=torch.float32)
    _lib.check(_lib.lib().snsde_sample_loglik_noise_reduce(_ptr(grad_entry), rows, W, _ptr(partial), _ptr(out),
                                                           C.c_void_p(torch.cuda.current_stream(grad_entry.device).cuda_stream)),
               'snsde_sample_loglik_noise_reduce')
    return out


def sample_loglik_noise_backward(grad_logpx, grad_bound, ys, target, mask, log_std, logpx, count, samples, members=1, log_weight=None,
                                 norm=False, grad_target=True, grad_log_weight=True, grad_log_std=True):
    """`sample_loglik_backward` for a tensor noise: (dL/d ys, dL/d target, dL/d log_weight, dL/d log_std) from dL/d logpx and
    dL/d bound and the forward's logpx and count, bypassing autograd: one launch of snsde_sample_loglik_noise_backward and, for a
    (W,) log_std, `sample_loglik_noise_reduce` of its per-entry plane.  dL/d log_std has log_std's shape (for a 0-dim log_std: (W,), the gradient of its expansion); each optional gradient
    is None when not wanted.  Contiguous float32 CUDA tensors; log_std is (W,) or target's shape."""
    ls, entry = _loglik_noise_arg(LOGLIK_DEFAULT_STD, log_std, target)
    ls = ls.contiguous()      # (a 0-dim log_std arrives as a stride-0 view of W elements)
    S, M, lead, G, W, N, mask, _, _ = _loglik_args(ys, samples, target, mask, LOGLIK_DEFAULT_STD, members, log_weight)
    _check_f32('ys', ys)
    _check_f32('target', target)
    _check_f32('mask', mask)
    _check_f32('log_std', ls)
    _check_f32('logpx', logpx, (G, N))
    _check_f32('count', count, (G,))
    for name, t, shape in (('grad_logpx', grad_logpx, (G, N)), ('grad_bound', grad_bound, (G,)), ('log_weight', log_weight, (G, N))):
        if t is not None:
            _check_f32(name, t, shape)
    return _sample_loglik_noise_backward_launch(grad_logpx, grad_bound, ys, target, mask, log_weight, ls, logpx, count, S, M, entry,
                                                bool(norm), grad_target, grad_log_weight, grad_log_std)


def _sample_loglik_noise_backward_launch(grad_logpx, grad_bound, ys, target, mask, logw, ls, logpx, count, S, M, entry, norm,
                                         grad_target, grad_logw, grad_ls):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    gys = torch.empty_like(ys)
    gt = torch.empty_like(target) if grad_target else None
    glw = torch.empty_like(logpx) if grad_logw else None
    gls = torch.empty_like(target) if grad_ls else None      # (the per-entry plane, in both modes)
    _lib.check(_lib.lib().snsde_sample_loglik_noise_backward(_ptr(grad_logpx), _ptr(grad_bound), _ptr(ys), _ptr(target), _ptr(mask),
                                                             _ptr(logw), _ptr(ls), _ptr(logpx), _ptr(count), _outer(lead), M, G, S, W,
                                                             _lib.NOISE_ENTRY if entry else _lib.NOISE_CHANNEL, int(norm), _ptr(gys),
                                                             _ptr(gt), _ptr(glw), _ptr(gls),
                                                             C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_loglik_noise_backward')
    if grad_ls and not entry:
        gls = sample_loglik_noise_reduce(gls)
    return gys, gt, glw, gls


class _SampleLoglikNoise(torch.autograd.Function):
    """sample_loglik with a tensor noise, of CUDA float32 tensors of which one requires grad: snsde_sample_loglik_noise, and
    snsde_sample_loglik_noise_backward (plus the fixed-order reduce for a per-channel log_std) as its backward, from the saved
    logpx and count.  count and sqerr carry no gradient; mask receives none."""

    @staticmethod
    def forward(ctx, ys, target, mask, logw, ls, S, M, entry, norm):
        ysc, tc, mc, lsc = (t.detach().contiguous() for t in (ys, target, mask, ls))
        lw = None if logw is None else logw.detach().contiguous()
        bound, logpx, count, sqerr = _sample_loglik_noise_launch(ysc, tc, mc, lw, lsc, S, M, entry, norm)
        ctx.S, ctx.M, ctx.entry, ctx.norm, ctx.has_logw = S, M, entry, norm, lw is not None
        ctx.save_for_backward(ysc, tc, mc, lsc, logpx, count, *(() if lw is None else (lw,)))
        ctx.mark_non_differentiable(count, sqerr)
        ctx.set_materialize_grads(False)
        return bound, logpx, count, sqerr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_bound, grad_logpx, grad_count, grad_sqerr):
        ys, target, mask, ls, logpx, count = ctx.saved_tensors[:6]
        lw = ctx.saved_tensors[6] if ctx.has_logw else None
        gb = None if grad_bound is None else grad_bound.to(torch.float32).contiguous()
        gl = None if grad_logpx is None else grad_logpx.to(torch.float32).contiguous()
        gys, gt, glw, gls = _sample_loglik_noise_backward_launch(gl, gb, ys, target, mask, lw, ls, logpx, count, ctx.S, ctx.M, ctx.entry,
                                                                 ctx.norm, ctx.needs_input_grad[1],
                                                                 ctx.has_logw and ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        return (gys if ctx.needs_input_grad[0] else None), gt, None, glw, gls, None, None, None, None


SampleClass = collections.namedtuple('SampleClass', 'nll xent logp probs entropy expected_entropy mutual_information')


def _class_args(logits, samples, labels, members, binary, class_weight, log_weight):
    """(S, M, lead, G, W, N, classes, labels) of a classification over sample paths; the argument errors of `sample_class`.
    labels come back as int32 (values beyond its range saturate, which keeps them out of range), or None."""
    S, M, lead, G, W = _score_dims(logits, samples, members)
    N = M * S
    if not logits.dtype.is_floating_point:
        raise ValueError(f'logits must be a floating-point tensor, got {logits.dtype}')
    if binary and W != 1:
        raise ValueError(f'binary=True takes one logit per path (a last axis of 1), got a last axis of {W}')
    classes = 2 if binary else W
    if labels is not None:
        if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise ValueError(f'labels must be an integer tensor of class indices (< 0: unlabelled), got {labels.dtype}')
        if tuple(labels.shape) != lead + (G,):
            raise ValueError(f'labels has shape {tuple(labels.shape)}, expected {lead + (G,)} (one label per input row)')
        if labels.dtype != torch.int32:
            labels = (labels.clamp(-1, 2 ** 31 - 1) if labels.dtype == torch.int64 else labels).to(torch.int32)
    if class_weight is not None and tuple(class_weight.shape) != (classes,):
        raise ValueError(f'class_weight has shape {tuple(class_weight.shape)}, expected {(classes,)} (one weight per class)')
    if log_weight is not None and tuple(log_weight.shape) != lead + (G, N):
        raise ValueError(f'log_weight has shape {tuple(log_weight.shape)}, expected {lead + (G, N)} (one log importance weight per '
                         f'input row and pooled path)')
    return S, M, lead, G, W, N, classes, labels


def sample_class(logits, samples, labels=None, members=1, binary=False, class_weight=None, log_weight=None, stats=False):
    """Classify with the sample paths of a solve: the predictive (Bayesian model average) negative log-likelihood of the labels,
    and the predictive distribution with its uncertainty split.  logits is (..., B S, C) - one row of class logits per path, path
    index b S + s - or, with members = M > 1, (..., M, B S, C): the N = M S paths of an input row are pooled, n = m S + s.
    binary=True: the last axis is 1 and the two class logits of a path are (0, z) (the BCE-with-logits layout).  labels is an
    integer tensor (..., B) (any integer dtype, converted once), < 0 marks an unlabelled row; None: no row is labelled (pure
    prediction).  With lp_n = log_softmax(z_n), a_n = lp_n[y], w = class_weight[y] (None: 1):
        nll[b]      = -w (logsumexp_n(a_n + log_weight[b, n]) - log N)    the loss whose mean trains the model average
        xent[b]     = -w mean_n a_n                                       the expected cross-entropy (the Jensen bound, >= nll)
        logp[b, n]  = a_n                                                 (..., B, N)
        probs[b, c] = mean_n softmax(z_n)[c]                              (..., B, C); binary: (..., B, 1), the class-1 probability
        entropy     = H[probs]                                            total uncertainty
        expected_entropy   = mean_n H[softmax(z_n)]                       the aleatoric part
        mutual_information = max(entropy - expected_entropy, 0)           the epistemic part (BALD)
    Returns nll, or the named tuple SampleClass(nll, xent, logp, probs, entropy, expected_entropy, mutual_information) with
    stats=True.  class_weight = (1, pos_weight) with binary=True reproduces BCEWithLogitsLoss(pos_weight) at S = 1.
    log_weight (..., B, N) is an optional log importance weight, as in `sample_loglik`.
    Every logsumexp subtracts its maximum; a -Inf logit is a class of probability zero with a zero gradient; an unlabelled row
    has nll = xent = logp = 0 and an exactly zero gradient while its probs and entropies are computed all the same; a label >= C
    gives NaN in that row's nll, xent, logp and gradient; a NaN logit poisons its own row only.
    Differentiable in logits and log_weight through nll, xent and logp.  probs, entropy, expected_entropy and
    mutual_information are returned detached (no gradient), and class_weight receives none.
    CUDA float32 inputs with N <= 256: one launch of snsde_sample_class (the slab read once and staged in LDS, deterministic,
    capturable) - inside an autograd node whose backward is snsde_sample_class_backward when an input requires grad.  Other
    tensors: `sample_class_tensor_ops`."""
    binary, stats = bool(binary), bool(stats)
    S, M, lead, G, W, N, classes, lab = _class_args(logits, samples, labels, members, binary, class_weight, log_weight)
    floats = tuple(t for t in (class_weight, log_weight) if t is not None)
    if _score_native(logits, N, *floats) and (lab is None or (lab.is_cuda and lab.device == logits.device)):
        if (logits.requires_grad or (log_weight is not None and log_weight.requires_grad)) and torch.is_grad_enabled():
            out = _SampleClass.apply(logits, lab, log_weight, class_weight, S, M, binary)
        else:
            out = _sample_class_launch(logits.contiguous(), None if lab is None else lab.contiguous(),
                                       None if log_weight is None else log_weight.contiguous(),
                                       None if class_weight is None else class_weight.contiguous(), S, M, binary)
        if not stats:
            return out[0]
        return SampleClass(*out, (out[4] - out[5]).clamp_min(0))
    return sample_class_tensor_ops(logits, S, lab, M, binary, class_weight, log_weight, stats)


def sample_class_tensor_ops(logits, samples, labels=None, members=1, binary=False, class_weight=None, log_weight=None, stats=False):
    """`sample_class` stated in tensor ops (any device and floating dtype; autograd differentiates it): log_softmax over the
    classes, logsumexp over the paths, torch.where for unlabelled rows.  What `sample_class` runs off the kernels' domain, and
    the baseline the kernels are timed against."""
    binary, stats = bool(binary), bool(stats)
    S, M, lead, G, W, N, classes, lab = _class_args(logits, samples, labels, members, binary, class_weight, log_weight)
    x = _pooled(logits, S, M, lead, G, W)                                          # (..., G, N, W)
    if binary:
        x = torch.cat([torch.zeros_like(x), x], dim=-1)
    lp = torch.log_softmax(x, dim=-1)                                              # (..., G, N, classes)
    zero = lp.new_zeros(())
    lab = torch.full(lead + (G,), -1, device=lp.device) if lab is None else lab.to(torch.int64)
    unlabelled, beyond = lab < 0, lab >= classes
    pick = lab.clamp(0, classes - 1)                                               # (selects; never out of range)
    a = lp.gather(-1, pick[..., None, None].expand(lead + (G, N, 1))).squeeze(-1)
    a = torch.where(beyond[..., None], lp.new_full((), float('nan')), a)
    logp = torch.where(unlabelled[..., None], zero, a)
    w = 1.0 if class_weight is None else class_weight.detach().to(lp.dtype)[pick]
    at = logp if log_weight is None else logp + log_weight.to(lp.dtype)
    nll = torch.where(unlabelled, zero, -w * (torch.logsumexp(at, dim=-1) - math.log(N)))
    xent = torch.where(unlabelled, zero, -w * logp.mean(dim=-1))
    if not stats:
        return nll
    with torch.no_grad():      # (metrics: no gradient)
        p = lp.exp()
        pbar = p.mean(dim=-2)
        entropy = -torch.special.xlogy(pbar, pbar).sum(dim=-1)
        expent = -torch.where(p == 0, zero, p * lp).sum(dim=-1).mean(dim=-1)
        probs = pbar[..., 1:] if binary else pbar
    return SampleClass(nll, xent, logp, probs, entropy, expent, (entropy - expent).clamp_min(0))


def _sample_class_launch(logits, labels, logw, cw, S, M, binary):
    S_, M_, lead, G, W = _score_dims(logits, S, M)
    N = M * S
    new = lambda *shape: torch.empty(lead + shape, device=logits.device, dtype=torch.float32)
    nll, xent, entropy, expent, logp, probs = new(G), new(G), new(G), new(G), new(G, N), new(G, W)
    _lib.check(_lib.lib().snsde_sample_class(_ptr(logits), _ptr(labels), _ptr(logw), _ptr(cw), _outer(lead), M, G, S, W, int(binary),
                                             _ptr(logp), _ptr(nll), _ptr(xent), _ptr(probs), _ptr(entropy), _ptr(expent),
                                             C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)), 'snsde_sample_class')
    return nll, xent, logp, probs, entropy, expent


def sample_class_backward(grad_nll, grad_xent, grad_logp, logits, samples, labels=None, members=1, binary=False, class_weight=None,
                          log_weight=None, grad_log_weight=True):
    """(dL/d logits, dL/d log_weight) of `sample_class` from dL/d nll (..., B), dL/d xent (..., B) and dL/d logp (..., B, N) - each
    may be None: one launch of snsde_sample_class_backward.  dL/d log_weight is None when grad_log_weight=False.  Contiguous
    float32 CUDA tensors (labels: a contiguous integer CUDA tensor), shapes as for `sample_class`."""
    S, M, lead, G, W, N, classes, lab = _class_args(logits, samples, labels, members, bool(binary), class_weight, log_weight)
    _check_f32('logits', logits)
    for name, t, shape in (('grad_nll', grad_nll, lead + (G,)), ('grad_xent', grad_xent, lead + (G,)), ('grad_logp', grad_logp, lead + (G, N)),
                           ('log_weight', log_weight, lead + (G, N)), ('class_weight', class_weight, (classes,))):
        if t is not None:
            _check_f32(name, t, shape)
    if lab is not None and not (lab.is_cuda and lab.is_contiguous()):
        raise ValueError('labels must be a contiguous integer CUDA tensor')
    return _sample_class_backward_launch(grad_nll, grad_xent, grad_logp, logits, lab, log_weight, class_weight, S, M, bool(binary),
                                         grad_log_weight)


def _sample_class_backward_launch(grad_nll, grad_xent, grad_logp, logits, labels, logw, cw, S, M, binary, grad_logw):
    S_, M_, lead, G, W = _score_dims(logits, S, M)
    gz = torch.empty_like(logits)
    glw = torch.empty(lead + (G, M * S), device=logits.device, dtype=torch.float32) if grad_logw else None
    _lib.check(_lib.lib().snsde_sample_class_backward(_ptr(grad_nll), _ptr(grad_xent), _ptr(grad_logp), _ptr(logits), _ptr(labels),
                                                      _ptr(logw), _ptr(cw), _outer(lead), M, G, S, W, int(binary), _ptr(gz), _ptr(glw),
                                                      C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)),
               'snsde_sample_class_backward')
    return gz, glw


class _SampleClass(torch.autograd.Function):
    """sample_class of CUDA float32 tensors of which one requires grad: the forward kernel, and snsde_sample_class_backward as its
    backward (the row statistics are formed again from the saved logits).  probs, entropy and expent carry no gradient; labels and
    class_weight receive none."""

    @staticmethod
    def forward(ctx, logits, labels, logw, cw, S, M, binary):
        zc = logits.detach().contiguous()
        lab = None if labels is None else labels.contiguous()
        lw = None if logw is None else logw.detach().contiguous()
        cwc = None if cw is None else cw.detach().contiguous()
        out = _sample_class_launch(zc, lab, lw, cwc, S, M, binary)
        ctx.S, ctx.M, ctx.binary = S, M, binary
        ctx.has = (lab is not None, lw is not None, cwc is not None)
        ctx.save_for_backward(zc, *(t for t in (lab, lw, cwc) if t is not None))
        ctx.mark_non_differentiable(*out[3:])
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_nll, grad_xent, grad_logp, *unused):
        saved = list(ctx.saved_tensors)
        zc = saved.pop(0)
        lab, lw, cwc = (saved.pop(0) if h else None for h in ctx.has)
        f = lambda g: None if g is None else g.to(torch.float32).contiguous()
        gz, glw = _sample_class_backward_launch(f(grad_nll), f(grad_xent), f(grad_logp), zc, lab, lw, cwc, ctx.S, ctx.M, ctx.binary,
                                                lw is not None and ctx.needs_input_grad[2])
        return (gz if ctx.needs_input_grad[0] else None), None, glw, None, None, None, None


SampleResample = collections.namedtuple('SampleResample', 'state log_weight ancestor ess logz resampled')


def _resample_args(state, samples, log_weight, log_increment, u, threshold, stratified, differentiable=False):
    """(S, lead, B, W, threshold) of a resampling step; the argument errors of `sample_resample`.  u=None is not checked."""
    S = check_samples(samples)
    if state.dim() < 2 or state.shape[-2] % S:
        raise ValueError(f'state has shape {tuple(state.shape)}: its second-to-last axis must hold a whole number of groups of {S} paths')
    lead, B, W = tuple(state.shape[:-2]), state.shape[-2] // S, state.shape[-1]
    if not state.dtype.is_floating_point or not log_weight.dtype.is_floating_point:
        raise ValueError(f'state and log_weight must be floating-point tensors, got {state.dtype} and {log_weight.dtype}')
    if tuple(log_weight.shape) != lead + (B, S):
        raise ValueError(f'log_weight has shape {tuple(log_weight.shape)}, expected {lead + (B, S)} (one carried log-weight per path)')
    if log_increment is not None and tuple(log_increment.shape) != lead + (B, S):
        raise ValueError(f'log_increment has shape {tuple(log_increment.shape)}, expected {lead + (B, S)} (the shape of log_weight)')
    want = lead + ((B, S) if stratified else (B,))
    if u is not None and tuple(u.shape) != want:
        raise ValueError(f'u has shape {tuple(u.shape)}, expected {want} (one uniform per ' + ('path' if stratified else 'group') +
                         f' with stratified={stratified})')
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or math.isnan(threshold):
        raise ValueError(f'threshold must be a number (resample where ess < threshold * samples; <= 0 never, >= 1 always), got {threshold!r}')
    tensors = [t for t in (state, log_weight, log_increment) if t is not None]
    if not differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise ValueError('sample_resample is inference only: state, log_weight or log_increment requires grad (use torch.no_grad() or '
                         'detach()); resampling has no backward')
    return S, lead, B, W, float(threshold)


def sample_resample(state, samples, log_weight, log_increment=None, u=None, threshold=0.5, stratified=False, generator=None,
                    differentiable=False):
    """One step of the bootstrap particle filter on the sample paths of a solve: weigh the S paths of every input row by the
    newest observation and resample them.  state is (..., B S, W) - the last state of a solve with options={'samples': S}, path
    b S + s; the leading axes (the members of an ensemble) fold into the groups, members are never pooled - log_weight (..., B, S)
    the carried log-weight and log_increment (..., B, S) the log-likelihood of the newest observation per path (None: 0; for
    example `sample_loglik(..., stats=True)`'s logpx of a readout).  With a = log_weight + log_increment, e_n = exp(a_n - max a)
    and P_n = e_0 + .. + e_n:
        logz[b] = logsumexp_n a_n - log S                                 ess[b] = P_{S-1}^2 / sum_n e_n^2
    A row is resampled where threshold >= 1, or where ess < threshold S (threshold <= 0: never):
        ancestor[b, j] = #{n < S-1 : P_n <= ((j + u_j) / S) P_{S-1}}      systematic: u_j = u[b]; stratified=True: u[b, j]
        state[b S + j] = state[b S + ancestor[b, j]]                       log_weight[b, j] = logz[b]
    and elsewhere ancestor is the identity, state a copy and log_weight = a.  Either way logsumexp(log_weight) - log S = logz: the
    returned weights carry the evidence, and handed to `sample_loglik` as log_weight they make its bound the running log marginal
    likelihood log p(y_1..k).  u (..., B) - stratified: (..., B, S) - holds uniforms in [0, 1); None draws torch.rand on the
    state's device with `generator`.  Returns SampleResample(state, log_weight, ancestor (int32), ess, logz, resampled (int32)).
    A path with e_n == 0 (a -Inf weight) is never an ancestor; a row whose a are all -Inf is left as it is with ess = 0 and
    logz = -Inf; a row with a NaN or +Inf in a is left as it is with ess = logz = NaN and touches no other row; state is only
    moved, NaN and Inf included.  By default inference only: an input that requires grad under enabled autograd is a ValueError.
    differentiable=True makes state, log_weight and logz differentiable in state, log_weight and log_increment with the
    ancestors held fixed: the ancestors, u and the threshold are constants of the backward,
        d state[b S + n] = sum_{j : ancestor[b, j] == n} d state_out[b S + j]
        d a[b, n]        = (d logz[b] + sum_j d log_weight_out[b, j]) softmax(a[b])_n      (not resampled: d log_weight_out[b, n] +
                                                                                            d logz[b] softmax(a[b])_n)
    which is the estimator of the filtering variational objectives (FIVO, Maddison et al. 2017): the score-function term of the
    resampling decision is dropped, so the gradient of E[logz] is biased wherever a row is resampled, with a far smaller
    variance.  A path with e_n == 0 receives exact zeros; a row left as it is for its NaN, +Inf or all -Inf weights passes its
    gradients through unchanged.  ess, ancestor and resampled carry no gradient.
    CUDA float32 inputs with S <= 256: one launch of snsde_sample_resample (deterministic for a given u, capturable with u a
    device tensor), and one of snsde_sample_resample_backward in the backward.  Other tensors: `sample_resample_tensor_ops`."""
    stratified, differentiable = bool(stratified), bool(differentiable)
    S, lead, B, W, threshold = _resample_args(state, samples, log_weight, log_increment, u, threshold, stratified, differentiable)
    if u is None:
        u = torch.rand(lead + ((B, S) if stratified else (B,)), device=state.device, dtype=log_weight.dtype, generator=generator)
    others = tuple(t for t in (log_weight, log_increment, u) if t is not None)
    if _score_native(state, S, *others):
        if differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in (state, log_weight, log_increment) if t is not None):
            return SampleResample(*_SampleResample.apply(state, log_weight, log_increment, u.detach(), S, threshold, stratified))
        return _sample_resample_launch(state.detach().contiguous(), log_weight.detach().contiguous(),
                                       None if log_increment is None else log_increment.detach().contiguous(), u.detach().contiguous(), S,
                                       threshold, stratified)
    return sample_resample_tensor_ops(state, S, log_weight, log_increment, u, threshold, stratified, differentiable=differentiable)


def sample_resample_tensor_ops(state, samples, log_weight, log_increment=None, u=None, threshold=0.5, stratified=False, generator=None,
                               differentiable=False):
    """`sample_resample` stated in tensor ops (any device and floating dtype): logsumexp, cumsum, searchsorted, gather and where.
    What `sample_resample` runs off the kernel's domain, and the baseline the kernel is timed against.  differentiable=True: the
    decision and the ancestors are formed from detached values as before, and state, log_weight and logz are then formed from the
    inputs themselves by gather, logsumexp and where, whose autograd is the backward `sample_resample` states."""
    stratified, differentiable = bool(stratified), bool(differentiable)
    S, lead, B, W, threshold = _resample_args(state, samples, log_weight, log_increment, u, threshold, stratified, differentiable)
    if u is None:
        u = torch.rand(lead + ((B, S) if stratified else (B,)), device=state.device, dtype=log_weight.dtype, generator=generator)
    G = _outer(lead) * B
    a = log_weight if log_increment is None else log_weight + log_increment.to(log_weight.dtype)
    a = a.detach().reshape(G, S)
    x = state.detach().reshape(G, S, W)
    uu = u.detach().to(a.dtype).reshape(G, S if stratified else 1)
    nan, inf = a.new_full((), float('nan')), float('inf')
    mx = a.max(dim=-1, keepdim=True).values
    bad = (torch.isnan(a) | (a == inf)).any(dim=-1)                   # a NaN or +Inf: the row is left as it is
    dead = ~bad & (mx[:, 0] == -inf)                                  # all -Inf
    kept = bad | dead
    e = torch.exp(a - torch.where(kept[:, None], torch.zeros_like(mx), mx))
    e = torch.where(kept[:, None], torch.ones_like(e), e)             # (a stand-in that keeps the arithmetic below finite)
    P = torch.cumsum(e, dim=-1)
    total = P[:, -1:]
    logz = torch.where(bad, nan, torch.logsumexp(torch.where(bad[:, None], torch.zeros_like(a), a), dim=-1) - math.log(S))
    ess = torch.where(bad, nan, torch.where(dead, torch.zeros_like(logz), total[:, 0] ** 2 / (e * e).sum(dim=-1)))
    res = ~kept & (ess < threshold * S if 0 < threshold < 1 else torch.full_like(kept, threshold >= 1))
    j = torch.arange(S, device=a.device)
    t = ((j.to(a.dtype) + uu) / S) * total                            # (G, S)
    count = torch.searchsorted(P[:, :S - 1].contiguous(), t.contiguous(), right=True) if S > 1 else torch.zeros_like(t, dtype=torch.int64)
    alive = e > 0                                                     # a path with e_n == 0 is never an ancestor
    first = alive.to(torch.int8).argmax(dim=-1, keepdim=True)
    last = S - 1 - alive.flip(-1).to(torch.int8).argmax(dim=-1, keepdim=True)
    anc = torch.where(res[:, None], torch.minimum(torch.maximum(count, first), last), j.expand(G, S))
    if differentiable:
        # the three differentiable outputs again, from the inputs with their graph: the same values (a masked row contributes the
        # constants it had above, and no gradient through logz: where() hands its unselected side an exact zero)
        x = state.reshape(G, S, W)
        ag = (log_weight if log_increment is None else log_weight + log_increment.to(log_weight.dtype)).reshape(G, S)
        lse = torch.logsumexp(torch.where(kept[:, None], torch.zeros_like(a), ag), dim=-1) - math.log(S)
        logz = torch.where(kept, logz, lse)
        a = ag
    out = x.gather(1, anc[:, :, None].expand(G, S, W))
    logw = torch.where(res[:, None], logz[:, None], a)
    return SampleResample(out.reshape(state.shape), logw.reshape(lead + (B, S)), anc.to(torch.int32).reshape(lead + (B, S)),
                          ess.reshape(lead + (B,)), logz.reshape(lead + (B,)), res.to(torch.int32).reshape(lead + (B,)))


def _sample_resample_launch(state, logw, loginc, u, S, threshold, stratified):
    lead, B, W = tuple(state.shape[:-2]), state.shape[-2] // S, state.shape[-1]
    G = _outer(lead) * B
    new = lambda shape, dtype: torch.empty(lead + shape, device=state.device, dtype=dtype)
    out, logw_out, anc = torch.empty_like(state), new((B, S), torch.float32), new((B, S), torch.int32)
    ess, logz, res = new((B,), torch.float32), new((B,), torch.float32), new((B,), torch.int32)
    _lib.check(_lib.lib().snsde_sample_resample(_ptr(state), _ptr(logw), _ptr(loginc), _ptr(u), G, S, W, int(stratified), threshold,
                                                _ptr(out), _ptr(logw_out), _ptr(anc), _ptr(ess), _ptr(logz), _ptr(res),
                                                C.c_void_p(torch.cuda.current_stream(state.device).cuda_stream)), 'snsde_sample_resample')
    return SampleResample(out, logw_out, anc, ess, logz, res)


def sample_resample_backward(grad_state, grad_log_weight, grad_logz, log_weight, log_increment, ancestor, resampled, samples):
    """(dL/d state, dL/d a) of `sample_resample(..., differentiable=True)` from dL/d of its state (..., B S, W), log_weight
    (..., B, S) and logz (..., B) - each may be None - and the step's log_weight, log_increment (None: 0), ancestor and resampled:
    one launch of snsde_sample_resample_backward.  dL/d a is the gradient of log_weight and of log_increment alike.  Contiguous
    float32 (ancestor, resampled: int32) CUDA tensors; the width W is read off grad_state, which may therefore not be None here
    unless `samples` is a pair (S, W)."""
    S, W = samples if isinstance(samples, tuple) else (samples, None if grad_state is None else grad_state.shape[-1])
    S = check_samples(S)
    if W is None:
        raise ValueError('grad_state is None: pass samples=(S, W) to state the width of the state')
    lead, B = tuple(log_weight.shape[:-2]), log_weight.shape[-2]
    _check_f32('log_weight', log_weight, lead + (B, S))
    for name, t, shape in (('grad_state', grad_state, lead + (B * S, W)), ('grad_log_weight', grad_log_weight, lead + (B, S)),
                           ('grad_logz', grad_logz, lead + (B,)), ('log_increment', log_increment, lead + (B, S))):
        if t is not None:
            _check_f32(name, t, shape)
    for name, t, shape in (('ancestor', ancestor, lead + (B, S)), ('resampled', resampled, lead + (B,))):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and tuple(t.shape) == shape):
            raise ValueError(f'{name} must be a contiguous int32 CUDA tensor of shape {shape}')
    return _sample_resample_backward_launch(grad_state, grad_log_weight, grad_logz, log_weight, log_increment, ancestor, resampled, S, W)


def _sample_resample_backward_launch(gso, glw, glz, logw, loginc, anc, res, S, W):
    lead, B = tuple(logw.shape[:-2]), logw.shape[-2]
    G = _outer(lead) * B
    gs = torch.empty(lead + (B * S, W), device=logw.device, dtype=torch.float32)
    ga = torch.empty_like(logw)
    _lib.check(_lib.lib().snsde_sample_resample_backward(_ptr(gso), _ptr(glw), _ptr(glz), _ptr(logw), _ptr(loginc), _ptr(anc), _ptr(res),
                                                         G, S, W, _ptr(gs), _ptr(ga),
                                                         C.c_void_p(torch.cuda.current_stream(logw.device).cuda_stream)),
               'snsde_sample_resample_backward')
    return gs, ga


class _SampleResample(torch.autograd.Function):
    """sample_resample(differentiable=True) of CUDA float32 tensors of which one requires grad: the forward kernel, and
    snsde_sample_resample_backward as its backward (the weights are formed again from the saved log_weight and log_increment;
    the ancestors are constants).  ancestor, ess and resampled carry no gradient; u receives none."""

    @staticmethod
    def forward(ctx, state, logw, loginc, u, S, threshold, stratified):
        lw = logw.detach().contiguous()
        inc = None if loginc is None else loginc.detach().contiguous()
        out = _sample_resample_launch(state.detach().contiguous(), lw, inc, u.contiguous(), S, threshold, stratified)
        ctx.S, ctx.W, ctx.has_inc = S, state.shape[-1], inc is not None
        ctx.save_for_backward(lw, out.ancestor, out.resampled, *(() if inc is None else (inc,)))
        ctx.mark_non_differentiable(out.ancestor, out.ess, out.resampled)
        ctx.set_materialize_grads(False)
        return tuple(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_state, grad_logw, unused_anc, unused_ess, grad_logz, unused_res):
        lw, anc, res = ctx.saved_tensors[:3]
        inc = ctx.saved_tensors[3] if ctx.has_inc else None
        f = lambda g: None if g is None else g.to(torch.float32).contiguous()
        gs, ga = _sample_resample_backward_launch(f(grad_state), f(grad_logw), f(grad_logz), lw, inc, anc, res, ctx.S, ctx.W)
        need = ctx.needs_input_grad
        return (gs if need[0] else None), (ga if need[1] else None), (ga if ctx.has_inc and need[2] else None), None, None, None, None


def filter_paths(ys, ancestors, samples):
    """The surviving trajectories of a particle filter.  ys (T, B S, H) holds the states BEFORE each resampling and ancestors
    (T, B, S) the resampling of each step (`sdeint_filter`'s ys and ancestor): slot p of ys[k + 1] continues slot
    ancestors[k][p] of ys[k].  Traced back from the last step - i_{T-1}[p] = p, i_k = ancestors[k][i_{k+1}] - the result
    (T, B S, H) holds ys[k][i_k[p]] in slot p: its last entry is ys[-1], and ancestors[-1] (the resampling after the last state)
    is not used.  Tensor ops: the index composition is T B S ints."""
    S = check_samples(samples)
    if ys.dim() != 3 or ys.shape[1] % S:
        raise ValueError(f'ys has shape {tuple(ys.shape)}, expected (T, B S, H) with a whole number of groups of {S} paths')
    T, B, H = ys.shape[0], ys.shape[1] // S, ys.shape[2]
    if tuple(ancestors.shape) != (T, B, S) or ancestors.dtype.is_floating_point or ancestors.dtype == torch.bool:
        raise ValueError(f'ancestors must be an integer tensor of shape {(T, B, S)}, got {ancestors.dtype} {tuple(ancestors.shape)}')
    anc = ancestors.to(device=ys.device, dtype=torch.int64)
    idx = torch.arange(S, device=ys.device).expand(B, S)
    picks = [idx]
    for k in range(T - 2, -1, -1):
        idx = anc[k].gather(1, idx)
        picks.append(idx)
    picks = torch.stack(picks[::-1])                                   # (T, B, S)
    return ys.reshape(T, B, S, H).gather(2, picks[..., None].expand(T, B, S, H)).reshape(T, B * S, H)


def quantile_positions(q, N):
    """Order-statistic positions of the levels q among N samples, torch.quantile's 'linear' rule: pos = q (N - 1) in float64,
    k = floor(pos), frac = float32(pos - k).  Returns (k, frac) as lists; ValueError for a level outside [0, 1] or no level."""
    try:
        qs = [float(v) for v in (q.tolist() if isinstance(q, (torch.Tensor, np.ndarray)) else q)]
    except TypeError:
        qs = [float(q)]
    if not qs or any(not 0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f'q must hold at least one level, each in [0, 1], got {q!r}')
    ks, fracs = [], []
    for v in qs:
        pos = v * (N - 1)
        k = int(np.floor(pos))
        frac = float(np.float32(pos - k))
        if frac >= 1.0:      # (pos - k rounds to 1 in float32: the next order statistic itself)
            k, frac = k + 1, 0.0
        ks.append(k)
        fracs.append(frac)
    return ks, fracs


def _quantile_args(ks, fracs):
    n = len(ks)
    return n, (C.c_int32 * n)(*ks), (C.c_float * n)(*fracs)


def sample_quantiles(ys, samples, q, members=1, log_weight=None):
    """Quantiles of the sample paths of a solve at the levels q (a sequence of numbers in [0, 1]): ys as for `sample_crps`, the
    result (len(q), ..., B, W).  Linear interpolation between order statistics (torch.quantile's 'linear' rule): with
    pos = q (N - 1), k = floor(pos) and frac = float32(pos - k), the value is x_(k), or fma(frac, x_(k+1) - x_(k), x_(k)) where
    frac != 0; ties are ordered by index.  Differentiable in ys: the gradient goes to the one or two samples that set the value.
    A sample set that holds a NaN has no order: NaN at every level (torch.quantile's rule), on every route.  A set with +-Inf
    and no NaN follows the formula: an order statistic may be +-Inf, and interpolating (frac != 0) from -Inf or between equal
    infinities is NaN.  The gradient of a set whose value is NaN is a derivative of nothing but a function of the inputs alone:
    the kernel gives a NaN sample an exact zero and the finite samples, ranked among themselves, the terms of the ranks they
    hold; the tensor-op route gives the whole set zeros.
    CUDA float32 input with N <= 256 and at most 8 levels: one launch of snsde_sample_quantiles (backward:
    snsde_sample_quantiles_backward); other tensors: a stable sort in tensor ops.
    log_weight (..., B, N) gives the weighted quantiles: the live samples are ranked, the node of a sample is
    p_n = A_n / (1 - w_n) with A_n the weight ranked before it (0 and 1 at the two ends), and a level interpolates linearly between
    the two nodes around it - r / (N - 1) at equal weights, the rule above: see `sample_quantiles_weighted_tensor_ops`.  The
    weights carry no gradient."""
    if log_weight is not None:
        return _sample_quantiles_weighted(ys, samples, q, members, log_weight)
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    ks, fracs = quantile_positions(q, N)
    if _score_native(ys, N) and len(ks) <= SCORE_MAX_QUANTILES:
        if ys.requires_grad and torch.is_grad_enabled():
            return _SampleQuantiles.apply(ys, S, M, tuple(ks), tuple(fracs))
        return _sample_quantiles_launch(ys.contiguous(), S, M, ks, fracs)
    x = _pooled(ys, S, M, lead, G, W)
    xs = torch.sort(x, dim=-2, stable=True).values
    out = []
    for k, frac in zip(ks, fracs):
        lo = xs[..., k, :]
        out.append(lo if frac == 0.0 else lo + frac * (xs[..., k + 1, :] - lo))
    out = torch.stack(out)
    # a set that holds a NaN has no order: NaN at every level (the sort puts a NaN last, which would leave the low levels finite)
    return torch.where(torch.isnan(x).any(dim=-2), torch.full_like(out[:1], float('nan')), out)


def _sample_quantiles_launch(ys, S, M, ks, fracs):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    n_q, k, frac = _quantile_args(ks, fracs)
    out = torch.empty((n_q,) + lead + (G, W), device=ys.device, dtype=torch.float32)
    _lib.check(_lib.lib().snsde_sample_quantiles(_ptr(ys), _outer(lead), M, G, S, W, n_q, k, frac, _ptr(out),
                                                 C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)), 'snsde_sample_quantiles')
    return out


def sample_quantiles_backward(grad_out, ys, samples, ks, fracs, members=1):
    """dL/d ys of `sample_quantiles` from dL/d out (len(ks), ..., B, W) at the positions (ks, fracs) of `quantile_positions`: one
    launch of snsde_sample_quantiles_backward.  Contiguous float32 CUDA tensors."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    n_q, k, frac = _quantile_args(ks, fracs)
    _check_f32('ys', ys)
    _check_f32('grad_out', grad_out, (n_q,) + lead + (G, W))
    gys = torch.empty_like(ys)
    _lib.check(_lib.lib().snsde_sample_quantiles_backward(_ptr(grad_out), _ptr(ys), _outer(lead), M, G, S, W, n_q, k, frac, _ptr(gys),
                                                          C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_quantiles_backward')
    return gys


class _SampleQuantiles(torch.autograd.Function):
    """sample_quantiles of a CUDA float32 tensor that requires grad: the forward kernel, and snsde_sample_quantiles_backward as its backward."""

    @staticmethod
    def forward(ctx, ys, S, M, ks, fracs):
        ysc = ys.detach().contiguous()
        ctx.S, ctx.M, ctx.ks, ctx.fracs = S, M, ks, fracs
        ctx.save_for_backward(ysc)
        return _sample_quantiles_launch(ysc, S, M, ks, fracs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ys, = ctx.saved_tensors
        return sample_quantiles_backward(grad_out.to(torch.float32).contiguous(), ys, ctx.S, ctx.ks, ctx.fracs, ctx.M), None, None, None, None


# ---- weighted sample sets (csrc/snsde_weighted.hip): log_weight= of sample_stats, sample_crps and sample_quantiles ------------

def _check_log_weight(log_weight, ys, shape):
    """The argument errors of a log_weight (..., B, N) that goes with ys."""
    if not isinstance(log_weight, torch.Tensor) or not log_weight.dtype.is_floating_point:
        raise ValueError(f'log_weight must be a floating-point tensor, got {getattr(log_weight, "dtype", type(log_weight))}')
    if tuple(log_weight.shape) != tuple(shape):
        raise ValueError(f'log_weight has shape {tuple(log_weight.shape)}, expected {tuple(shape)} (one log-weight per pooled path of an '
                         f'input row, the leading axes of ys)')
    if log_weight.device != ys.device:
        raise ValueError(f'log_weight is on {log_weight.device}, ys on {ys.device}')
    if log_weight.requires_grad and torch.is_grad_enabled():
        raise ValueError('log_weight requires grad: the weighted statistics and scores are differentiable in ys and target only (the '
                         'weights are fixed; detach() them)')


def normalised_weights(log_weight, dtype=None):
    """(w, live, D') of log-weights (..., N), the definitions every weighted function shares: mx = max a, e = exp(a - mx),
    P = sum e, w = e / P, D' = sum w (1 - w).  live is False for a dead sample: e == 0 (a -Inf weight, or exp underflowed) in a
    group whose P is a number; such a sample is selected out of everything by torch.where.  A group whose weights are all -Inf, or
    that holds a NaN or +Inf weight, has P = NaN and every w = NaN: NaN in all its results, by the arithmetic.  No gradient."""
    with torch.no_grad():
        a = log_weight.detach() if dtype is None else log_weight.detach().to(dtype)
        skip = torch.isnan(a)
        mx = torch.where(skip, torch.full_like(a, float('-inf')), a).amax(dim=-1, keepdim=True)      # (fmaxf skips a NaN)
        e = torch.exp(a - mx)
        P = e.sum(dim=-1, keepdim=True)
        w = e / P
        live = ~((e == 0) & ~torch.isnan(P))
        return w, live, (w * (1 - w)).sum(dim=-1)


def _stats_weighted_args(ys, samples, var, log_weight):
    S = check_samples(samples)
    if ys.dim() < 2 or ys.shape[-2] % S:
        raise ValueError(f'ys has shape {tuple(ys.shape)}: its second-to-last axis must hold a whole number of groups of {S} paths')
    if var and S < 2:
        raise ValueError('the unbiased variance needs samples >= 2')
    lead, G, W = tuple(ys.shape[:-2]), ys.shape[-2] // S, ys.shape[-1]
    _check_log_weight(log_weight, ys, lead + (G, S))
    return S, lead, G, W


def _sample_stats_weighted(ys, samples, var, log_weight):
    S, lead, G, W = _stats_weighted_args(ys, samples, var, log_weight)
    if _score_native(ys, S, log_weight):
        if ys.requires_grad and torch.is_grad_enabled():
            mean, vout = _SampleStatsWeighted.apply(ys, log_weight.detach(), S, bool(var))
        else:
            mean, vout = _sample_stats_weighted_launch(ys.contiguous(), log_weight.contiguous(), S, bool(var))
        return mean, (vout if var else None)
    return sample_stats_weighted_tensor_ops(ys, S, log_weight, var)


def sample_stats_weighted_tensor_ops(ys, samples, log_weight, var=True):
    """`sample_stats(..., log_weight=)` stated in tensor ops (any device and floating dtype; autograd differentiates it in ys).
    With (w, live, D') = normalised_weights(log_weight) and the dead samples selected out,
        mean = sum_n w_n x_n        var = sum_n w_n (x_n - mean)^2 / D'
    - the reliability-weights unbiased estimator, / (S - 1) at equal weights; a single live sample gives var = 0 / 0 = NaN."""
    S, lead, G, W = _stats_weighted_args(ys, samples, var, log_weight)
    w, live, Dp = normalised_weights(log_weight, ys.dtype)
    w, live = w.unsqueeze(-1), live.unsqueeze(-1)
    x = torch.where(live, ys.reshape(lead + (G, S, W)), torch.zeros((), dtype=ys.dtype, device=ys.device))
    mean = (w * x).sum(dim=-2)
    if not var:
        return mean, None
    return mean, (w * (x - mean.unsqueeze(-2)).square()).sum(dim=-2) / Dp.unsqueeze(-1)


def _sample_stats_weighted_launch(ys, logw, S, var):
    W = ys.shape[-1]
    out_shape = tuple(ys.shape[:-2]) + (ys.shape[-2] // S, W)
    mean = torch.empty(out_shape, device=ys.device, dtype=torch.float32)
    vout = torch.empty(out_shape, device=ys.device, dtype=torch.float32) if var else None
    _lib.check(_lib.lib().snsde_sample_stats_weighted(_ptr(ys), _ptr(logw), ys.numel() // (S * W), S, W, _ptr(mean), _ptr(vout),
                                                      C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_stats_weighted')
    return mean, vout


def sample_stats_weighted_backward(grad_mean, grad_var, ys, log_weight, mean, samples):
    """dL/d ys of the weighted `sample_stats` from dL/d mean and dL/d var (None: no variance term), the weights fixed: one launch
    of snsde_sample_stats_weighted_backward.  ys (..., B S, H), log_weight (..., B, S), the others (..., B, H): contiguous float32
    CUDA tensors."""
    S, W = int(samples), ys.shape[-1]
    _check_f32('ys', ys)
    _check_f32('log_weight', log_weight, tuple(ys.shape[:-2]) + (ys.shape[-2] // S, S))
    _check_f32('grad_mean', grad_mean, tuple(ys.shape[:-2]) + (ys.shape[-2] // S, W))
    if grad_var is not None:
        _check_f32('grad_var', grad_var, tuple(grad_mean.shape))
        _check_f32('mean', mean, tuple(grad_mean.shape))
    out = torch.empty_like(ys)
    _lib.check(_lib.lib().snsde_sample_stats_weighted_backward(_ptr(grad_mean), _ptr(grad_var), _ptr(ys), _ptr(log_weight),
                                                               _ptr(mean if grad_var is not None else None), ys.numel() // (S * W), S, W,
                                                               _ptr(out), C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_stats_weighted_backward')
    return out


class _SampleStatsWeighted(torch.autograd.Function):
    """The weighted sample_stats of a CUDA float32 tensor that requires grad: snsde_sample_stats_weighted and its _backward."""

    @staticmethod
    def forward(ctx, ys, logw, S, var):
        ysc, lw = ys.detach().contiguous(), logw.contiguous()
        mean, vout = _sample_stats_weighted_launch(ysc, lw, S, var)
        ctx.S, ctx.var = S, var
        ctx.save_for_backward(ysc, lw, mean)
        if not var:
            vout = mean.new_empty(0)
            ctx.mark_non_differentiable(vout)
        return mean, vout

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mean, grad_var):
        ys, lw, mean = ctx.saved_tensors
        gm = torch.zeros_like(mean) if grad_mean is None else grad_mean.to(torch.float32).contiguous()
        gv = grad_var.to(torch.float32).contiguous() if ctx.var and grad_var is not None else None
        return sample_stats_weighted_backward(gm, gv, ys, lw, mean, ctx.S), None, None, None


def _crps_weighted_args(ys, samples, target, fair, members, log_weight):
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    if tuple(target.shape) != lead + (G, W):
        raise ValueError(f'target has shape {tuple(target.shape)}, expected {lead + (G, W)} (one observation per input row and column)')
    if fair and N < 2:
        raise ValueError('the fair (unbiased) score needs at least 2 pooled samples')
    _check_log_weight(log_weight, ys, lead + (G, N))
    return S, M, lead, G, W, N


def _sample_crps_weighted(ys, samples, target, fair, members, rank, log_weight):
    S, M, lead, G, W, N = _crps_weighted_args(ys, samples, target, fair, members, log_weight)
    fair, rank = bool(fair), bool(rank)
    if _score_native(ys, N, target, log_weight):
        if (ys.requires_grad or target.requires_grad) and torch.is_grad_enabled():
            crps, rk, ti = _SampleCRPSWeighted.apply(ys, target, log_weight.detach(), S, M, fair, rank)
        else:
            crps, rk, ti = _sample_crps_weighted_launch(ys.contiguous(), target.contiguous(), log_weight.contiguous(), S, M, fair, rank)
        return (crps, rk, ti) if rank else crps
    return sample_crps_weighted_tensor_ops(ys, S, target, log_weight, fair, M, rank)


def sample_crps_weighted_tensor_ops(ys, samples, target, log_weight, fair=True, members=1, rank=False):
    """`sample_crps(..., log_weight=)` stated in tensor ops (any device and floating dtype; autograd differentiates it in ys and
    target).  With (w, live, D') = normalised_weights(log_weight), the dead samples selected out, d_n = x_n - y and
    C_n = sum_j w_j [x_j < x_n] - sum_j w_j [x_j > x_n] from a sort and a cumulative sum of each column (no (.., N, N, ..) term),
        crps = sum_n w_n |d_n| - sum_n w_n C_n d_n / D,  D = D' (fair) or 1;    rank = sum_n w_n [x_n < y], ties = sum_n w_n [x_n == y]."""
    S, M, lead, G, W, N = _crps_weighted_args(ys, samples, target, fair, members, log_weight)
    w, live, Dp = normalised_weights(log_weight, ys.dtype)
    w, live = w.unsqueeze(-1), live.unsqueeze(-1)
    x = torch.where(live, _pooled(ys, S, M, lead, G, W), torch.zeros((), dtype=ys.dtype, device=ys.device))
    d = x - target.unsqueeze(-2)
    with torch.no_grad():      # (the weights are fixed: no gradient)
        xt = x.transpose(-1, -2).contiguous()                                     # (..., G, W, N)
        xs, order = torch.sort(xt, dim=-1)
        ws = w.transpose(-1, -2).expand(xt.shape).gather(-1, order)
        cs = torch.cat((torch.zeros_like(ws[..., :1]), torch.cumsum(ws, dim=-1)), dim=-1)
        below = cs.gather(-1, torch.searchsorted(xs, xt, right=False))
        above = cs[..., -1:] - cs.gather(-1, torch.searchsorted(xs, xt, right=True))
        c = (below - above).transpose(-1, -2)
    D = Dp.unsqueeze(-1) if fair else 1.0
    # (sum_n w_n C_n = 0: the second sum does not depend on the observation, and is not differentiated through it - in floating
    # point the sum is not exactly zero, and near collapse it is divided by a small D')
    crps = (w * d.abs()).sum(dim=-2) - (w * c * (x - target.detach().unsqueeze(-2))).sum(dim=-2) / D
    if not rank:
        return crps
    with torch.no_grad():
        return crps, (w * (d < 0)).sum(dim=-2).to(torch.float32), (w * (d == 0)).sum(dim=-2).to(torch.float32)


def _sample_crps_weighted_launch(ys, target, logw, S, M, fair, rank):
    G, W = ys.shape[-2] // S, ys.shape[-1]
    crps = torch.empty_like(target)
    rk = torch.empty_like(target) if rank else None
    ti = torch.empty_like(target) if rank else None
    _lib.check(_lib.lib().snsde_sample_crps_weighted(_ptr(ys), _ptr(target), _ptr(logw), ys.numel() // (M * G * S * W), M, G, S, W, int(fair),
                                                     _ptr(crps), _ptr(rk), _ptr(ti),
                                                     C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_crps_weighted')
    return crps, rk, ti


def sample_crps_weighted_backward(grad_crps, ys, target, log_weight, samples, fair=True, members=1, grad_target=True):
    """(dL/d ys, dL/d target) of the weighted `sample_crps` from dL/d crps, the weights fixed: one launch of
    snsde_sample_crps_weighted_backward (dL/d target None when grad_target=False).  Contiguous float32 CUDA tensors."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    _check_f32('ys', ys)
    _check_f32('target', target, lead + (G, W))
    _check_f32('grad_crps', grad_crps, lead + (G, W))
    _check_f32('log_weight', log_weight, lead + (G, M * S))
    gys = torch.empty_like(ys)
    gt = torch.empty_like(target) if grad_target else None
    _lib.check(_lib.lib().snsde_sample_crps_weighted_backward(_ptr(grad_crps), _ptr(ys), _ptr(target), _ptr(log_weight), _outer(lead), M, G, S,
                                                              W, int(bool(fair)), _ptr(gys), _ptr(gt),
                                                              C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_crps_weighted_backward')
    return gys, gt


class _SampleCRPSWeighted(torch.autograd.Function):
    """The weighted sample_crps of CUDA float32 tensors of which one requires grad: snsde_sample_crps_weighted and its _backward."""

    @staticmethod
    def forward(ctx, ys, target, logw, S, M, fair, rank):
        ysc, tc, lw = ys.detach().contiguous(), target.detach().contiguous(), logw.contiguous()
        crps, rk, ti = _sample_crps_weighted_launch(ysc, tc, lw, S, M, fair, rank)
        ctx.S, ctx.M, ctx.fair = S, M, fair
        ctx.save_for_backward(ysc, tc, lw)
        if not rank:
            rk, ti = crps.new_empty(0), crps.new_empty(0)
        ctx.mark_non_differentiable(rk, ti)
        return crps, rk, ti

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_crps, grad_rank, grad_ties):
        ys, target, lw = ctx.saved_tensors
        g = torch.zeros_like(target) if grad_crps is None else grad_crps.to(torch.float32).contiguous()
        gys, gt = sample_crps_weighted_backward(g, ys, target, lw, ctx.S, ctx.fair, ctx.M, grad_target=ctx.needs_input_grad[1])
        return (gys if ctx.needs_input_grad[0] else None), gt, None, None, None, None, None


def quantile_levels(q):
    """The levels q as a list of float32-representable numbers; ValueError for a level outside [0, 1] or no level."""
    try:
        qs = [float(v) for v in (q.tolist() if isinstance(q, (torch.Tensor, np.ndarray)) else q)]
    except TypeError:
        qs = [float(q)]
    if not qs or any(not 0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f'q must hold at least one level, each in [0, 1], got {q!r}')
    return [float(np.float32(v)) for v in qs]


def _sample_quantiles_weighted(ys, samples, q, members, log_weight):
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    qs = quantile_levels(q)
    _check_log_weight(log_weight, ys, lead + (G, N))
    if _score_native(ys, N, log_weight) and len(qs) <= SCORE_MAX_QUANTILES:
        if ys.requires_grad and torch.is_grad_enabled():
            return _SampleQuantilesWeighted.apply(ys, log_weight.detach(), S, M, tuple(qs))
        return _sample_quantiles_weighted_launch(ys.contiguous(), log_weight.contiguous(), S, M, qs)
    return sample_quantiles_weighted_tensor_ops(ys, S, q, log_weight, M)


def sample_quantiles_weighted_tensor_ops(ys, samples, q, log_weight, members=1):
    """`sample_quantiles(..., log_weight=)` stated in tensor ops (any device and floating dtype; autograd differentiates it in ys).
    With (w, live, .) = normalised_weights(log_weight), only the F live samples of a group are ranked (ties by index); A_n is the
    weight ranked before sample n and its node p_n = A_n / (1 - w_n), by definition 0 for rank 0 and 1 for rank F - 1.  For a level
    q (rounded to float32): lo = the sample of largest rank with p <= q, hi = the next rank,
    frac = clamp((q - p_lo) / (p_hi - p_lo), 0, 1) and the value is x_lo where lo is the last rank or frac == 0, else
    x_lo + frac (x_hi - x_lo).  A live NaN makes every level of its column NaN (gradient: zeros); an unusable weight set NaN."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    N = M * S
    qs = quantile_levels(q)
    _check_log_weight(log_weight, ys, lead + (G, N))
    w, live, _ = normalised_weights(log_weight, ys.dtype)
    zero = torch.zeros((), dtype=ys.dtype, device=ys.device)
    x = torch.where(live.unsqueeze(-1), _pooled(ys, S, M, lead, G, W), zero).transpose(-1, -2)      # (..., G, W, N)
    with torch.no_grad():
        dead = (~live).unsqueeze(-2).expand(x.shape)
        has_nan = (torch.isnan(x) & ~dead).any(dim=-1)
        first = torch.sort(torch.where(torch.isnan(x), zero, x), dim=-1, stable=True).indices
        order = first.gather(-1, torch.sort(dead.gather(-1, first).to(torch.int8), dim=-1, stable=True).indices)      # the live first
        ws = w.unsqueeze(-2).expand(x.shape).gather(-1, order)
        F = live.sum(dim=-1)[..., None, None]                                                      # (..., G, 1, 1)
        r = torch.arange(N, device=x.device).expand(x.shape)
        p = torch.cat((torch.zeros_like(ws[..., :1]), torch.cumsum(ws, dim=-1)[..., :-1]), dim=-1) / (1 - ws)
        p = torch.where(r == F - 1, torch.ones_like(p), p)
        p = torch.where(r == 0, torch.zeros_like(p), p)
        p = torch.where(r >= F, torch.full_like(p, float('inf')), p)
        bad = torch.isnan(w).any(dim=-1)[..., None]                                                # (..., G, 1)
    xs = x.gather(-1, order)
    nan = torch.full((), float('nan'), dtype=ys.dtype, device=ys.device)
    poison = torch.where(bad[..., None], xs, zero).sum(dim=-1) * nan      # (an unusable weight set: NaN, and a NaN gradient to every sample of the group)
    out = []
    for level in qs:
        with torch.no_grad():
            lo = torch.where(p <= level, r, torch.zeros_like(r)).amax(dim=-1, keepdim=True)
            hi = torch.clamp(lo + 1, max=N - 1)
            plo, phi = p.gather(-1, lo), p.gather(-1, hi)
            frac = torch.clamp((level - plo) / (phi - plo), 0, 1)
            flat = (lo == F - 1) | (frac == 0) | has_nan[..., None] | bad[..., None]
            frac = torch.where(flat, torch.zeros_like(frac), frac)
        xlo, xhi = xs.gather(-1, lo), xs.gather(-1, hi)
        v = torch.where(flat, xlo, xlo + frac * (torch.where(flat, xlo, xhi) - xlo))[..., 0]
        out.append(torch.where(bad, poison, torch.where(has_nan, nan, v)))
    return torch.stack(out)


def _level_args(qs):
    return len(qs), (C.c_float * len(qs))(*qs)


def _sample_quantiles_weighted_launch(ys, logw, S, M, qs):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    n_q, q = _level_args(qs)
    out = torch.empty((n_q,) + lead + (G, W), device=ys.device, dtype=torch.float32)
    _lib.check(_lib.lib().snsde_sample_quantiles_weighted(_ptr(ys), _ptr(logw), _outer(lead), M, G, S, W, n_q, q, _ptr(out),
                                                          C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_quantiles_weighted')
    return out


def sample_quantiles_weighted_backward(grad_out, ys, log_weight, samples, q, members=1):
    """dL/d ys of the weighted `sample_quantiles` from dL/d out (len(q), ..., B, W), the weights fixed: one launch of
    snsde_sample_quantiles_weighted_backward.  Contiguous float32 CUDA tensors."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    n_q, qa = _level_args(quantile_levels(q))
    _check_f32('ys', ys)
    _check_f32('log_weight', log_weight, lead + (G, M * S))
    _check_f32('grad_out', grad_out, (n_q,) + lead + (G, W))
    gys = torch.empty_like(ys)
    _lib.check(_lib.lib().snsde_sample_quantiles_weighted_backward(_ptr(grad_out), _ptr(ys), _ptr(log_weight), _outer(lead), M, G, S, W, n_q,
                                                                   qa, _ptr(gys), C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_quantiles_weighted_backward')
    return gys


class _SampleQuantilesWeighted(torch.autograd.Function):
    """The weighted sample_quantiles of a CUDA float32 tensor that requires grad: snsde_sample_quantiles_weighted and its _backward."""

    @staticmethod
    def forward(ctx, ys, logw, S, M, qs):
        ysc, lw = ys.detach().contiguous(), logw.contiguous()
        ctx.S, ctx.M, ctx.qs = S, M, qs
        ctx.save_for_backward(ysc, lw)
        return _sample_quantiles_weighted_launch(ysc, lw, S, M, list(qs))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ys, lw = ctx.saved_tensors
        return sample_quantiles_weighted_backward(grad_out.to(torch.float32).contiguous(), ys, lw, ctx.S, ctx.qs, ctx.M), None, None, None, None


def _energy_weighted_args(ys, samples, target, fair, members, path, log_weight, mask):
    """(S, M, lead, G, W, N, result shape, mask tensor or None, nan_missing) of a weighted / masked energy score; its argument
    errors.  mask='nan': no tensor, nan_missing True.  A mask tensor of another dtype than ys becomes (mask != 0) in ys' dtype."""
    S, M, lead, G, W, N, out_shape = _energy_dims(ys, samples, target, fair, members, path)
    if log_weight is not None:
        _check_log_weight(log_weight, ys, (G, N) if path else lead + (G, N))
    nan_missing = False
    if isinstance(mask, str):
        if mask != 'nan':
            raise ValueError(f"mask must be None, 'nan' (a NaN target is a gap) or a tensor of the shape of target, got {mask!r}")
        mask, nan_missing = None, True
    elif mask is not None:
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(target.shape):
            raise ValueError(f'mask has shape {tuple(getattr(mask, "shape", ()))}, expected {tuple(target.shape)} (the shape of target)')
        if mask.device != ys.device:
            raise ValueError(f'mask is on {mask.device}, ys on {ys.device}')
        mask = mask.detach()
        if mask.dtype != ys.dtype:
            mask = (mask != 0).to(ys.dtype)
    return S, M, lead, G, W, N, out_shape, mask, nan_missing


def _sample_energy_weighted(ys, samples, target, fair, members, path, log_weight, mask):
    fair, path = bool(fair), bool(path)
    S, M, lead, G, W, N, out_shape, mk, nan_missing = _energy_weighted_args(ys, samples, target, fair, members, path, log_weight, mask)
    others = (target,) + (() if log_weight is None else (log_weight,)) + (() if mk is None else (mk,))
    if _score_native(ys, N, *others):
        lw = None if log_weight is None else log_weight.detach()
        if (ys.requires_grad or target.requires_grad) and torch.is_grad_enabled():
            return _SampleEnergyWeighted.apply(ys, target, lw, mk, S, M, fair, path, nan_missing)
        return _sample_energy_weighted_launch(ys.contiguous(), target.contiguous(), None if lw is None else lw.contiguous(),
                                              None if mk is None else mk.contiguous(), S, M, fair, path, nan_missing)
    return sample_energy_weighted_tensor_ops(ys, S, target, log_weight, 'nan' if nan_missing else mk, fair, M, path)


def sample_energy_weighted_tensor_ops(ys, samples, target, log_weight=None, mask=None, fair=True, members=1, path=False):
    """`sample_energy(..., log_weight=, mask=)` stated in tensor ops (any device and floating dtype; autograd differentiates it in
    ys and target).  torch.where on the mask puts exact zeros in the unobserved coordinates of every sample and of the
    observation - selected, never multiplied, so NaN / Inf there reaches no value and the gradient there is an exact zero - and,
    with (w, live, D') = normalised_weights(log_weight), in the rows of the dead samples; then, from direct differences
    (torch.linalg.vector_norm, and torch.cdist in its direct-difference mode, sliced as in `sample_energy_tensor_ops`),
        energy = sum_n w_n ||x_n - y|| - sum_{n,j} w_n w_j ||x_n - x_j|| / (2 D),  D = D' (fair) or 1
    the dead pairs selected out; without log_weight w = 1 / N and D = (N - 1) / N or 1, written as / N and / (2 N D)."""
    fair, path = bool(fair), bool(path)
    S, M, lead, G, W, N, out_shape, mk, nan_missing = _energy_weighted_args(ys, samples, target, fair, members, path, log_weight, mask)
    if ys.numel() == 0:
        return ys.new_zeros(out_shape)
    x, y = _pooled(ys, S, M, lead, G, W), target.to(ys.dtype)            # (..., G, N, W), (..., G, W)
    obs = ~torch.isnan(y.detach()) if nan_missing else (None if mk is None else mk != 0)
    if path:      # every leading axis joins the vector: (G, N, outer W)
        O = _outer(lead)
        x = x.reshape(O, G, N, W).permute(1, 2, 0, 3).reshape(G, N, O * W)
        y = y.reshape(O, G, W).permute(1, 0, 2).reshape(G, O * W)
        obs = None if obs is None else obs.reshape(O, G, W).permute(1, 0, 2).reshape(G, O * W)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    if obs is not None:
        x, y = torch.where(obs.unsqueeze(-2), x, zero), torch.where(obs, y, zero)
    if log_weight is None:
        w = pair = None
    else:
        w, live, Dp = normalised_weights(log_weight, x.dtype)
        x = torch.where(live.unsqueeze(-1), x, zero)
        pair = torch.where(live.unsqueeze(-1) & live.unsqueeze(-2), w.unsqueeze(-1) * w.unsqueeze(-2), zero)      # (..., G, N, N)
    rn = torch.linalg.vector_norm(x - y.unsqueeze(-2), dim=-1)           # (..., G, N)
    a = rn.sum(dim=-1) / N if w is None else torch.where(live, w * rn, zero).sum(dim=-1)
    flat = x.reshape((-1, N, x.shape[-1]))
    fpair = None if pair is None else pair.reshape((-1, N, N))
    step = max(1, _CDIST_MAX_PLANE // (N * N))
    sums = []
    for i in range(0, flat.shape[0], step):
        plane = torch.cdist(flat[i:i + step], flat[i:i + step], compute_mode='donot_use_mm_for_euclid_dist')
        sums.append((plane if fpair is None else fpair[i:i + step] * plane).sum(dim=(-2, -1)))
    b = (sums[0] if len(sums) == 1 else torch.cat(sums)).reshape(a.shape)
    if w is None:
        return a - b / (2 * N * (N - 1 if fair else N))
    return a - (b / (2 * Dp) if fair else b / 2)


def _sample_energy_weighted_launch(ys, target, logw, mask, S, M, fair, path, nan_missing):
    S_, M_, lead, G, W = _score_dims(ys, S, M)
    energy = torch.empty((G,) if path else lead + (G,), device=ys.device, dtype=torch.float32)
    _lib.check(_lib.lib().snsde_sample_energy_weighted(_ptr(ys), _ptr(target), _ptr(logw), _ptr(mask), _outer(lead), M, G, S, W, int(fair),
                                                       int(path), int(nan_missing), _ptr(energy),
                                                       C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_energy_weighted')
    return energy


def sample_energy_weighted_backward(grad_energy, ys, target, samples, log_weight=None, mask=None, fair=True, members=1, path=False,
                                    grad_target=True):
    """(dL/d ys, dL/d target) of `sample_energy(..., log_weight=, mask=)` from dL/d energy, the weights fixed: one launch of
    snsde_sample_energy_weighted_backward (dL/d target None when grad_target=False).  Contiguous float32 CUDA tensors, ys
    (..., B S, W) or (..., M, B S, W), target (..., B, W), grad_energy (..., B) or, under path, (B,); log_weight (..., B, N) or,
    under path, (B, N), or None; mask a float32 tensor of the shape of target, 'nan', or None."""
    S, M, lead, G, W = _score_dims(ys, samples, members)
    path, nan_missing = bool(path), isinstance(mask, str) and mask == 'nan'
    if isinstance(mask, str) and not nan_missing:
        raise ValueError(f"mask must be None, 'nan' or a tensor of the shape of target, got {mask!r}")
    mask = None if nan_missing else mask
    _check_f32('ys', ys)
    _check_f32('target', target, lead + (G, W))
    _check_f32('grad_energy', grad_energy, (G,) if path else lead + (G,))
    if log_weight is not None:
        _check_f32('log_weight', log_weight, (G, M * S) if path else lead + (G, M * S))
    if mask is not None:
        _check_f32('mask', mask, lead + (G, W))
    gys = torch.empty_like(ys)
    gt = torch.empty_like(target) if grad_target else None
    _lib.check(_lib.lib().snsde_sample_energy_weighted_backward(_ptr(grad_energy), _ptr(ys), _ptr(target), _ptr(log_weight), _ptr(mask),
                                                                _outer(lead), M, G, S, W, int(bool(fair)), int(path), int(nan_missing),
                                                                _ptr(gys), _ptr(gt),
                                                                C.c_void_p(torch.cuda.current_stream(ys.device).cuda_stream)),
               'snsde_sample_energy_weighted_backward')
    return gys, gt


class _SampleEnergyWeighted(torch.autograd.Function):
    """The weighted / masked sample_energy of CUDA float32 tensors of which one requires grad: snsde_sample_energy_weighted and its
    _backward."""

    @staticmethod
    def forward(ctx, ys, target, logw, mask, S, M, fair, path, nan_missing):
        ysc, tc = ys.detach().contiguous(), target.detach().contiguous()
        lw, mk = None if logw is None else logw.contiguous(), None if mask is None else mask.contiguous()
        ctx.S, ctx.M, ctx.fair, ctx.path, ctx.nan_missing = S, M, fair, path, nan_missing
        ctx.has = (lw is not None, mk is not None)
        ctx.save_for_backward(ysc, tc, *(t for t in (lw, mk) if t is not None))
        return _sample_energy_weighted_launch(ysc, tc, lw, mk, S, M, fair, path, nan_missing)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_energy):
        ys, target, *rest = ctx.saved_tensors
        lw = rest.pop(0) if ctx.has[0] else None
        mk = rest.pop(0) if ctx.has[1] else None
        gys, gt = sample_energy_weighted_backward(grad_energy.to(torch.float32).contiguous(), ys, target, ctx.S, lw,
                                                  'nan' if ctx.nan_missing else mk, ctx.fair, ctx.M, ctx.path,
                                                  grad_target=ctx.needs_input_grad[1])
        return (gys if ctx.needs_input_grad[0] else None), gt, None, None, None, None, None, None, None


def filter_particles(ys, ancestor, samples):
    """The particle sets that a particle filter's weights belong to.  `sdeint_filter`'s ys (T, B S, H) holds the states BEFORE each
    resampling and its log_weight (T, B, S) the weights AFTER it; this gathers every step's states through that step's own
    resampling, out[k, b S + j] = ys[k, b S + ancestor[k, b, j]] (the identity wherever the step did not resample), so that
    out[k] with log_weight[k] is the weighted sample set of time k:
        sample_stats(filter_particles(r.ys, r.ancestor, S), S, log_weight=r.log_weight)
    is the filtered mean and variance of all T times in one launch (`sample_crps` and `sample_quantiles` likewise).  Unlike
    `filter_paths` nothing is traced back through earlier steps.  ys may carry further leading axes: (..., B S, H) against
    ancestor (..., B, S)."""
    S = check_samples(samples)
    if ys.dim() < 2 or ys.shape[-2] % S:
        raise ValueError(f'ys has shape {tuple(ys.shape)}, expected (..., B S, H) with a whole number of groups of {S} paths')
    lead, B, H = tuple(ys.shape[:-2]), ys.shape[-2] // S, ys.shape[-1]
    if tuple(ancestor.shape) != lead + (B, S) or ancestor.dtype.is_floating_point or ancestor.dtype == torch.bool:
        raise ValueError(f'ancestor must be an integer tensor of shape {lead + (B, S)}, got {ancestor.dtype} {tuple(ancestor.shape)}')
    anc = ancestor.to(device=ys.device, dtype=torch.int64)
    return ys.reshape(lead + (B, S, H)).gather(-2, anc[..., None].expand(lead + (B, S, H))).reshape(ys.shape)


def spline_grad_native():
    """False under SNSDE_SPLINE_GRAD=torch: the spline constructors then differentiate their tensor-op statement with autograd
    (the in-repo cross-check of the HIP adjoint, and the route that supports double backward).  Read at every call."""
    return os.environ.get('SNSDE_SPLINE_GRAD', '') != 'torch'


def spline_coeffs(times, X, kind='natural'):
    """Packed spline coefficients (B, L-1, 4C) on the GPU; times (L,), X (B, L, C) CUDA float32 with NaN = missing.
    An X that requires grad gets the same kernel inside one autograd node whose backward is `spline_coeffs_backward`."""
    if X.requires_grad and torch.is_grad_enabled():
        return _SplineCoeffs.apply(times, X, kind)
    return _spline_coeffs(times, X, kind)


def _spline_coeffs(times, X, kind):
    _check_f32('X', X)
    _check_f32('times', times)
    B, L, Cn = X.shape
    out = torch.empty((B, L - 1, 4 * Cn), device=X.device, dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
    lib = _lib.lib()
    if kind == 'natural':
        ws = torch.empty(lib.snsde_spline_workspace_bytes(B, L, Cn), device=X.device, dtype=torch.uint8)
        _lib.check(lib.snsde_natural_cubic_coeffs(_ptr(times), _ptr(X), B, L, Cn, _ptr(out), _ptr(ws), ws.numel(), stream),
                   'snsde_natural_cubic_coeffs')
        torch.cuda.current_stream(X.device).synchronize()    # workspace is released on return
    else:
        _lib.check(lib.snsde_hermite_coeffs(_ptr(times), _ptr(X), B, L, Cn, _ptr(out), stream), 'snsde_hermite_coeffs')
    return out


def spline_coeffs_backward(times, X, grad_coeffs, kind='natural'):
    """grad_X (B, L, C) = J^T grad_coeffs for the construction `spline_coeffs(times, X, kind)`: one launch of the adjoint kernel
    (snsde_natural_cubic_coeffs_backward / snsde_hermite_coeffs_backward).  X is read for its NaN mask only; missing entries get
    exactly 0.  Enqueue-only: the natural adjoint's workspace comes from the caching allocator on the launch stream, which hands
    the block to nobody else before the kernel has run, so there is no host synchronisation here."""
    _check_f32('X', X)
    _check_f32('times', times)
    B, L, Cn = X.shape
    _check_f32('grad_coeffs', grad_coeffs, (B, L - 1, 4 * Cn))
    if tuple(times.shape) != (L,):
        raise ValueError(f'times has shape {tuple(times.shape)}, expected {(L,)}')
    grad_X = torch.empty((B, L, Cn), device=X.device, dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
    lib = _lib.lib()
    if kind == 'natural':
        ws = torch.empty(lib.snsde_spline_backward_workspace_bytes(B, L, Cn), device=X.device, dtype=torch.uint8)
        _lib.check(lib.snsde_natural_cubic_coeffs_backward(_ptr(times), _ptr(X), _ptr(grad_coeffs), B, L, Cn, _ptr(grad_X),
                                                           _ptr(ws), ws.numel(), stream), 'snsde_natural_cubic_coeffs_backward')
    else:
        _lib.check(lib.snsde_hermite_coeffs_backward(_ptr(times), _ptr(X), _ptr(grad_coeffs), B, L, Cn, _ptr(grad_X), stream),
                   'snsde_hermite_coeffs_backward')
    return grad_X


class _SplineCoeffs(torch.autograd.Function):
    """X -> packed coefficients with the HIP adjoint as its backward.  The forward is the kernel the no-grad call runs (same
    bits); the map is linear in the observed values, so the backward needs `times` and the NaN mask of X and nothing else."""

    @staticmethod
    def forward(ctx, times, X, kind):
        ctx.save_for_backward(times, X)
        ctx.kind = kind
        return _spline_coeffs(times, X, kind)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_coeffs):
        times, X = ctx.saved_tensors
        return None, spline_coeffs_backward(times, X, grad_coeffs.contiguous(), ctx.kind), None


def spline_evaluate(coeffs, index, frac, derivative=False):
    B, Lm1, C4 = coeffs.shape
    _check_f32('coeffs', coeffs)
    out = torch.empty((B, C4 // 4), device=coeffs.device, dtype=torch.float32)
    stream = torch.cuda.current_stream(coeffs.device)
    _lib.check(_lib.lib().snsde_spline_evaluate(_ptr(coeffs), B, Lm1 + 1, C4 // 4, int(index), float(frac),
                                                int(bool(derivative)), _ptr(out), C.c_void_p(stream.cuda_stream)),
               'snsde_spline_evaluate')
    return out
