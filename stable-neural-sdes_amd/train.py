"""Training driver around the fused solver: the engine's equivalent of the reference's `common_sde.py`
(benchmark_classification/common_sde.py:16-23 regulariser, :49-92 metrics, :107-216 loop, :248-298 main;
benchmark_forecasting/common_sde.py for the regression variant).  The reference's own file also runs unchanged on
`stable_neural_sdes_amd.install()`; this module is the same loop written for one-process-per-GPU training:

  * the weight regulariser  scaling * sum_p ||p||  is ONE multi-tensor norm launch over the vector field's parameters
    (torch._foreach_norm) instead of one reduction + one add per parameter tensor per batch;
  * evaluation keeps every running sum (loss, correct count, confusion matrix, the scores for AUROC / average precision)
    on the device and synchronises with the host ONCE per pass over a dataloader instead of once per batch; AUROC and
    average precision are computed on the device from one sort (ties handled as sklearn does);
  * under an initialised process group (one rank per GPU) the model is wrapped in DistributedDataParallel (RCCL
    all-reduce of gradients, bucketed by DDP), metric sums are all-reduced, and the solver's Philox row offsets default
    to rank * local batch (torchsde._sdeint_hip), so ranks never integrate against the same Brownian rows;
  * the best model is restored with in-place copies, which keeps the engine's parameter arena (engine.flatten_params)
    valid; the reference re-points `parameter.data`, which the arena also survives (address check) at the price of one
    re-flatten.

Same entry points and semantics as the reference: `main(...)`, `make_model(...)`, `_train_loop`, `_evaluate_metrics`,
`_add_weight_regularisation` (Adam with weight_decay = 0.01 lr, ReduceLROnPlateau(patience=5) on the chosen metric,
termination after 50 epochs without improvement of the training loss / accuracy, best model by validation accuracy).
"""
import copy
import json
import math
import os

import numpy as np
import torch

from . import modules


class AttrDict(dict):
    def __setattr__(self, key, value):
        self[key] = value

    def __getattr__(self, item):
        try:
            return self[item]
        except KeyError as exc:
            raise AttributeError(item) from exc


def add_weight_regularisation(loss_fn, regularise_parameters, scaling=0.01, mode='l2'):
    """loss + scaling * sum over trainable tensors of ||p||_2 (classification benchmark) or ||p||_1 (`mode='l1'`,
    forecasting benchmark).  One multi-tensor norm launch."""
    if mode not in ('l1', 'l2', None):
        raise ValueError("mode must be 'l1', 'l2' or None")

    def new_loss_fn(pred_y, true_y):
        total = loss_fn(pred_y, true_y)
        ps = [p for p in regularise_parameters.parameters() if p.requires_grad]
        if mode is None or not ps:
            return total
        norms = torch._foreach_norm(ps, 1 if mode == 'l1' else 2)
        return total + scaling * torch.stack(norms).sum()
    return new_loss_fn


def crps_loss(samples, fair=True, members=1):
    """loss_fn(pred, true) for `train_loop` / `GraphedStep` / `evaluate_metrics`: the mean continuous ranked probability score
    (engine.sample_crps) of a model solved with options={'samples': S}.  pred has one row per path, as the wrappers return it in
    both modes - (B S, ...), or (M, B S, ...) from an `Ensemble` of `members` = M models, whose paths are pooled; true is
    (B, ...).  Trailing axes are flattened to the width; the result is the mean over the elements of true."""
    from . import engine
    S = engine.check_samples(samples)

    lead = 1 if members > 1 else 0      # (an Ensemble's leading member axis)

    def loss_fn(pred_y, true_y):
        want = ((members,) if lead else ()) + (S * true_y.shape[0],) if true_y.dim() else None
        if want is None or tuple(pred_y.shape[:lead + 1]) != want:
            raise ValueError(f'crps_loss(samples={S}, members={members}): pred has shape {tuple(pred_y.shape)} for a target of shape '
                             f'{tuple(true_y.shape)}: expected {"(members, " if lead else "("}samples x target rows, ...)')
        pred = pred_y.reshape(want + (-1,))
        true = true_y.reshape(true_y.shape[0], -1).to(pred.dtype)
        return engine.sample_crps(pred, S, true, fair=fair, members=members).mean()
    return loss_fn


def energy_loss(samples, fair=True, members=1, masked=False):
    """loss_fn(pred, true) for `train_loop` / `GraphedStep` / `evaluate_metrics`: the mean energy score (engine.sample_energy)
    of a model solved with options={'samples': S} - the multivariate score, which also judges the dependence between the
    components of a forecast.  pred and true as for `crps_loss`: (B S, ...) or (M, B S, ...), and (B, ...).  Trailing axes are
    flattened into the vector, so a wrapper that returns (B S, T, out) is scored on the whole forecast path; the result is the
    mean over the rows of true.  masked=True scores a target with gaps, `iwae_loss`'s convention: a NaN in true marks a missing
    entry, and data that carries its own mask is passed as true = (values, mask); the norms then run over the observed entries
    of a row only, and a row with nothing observed adds 0."""
    from . import engine
    S = engine.check_samples(samples)

    lead = 1 if members > 1 else 0      # (an Ensemble's leading member axis)

    def loss_fn(pred_y, true_y):
        mask = None
        if masked:
            true_y, mask = true_y if isinstance(true_y, (tuple, list)) else (true_y, None)
        want = ((members,) if lead else ()) + (S * true_y.shape[0],) if true_y.dim() else None
        if want is None or tuple(pred_y.shape[:lead + 1]) != want:
            raise ValueError(f'energy_loss(samples={S}, members={members}): pred has shape {tuple(pred_y.shape)} for a target of shape '
                             f'{tuple(true_y.shape)}: expected {"(members, " if lead else "("}samples x target rows, ...)')
        if mask is not None and tuple(mask.shape) != tuple(true_y.shape):
            raise ValueError(f'energy_loss: the mask has shape {tuple(mask.shape)} for a target of shape {tuple(true_y.shape)}')
        pred = pred_y.reshape(want + (-1,))
        true = true_y.reshape(true_y.shape[0], -1).to(pred.dtype)
        if not masked:
            return engine.sample_energy(pred, S, true, fair=fair, members=members).mean()
        return engine.sample_energy(pred, S, true, fair=fair, members=members, mask='nan' if mask is None else mask.reshape(true.shape)).mean()
    return loss_fn


class ObservationNoise(torch.nn.Module):
    """A model together with the observation noise it is scored under: `forward` is the wrapped model's, and `log_std` is an
    nn.Parameter of shape (channels,) - the log standard deviation of the noise per output channel, initialised to log(std) -
    which `iwae_loss(S, noise=this)` reads at every call.  Because the module wraps the model, a `make_model()` given to `main`
    can return (ObservationNoise(model, channels), vector_field): `net.parameters()` reaches the noise, the optimizer (and a
    recorded `GraphedStep`) updates it in place, and `main` needs no further argument.  The wrapped model's entries of
    `state_dict()` carry the prefix `model.` (`model.<name>`), beside `log_std`.  per_step=T (an integer; default False) gives
    every one of the T output times its own scale: log_std is then (T, channels), for a model that returns (B S, T, channels)."""

    def __init__(self, model, channels, std=0.1, per_step=False):
        super().__init__()
        if isinstance(channels, bool) or not isinstance(channels, int) or channels < 1:
            raise ValueError(f'channels must be an integer >= 1 (the output channels of the model), got {channels!r}')
        if isinstance(std, bool) or not isinstance(std, (int, float)) or not math.isfinite(std) or std <= 0:
            raise ValueError(f'std must be a finite number > 0 (the initial standard deviation of the noise), got {std!r}')
        if per_step is not False and (isinstance(per_step, bool) or not isinstance(per_step, int) or per_step < 1):
            raise ValueError(f'per_step must be False or the number of output times (an integer >= 1), got {per_step!r}')
        self.model = model
        shape = (channels,) if per_step is False else (per_step, channels)
        self.log_std = torch.nn.Parameter(torch.full(shape, math.log(float(std)), dtype=torch.float32))

    def forward(self, *args, **kwargs):
        return self.model(*args, **kwargs)

    @property
    def std(self):
        return self.log_std.detach().exp()


def _flat_log_std(noise, trailing, width):
    """noise.log_std as the (width,) vector of a prediction whose trailing axes `trailing` are flattened into the width: a tensor
    of the trailing shape (or already flat) as it is, (channels,) = trailing[-1:] repeated over the axes in front of it."""
    ls = noise.log_std
    if tuple(ls.shape) in (tuple(trailing), (width,)):
        return ls.reshape(width)
    if trailing and tuple(ls.shape) == (trailing[-1],):
        return ls.expand(trailing).reshape(width)
    raise ValueError(f'iwae_loss: noise.log_std has shape {tuple(ls.shape)} for a prediction of {tuple(trailing)} per path: expected '
                     f'{tuple(trailing[-1:])} (per channel) or {tuple(trailing)}')


def iwae_loss(samples, std=0.1, members=1, norm=False, noise=None):
    """loss_fn(pred, true) for `train_loop` / `GraphedStep` / `evaluate_metrics`: minus the mean importance-weighted bound
    (engine.sample_loglik) of a model solved with options={'samples': S} against a partially observed target - the multi-sample
    ELBO / IWAE objective on data with gaps.  pred and true as for `energy_loss`: (B S, ...) or (M, B S, ...), and (B, ...);
    trailing axes are flattened into the vector.  A NaN in true marks a missing entry (the mask is ~isnan(true)); data that
    carries its own mask is passed as true = (values, mask).  std is the standard deviation of the observation noise; norm
    divides each row's likelihood by its number of observed entries.
    noise: an `ObservationNoise`, or any object with a tensor `.log_std`, replaces the constant std by a learned scale per
    output channel (sample_loglik(log_std=)); it is read at every call, not captured by value, so a parameter that the optimizer
    updates in place is followed - also inside a recorded `GraphedStep`.  The trailing axes (T, out) of a prediction are
    flattened into the vector, component t out + c, so the (out,) log_std is tiled T times into a (T out,) vector - T out
    floats; the slab and the (B, T out) planes are not copied - and scored in the kernel's per-channel mode at width T out.
    noise together with a std other than the default is a ValueError."""
    from . import engine
    S = engine.check_samples(samples)
    if noise is not None:
        if isinstance(std, bool) or std != engine.LOGLIK_DEFAULT_STD:
            raise ValueError(f'iwae_loss: noise and std both describe the observation noise: give one of them (std is {std!r})')
        if not isinstance(getattr(noise, 'log_std', None), torch.Tensor):
            raise ValueError(f'iwae_loss: noise must have a tensor attribute log_std (an ObservationNoise), got {noise!r}')

    lead = 1 if members > 1 else 0      # (an Ensemble's leading member axis)

    def loss_fn(pred_y, true_y):
        true_y, mask = true_y if isinstance(true_y, (tuple, list)) else (true_y, None)
        want = ((members,) if lead else ()) + (S * true_y.shape[0],) if true_y.dim() else None
        if want is None or tuple(pred_y.shape[:lead + 1]) != want:
            raise ValueError(f'iwae_loss(samples={S}, members={members}): pred has shape {tuple(pred_y.shape)} for a target of shape '
                             f'{tuple(true_y.shape)}: expected {"(members, " if lead else "("}samples x target rows, ...)')
        if mask is not None and tuple(mask.shape) != tuple(true_y.shape):
            raise ValueError(f'iwae_loss: the mask has shape {tuple(mask.shape)} for a target of shape {tuple(true_y.shape)}')
        pred = pred_y.reshape(want + (-1,))
        true = true_y.reshape(true_y.shape[0], -1).to(pred.dtype)
        mask = None if mask is None else mask.reshape(true.shape).to(pred.dtype)
        if noise is None:
            return -engine.sample_loglik(pred, S, true, mask=mask, std=std, members=members, norm=norm).mean()
        ls = _flat_log_std(noise, tuple(pred_y.shape[lead + 1:]), pred.shape[-1]).to(pred.dtype)
        return -engine.sample_loglik(pred, S, true, mask=mask, members=members, norm=norm, log_std=ls).mean()
    return loss_fn


def mc_class_loss(samples, members=1, binary=False, pos_weight=None, class_weight=None, objective='predictive'):
    """loss_fn(pred, true) for `train_loop` / `GraphedStep` / `evaluate_metrics`: classification with a model solved with
    options={'samples': S} (engine.sample_class).  pred has one row of logits per path - (B S, C), or (M, B S, C) from an
    `Ensemble` of `members` = M models, whose paths are pooled; binary=True: one logit per path, (B S,) or (B S, 1) (the
    `SqueezeEnd` / BCEWithLogitsLoss layout).  true is (B,): integer class indices, or 0 / 1 of any dtype for binary; a label
    < 0 marks an unlabelled row, which adds 0.  objective='predictive' is the negative log-likelihood of the model average,
    -log((1 / N) sum_n softmax(z_n)[y]); 'expected' is the mean cross-entropy of the paths (what replicating the labels S times
    gives: the looser Jensen bound).  class_weight (C,) weighs the rows by the weight of their class; pos_weight (binary only)
    is class_weight = (1, pos_weight).  The reduction is the mean over the rows of true - BCEWithLogitsLoss's convention, NOT
    cross_entropy(weight=)'s division by the summed weights."""
    from . import engine
    S = engine.check_samples(samples)
    if objective not in ('predictive', 'expected'):
        raise ValueError(f"objective must be 'predictive' or 'expected', got {objective!r}")
    if pos_weight is not None and (not binary or class_weight is not None):
        raise ValueError('pos_weight belongs to binary=True and replaces class_weight: give one of the two')
    lead = 1 if members > 1 else 0      # (an Ensemble's leading member axis)
    weights = {}

    def weight(like):      # (per device and dtype, formed once: nothing is allocated inside a recorded step after the first)
        key = (like.device, like.dtype)
        if key not in weights:
            if pos_weight is not None:
                w = torch.cat([torch.ones(1), torch.as_tensor(pos_weight, dtype=torch.float32).detach().reshape(1).cpu()])
            else:
                w = torch.as_tensor(class_weight, dtype=torch.float32).detach()
            weights[key] = w.to(device=like.device, dtype=like.dtype)
        return weights[key]

    def loss_fn(pred_y, true_y):
        want = ((members,) if lead else ()) + (S * true_y.shape[0],) if true_y.dim() == 1 else None
        tail = tuple(pred_y.shape[lead + 1:])
        if want is None or tuple(pred_y.shape[:lead + 1]) != want or (tail not in ((), (1,)) if binary else len(tail) != 1):
            raise ValueError(f'mc_class_loss(samples={S}, members={members}, binary={bool(binary)}): pred has shape '
                             f'{tuple(pred_y.shape)} for labels of shape {tuple(true_y.shape)}: expected '
                             f'{"(members, " if lead else "("}samples x labels{")" if binary else ", classes)"}')
        pred = pred_y.reshape(want + (1,)) if binary else pred_y
        labels = true_y if not (true_y.dtype.is_floating_point or true_y.dtype == torch.bool) else true_y.to(torch.int32)
        w = None if pos_weight is None and class_weight is None else weight(pred)
        if objective == 'predictive':
            return engine.sample_class(pred, S, labels, members=members, binary=binary, class_weight=w).mean()
        return engine.sample_class(pred, S, labels, members=members, binary=binary, class_weight=w, stats=True).xent.mean()
    return loss_fn


class SqueezeEnd(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, *args, **kwargs):
        return self.model(*args, **kwargs).squeeze(-1)


def count_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def binary_ranking_metrics(scores, labels):
    """(AUROC, average precision) of binary labels from one descending sort on the scores' device; tied scores form one
    threshold (the convention of sklearn.metrics.roc_auc_score / average_precision_score)."""
    scores = scores.reshape(-1).double()
    labels = labels.reshape(-1).double()
    n_pos, n = labels.sum(), labels.numel()
    n_neg = n - n_pos
    if n == 0 or float(n_pos) == 0.0 or float(n_neg) == 0.0:
        return float('nan'), float('nan')
    order = torch.argsort(scores, descending=True, stable=True)
    s, y = scores[order], labels[order]
    last = torch.ones_like(s, dtype=torch.bool)          # last element of every run of equal scores
    last[:-1] = s[1:] != s[:-1]
    tp = torch.cumsum(y, 0)[last]
    fp = torch.cumsum(1.0 - y, 0)[last]
    zero = torch.zeros(1, dtype=tp.dtype, device=tp.device)
    tp0, fp0 = torch.cat([zero, tp]), torch.cat([zero, fp])
    auroc = torch.trapz(tp0 / n_pos, fp0 / n_neg)
    precision = tp / (tp + fp)
    ap = ((tp0[1:] - tp0[:-1]) / n_pos * precision).sum()
    return float(auroc), float(ap)


def _world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist
    return None


def evaluate_metrics(dataloader, model, times, loss_fn, num_classes, device, kwargs, samples=1, members=1):
    """One pass over `dataloader` (batches = (*coeffs, true_y, lengths)): loss, accuracy, confusion matrix and, for two
    classes, AUROC / average precision.  num_classes=None: regression (loss only).  One host synchronisation.
    samples=S, members=M with N = M S > 1: the model returns one row of logits per path ((B S, C), (M, B S, C); two classes:
    one logit per path); the guess is the argmax of the averaged probabilities (engine.sample_class; two classes: pbar(1) >
    0.5), the AUROC / AP scores are pbar(1), and the metrics gain `predictive_nll` and `mutual_information` (means over the
    rows)."""
    from . import engine
    pooled = num_classes is not None and engine.check_samples(samples) * members > 1
    dist = _world()
    with torch.no_grad():
        loss_sum = torch.zeros((), device=device, dtype=torch.float64)
        correct = torch.zeros((), device=device, dtype=torch.float64)
        extra = torch.zeros(2, device=device, dtype=torch.float64)      # (sums of predictive_nll, mutual_information)
        size = 0
        confusion = None if num_classes is None else torch.zeros(num_classes * num_classes, device=device, dtype=torch.int64)
        scores, labels = [], []
        for batch in dataloader:
            batch = tuple(b.to(device, non_blocking=True) for b in batch)
            *coeffs, true_y, lengths = batch
            pred_y = model(times, coeffs, lengths, **kwargs)
            bs = true_y.size(0)
            size += bs
            loss_sum += loss_fn(pred_y, true_y).double() * bs
            if num_classes is None:
                continue
            truth = true_y.to(torch.int64)
            if pooled:
                binary = num_classes == 2
                logits = pred_y.reshape(tuple(pred_y.shape[:2 if members > 1 else 1]) + (1,)) if binary else pred_y
                st = engine.sample_class(logits, samples, truth, members=members, binary=binary, stats=True)
                extra += torch.stack([st.nll.sum(), st.mutual_information.sum()]).double()
                guess = (st.probs[:, 0] > 0.5).to(torch.int64) if binary else torch.argmax(st.probs, dim=1)
                pred_y = st.probs[:, 0]      # (the score of the ranking metrics)
            else:
                guess = (pred_y > 0).to(torch.int64) if num_classes == 2 else torch.argmax(pred_y, dim=1)
            correct += (guess == truth).sum()
            confusion += torch.bincount(truth.reshape(-1) * num_classes + guess.reshape(-1), minlength=num_classes * num_classes)
            if num_classes == 2:
                scores.append(pred_y.detach().reshape(-1))
                labels.append(true_y.detach().reshape(-1))
        sums = torch.stack([loss_sum, correct, torch.tensor(float(size), device=device, dtype=torch.float64)])
        if dist is not None:
            dist.all_reduce(sums)
            if confusion is not None:
                dist.all_reduce(confusion)
        metrics = AttrDict(dataset_size=int(sums[2].item()))
        total = max(metrics.dataset_size, 1)
        metrics.loss = float(sums[0]) / total            # assumes 'mean' reduction in the loss function
        if pooled:
            if dist is not None:
                dist.all_reduce(extra)
            metrics.predictive_nll, metrics.mutual_information = float(extra[0]) / total, float(extra[1]) / total
        if num_classes is not None:
            metrics.accuracy = float(sums[1]) / total
            metrics.confusion = confusion.reshape(num_classes, num_classes).cpu().numpy().astype(np.float64)
        if num_classes == 2 and scores:
            sc, lb = torch.cat(scores), torch.cat(labels)
            if dist is not None:       # ragged all-gather through padding to the largest shard
                n = torch.tensor([sc.numel()], device=device)
                ns = [torch.zeros_like(n) for _ in range(dist.get_world_size())]
                dist.all_gather(ns, n)
                m = int(max(int(x) for x in ns))
                pad = lambda t: torch.cat([t, t.new_zeros(m - t.numel())])
                gs = [sc.new_zeros(m) for _ in ns]
                gl = [lb.new_zeros(m) for _ in ns]
                dist.all_gather(gs, pad(sc))
                dist.all_gather(gl, pad(lb))
                sc = torch.cat([g[:int(k)] for g, k in zip(gs, ns)])
                lb = torch.cat([g[:int(k)] for g, k in zip(gl, ns)])
            metrics.auroc, metrics.average_precision = binary_ranking_metrics(sc, lb)
        return metrics


class GraphedStep:
    """The training step of the loop below - forward, loss, backward, optimizer step - recorded into one CUDA/HIP graph per
    batch shape and replayed with each batch copied into the recording's input buffers (the step is launch-bound: ~60
    kernels; replaying takes about two thirds of the eager time).  The solver draws fresh Brownian increments
    on every replay from a device-resident Philox key (torchsde.prepare_graph_capture).  The first `warmup` batches of a
    shape run eagerly (on a side stream, as capture requires); a learning-rate change drops the recordings (the rate is a
    constant of the recorded optimizer kernel).  Needs an optimizer created with capturable=True."""

    def __init__(self, model, times, optimizer, loss_fn, kwargs, device, warmup=3, log=None):
        from . import torchsde as _T
        _T.prepare_graph_capture(device)
        self.model, self.times, self.opt, self.loss_fn, self.kwargs = model, times, optimizer, loss_fn, kwargs
        self.device, self.warmup = device, warmup
        self.entries, self.lrs = {}, None
        self.side = torch.cuda.Stream(device)
        self.replays = 0
        self.log = log or (lambda msg: None)
        self.disabled = None          # reason the recordings were given up (a model that is not capture-safe): eager steps from then on

    def _step(self, coeffs, y, lengths):
        pred = self.model(self.times, coeffs, lengths, **self.kwargs)
        loss = self.loss_fn(pred, y)
        loss.backward()
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)

    def _eager(self, coeffs, y, lengths):
        """One eager step with the reference loop's handling of a failing batch (common_sde.py:157-166: an AssertionError of a
        batch is reported and the loop goes on)."""
        try:
            self._step(list(coeffs), y, lengths)
        except AssertionError as exc:
            self.log('Caught AssertionError: ' + str(exc))
            self.opt.zero_grad(set_to_none=True)

    def __call__(self, coeffs, y, lengths):
        if self.disabled is not None:
            return self._eager(coeffs, y, lengths)
        lrs = tuple(float(g['lr']) for g in self.opt.param_groups)
        if lrs != self.lrs:
            self.entries, self.lrs = {}, lrs
        batch = tuple(coeffs) + (y, lengths)
        key = tuple((tuple(b.shape), b.dtype) for b in batch)
        entry = self.entries.setdefault(key, {'seen': 0, 'graph': None, 'static': None})
        if entry['graph'] is None:
            if entry['seen'] < self.warmup:          # eager steps of this shape, on the side stream
                entry['seen'] += 1
                self.side.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self.side):
                    self._eager(coeffs, y, lengths)
                torch.cuda.current_stream(self.device).wait_stream(self.side)
                return
            static = tuple(b.clone() for b in batch)
            torch.cuda.synchronize(self.device)
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._step(list(static[:-2]), static[-2], static[-1])
            except Exception as exc:                  # a host sync, .item(), an allocation the capture cannot take, a failing batch ...
                self.disabled = f'{type(exc).__name__}: {exc}'
                self.log('GraphedStep: the training step cannot be recorded (' + self.disabled.splitlines()[0] +
                         '); eager steps from here on')
                self.entries = {}
                torch.cuda.synchronize(self.device)
                self.opt.zero_grad(set_to_none=True)  # (nothing of the failed recording ran; drop gradients it may have allocated)
                return self._eager(coeffs, y, lengths)
            entry['graph'], entry['static'] = graph, static
            graph.replay()                            # (the capture itself does not execute: run this batch's step now)
            self.replays += 1
            return
        for dst, src in zip(entry['static'], batch):
            dst.copy_(src, non_blocking=True)
        entry['graph'].replay()
        self.replays += 1


def train_loop(train_dataloader, val_dataloader, model, times, optimizer, loss_fn, max_epochs, num_classes, device, kwargs,
               step_mode, log=None, plateau_terminate=None, graph_steps=False, samples=1, members=1):
    """The reference's epoch loop (common_sde.py:107-216).  Returns the history; `model` ends with the best parameters
    (validation accuracy for classification, validation loss for regression).  graph_steps=True replays the training step
    from a CUDA/HIP graph (GraphedStep; one process, CUDA, optimizer with capturable=True).  samples, members: the sample
    paths per row and ensemble members behind the model's logits, for `evaluate_metrics`."""
    modes = {'trainloss': 'min', 'valloss': 'min', 'valaccuracy': 'max', 'valauc': 'max', 'none': None}
    if step_mode not in modes:
        raise ValueError(f'step_mode must be one of {sorted(modes)}')
    scheduler = None
    if modes[step_mode] is not None:
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=5, mode=modes[step_mode])
    if plateau_terminate is None:
        plateau_terminate = 100 if step_mode == 'none' else 50
    log = log or (lambda msg: None)
    model.train()
    best_state = copy.deepcopy(model.state_dict())
    best_train_loss, best_train_loss_epoch = math.inf, 0
    best_train_accuracy, best_train_accuracy_epoch = 0.0, 0
    best_val = -math.inf
    history = []
    graphed = GraphedStep(model, times, optimizer, loss_fn, kwargs, torch.device(device), log=log) if graph_steps else None
    for epoch in range(max_epochs):
        sampler = getattr(train_dataloader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)
        for batch in train_dataloader:
            batch = tuple(b.to(device, non_blocking=True) for b in batch)
            *train_coeffs, train_y, lengths = batch
            if graphed is not None:
                graphed(train_coeffs, train_y, lengths)
                continue
            try:
                pred_y = model(times, train_coeffs, lengths, **kwargs)
                loss = loss_fn(pred_y, train_y)
                loss.backward()
                optimizer.step()
                optimizer.zero_grad(set_to_none=True)
            except AssertionError as exc:          # the reference swallows assertion failures of a batch and goes on
                log('Caught AssertionError: ' + str(exc))
                optimizer.zero_grad(set_to_none=True)
        model.eval()
        train_metrics = evaluate_metrics(train_dataloader, model, times, loss_fn, num_classes, device, kwargs, samples, members)
        val_metrics = evaluate_metrics(val_dataloader, model, times, loss_fn, num_classes, device, kwargs, samples, members)
        model.train()
        if train_metrics.loss * 1.0001 < best_train_loss:
            best_train_loss, best_train_loss_epoch = train_metrics.loss, epoch
        if num_classes is not None and train_metrics.accuracy > best_train_accuracy * 1.001:
            best_train_accuracy, best_train_accuracy_epoch = train_metrics.accuracy, epoch
        score = val_metrics.accuracy if num_classes is not None else -val_metrics.loss
        if score > best_val:
            best_val = score
            best_state = copy.deepcopy(model.state_dict())
        line = f'Epoch: {epoch}  Train loss: {train_metrics.loss:.3}'
        if num_classes is not None:
            line += f'  Train accuracy: {train_metrics.accuracy:.3}'
        if 'auroc' in train_metrics:
            line += f'  Train auroc: {train_metrics.auroc:.3}'
        line += f'  Val loss: {val_metrics.loss:.3}'
        if num_classes is not None:
            line += f'  Val accuracy: {val_metrics.accuracy:.3}'
        if 'auroc' in val_metrics:
            line += f'  Val auroc: {val_metrics.auroc:.3}'
        log(line)
        if scheduler is not None:
            scheduler.step({'trainloss': train_metrics.loss, 'valloss': val_metrics.loss,
                            'valaccuracy': val_metrics.get('accuracy', 0.0), 'valauc': val_metrics.get('auroc', 0.0)}[step_mode])
        history.append(AttrDict(epoch=epoch, train_metrics=train_metrics, val_metrics=val_metrics,
                                lr=optimizer.param_groups[0]['lr']))
        if epoch > best_train_loss_epoch + plateau_terminate:
            log(f'Breaking because of no improvement in training loss for {plateau_terminate} epochs.')
            break
        if num_classes is not None and epoch > best_train_accuracy_epoch + plateau_terminate:
            log(f'Breaking because of no improvement in training accuracy for {plateau_terminate} epochs.')
            break
    model.load_state_dict(best_state)       # in-place copies: the solver's parameter arena stays where it is
    return history


class _Encoder(json.JSONEncoder):
    def default(self, o):
        if isinstance(o, (torch.Tensor, np.ndarray)):
            return o.tolist()
        return super().default(o)


def save_results(directory, name, result):
    """results-sde/<name>/<run number> (JSON), as the reference's _save_results."""
    loc = os.path.join(directory, name)
    os.makedirs(loc, exist_ok=True)
    num = max([int(f) for f in os.listdir(loc) if f.isdigit()] + [-1]) + 1
    out = {k: v for k, v in result.items() if not k.endswith('_dataloader')}
    out['model'] = str(out['model'])
    path = os.path.join(loc, str(num))
    with open(path, 'w') as f:
        json.dump(out, f, cls=_Encoder)
    return path


def make_model(name, input_channels, output_channels, hidden_channels, hidden_hidden_channels, num_hidden_layers,
               use_intensity=False, initial=True):
    """common_sde.make_model for the SDE entries (common_sde.py:301-342): returns a factory () -> (model, vector field);
    `use_intensity` belongs to the reference's non-SDE baselines (GRU-ODE etc.) and is ignored."""
    def factory():
        return modules.make_sde_model(name, input_channels, output_channels, hidden_channels, hidden_hidden_channels,
                                      num_hidden_layers, initial=initial)
    return factory


def main(name, model_name, times, train_dataloader, val_dataloader, test_dataloader, device, make_model, num_classes,
         max_epochs, lr, kwargs, step_mode, pos_weight=torch.tensor(1), results_dir=None, log=print, regularise='l2',
         graph_steps=None, shard_invariant=False, loss=None, samples=1, members=1):
    """common_sde.main (common_sde.py:248-298): build, train, evaluate; `num_classes=None` trains a regression model with
    the mean-squared error (the forecasting benchmark).  Results are written only when `name` and `results_dir` are set.
    graph_steps: replay the training step from a CUDA/HIP graph (GraphedStep) - the step of these models is bound by the host
    (whole-model neurallnsde step: 1.43 ms eager, 0.88 ms replayed, 0.61 ms for its solve).  None (default) = wherever it is eligible:
    one process, CUDA device; False = eager steps; True = required where eligible (still eager under DDP / on the CPU).
    shard_invariant (default off): every solve passes options={'global_rows': 'world'} - under a process group the kernels are
    planned for world_size x the local batch, so each rank's rows evolve as they would in the unsharded batch on one device.
    loss: a callable loss(pred, true) that replaces the default base loss (e.g. `crps_loss(S)` for a model solved with
    options={'samples': S}); the weight regulariser is added to it as to the default.
    samples, members: what `evaluate_metrics` needs to read a classifier's logits when they come one row per sample path
    (`main(..., loss=mc_class_loss(S), samples=S)` with kwargs options={'samples': S, 'sample_grad': True})."""
    device = torch.device(device)
    if shard_invariant:
        kwargs = dict(kwargs, options=dict(kwargs.get('options') or {}, global_rows='world'))
    times = times.to(device)
    on_gpu = device.type == 'cuda'
    baseline_memory = None
    if on_gpu:
        torch.cuda.reset_peak_memory_stats(device)
        baseline_memory = torch.cuda.memory_allocated(device)
    model, regularise_parameters = make_model()
    if num_classes == 2:
        model = SqueezeEnd(model)
        base_loss = torch.nn.BCEWithLogitsLoss(pos_weight=pos_weight.to(device))
    elif num_classes is None:
        base_loss = torch.nn.functional.mse_loss
    else:
        base_loss = torch.nn.functional.cross_entropy
    if loss is not None:
        base_loss = loss
    loss_fn = add_weight_regularisation(base_loss, regularise_parameters, mode=regularise)
    model.to(device)
    dist = _world()
    net = model
    if dist is not None:
        net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[device.index] if on_gpu else None)
    # same update rule as the reference's Adam (common_sde.py:287); on the GPU the single-launch implementation instead of
    # the default multi-tensor one (~15 launches per step for these models)
    graph_steps = (graph_steps is None or bool(graph_steps)) and on_gpu and dist is None
    optimizer = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=lr * 0.01, fused=True if on_gpu else None,
                                 capturable=graph_steps)
    history = train_loop(train_dataloader, val_dataloader, net, times, optimizer, loss_fn, max_epochs, num_classes, device,
                         kwargs, step_mode, log=log if (dist is None or dist.get_rank() == 0) else None, graph_steps=graph_steps,
                         samples=samples, members=members)
    net.eval()
    train_metrics = evaluate_metrics(train_dataloader, net, times, loss_fn, num_classes, device, kwargs, samples, members)
    val_metrics = evaluate_metrics(val_dataloader, net, times, loss_fn, num_classes, device, kwargs, samples, members)
    test_metrics = evaluate_metrics(test_dataloader, net, times, loss_fn, num_classes, device, kwargs, samples, members)
    memory_usage = torch.cuda.max_memory_allocated(device) - baseline_memory if on_gpu else None
    result = AttrDict(name=name, model_name=model_name, times=times, memory_usage=memory_usage,
                      baseline_memory=baseline_memory, num_classes=num_classes, train_dataloader=train_dataloader,
                      val_dataloader=val_dataloader, test_dataloader=test_dataloader, model=model,
                      parameters=count_parameters(model), history=history, train_metrics=train_metrics,
                      val_metrics=val_metrics, test_metrics=test_metrics)
    if name is not None and results_dir is not None and (dist is None or dist.get_rank() == 0):
        result.saved_to = save_results(results_dir, name, result)
    return result


# the reference's private names
_add_weight_regularisation = add_weight_regularisation
_evaluate_metrics = evaluate_metrics
_train_loop = train_loop
_SqueezeEnd = SqueezeEnd
_AttrDict = AttrDict
_count_parameters = count_parameters
