#!/usr/bin/env python
"""Golden vectors of the interpolation benchmark's training objective (build container only; needs /root/reference).

Run:  python tests/golden/make_loglik_golden.py        (writes tests/golden/loglik.npz)

The reference's benchmark_interpolation/utils.py is imported from where it lies, over empty stand-ins for the packages it
imports at module level and that are absent here (physionet, person_activity, sklearn, torchcde: none of them is touched by the
three functions called).  The fixture holds data only: seeded inputs in the reference's sample-major (k, B, T, D) layout with
zero-filled missing entries, and what the reference's own log_normal_pdf / compute_losses / mean_squared_error give for them,
with the training loop's loss line (sde_interpolation.py:209, inline there) applied to those results.  float32 throughout, as
the benchmark runs."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G      # noqa: E402

B, T, D, STD = 4, 5, 3, 0.1


def load_utils():
    names = {'physionet': ('PhysioNet', 'get_data_min_max', 'variable_time_collate_fn2'), 'person_activity': ('PersonActivity',),
             'sklearn': ('model_selection', 'metrics'), 'torchcde': ()}
    for name, attrs in names.items():
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location('ref_interp_utils', os.path.join(G.REF_ROOT, 'benchmark_interpolation', 'utils.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    torch.set_num_threads(1)
    ref = load_utils()
    gen = torch.Generator().manual_seed(2024)
    out = {'std': np.float64(STD)}
    for k in (1, 3):
        data = torch.randn(B, T, D, generator=gen)
        mask = (torch.rand(B, T, D, generator=gen) > 0.4).float()
        mask[:, 0, 0] = 1.0                                   # (every row observes something: args.norm divides by the count)
        data = data * mask                                    # zero-filled missing entries, as the benchmark's loaders leave them
        pred = data.unsqueeze(0) + 0.15 * torch.randn(k, B, T, D, generator=gen)
        qm, qlv = 0.3 * torch.randn(B, 2, 4, generator=gen), 0.2 * torch.randn(B, 2, 4, generator=gen)
        batch = torch.cat([data, mask, torch.linspace(0, 1, T).expand(B, T).unsqueeze(-1)], dim=-1)
        out[f'k{k}/data'], out[f'k{k}/mask'], out[f'k{k}/pred'] = G.npy(data), G.npy(mask), G.npy(pred)
        out[f'k{k}/qz0_mean'], out[f'k{k}/qz0_logvar'] = G.npy(qm), G.npy(qlv)
        noise_logvar = 2.0 * torch.log(torch.zeros(pred.size()) + STD)
        out[f'k{k}/pdf'] = G.npy(ref.log_normal_pdf(data, pred, noise_logvar, mask))      # (k, B, T, D): the per-element terms
        out[f'k{k}/mse'] = G.npy(ref.mean_squared_error(data, pred.mean(0), mask))
        for norm in (False, True):
            args = types.SimpleNamespace(std=STD, norm=norm, k_iwae=k)
            logpx, kl = ref.compute_losses(D, batch, qm, qlv, pred, args, 'cpu')
            key = f'k{k}/norm{int(norm)}'
            out[f'{key}/logpx'], out[f'{key}/analytic_kl'] = G.npy(logpx), G.npy(kl)
            for kl_coef in (0.0, 0.5):
                loss = -(torch.logsumexp(logpx - kl_coef * kl, dim=0).mean(0) - np.log(args.k_iwae))
                out[f'{key}/loss_kl{kl_coef}'] = G.npy(loss)
                print(f'k={k} norm={norm} kl_coef={kl_coef}: loss {float(loss):.4f} mse {float(out[f"k{k}/mse"]):.5f}')
    G.save('loglik.npz', out)


if __name__ == '__main__':
    main()
