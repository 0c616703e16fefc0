#!/usr/bin/env python
"""Routing table of the library's host-only queries: tests/golden/routes.npz.

A few thousand snsde_solve descriptors - a seeded random sample over the shapes, options, methods, `kernel` values, batch sizes
(the 32-bit save-offset edge included), flags, variant switches, supplied tables and training-mode pointers, plus the BASELINE.json
workloads and the (input_option, noise_option) pairs of the reference's make_model - and, for each, the answers of every query that
decides or reports a kernel family without touching the GPU:

  snsde_forward_path, snsde_backward_supported, snsde_workspace_bytes, snsde_backward_workspace_bytes,
  snsde_save_layout (return code, act_slots, stage_planes, delta_slots), snsde_param_gradients_workspace_bytes.

None of these queries dereferences a pointer of the descriptor: the device pointers are set to small dummy values where a case
needs them non-null (training mode, a supplied table, a device-resident Philox key).  tests/test_routes_cpu.py replays every row
against the current library; a routing change shows up there as the rows it moved.

Run from the repo root against a built library:  python tests/golden/make_route_golden.py
(SNSDE_LIB=/path/to/libsnsde.so picks another build, e.g. the one of the commit a change starts from.)
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# descriptor columns (int64); `ptrs` is a bit set over PTRS: which pointer fields are non-null
FIELDS = ('C', 'H', 'HH', 'NL', 'io', 'no', 'act', 'drift', 'diff', 'timef', 'batch', 'knots', 'n_steps', 'n_out', 'method',
          'kernel', 'flags', 'kl_column1', 'ptrs')
PTRS = ('noise_table', 'act_save', 'traj', 'dW_out', 'stage_save', 'dU_out', 'dW', 'dU', 'seed_dev', 'srk_tab', 'z0_weight',
        'z0_bias', 'workspace')
TRAIN = ('act_save', 'traj', 'dW_out', 'stage_save', 'dU_out')
ANSWERS = ('forward_path', 'backward_supported', 'workspace_bytes', 'backward_workspace_bytes', 'save_layout_rc', 'act_slots',
           'stage_planes', 'delta_slots', 'param_gradients_workspace_bytes')


def _bits(names):
    return sum(1 << PTRS.index(n) for n in names)


def _row(C_, H, NL, io, no, batch, method, kernel=0, flags=0, HH=None, act=0, drift=0, diff=0, timef=0, knots=101, n_steps=100,
         n_out=2, kl_column1=0, ptrs=()):
    d = dict(C=C_, H=H, HH=H if HH is None else HH, NL=NL, io=io, no=no, act=act, drift=drift, diff=diff, timef=timef, batch=batch,
             knots=knots, n_steps=n_steps, n_out=n_out, method=method, kernel=kernel, flags=flags, kl_column1=kl_column1,
             ptrs=_bits(ptrs) | _bits(('workspace',)))
    return [d[f] for f in FIELDS]


def descriptors(seed=20261016, n_random=3600):
    rows = []
    # BASELINE.json workloads (K1 the tutorial's Neural LSDE field, K2 LNSDE, K3 GSDE, K4 the sepsis-shaped 3_18, K5 Milstein at
    # H = 256) and the pairs make_model builds, under every `kernel` value, inference and training, with the A/B flags
    base = [(1, 32, 2, 3, 0, 256, 50, dict(act=1, drift=1, diff=1, timef=1)),          # K1: compose_ode (LipSwish, linear drift)
            (1, 32, 2, 4, 12, 256, 50, dict(drift=1, diff=1, noise_table=True)),       # K1: LatentSDE mapping (supplied table)
            (21, 128, 2, 4, 17, 1024, 100, {}), (21, 128, 2, 6, 17, 4096, 200, {}), (34, 64, 2, 3, 18, 2048, 100, {}),
            (21, 256, 2, 4, 17, 1024, 100, {})]
    for C_, H, NL, io, no, B, N, extra in base:
        extra = dict(extra)
        table = extra.pop('noise_table', False)
        for method in (0, 1, 2):
            for kernel in range(6):
                for flags in (0, 4, 8):
                    for train in (False, True):
                        ptrs = (TRAIN if train else ()) + (('noise_table',) if table else ()) + (('srk_tab',) if method == 2 else ())
                        rows.append(_row(C_, H, NL, io, no, B, method, kernel, flags, knots=N + 1, n_steps=N, ptrs=ptrs, **extra))
    for io, no in ((1, 0), (1, 18), (2, 16), (4, 17), (6, 17)):
        for method in (0, 1, 2):
            for H in (16, 32, 64, 128, 256):
                for B in (256, 1024, 4096):
                    for C_ in (21, 69):
                        for train in (False, True):
                            rows.append(_row(C_, H, 2, io, no, B, method, ptrs=TRAIN if train else ()))
    # the seeded sample
    rng = np.random.default_rng(seed)
    Hs, Cs = (16, 32, 48, 64, 128, 256), (2, 5, 14, 21, 33, 69, 81)
    for _ in range(n_random):
        H = int(rng.choice(Hs))
        HH = H if rng.random() < 0.95 else H // 2 + 8
        io, no, method, kernel = int(rng.integers(0, 7)), int(rng.integers(0, 20)), int(rng.integers(0, 3)), int(rng.integers(0, 6))
        r = rng.random()
        if r < 0.15:                       # the 32-bit save-offset edge: 16 B H >= 2^32 <=> B H >= 2^28
            edge = (1 << 28) // H
            B = int(min(edge + int(rng.integers(-1, 1)), 1 << 21))
        elif r < 0.3:                      # the wave-pair / flavour thresholds
            B = int(rng.choice((4, 37, 1024, 2048, 6143, 6144, 6145, 8192)))
        else:
            B = int(np.exp(rng.uniform(np.log(4), np.log(1 << 21))))
        flags = int(sum(f for f in (1, 2, 4, 8) if rng.random() < 0.25))
        act = drift = diff = timef = 0
        if rng.random() < 0.3:             # the variant switches of the tutorial fields
            act, drift, timef = int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 2))
            diff = int(rng.integers(0, 3)) if no in (18, 19) else int(rng.integers(0, 2))
        ptrs = []
        if rng.random() < 0.2:
            ptrs.append('noise_table')
            if rng.random() < 0.7:
                no = int(rng.choice((12, 13)))
        kl = 0
        if rng.random() < 0.15:
            kl = int(rng.integers(2, H + 1))
            if rng.random() < 0.6:         # the LatentSDE mapping the kl column serves
                no, drift, diff, io = 12, 1, 1, int(rng.choice((1, 3, 4)))
                if 'noise_table' not in ptrs:
                    ptrs.append('noise_table')
        if rng.random() < 0.5:
            ptrs += list(TRAIN)
        for p in ('seed_dev', 'dW', 'z0_weight'):
            if rng.random() < 0.2:
                ptrs.append(p)
        if 'z0_weight' in ptrs:
            ptrs.append('z0_bias')
        if 'dW' in ptrs and method == 2:
            ptrs.append('dU')
        if method == 2:
            ptrs.append('srk_tab')
        knots = int(rng.choice((9, 33, 101)))
        n_steps = knots - 1 if rng.random() < 0.7 else int(rng.integers(1, 3 * knots))
        rows.append(_row(int(rng.choice(Cs)), H, int(rng.integers(1, 6)), io, no, B, method, kernel, flags, HH=HH, act=act,
                         drift=drift, diff=diff, timef=timef, knots=knots, n_steps=n_steps, n_out=int(rng.integers(2, 5)),
                         kl_column1=kl, ptrs=ptrs))
    return np.array(rows, np.int64)


def solve_struct(row):
    from stable_neural_sdes_amd import _lib
    d = dict(zip(FIELDS, (int(v) for v in row)))
    s = _lib.Solve()
    s.model = _lib.Model(d['C'], d['H'], d['HH'], d['NL'], d['io'], d['no'], d['act'], d['drift'], d['diff'], d['timef'])
    for f in ('batch', 'knots', 'n_steps', 'n_out', 'method', 'kernel', 'flags', 'kl_column1'):
        setattr(s, f, d[f])
    for i, p in enumerate(PTRS):
        if d['ptrs'] >> i & 1:
            setattr(s, p, C.c_void_p(256 * (i + 1)))      # never dereferenced by a host-only query
    return s


def answers(row):
    """The host-only queries' answers for one descriptor row (ANSWERS order)."""
    from stable_neural_sdes_amd import _lib
    lib = _lib.lib()
    s = solve_struct(row)
    b = _lib.Backward()
    b.fwd = s
    a, p, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = lib.snsde_save_layout(C.byref(s), C.byref(a), C.byref(p), C.byref(d))
    return [lib.snsde_forward_path(C.byref(s)), lib.snsde_backward_supported(C.byref(s)), lib.snsde_workspace_bytes(C.byref(s)),
            lib.snsde_backward_workspace_bytes(C.byref(b)), rc, a.value, p.value, d.value,
            lib.snsde_param_gradients_workspace_bytes(C.byref(b))]


def main():
    desc = descriptors()
    ans = np.array([answers(r) for r in desc], np.int64)
    out = os.path.join(HERE, 'routes.npz')
    np.savez_compressed(out, desc=desc, answers=ans, fields=np.array(FIELDS), ptrs=np.array(PTRS), answer_names=np.array(ANSWERS))
    print(out, desc.shape, os.path.getsize(out), 'bytes;', 'paths:', np.bincount(ans[:, 0]).tolist(),
          'backward modes:', np.bincount(ans[:, 1]).tolist())


if __name__ == '__main__':
    main()
