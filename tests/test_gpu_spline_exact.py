"""The two HIP spline construction kernels (snsde_natural_cubic_coeffs, snsde_hermite_coeffs, through `engine.spline_coeffs`, i.e.
the C ABI) against the exact-rational known answers of tests/golden/spline_exact.npz.  The fixture is the only input.

Each case (one `times` vector, S series, L <= 12) is laid out as (B, L, C) three ways:

    per series   (1, L, 1), S launches;
    padded       (ceil(S / 5), L, 5), series repeated to fill the last row;
    two blocks   (43, L, 3) = 129 series in a fixed shuffled order: the kernels launch 128 lanes per block with [L][S] workspaces,
                 so this is one full block plus one lane of a second.

Asserted for both kernels and every layout (tests/spline_exact_cases.check): finite output; the float32 bound (4 x the float32
oracle's own error against the exact values, per kind and component - nothing in it comes from a kernel); exact 0.0 where exact
arithmetic and any correct float32 construction give 0; the float32 image of the rational, bit for bit, on the series where no
float32 operation rounds.  Every copy of a series, in whichever (b, c) slot and layout it sits, returns the same bits: that covers
the neighbour-lane workspace indexing and the strided reads.  And kernel and host tensor-op path agree within twice the bound on
the same inputs, because each is within the bound of the exact value.

Measured on one MI355X (profiles/spline_exact_margins.txt): in every case and layout the kernels' error equals the float32
oracle's (largest ratio to e32: 1.00, allowed 4), and the Hermite kernel agrees with the host path bit for bit."""
import signal

import numpy as np
import pytest
import torch

from stable_neural_sdes_amd import engine
from tests import spline_exact_cases as E

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    def fire(*_):
        raise TimeoutError('exact-spline GPU test exceeded its time limit')
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(60)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def layouts(tag):
    """[(label, [(B, C, rows)])]: `rows` (B * C,) names the case's series that sits in slot b * C + c."""
    S = E.case(tag)['X'].shape[0]
    padded_B = -(-S // 5)
    shuffled = np.random.default_rng(129).permutation(129) % S
    return [('hip 1x1', [(1, 1, np.array([s])) for s in range(S)]),
            ('hip Bx5', [(padded_B, 5, np.arange(padded_B * 5) % S)]),
            ('hip 43x3', [(43, 3, shuffled)])]


_KERNEL = {}


def kernel(kind, tag):
    """{label: (rows, coefficients (len(rows), L-1, 4) float32)} from the kernel, computed once per (kind, case)."""
    if (kind, tag) not in _KERNEL:
        c = E.case(tag)
        t = torch.from_numpy(c['times'].copy()).to(DEV)
        L = c['times'].shape[0]
        res = {}
        for label, calls in layouts(tag):
            rows_all, got_all = [], []
            for B, Cn, rows in calls:
                X = np.ascontiguousarray(c['X'][rows].reshape(B, Cn, L).transpose(0, 2, 1))        # (B, L, C)
                out = engine.spline_coeffs(t, torch.from_numpy(X).to(DEV), kind)
                torch.cuda.synchronize()
                assert out.dtype == torch.float32 and tuple(out.shape) == (B, L - 1, 4 * Cn)
                rows_all.append(rows)
                got_all.append(E.as_series(out.cpu().numpy(), Cn))
            res[label] = (np.concatenate(rows_all), np.concatenate(got_all))
        _KERNEL[(kind, tag)] = res
    return _KERNEL[(kind, tag)]


@pytest.mark.parametrize('tag', E.CASES)
@pytest.mark.parametrize('kind', E.KINDS)
def test_kernel_against_the_exact_values_in_every_layout(kind, tag):
    res = kernel(kind, tag)
    S = E.case(tag)['X'].shape[0]
    for label, (rows, got) in res.items():
        assert set(rows.tolist()) == set(range(S))           # every series of the case is in every layout
        E.check(kind, tag, got, label, series=rows)


@pytest.mark.parametrize('tag', E.CASES)
@pytest.mark.parametrize('kind', E.KINDS)
def test_every_copy_of_a_series_returns_the_same_bits(kind, tag):
    res = kernel(kind, tag)
    rows = np.concatenate([r for r, _ in res.values()])
    bits = np.concatenate([g for _, g in res.values()]).view(np.uint32)
    first = {}
    for i, s in enumerate(rows.tolist()):
        first.setdefault(s, i)
    ref = bits[[first[s] for s in rows.tolist()]]
    bad = np.flatnonzero((bits != ref).any(axis=(1, 2)))
    assert len(rows) == E.case(tag)['X'].shape[0] + 5 * (-(-E.case(tag)['X'].shape[0] // 5)) + 129
    assert bad.size == 0, (kind, tag, 'copies that differ from the first copy of their series (flat index, series)',
                           [(int(i), int(rows[i])) for i in bad[:8]])


@pytest.mark.parametrize('tag', E.CASES)
@pytest.mark.parametrize('kind', E.KINDS)
def test_kernel_and_host_tensor_ops_agree_within_twice_the_bound(kind, tag, monkeypatch):
    """The CPU / GPU disagreement a natural spline through two knots produced.  Host path: CPU float32 tensors, and the same
    statements on the GPU (the route an X that requires grad takes under SNSDE_SPLINE_GRAD=torch)."""
    rows, got = kernel(kind, tag)['hip Bx5']
    S = E.case(tag)['X'].shape[0]
    got = got[:S]
    assert (rows[:S] == np.arange(S)).all()
    allowed = 2 * E.BOUND_FACTOR * E.e32(kind) * E.scales(kind, tag)
    monkeypatch.setenv('SNSDE_SPLINE_GRAD', 'torch')
    for label, host in (('host cpu', E.host_coeffs(kind, tag)),
                        ('host gpu', E.host_coeffs(kind, tag, device=DEV, requires_grad=True))):
        diff = np.abs(got.astype(np.float64) - host.astype(np.float64)).max(axis=(0, 1))
        E.report(f'{kind:8s} {tag:12s} hip - {label}  ' + '  '.join(f'{v:.3e}' for v in diff) + '   allowed  '
                 + '  '.join(f'{v:.3e}' for v in allowed))
        assert np.isfinite(host).all()
        assert (diff <= allowed).all(), (kind, tag, label, diff, allowed)
        zero = E.case(tag)['zero_' + kind]
        assert (host[zero] == 0.0).all() and (got[zero] == 0.0).all(), (kind, tag, label)
