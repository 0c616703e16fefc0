"""engine.SolveConfig, and every plan query built from it, against the answers of the commit before the record existed.

tests/golden/plans.npz holds, for the grid of tests/golden/make_plan_golden.py, what engine.forward_path, engine.forward_kernel /
engine.backward_kernel on engine.query_descriptor and engine.backward_mode answered on that commit, and the descriptor fields they
asked with.  The library is the same; only the host code that writes the descriptors changed.  No GPU: the queries are host-side."""
import importlib.util
import os

import numpy as np
import pytest

from stable_neural_sdes_amd import _lib, engine

HERE = os.path.dirname(os.path.abspath(__file__))
FIELD_COLUMNS = ('flags', 'members', 'samples', 'global_rows', 'method', 'kernel')
ANSWER_COLUMNS = ('forward_path', 'forward_kernel', 'backward_kernel', 'backward_mode')


def _maker():
    spec = importlib.util.spec_from_file_location('make_plan_golden', os.path.join(HERE, 'golden', 'make_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def plans():
    """(maker module, rows of the grid, golden columns, the same columns recomputed with this tree's engine)."""
    mk = _maker()
    rows = list(mk.grid())
    golden = dict(np.load(os.path.join(HERE, 'golden', 'plans.npz')))
    assert tuple(golden) == mk.COLUMNS and all(len(v) == len(rows) for v in golden.values())
    now = mk.table(engine, rows)
    return mk, rows, golden, {c: now[:, i] for i, c in enumerate(mk.COLUMNS)}


def test_the_golden_covers_every_path_and_mode(plans):
    mk, rows, golden, _ = plans
    assert os.path.getsize(os.path.join(HERE, 'golden', 'plans.npz')) < 1 << 20
    assert set(golden['forward_path'].tolist()) == set(range(len(_lib.PATHS)))
    assert set(golden['backward_mode'].tolist()) == {0, 1, 2}
    assert np.count_nonzero(golden['forward_path'] != _lib.PATHS.index('none')) * 10 >= len(rows)


def test_every_answer_is_the_parents(plans):
    _, rows, golden, now = plans
    for c in ANSWER_COLUMNS:
        moved = np.flatnonzero(golden[c] != now[c])
        assert moved.size == 0, (c, moved.size, rows[moved[0]], int(golden[c][moved[0]]), int(now[c][moved[0]]))


def _canonical(mk, row):
    """The row as SolveConfig normalises it: members / samples of 1 are 0, opt-ins without their carrier are cleared."""
    return dict(row, members=0 if row['members'] == 1 else row['members'], samples=0 if row['samples'] == 1 else row['samples'],
                opt_ins=mk.carriers(row))


def test_descriptor_fields_are_the_parents_where_nothing_is_dropped(plans):
    """Rows on which the record drops nothing (members and samples are 0 or > 1, every set opt-in has its carrier): the descriptor's
    fields are the parent's.  The other rows are degenerate - the parent's query_descriptor wrote members = 1 / samples = 1 and
    flags the library ignores there - and now ask with the descriptor of their canonical row: the same row with members / samples of 1
    as 0 and the ineffective opt-ins cleared.  test_every_answer_is_the_parents shows no answer moved on them."""
    mk, rows, golden, now = plans
    same = np.array([_canonical(mk, r) == r for r in rows])
    assert 0 < np.count_nonzero(same) < len(rows)
    for c in FIELD_COLUMNS:
        moved = np.flatnonzero(same & (golden[c] != now[c]))
        assert moved.size == 0, (c, moved.size, rows[moved[0]], int(golden[c][moved[0]]), int(now[c][moved[0]]))
    degenerate = np.flatnonzero(~same)
    canon = mk.table(engine, [_canonical(mk, rows[i]) for i in degenerate])
    for i, c in enumerate(mk.COLUMNS):
        moved = np.flatnonzero(now[c][degenerate] != canon[:, i])
        assert moved.size == 0, (c, moved.size, rows[degenerate[moved[0]]])


def _config(**kw):
    model = engine.model_struct(3, 64, 64, 2, 4, 17)
    args = dict(model=model, batch=24, knots=8, n_steps=6, n_out=2)
    args.update(kw)
    return engine.SolveConfig.of(**args)


def test_one_member_and_one_sample_are_none():
    assert _config(members=1) == _config(members=0) == _config()
    assert _config(samples=1) == _config(samples=0) == _config()
    assert _config(members=3).members == 3 and _config(samples=2).samples == 2


def test_opt_ins_without_their_carrier_are_dropped():
    plain = _config()
    for name in ('sample_grad', 'bf16_grad', 'ensemble_grad', 'ensemble_samples', 'ensemble_nets', 'ensemble_nets_grad'):
        assert _config(**{name: True}) == plain, name
        assert _config(members=1, samples=1, **{name: True}) == plain, name
    assert _config(samples=2, sample_grad=True).sample_grad and _config(precision='bf16', bf16_grad=True).bf16_grad
    for name in ('ensemble_grad', 'ensemble_nets', 'ensemble_nets_grad'):
        assert getattr(_config(members=3, **{name: True}), name)
    assert not _config(members=3, ensemble_samples=True).ensemble_samples and not _config(samples=2, ensemble_samples=True).ensemble_samples
    assert _config(members=3, samples=2, ensemble_samples=True).ensemble_samples


def test_unknown_method_kernel_and_precision_raise_as_before():
    with pytest.raises(KeyError):
        _config(method='heun')
    with pytest.raises(KeyError):
        _config(kernel='fast')
    with pytest.raises(ValueError, match='precision must be one of'):
        _config(precision='fp16')


# a second value for every field of the record (with the carriers that keep an opt-in alive)
_CARRIED = dict(members=3, samples=2, precision='bf16')
_OTHER = dict(model=engine.model_struct(3, 128, 128, 2, 4, 17), batch=48, knots=9, n_steps=7, n_out=3, method='srk', kernel='mfma4',
              precision='fp32', exact_order=True, stream_all=True, two_tile=True, lean_general=True, sample_grad=True, bf16_grad=True,
              ensemble_grad=True, ensemble_samples=True, ensemble_nets=True, ensemble_nets_grad=True, samples=4, members=6, global_rows=96,
              dW=True, noise_table=True, row_out=True, seed_dev=True, training=True, kl_column=5)


def test_equal_configs_hash_equal_and_every_field_tells_configs_apart():
    base = _config(**_CARRIED)
    assert base == _config(**_CARRIED) and hash(base) == hash(_config(**_CARRIED))
    assert set(_OTHER) == set(engine.SolveConfig._fields)
    seen = {base}
    for name, value in _OTHER.items():
        other = _config(**dict(_CARRIED, **{name: value}))
        assert other != base and getattr(other, name) != getattr(base, name), name
        assert other == base.replace(**{name: value}), name
        seen.add(other)
    assert len(seen) == len(_OTHER) + 1


def test_the_switches_of_the_size_cache_are_in_the_identity_row_offset_and_seed_are_not():
    fields = engine.SolveConfig._fields
    for name in ('stream_all', 'two_tile', 'lean_general'):
        assert name in fields and _config(**{name: True}) != _config()
    assert 'row_offset' not in fields and 'seed' not in fields and 'seed_dev' in fields
    a, b = engine._describe(_config(), row_offset=0), engine._describe(_config(), row_offset=8)
    assert (a.row_offset, b.row_offset) == (0, 8)


def test_the_flag_table_covers_every_flag_of_the_binding():
    flags = {n: v for n, v in vars(_lib).items() if n.startswith('FLAG_')}
    owned_elsewhere = {'FLAG_REUSE_PREPARED', 'FLAG_BF16_OPERANDS', 'FLAG_BF16_GRAD'}      # SolveCall.launch; engine.precision_flags
    assert owned_elsewhere <= set(flags)
    table = dict(engine._FLAG_TABLE)
    assert len(table) == len(engine._FLAG_TABLE) and set(table) <= set(engine.SolveConfig._fields)
    assert sorted(table.values()) == sorted(v for n, v in flags.items() if n not in owned_elsewhere)
    for name, bit in engine._FLAG_TABLE:
        assert flags['FLAG_' + name.upper()] == bit
        assert _config(**dict(_CARRIED, **{name: True})).flags == _config(**_CARRIED).flags | bit
    assert _config(precision='bf16').flags == _lib.FLAG_BF16_OPERANDS
    assert _config(precision='bf16', bf16_grad=True).flags == _lib.FLAG_BF16_OPERANDS | _lib.FLAG_BF16_GRAD


def test_the_bool_checks_keep_their_messages():
    for check, name in ((engine.check_sample_grad, 'sample_grad'), (engine.check_bf16_grad, 'bf16_grad'),
                        (engine.check_ensemble_grad, 'ensemble_grad'), (engine.check_ensemble_samples, 'ensemble_samples'),
                        (engine.check_ensemble_nets, 'ensemble_nets'), (engine.check_ensemble_nets_grad, 'ensemble_nets_grad')):
        assert check(True) is True and check(False) is False
        with pytest.raises(ValueError, match=rf'^{name} must be a bool \(.*\), got 1$'):
            check(1)
