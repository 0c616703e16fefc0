"""The save format's public answers: snsde_act_slots and snsde_save_layout answer as recorded in tests/golden/save_layout.npz
(tests/golden/make_save_layout_golden.py, taken before the slot layout moved into csrc/snsde_save_layout.h) over the whole domain
of hidden layers, noise options, methods, activations, H and the two batch sizes that straddle the wave-pair adjoint.  No GPU."""
import numpy as np

from tests.golden.make_save_layout_golden import ACTIVATIONS, ANSWERS, FIELDS, NOISE, answers, descriptors
from tests.helpers import load


def test_save_layout_answers_are_unchanged():
    g = load('save_layout.npz')
    assert tuple(g['fields']) == FIELDS and tuple(g['answer_names']) == ANSWERS
    desc, want = g['desc'], g['answers']
    assert np.array_equal(desc, descriptors()) and len(desc) == 4 * len(NOISE) * 3 * len(ACTIVATIONS) * 2 * 2
    # both answers of the wave-pair adjoint are in the table: no delta planes at the small batch, some at the large one
    col = {f: desc[:, i] for i, f in enumerate(FIELDS)}
    w4 = (col['H'] == 64) & (col['no'] == 18) & (col['method'] == 0) & (col['act'] == 0) & (col['NL'] == 2)
    dslots = want[:, ANSWERS.index('delta_slots')]
    assert set(dslots[w4 & (col['batch'] == 8)]) == {0} and (dslots[w4 & (col['batch'] == 8192)] > 0).all()
    moved = [(dict(zip(FIELDS, map(int, row))), dict(zip(ANSWERS, map(int, exp))), got)
             for row, exp in zip(desc, want) for got in [[int(v) for v in answers(row)]] if got != [int(v) for v in exp]]
    assert not moved, f'{len(moved)} rows moved, e.g. {moved[:3]}'
