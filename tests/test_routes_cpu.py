"""The routing table: every host-only query of the library (snsde_forward_path, snsde_backward_supported, the three workspace
sizes, snsde_save_layout) answers as recorded in tests/golden/routes.npz (tests/golden/make_route_golden.py) for a few thousand
descriptors.  A change of which kernel a descriptor routes to shows up here as the rows it moved.  No GPU compute."""
import collections

import numpy as np

from tests.golden.make_route_golden import ANSWERS, FIELDS, PTRS, answers
from tests.helpers import load

KERNEL_NAMES = {3: 'mfma16', 4: 'mfma4', 5: 'w4'}
# Rows whose recorded answers disagreed with the launch of the same descriptor when the table was taken, and how many of them
# there are.  Under an explicit kernel = mfma16 / mfma4 / w4, snsde_backward_supported planned the forward with the batch-chosen
# tile flavour and answered 1 (MFMA adjoint), while snsde_solve_backward planned it with the requested flavour, found no adjoint
# plan and returned SNSDE_ERR_UNSUPPORTED.  Both now plan with the requested flavour: the answer is the generic adjoint (2) or
# none (0), and snsde_param_gradients_workspace_bytes (mode 1 only) follows with 0.
KNOWN_CHANGES = {'mfma16': 51, 'mfma4': 2, 'w4': 179}


def _known_change(d, exp, got):
    e, g = dict(zip(ANSWERS, exp)), dict(zip(ANSWERS, got))
    moved = {a for a in ANSWERS if e[a] != g[a]}
    return (d['kernel'] in KERNEL_NAMES and e['backward_supported'] == 1 and g['backward_supported'] in (0, 2) and
            g['param_gradients_workspace_bytes'] == 0 and moved <= {'backward_supported', 'param_gradients_workspace_bytes'})


def test_routing_table_is_unchanged():
    g = load('routes.npz')
    assert tuple(g['fields']) == FIELDS and tuple(g['ptrs']) == PTRS and tuple(g['answer_names']) == ANSWERS
    desc, want = g['desc'], g['answers']
    assert len(desc) > 4000
    moved, known = [], collections.Counter()
    for row, exp in zip(desc, want):
        got = [int(v) for v in answers(row)]
        exp = [int(v) for v in exp]
        if got == exp:
            continue
        d = dict(zip(FIELDS, (int(v) for v in row)))
        if _known_change(d, exp, got):
            known[KERNEL_NAMES[d['kernel']]] += 1
        else:
            moved.append((d, {a: (e, o) for a, e, o in zip(ANSWERS, exp, got) if e != o}))
    assert not moved, f'{len(moved)} rows moved, e.g. {moved[:3]}'
    assert dict(known) == KNOWN_CHANGES
