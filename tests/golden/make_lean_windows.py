#!/usr/bin/env python3
"""Records tests/golden/lean_windows.npz: the outputs of every case of tests/lean_windows_cases.py on the GPU, from the library
named by SNSDE_LIB.  The committed fixture was recorded on an MI355X from the library of the commit before the lean forward kernel's
filler work was spread over its operand-read windows (csrc/snsde_m4_kernel.h: LEAN_GPART_MODE, LEAN_CARRY_MODE):
    SNSDE_LIB=<that commit's libsnsde.so> python tests/golden/make_lean_windows.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import lean_windows_cases as W      # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'lean_windows.npz')
arrays = {}
for name in W.CASES:
    for key, val in W.run(name).items():
        assert np.isfinite(val).all() if val.dtype.kind == 'f' else True, (name, key)
        arrays[f'{name}/{key}'] = val
np.savez_compressed(out, **arrays)
print(f'{out}: {len(arrays)} arrays of {len(W.CASES)} cases, {os.path.getsize(out)} bytes, library {os.environ.get("SNSDE_LIB", "libsnsde.so")}')
