"""The step loops of the lean forward kernels stay on the scalar unit (csrc/snsde_m4_kernel.h and its m4s / m4s2 / m4t siblings:
n_end = readfirstlane(out_step[ko])): cross-compiled for gfx950 and read with tools/asm_mix.py.  For the K2 specialised
instantiation (inference and training mode), the general one and the first instantiation of each of the other three kernels: the
loop is left on a scalar condition, no scalar memory load sits between its barriers (the hand-counted lgkmcnt waits of the layer
GEMMs rely on LDS returning in order; a scalar load shares the counter and may not), the layer MFMAs are all there, no scratch.
Instruction counts of the VALU / SALU mix are in profiles/scalar_loop_asm_mix.txt, not here."""
import importlib.util
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'stable-neural-sdes_amd', 'csrc')
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason='hipcc not found')

_spec = importlib.util.spec_from_file_location('asm_mix', os.path.join(ROOT, 'tools', 'asm_mix.py'))
asm_mix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(asm_mix)

# case -> source file, substring of the mangled kernel name (the first match in the listing), layer MFMAs of one step
K2 = 'CfgLILi128ELi1ELi2ELi1ELi%dELi0ELi0EE'
CASES = {
    'K2 specialised': ('snsde_m4_h128', 'CfgSpecINS_4' + K2 % 0 + 'ELi0EE', 104),
    'K2 specialised, training mode': ('snsde_m4_h128', 'CfgSpecINS_4' + K2 % 1 + 'ELi0EE', 104),
    'K2 general': ('snsde_m4_h128', 'snsde_m4_kernelINS_4' + K2 % 0 + 'EEEv', 104),
    'm4s': ('snsde_m4s_h256', 'snsde_m4s_kernel', 196),
    'm4s2': ('snsde_m4s2_h256', 'snsde_m4s2_kernel', 392),
    'm4t': ('snsde_m4t_h128', 'snsde_m4t_kernel', 208),
}


@pytest.fixture(scope='module')
def listings(tmp_path_factory):
    out = tmp_path_factory.mktemp('scalar_step_loop')
    files = sorted({c[0] for c in CASES.values()})

    def compile_one(name):
        dst = os.path.join(out, name + '.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-DSNSDE_DEV_SUBSET', '--cuda-device-only', '-S',
               '-I', os.path.join(ROOT, 'include'), '-I', CSRC, os.path.join(CSRC, name + '.hip'), '-o', dst]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return name, open(dst).read().split('\n')

    with ThreadPoolExecutor(max_workers=len(files)) as ex:
        return dict(ex.map(compile_one, files))


@pytest.mark.parametrize('case', list(CASES))
def test_step_loop_is_scalar(listings, case):
    src, key, mfmas = CASES[case]
    lines = listings[src]
    fn = asm_mix.kernel_lines(lines, key)
    loop = asm_mix.step_loop(fn)
    exits = asm_mix.loop_exits(fn, loop)
    assert asm_mix.left_on(fn, loop) == 'scalar', exits
    assert asm_mix.smem_after_first_barrier(loop) == []
    mix = asm_mix.mix(loop['lines'])
    assert mix['mfma'] == mfmas and mix['barrier'] == 4, dict(mix)
    assert asm_mix.kernel_resources(lines, key)['scratch'] == 0
