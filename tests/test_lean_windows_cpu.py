"""Where the instructions of the lean forward kernel's step loop sit (csrc/snsde_m4_kernel.h: LEAN_WIDE_READS, LEAN_GPART_MODE,
LEAN_CARRY_MODE): the K2 specialised instantiation cross-compiled for gfx950 and read with tools/asm_mix.py, in the
manner of tests/test_scalar_step_loop_cpu.py.  Two listings:
  * the product build: wide operand reads (one 64-lane ds_read_b128 per four k-blocks of the y / hidden / output layers), the
    diffusion term and the carried reads where the releases before it had them;
  * the `windows` development build (-DLEAN_GPART_MODE=1 -DLEAN_CARRY_MODE=1 -DLEAN_WIDE_READS=0): the diffusion term split over the
    operand-read windows behind barriers A and B, the next step's table row and [X | tau] operands read behind the output layer's
    operands.  Measured and not kept as the default (profiles/lean_windows_bench_ab.txt); the switches stay, as LEAN_PRIO_MODE does,
    and this file pins that they place the instructions where they say - hipcc moved the unpinned source once already.
The step loop of the commit before held 104 MFMAs, 4 barriers and 44 LDS instructions (profiles/lean_windows_timeline.txt).
Plus, without a compiler: every case of tests/lean_windows_cases.py plans the kernel it names."""
import importlib.util
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'stable-neural-sdes_amd', 'csrc')
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
needs_hipcc = pytest.mark.skipif(HIPCC is None, reason='hipcc not found')

_spec = importlib.util.spec_from_file_location('asm_mix', os.path.join(ROOT, 'tools', 'asm_mix.py'))
asm_mix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(asm_mix)

K2 = 'CfgSpecINS_4CfgLILi128ELi1ELi2ELi1ELi0ELi0ELi0EEELi0EE'
BUILDS = {'product': (), 'windows': ('-DLEAN_GPART_MODE=1', '-DLEAN_CARRY_MODE=1', '-DLEAN_WIDE_READS=0')}
PARENT = dict(mfma=104, barrier=4, ds=44)
WIDE_SAVES = 3 * (8 - 2)      # per step: three layers of KUH = 8 k-blocks, 8 reads by lanes 0-15 -> 2 reads by all lanes


@pytest.fixture(scope='module')
def loops(tmp_path_factory):
    out = tmp_path_factory.mktemp('lean_windows')

    def compile_one(name):
        dst = os.path.join(out, name + '.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-DSNSDE_DEV_SUBSET', *BUILDS[name], '--cuda-device-only', '-S',
               '-I', os.path.join(ROOT, 'include'), '-I', CSRC, os.path.join(CSRC, 'snsde_m4_h128.hip'), '-o', dst]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = open(dst).read().split('\n')
        fn = asm_mix.kernel_lines(lines, K2)
        return name, (lines, fn, asm_mix.step_loop(fn))

    with ThreadPoolExecutor(max_workers=len(BUILDS)) as ex:
        return dict(ex.map(compile_one, BUILDS))


def _ops(ins):
    return [x.split()[0] for x in ins]


@needs_hipcc
@pytest.mark.parametrize('build', list(BUILDS))
def test_the_step_loop_keeps_its_work_and_its_scalar_exit(loops, build):
    lines, fn, loop = loops[build]
    mix = asm_mix.mix(loop['lines'])
    assert mix['mfma'] == PARENT['mfma'] and mix['barrier'] == PARENT['barrier'], dict(mix)
    assert mix['ds'] == PARENT['ds'] - (WIDE_SAVES if build == 'product' else 0), dict(mix)
    assert asm_mix.left_on(fn, loop) == 'scalar', asm_mix.loop_exits(fn, loop)
    assert asm_mix.smem_after_first_barrier(loop) == []
    res = asm_mix.kernel_resources(lines, K2)
    assert res['scratch'] == 0 and res['vgprs'] <= 240, res


@needs_hipcc
def test_product_build_reads_each_layer_with_two_wide_reads(loops):
    _, _, loop = loops['product']
    top, after_a, after_b = asm_mix.operand_windows(loop)
    for w in (top, after_a, after_b):
        assert [x for x in _ops(w) if x.startswith('ds_read_b128')] == ['ds_read_b128'] * 2, w
        assert not any('exec' in x for x in w), w      # by all 64 lanes: no narrowed EXEC around them
    # every lane group's registers are broadcast: blgp 4 .. 7, a quarter of the layer MFMAs each (the [X | tau] block keeps blgp 4)
    mfma = [x for x in asm_mix.instructions(loop['lines']) if x.startswith('v_mfma')]
    per = {g: sum(f'blgp:{g}' in x for x in mfma) for g in (4, 5, 6, 7)}
    assert per == {4: 8 + 24, 5: 24, 6: 24, 7: 24}, per


@needs_hipcc
def test_windows_build_puts_valu_work_behind_both_hidden_and_output_reads(loops):
    _, _, loop = loops['windows']
    top, after_a, after_b = asm_mix.operand_windows(loop)
    # the agreed split of lean_tanh_rel<true>: the exponential behind barrier A, the reciprocal behind barrier B
    assert 'v_exp_f32_e32' in _ops(after_a) and 'v_rcp_f32_e32' not in _ops(after_a), after_a
    assert 'v_rcp_f32_e32' in _ops(after_b) and 'v_exp_f32_e32' not in _ops(after_b), after_b
    # the stash read and the noise-table load stay behind barrier A (two phases to land before the single vmcnt wait)
    assert 'global_load_dword' in _ops(after_a) and 'ds_read_b32' in _ops(after_a), after_a
    # the carried reads: 8 operand reads + table row (2) + [X | tau] (2) behind barrier B, the first wait leaves 10 in flight
    assert sum(x == 'ds_read_b128' for x in _ops(after_b)) == 12, after_b
    ins = asm_mix.instructions(loop['lines'])
    first_wait = next(x for x in ins[ins.index(after_b[-1]) + 1:] if x.startswith('s_waitcnt'))
    assert 'lgkmcnt(10)' in first_wait, first_wait


@needs_hipcc
def test_windows_build_leaves_no_read_between_the_y_store_and_the_closing_barrier(loops):
    _, _, loop = loops['windows']
    tail = asm_mix.closing_stretch(loop)
    assert not any(x.startswith('ds_read') for x in _ops(tail)), tail
    assert any(x.startswith('s_waitcnt') and 'lgkmcnt(0)' in x for x in tail), tail      # (covers what the last layer's waits left in flight)
    # and the product build still has them there, as the commit before
    assert sum(x == 'ds_read_b128' for x in _ops(asm_mix.closing_stretch(loops['product'][2]))) == 4


def test_every_case_plans_the_kernel_it_names():
    from stable_neural_sdes_amd import _lib, engine
    from tests import lean_windows_cases as W
    from tests.kernel_cases import descriptor
    for name, case in W.CASES.items():
        s = descriptor(case.launch)
        if case.kw.get('lean_general'):
            s.flags |= _lib.FLAG_LEAN_GENERAL
        assert engine.forward_kernel(s) == case.launch.fwd, (name, engine.forward_kernel(s, keys=True))
        if case.variant is not None:
            assert engine.lean_variant(s) == case.variant, (name, engine.lean_variant(s))
