#!/usr/bin/env python3
"""Instruction mix of the main (MFMA-bearing) loop of a kernel in a hipcc -S / -save-temps .s file, and how that loop is left.
usage: asm_mix.py file.s <kernel-name-substring> [--dump out.s]

Two views of the same kernel:
  * the REGION: the largest backward-branching stretch of the listing with > 20 MFMAs (a conditional branch or an unconditional
    s_branch back to an earlier label).  For the lean forward kernels that is the loop over the outputs with the step loop, its
    refill loop and every cold block inside; the mix line printed first counts it (the numbers of profiles/*_asm_mix.txt).
  * the STEP LOOP: the deepest loop of hipcc's own loop annotations ("Loop Header: Depth=", "in Loop: Header=") that holds
    > 20 MFMAs, with the blocks the compiler laid out behind its back edge.  step_loop() / loop_exits() / left_on() /
    smem_after_first_barrier() work on it: a loop left through s_cbranch_scc* has its counter and bound on the scalar unit, one
    left through s_cbranch_exec* / vcc* is an exec-masked (divergent-form) loop around the layer MFMAs.
The functions are imported by tests/test_scalar_step_loop_cpu.py and tests/test_lean_windows_cpu.py."""
import re
import sys
from collections import Counter

LABEL = re.compile(r'^\.L(BB\d+_\d+):')
FALLTHROUGH = re.compile(r'^; %bb\.(\d+):')
BRANCH = re.compile(r'^\s*(s_cbranch_\w+|s_branch)\s+\.L(BB\d+_\d+)')


def kernel_lines(lines, key):
    """The listing of the first kernel whose mangled name contains `key`, label line to s_endpgm."""
    start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and key in l and l.rstrip().split(':')[0].endswith('E'))
    end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
    return lines[start:end + 1]


def kernel_resources(lines, key):
    """{'vgprs', 'sgprs', 'scratch'} of that kernel from the comment block hipcc writes behind it."""
    start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and key in l and l.rstrip().split(':')[0].endswith('E'))
    out = {}
    for l in lines[start:]:
        for name, pat in (('sgprs', r'^; TotalNumSgprs: (\d+)'), ('vgprs', r'^; NumVgprs: (\d+)'), ('scratch', r'^; ScratchSize: (\d+)')):
            m = re.match(pat, l)
            if m and name not in out:
                out[name] = int(m.group(1))
        if len(out) == 3:
            return out
    raise ValueError('no resource comments behind ' + key)


def instructions(fn_lines):
    return [x.strip() for x in fn_lines if x.strip() and not x.strip().startswith((';', '.'))]


def mix(fn_lines):
    c = Counter()
    for x in instructions(fn_lines):
        op = x.split()[0]
        if op.startswith('v_mfma'): c['mfma'] += 1
        elif op.startswith('v_accvgpr'): c['accvgpr'] += 1
        elif op.startswith('ds_'): c['ds'] += 1
        elif op.startswith(('global_', 'buffer_', 'scratch_')): c['vmem'] += 1
        elif op.startswith('s_waitcnt'): c['waitcnt'] += 1
        elif op.startswith('s_barrier'): c['barrier'] += 1
        elif op.startswith('s_nop'): c['s_nop'] += 1
        elif op.startswith('s_cbranch'): c['branch'] += 1      # (s_branch counts as salu, as in the earlier profiles/*_asm_mix.txt)
        elif op.startswith(('s_load', 's_buffer_load')): c['smem'] += 1
        elif op.startswith('s_'): c['salu'] += 1
        elif op.startswith('v_'): c['valu'] += 1
        else: c['other'] += 1
    return c


def region(fn, min_mfma=20):
    """(first, last) line of the largest backward-branching stretch with more than min_mfma MFMAs."""
    labels = {}
    for i, l in enumerate(fn):
        m = LABEL.match(l)
        if m:
            labels[m.group(1)] = i
    best = None
    for i, l in enumerate(fn):
        m = BRANCH.match(l)
        if m and m.group(2) in labels and labels[m.group(2)] < i:
            a, b = labels[m.group(2)], i
            n = sum('v_mfma' in x for x in fn[a:b])
            if n > min_mfma and (best is None or b - a > best[1] - best[0]):
                best = (a, b)
    if best is None:
        raise ValueError(f'no backward-branching region with > {min_mfma} MFMAs')
    return best


def blocks(fn):
    """Basic blocks in layout order: dicts with name (BBf_n), first / last line, own loop header, and for a loop header its depth and
    parent loops.  Blocks start at a .LBB label or at a '; %bb.N:' fall-through comment."""
    fnum = next((LABEL.match(l).group(1).split('_')[0] for l in fn if LABEL.match(l)), 'BB0')
    out = []
    for i, l in enumerate(fn):
        m, f = LABEL.match(l), FALLTHROUGH.match(l)
        if not (m or f):
            continue
        name = m.group(1) if m else f'{fnum}_{f.group(1)}'
        note = [l]
        j = i + 1
        while j < len(fn) and fn[j].strip().startswith(';') and not FALLTHROUGH.match(fn[j]) and '#ASM' not in fn[j]:
            note.append(fn[j])
            j += 1
        note = ' '.join(note)
        b = {'name': name, 'first': i, 'loop': None, 'depth': 0, 'parents': []}
        h = re.search(r'This (?:Inner )?Loop Header: Depth=(\d+)', note)
        if h:
            b['loop'], b['depth'] = name, int(h.group(1))
            b['parents'] = re.findall(r'Parent Loop (BB\d+_\d+)', note)
        else:
            g = re.search(r'in Loop: Header=(BB\d+_\d+)', note)
            if g:
                b['loop'] = g.group(1)
        if out:
            out[-1]['last'] = i - 1
        out.append(b)
    if out:
        out[-1]['last'] = len(fn) - 1
    return out


def step_loop(fn, min_mfma=20):
    """The deepest annotated loop with more than min_mfma MFMAs (the small-H kernels have fewer than 20 per step): {'header', 'depth', 'blocks': member blocks in layout order, 'lines': their text}."""
    bl = blocks(fn)
    headers = {b['name']: b for b in bl if b['loop'] == b['name']}

    def inside(b, h):
        return b['loop'] is not None and (b['loop'] == h or h in headers.get(b['loop'], {'parents': []})['parents'])

    best = None
    for h, hb in headers.items():
        members = [b for b in bl if inside(b, h)]
        lines = [x for b in members for x in fn[b['first']:b['last'] + 1]]
        if sum('v_mfma' in x for x in lines) > min_mfma and (best is None or hb['depth'] > best['depth']):
            best = {'header': h, 'depth': hb['depth'], 'blocks': members, 'lines': lines}
    if best is None:
        raise ValueError(f'no annotated loop with > {min_mfma} MFMAs')
    return best


def loop_exits(fn, loop):
    """The conditional branches that decide whether the loop is left: [(opcode, target)] of every s_cbranch in a member block whose
    target or whose fall-through (the next block, or the s_branch right behind it) is outside the loop."""
    members = {b['name'] for b in loop['blocks']}
    bl = blocks(fn)
    at = {}
    for b in bl:
        for i in range(b['first'], b['last'] + 1):
            at[i] = b['name']
    out = []
    for b in loop['blocks']:
        for i in range(b['first'], b['last'] + 1):
            m = BRANCH.match(fn[i])
            if not m or m.group(1) == 's_branch':
                continue
            j = i + 1
            while j < len(fn) and (not fn[j].strip() or (fn[j].strip().startswith(';') and not FALLTHROUGH.match(fn[j]))):
                j += 1
            nxt = BRANCH.match(fn[j]) if j < len(fn) else None
            through = nxt.group(2) if nxt and nxt.group(1) == 's_branch' else at.get(j)
            if m.group(2) not in members or through not in members:
                out.append((m.group(1), m.group(2)))
    return out


def left_on(fn, loop=None):
    """'scalar' when every exit of the step loop is an s_cbranch_scc*, else 'exec-masked' (an exec or vcc condition among them)."""
    ex = loop_exits(fn, loop or step_loop(fn))
    if not ex:
        raise ValueError('step loop without an exit branch')
    return 'scalar' if all(op.startswith('s_cbranch_scc') for op, _ in ex) else 'exec-masked'


def smem_after_first_barrier(loop):
    """Scalar memory loads of the step loop from its first s_barrier on, in layout order (the blocks behind the back edge are cold
    paths entered from between the barriers, so they count).  The counted lgkmcnt waits of the layer GEMMs allow none."""
    ins = instructions(loop['lines'])
    first = next((i for i, x in enumerate(ins) if x.startswith('s_barrier')), len(ins))
    return [x for x in ins[first:] if x.startswith(('s_load', 's_buffer_load'))]


def operand_windows(loop):
    """The operand-read windows of the step loop in layout order: behind every s_barrier but the last (the closing barrier, followed by
    the back edge), the instructions from the first ds_read_b128 / ds_read_b64 (a layer's B operands) up to, not including, the first
    s_waitcnt lgkmcnt behind it.  What sits there issues while the operands are in flight.  For the lean forward kernel: the window at
    the top of the step (laid out behind the refill block's barrier), behind barrier A, behind barrier B."""
    ins = instructions(loop['lines'])
    bars = [i for i, x in enumerate(ins) if x.startswith('s_barrier')]
    out = []
    for b in bars[:-1]:
        i = next(k for k in range(b, len(ins)) if ins[k].startswith(('ds_read_b128', 'ds_read_b64')))
        k = next(k for k in range(i, len(ins)) if ins[k].startswith('s_waitcnt') and 'lgkmcnt' in ins[k])
        out.append(ins[i:k])
    return out


def closing_stretch(loop):
    """The instructions between the last LDS store in front of the step loop's last s_barrier in layout order (the lean forward kernel's
    y store and closing barrier; the cold blocks behind the back edge hold no barrier) and that barrier."""
    ins = instructions(loop['lines'])
    last = max(i for i, x in enumerate(ins) if x.startswith('s_barrier'))
    store = max(i for i in range(last) if ins[i].startswith('ds_write'))
    return ins[store + 1:last]


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split('\n')
    fn = kernel_lines(lines, key)
    if '--dump' in sys.argv:
        open(sys.argv[sys.argv.index('--dump') + 1], 'w').write('\n'.join(fn))
    a, b = region(fn)
    c = mix(fn[a:b])
    print(key, 'loop instrs', sum(c.values()), dict(c))
    try:
        lp = step_loop(fn)
    except ValueError as e:
        print('  step loop:', e)
        return
    sc = mix(lp['lines'])
    ex = loop_exits(fn, lp)
    print(f"  step loop {lp['header']} depth {lp['depth']}: instrs {sum(sc.values())} {dict(sc)}")
    print(f"  left on: {left_on(fn, lp)} ({', '.join(op + ' .L' + t for op, t in ex)}); scalar loads from the first barrier on: "
          f"{len(smem_after_first_barrier(lp))}; {kernel_resources(lines, key)}")
    for name, w in zip(('top', 'after A', 'after B'), operand_windows(lp)):
        c = mix(w)
        trans = [x.split()[0] for x in w if x.startswith(('v_exp_f32', 'v_rcp_f32'))]
        print(f"  window {name}: {c['ds']} LDS reads, {c['valu']} VALU ({', '.join(trans) or 'no transcendental'}), {c['vmem']} VMEM, {c['mfma']} MFMA")
    print(f"  y store -> closing barrier: {', '.join(x.split()[0] for x in closing_stretch(lp))}")


if __name__ == '__main__':
    main()
