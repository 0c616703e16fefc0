"""Wave-pair kernels (csrc/snsde_w4.hip) of two trees side by side: the resource figures of every instantiation and the disassembly of
the instantiations both trees have.  Input per tree: the assembly and the kernel-resource-usage remarks of one device-only compile,
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I csrc --offload-device-only -S -Rpass-analysis=kernel-resource-usage \
          csrc/snsde_w4.hip -o TREE.s 2> TREE.rem
    python tools/w4_ens_resources.py PARENT.s PARENT.rem THIS.s THIS.rem > profiles/ensemble_nets_grad_kernel_resources.txt
A kernel of this tree is matched to the parent's by its demangled name with a trailing `ENS = false` template argument dropped (the
adjoints gained that parameter: the mangled names of the one-model instantiations differ by it and by nothing else).  The
disassembly of a kernel is its lines between its label and the kernel descriptor behind its code, comments dropped and the function number of the local
labels (.LBB<n>_) removed.  An ENS instantiation is set beside the one-model instantiation of the same configuration (its sibling)."""
import re
import subprocess
import sys

FIG = ('VGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]')


def remarks(path):
    name, d = None, {}
    for line in open(path):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            d[name] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs|TotalSGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', line)
        if m and name:
            d[name][m.group(1)] = int(m.group(2))
    return d


def bodies(path, names):
    out, cur, want = {}, None, set(names)
    for line in open(path):
        if cur is None:
            m = re.match(r'(\S+):\s', line)
            if m and m.group(1) in want:
                cur, buf = m.group(1), []
            continue
        if line.startswith('\t.section') or line.startswith('.Lfunc_end'):      # (the kernel descriptor follows the code)
            out[cur], cur = buf, None
            continue
        line = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0].strip())
        if line:
            buf.append(line)
    return out


def demangle(names):
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    return {k: re.sub(r'snsde_w4::|^void ', '', re.sub(r'^void ', '', d)) for k, d in zip(names, dem)}


def key(dn):
    """(one-model name, ENS): the name with the ENS template argument removed"""
    m = re.match(r'(snsde_w4_(?:euler|srk)_kernel<CfgW<[^>]*>)(?:, (true|false))? ?>(.*)', dn)
    if m:
        return m.group(1) + ' >' + m.group(3), m.group(2) == 'true'
    m = re.match(r'(snsde_w4_euler_reverse_kernel<CfgW<[^>]*>, (?:true|false))(?:, (true|false))? ?>(.*)', dn)
    if m:
        return m.group(1) + '>' + m.group(3), m.group(2) == 'true'
    m = re.match(r'(snsde_w4_srk_reverse_kernel<CfgSR<[^>]*>)(?:, (true|false))? ?>(.*)', dn)
    if m:
        return m.group(1) + ' >' + m.group(3), m.group(2) == 'true'
    m = re.match(r'(snsde_w4_grad_reduce[12])_ens_kernel', dn)      # (W4GReduce, W4GStrides) beside the one-model (W4GReduce)
    if m:
        return m.group(1) + '_kernel(W4GReduce)', True
    return dn, False


def figures(v):
    return tuple(v.get(f, 0) for f in FIG) + (v.get('SGPRs Spill', 0), v.get('VGPRs Spill', 0))


def show(a, b):
    return ' | '.join(f'{x} -> {y}' for x, y in zip(a[:5], b[:5]))


if __name__ == '__main__':
    ps, pr, ns, nr = sys.argv[1:5]
    P, N = remarks(pr), remarks(nr)
    pd, nd = demangle(list(P)), demangle(list(N))
    pk = {key(pd[k]): k for k in P}
    pb, nb = bodies(ps, P), bodies(ns, N)
    same_fig = same_asm = 0
    rows, ens_rows, diff = [], [], []
    for k in N:
        name, ens = key(nd[k])
        if not ens:
            par = pk.get((name, False))
            if par is None:
                rows.append(f'? {nd[k]}: no such kernel in the parent')
                continue
            fa, fb = figures(P[par]), figures(N[k])
            asm = pb[par] == nb[k]
            same_fig += fa == fb
            same_asm += asm
            if fa != fb or not asm:
                diff.append(nd[k])
            rows.append(f"{'  ' if fa == fb and asm else '* '}{nd[k][:100]:100s} {show(fa, fb)} | asm {'identical' if asm else 'DIFFERS'} ({len(nb[k])} lines)")
    new_ens = parent_ens = 0
    for k in N:
        name, ens = key(nd[k])
        if ens:
            sib = next(q for q in N if key(nd[q]) == (name, False))
            fa, fb = figures(N[sib]), figures(N[k])
            known = (name, True) in pk
            parent_ens += known
            new_ens += not known
            par = fa[0] == fb[0] and fa[2] == fb[2] and fa[4] == fb[4]
            extra = ''
            if known:
                same = figures(P[pk[(name, True)]]) == fb and pb[pk[(name, True)]] == nb[k]
                extra = ' | the parent has it: ' + ('figures and asm identical' if same else 'DIFFERS from the parent')
                if not same:
                    diff.append(nd[k])
            ens_rows.append(f"{'+ ' if par else '! '}{nd[k][:100]:100s} {show(fa, fb)}{extra}")
            if not par:
                diff.append(nd[k] + ' (sibling parity)')
    n_one = sum(1 for k in N if not key(nd[k])[1])
    print('# csrc/snsde_w4.hip, parent commit against this tree (tools/w4_ens_resources.py; hipcc --offload-arch=gfx950 -O3 -std=c++17')
    print('# --offload-device-only -S -Rpass-analysis=kernel-resource-usage; cross-compiled, no GPU).  Per kernel instantiation:')
    print('# VGPRs | TotalSGPRs | scratch bytes/lane | static LDS bytes/block | occupancy waves/SIMD, parent -> this tree; spilled SGPRs / VGPRs')
    print('# are compared as well.  asm: the instructions between the kernel\'s label and the kernel descriptor behind them, comments dropped and the function')
    print('# number of local labels (.LBB<n>_) removed, compared line by line.  A kernel of this tree is matched to the parent\'s by its')
    print('# demangled name with the trailing ENS = false template argument dropped (the adjoints gained that parameter).')
    print('#')
    print(f'# one-model kernels (every kernel of the parent that is not an ENS instantiation): {n_one}; all figures equal: {same_fig}; '
          f'disassembly identical: {same_asm}')
    print(f'# ENS instantiations: {parent_ens} of the parent (inference forward), {new_ens} new (training forward, adjoints, reductions)')
    print(f'# kernels that differ from the parent or from their sibling in VGPRs / scratch / occupancy: {len(diff)}' + (': ' + '; '.join(diff) if diff else ''))
    print('## one-model kernels, parent -> this tree')
    print('\n'.join(rows))
    print('## ENS instantiations: the one-model sibling of THIS tree -> the ENS instantiation (+: same VGPRs, scratch and occupancy; !: not)')
    print('\n'.join(ens_rows))
