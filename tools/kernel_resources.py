"""Summarise hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of a compile) per kernel instantiation:
    hipcc ... -Rpass-analysis=kernel-resource-usage -c x.hip -o x.o 2> x.rem;  python tools/kernel_resources.py x.rem
With the listing of the same compile (hipcc ... --offload-device-only -S -o x.s) as a second argument, every line also carries the
kernel's instruction count, a digest of its instruction stream (directives, comments and labels dropped) and, with --mix, the
count of every mnemonic: two trees compile a kernel to the same code where the digests agree.
    python tools/kernel_resources.py x.rem x.s [--mix]"""
import hashlib
import re
import subprocess
import sys
from collections import Counter


def parse(path):
    name, d = None, {}
    for line in open(path):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            d[name] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', line)
        if m and name:
            d[name][m.group(1)] = int(m.group(2))
    return d


def streams(path):
    """{mangled kernel name: its instructions} of a hipcc -S listing, label line to s_endpgm; branch targets lose the function's
    index (.LBB7_3 -> .LBB_3), which depends on what else the file holds."""
    out, name = {}, None
    for line in open(path):
        m = re.match(r'(_Z\w+):', line)
        if m and name is None:
            name = m.group(1)
            out[name] = []
            continue
        x = line.strip()
        if name is None or not x or x.startswith((';', '.')):
            continue
        out[name].append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s*;.*$', '', x)))
        if x.startswith('s_endpgm'):
            name = None
    return out


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    d = parse(args[0])
    code = streams(args[1]) if len(args) > 1 else {}
    names = list(d)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    for k, dn in zip(names, dem):
        v = d[k]
        dn = re.sub(r'^void ', '', dn)
        dn = re.sub(r'snsde_mfma::', '', dn)
        dn = re.sub(r'\(anonymous namespace\)::', '', dn)
        line = (f"{dn[:110]:110s} vgpr {v.get('VGPRs')} agpr {v.get('AGPRs')} scratch {v.get('ScratchSize [bytes/lane]')} "
                f"lds {v.get('LDS Size [bytes/block]')} occ {v.get('Occupancy [waves/SIMD]')}")
        if k in code:
            line += f" instrs {len(code[k])} stream {hashlib.sha1(chr(10).join(code[k]).encode()).hexdigest()[:12]}"
            if '--mix' in sys.argv:
                line += ' mix ' + ' '.join(f'{op}:{n}' for op, n in sorted(Counter(x.split()[0] for x in code[k]).items()))
        print(line)
