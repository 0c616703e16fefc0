"""Runner of tools/ubench_mfma_bf16.hip: builds it (hipcc --offload-arch=gfx950) where the binary is missing or older than the
source, runs it on the current GPU and writes the table to profiles/ubench_mfma_bf16.txt (or the path given as argument).

    python tools/ubench_mfma_bf16.py [out.txt]
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'ubench_mfma_bf16.hip')
BIN = os.path.join(HERE, 'ubench_mfma_bf16')


def build():
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= os.path.getmtime(SRC):
        return BIN
    cc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    subprocess.run([cc, '--offload-arch=gfx950', '-O3', '-o', BIN, SRC], check=True)
    return BIN


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(HERE), 'profiles', 'ubench_mfma_bf16.txt')
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    text = r.stdout + r.stderr
    print(text, end='')
    if r.returncode != 0:
        raise SystemExit(f'ubench_mfma_bf16 exited with {r.returncode}')
    with open(out, 'w') as f:
        f.write('# tools/ubench_mfma_bf16.hip: cycles (s_memtime, shader clock) per group = one MFMA + k v_fma_f32, mean over the\n'
                '# waves of 256 workgroups; cycles/k-slot = cycles/group / k-slots per MFMA (bf16 4x4x4: 4, f32 4x4x1: 1)\n')
        f.write(text)


if __name__ == '__main__':
    main()
