#!/usr/bin/env python3
"""(CPU) Static instruction census of fit_lm_knot_kernel<false, true> -- the headline's instantiation -- as hipcc compiles
csrc/fit_knot.hip for gfx950 with the Makefile's flags: the whole kernel and the straight-line block that is one factorisation of
damped_solve (the basic block that holds its 16 MFMAs and its reciprocal roots), by class; registers / scratch / occupancy of all four
instantiations.  The per-item table of DESIGN 5.3c (round 7) is this tool's output, commit by commit.

    python tools/knot_count.py [file.s]        (an assembly file already made with --cuda-device-only -S is read instead of compiling)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-Wall', '-Wno-unused-result', '-Wno-unused-value', '-mllvm', '-disable-machine-licm']


def klass(op):
    for prefix, name in (('s_nop', 's_nop'), ('v_mfma', 'mfma'), ('ds_', 'lds'), ('v_', 'valu'), ('s_', 'salu')):
        if op.startswith(prefix):
            return name
    return 'other'


def census(lines):
    c = {'all': 0, 'valu': 0, 'packed': 0, 'lds': 0, 'salu': 0, 's_nop': 0, 'mfma': 0, 'other': 0}
    for ln in lines:
        t = ln.strip()
        if not t or t[0] in ';./' or t.endswith(':'):
            continue
        op = t.split()[0]
        c['all'] += 1
        c[klass(op)] += 1
        c['packed'] += op.startswith('v_pk_')
    return c


def main():
    if len(sys.argv) > 1:
        asm = open(sys.argv[1]).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, 'fit_knot.s')
            subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + ['--cuda-device-only', '-S', 'fit_knot.hip', '-o', out],
                                  cwd=os.path.join(ROOT, 'drone-sim-python_amd', 'csrc'))
            asm = open(out).read()
    body, on = [], False
    for ln in asm.splitlines():
        if re.match(r'^_Z\w*fit_lm_knot_kernelILb0ELb1E\w*:', ln):
            on = True
            continue
        if on and ln.startswith('.Lfunc_end'):
            break
        if on:
            body.append(ln)
    blocks = [[]]
    for ln in body:
        if re.match(r'^\.LBB\d+_\d+:', ln):
            blocks.append([])
        blocks[-1].append(ln)
    fact = max((b for b in blocks if any('v_mfma_f32_16x16x4' in x for x in b) and any('v_rsq_f32' in x for x in b)), key=len)
    print('fit_lm_knot_kernel<false, true>')
    print('  whole kernel  ', census(body))
    print('  factorisation ', census(fact))
    res = re.findall(r'^; (NumVgprs|ScratchSize|Occupancy): (\d+)', asm, re.M)
    names = re.findall(r'^\s+\.name:\s+\S*fit_lm_knot_kernelILb(\d)ELb(\d)E', asm, re.M)
    for i, (st, s9) in enumerate(names):
        r = dict(res[3 * i:3 * i + 3])
        print(f'  <STAMPS={st}, SEG9={s9}>: {r.get("NumVgprs")} VGPRs, scratch {r.get("ScratchSize")}, occupancy {r.get("Occupancy")}')


if __name__ == '__main__':
    main()
