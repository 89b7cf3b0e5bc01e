#!/usr/bin/env python3
"""(CPU) Static instruction census of the headline's instantiation of fit_lm_knot_kernel -- <false, true, 8> (no stamps, SEG9, the
floor of eight samples a segment; <false, true> before round 8) -- as hipcc compiles
csrc/fit_knot.hip for gfx950 with the Makefile's flags: the whole kernel and the straight-line block that is one factorisation of
damped_solve (the basic block that holds its 16 MFMAs and its reciprocal roots), by class; registers / scratch / occupancy of all four
instantiations; and (round 8) the evaluation's k-steps: every cluster of twenty or more accumulating MFMAs outside the factorisation,
with the instructions between its first and last v_mfma and the branches among them; and (round 9) the block of the isq forward
substitution, the one with the most v_readlane outside the factorisation's; and (round 10) the second-order evaluation's k-steps on a
line of their own, told from the first-order cluster by their A and B operand registers differing, beside the figure of the rolled
pass they replace.  The per-item tables of DESIGN 5.3c (rounds 7 to 10) are this tool's output, commit by commit.

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
    head = r'^_Z\w*fit_lm_knot_kernelILb0ELb1ELi8E\w*:' if 'fit_lm_knot_kernelILb0ELb1ELi8E' in asm else r'^_Z\w*fit_lm_knot_kernelILb0ELb1E\w*:'
    for ln in asm.splitlines():
        if re.match(head, ln):
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
    print('fit_lm_knot_kernel<false, true, 8>' if 'Li8E' in head else 'fit_lm_knot_kernel<false, true>')
    print('  whole kernel  ', census(body))
    print('  factorisation ', census(fact))
    # (round 9) the forward substitution of isq -- lmpar's || L^-1 (M delta / dxnorm) ||^2: the block with the most v_readlane outside
    # the factorisation's
    isq = max((b for b in blocks if b is not fact), key=lambda b: sum('v_readlane' in x for x in b))
    print('  isq           ', census(isq))
    # the evaluation's k-steps: accumulating MFMAs (a register block as C) outside the factorisation blocks, clustered by position.
    # A first-order k-step multiplies the rows by themselves (A and B are one register); a second-order k-step (round 10) has a
    # plain A operand and a weighted B operand: the two kinds are clustered apart and printed on lines of their own
    infact = {id(b) for b in blocks if any('v_rsq_f32' in x for x in b)}
    pos, n = {'evaluation': [], 'second-order': []}, 0
    for b in blocks:
        for ln in b:
            if 'v_mfma_f32_16x16x4' in ln and id(b) not in infact and not ln.rstrip().endswith(', 0'):
                ops = [o.strip() for o in ln.split(None, 1)[1].split(',')]
                pos['evaluation' if ops[1] == ops[2] else 'second-order'].append(n)
            n += 1
    flat = [ln for b in blocks for ln in b]
    for kind, pp in pos.items():
        clusters = [[]]
        for q in pp:
            if clusters[-1] and q - clusters[-1][-1] > 150:
                clusters.append([])
            clusters[-1].append(q)
        big = [cl for cl in clusters if len(cl) >= 20]
        for cl in big:
            span = flat[cl[0]:cl[-1] + 1]
            c = census(span)
            br = sum(1 for x in span if x.strip().startswith(('s_cbranch', 's_branch')))
            print(f'  {kind:<14} {len(cl)} v_mfma: {c["all"]} instructions from the first to the last, {br} branches, '
                  f'{sum(1 for x in span if x.startswith(".LBB"))} labels; valu {c["valu"]} lds {c["lds"]} salu {c["salu"]} s_nop {c["s_nop"]}')
        if kind == 'second-order':
            print('  second-order   ' + ('(' if big else 'no straight-line pass; ') + 'before round 10: one rolled loop a segment, 24 instructions a sample -- 2 v_mfma, '
                  '11 valu, 3 lds, 8 salu and s_nop -- so 1200 at K = 50' + (')' if big else ''))
    res = re.findall(r'^; (NumVgprs|ScratchSize|Occupancy): (\d+)', asm, re.M)
    names = re.findall(r'^\s+\.name:\s+\S*fit_lm_knot_kernelILb(\d)ELb(\d)E(?:Li(\d+)E)?', asm, re.M)
    sizes = re.findall(r'^; codeLenInByte = (\d+)', asm, re.M)
    for i, (st, s9, sm) in enumerate(names):
        r = dict(res[3 * i:3 * i + 3])
        print(f'  <STAMPS={st}, SEG9={s9}' + (f', SEGMIN={sm}' if sm else '') + f'>: {r.get("NumVgprs")} VGPRs, scratch {r.get("ScratchSize")}, '
              f'occupancy {r.get("Occupancy")}' + (f', {sizes[i]} bytes' if len(sizes) == len(names) else ''))


if __name__ == '__main__':
    main()
