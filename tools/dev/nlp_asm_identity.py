"""(CPU) The identity check of DESIGN.md 5.28 item 9 on two device assemblies of csrc/nlp_kernels.hip, function by function:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -mllvm -disable-machine-licm --cuda-device-only -S nlp_kernels.hip -o after.s
    (the same on the parent's file -> before.s)        python tools/dev/nlp_asm_identity.py before.s after.s

A function runs from its label to its .Lfunc_end.  The `__hip_cuid_` lines (a hash of the source text) are left out, and the function's own
index is taken out of its local labels and of the `; in Loop: Header=BB<n>_..` comments: a kernel added in the middle of the file renumbers
every function behind it.  Per function of the first file: `same`, or `DIFF` with the number of places that differ (comments out); `NEW`
for what only the second file has."""
import re, sys, subprocess, difflib
def funcs(path):
    out = {}; name = None; buf = None
    for line in open(path):
        if '__hip_cuid_' in line: continue
        m = re.match(r'^(_Z\w+|nlp_\w+):', line)
        if m and name is None:
            name = m.group(1); buf = out.setdefault(name, [])
        if name:
            buf.append(re.sub(r'\s+;', ' ;', re.sub(r'BB\d+_', 'BBn_', re.sub(r'(\.L[A-Za-z_]*?)\d+(_|:|\b)', r'\1n\2', line))))     # (the comment column of a label line moves with the label's width)
            if line.startswith('.Lfunc_end'):
                name = None
    return out
a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
def dem(n):
    return subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()[:70]
for n in a:
    if n not in b: print('GONE', dem(n)); continue
    if a[n] == b[n]: print('same ', len(a[n]), dem(n))
    else:
        ca = [l for l in a[n] if not l.lstrip().startswith(';')]; cb = [l for l in b[n] if not l.lstrip().startswith(';')]
        sm = difflib.SequenceMatcher(None, ca, cb, autojunk=False)
        print('DIFF ', len(a[n]), len(b[n]), 'places', len([o for o in sm.get_opcodes() if o[0] != 'equal']), dem(n))
for n in b:
    if n not in a: print('NEW  ', len(b[n]), dem(n))
