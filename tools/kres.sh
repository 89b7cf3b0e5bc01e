#!/bin/bash
# Resource usage (VGPRs, scratch, occupancy) of every kernel of one translation unit of csrc/, as hipcc reports it for the SHIPPED
# build: the compile line is the one the Makefile's rule gives that file (FITFLAGS where the rule applies them, none elsewhere).
# usage: tools/kres.sh fit_kernels.hip [grep pattern]
cd "$(dirname "$0")/../drone-sim-python_amd/csrc" || exit 1
src=${1:-fit_kernels.hip}
obj=${src%.*}.o
line=$(make -n -B "$obj" | grep -- "-c $src") || { echo "kres.sh: the Makefile has no rule that compiles $src" >&2; exit 1; }
${line% -o *} -Rpass-analysis=kernel-resource-usage -o /tmp/kres.o 2> /tmp/kres.txt
python3 ../../tools/res_usage.py /tmp/kres.txt | grep -E "${2:-.}"
