#!/bin/bash
# Register / scratch / LDS use of the built kernels whose names match $1 (regex): a filter over
# the resource-usage remarks the build keeps beside each kernel object: build_obj/*.ru, or, for
# a `make variants VARIANT_NAME=<name>` build, OBJDIR=build_variants/obj_<name> (both relative to
# the repository root, where the Makefile's OBJDIR and VARIANTS_DIR point).
cd "$(dirname "$0")/.."
cat "${OBJDIR:-build_obj}"/dmt_kernels_*.o.ru |
  python3 -c '
import re, sys
pat = re.compile(sys.argv[1]); cur = None; out = {}
for l in sys.stdin:
    m = re.search(r"Function Name: (\S+)", l)
    if m: cur = m.group(1); out[cur] = {}; continue
    m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", l)
    if m and cur: out[cur][m.group(1).split()[0]] = int(m.group(2))
for k, v in out.items():
    if pat.search(k): print(k[:90], v)
' "${1:-.}"
