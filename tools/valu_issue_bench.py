#!/usr/bin/env python3
"""Driver of tools/valu_issue_bench.hip: build the stand-alone program for gfx950 when it is missing or older than
its source, run it once on device 0 and write its markdown table (cycles per MFMA gap of v_mfma_f32_32x32x16_f16
with scalar / packed f32 fillers and the four forms of the fp16-pair residual, at one and two waves per SIMD).

    python tools/valu_issue_bench.py --out profiles/r16/valu_issue_table.md
    python tools/valu_issue_bench.py --build-only          # cross-compile, no GPU needed
"""

import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'valu_issue_bench.hip')
EXE = os.path.join(HERE, 'valu_issue_bench')


def build() -> None:
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= os.path.getmtime(SRC):
        return
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-O3', '--offload-arch=gfx950', SRC, '-o', EXE], check=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the table to this file as well as to stdout')
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--timeout', type=float, default=240.0, help='seconds allowed for the one run')
    a = ap.parse_args()
    build()
    if a.build_only:
        return 0
    return subprocess.run([EXE] + ([a.out] if a.out else []), timeout=a.timeout).returncode


if __name__ == '__main__':
    sys.exit(main())
