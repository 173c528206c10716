#!/usr/bin/env python3
"""Register, scratch, occupancy and LDS use of every __global__ of the engine,
from the compiler's own remarks (no GPU needed).

Compiles the engine sources with the flags of ksched_amd/_build.py plus
-Rpass-analysis=kernel-resource-usage (device code only, nothing is written)
and prints one row per kernel. Occupancy is waves per SIMD: on gfx950 a kernel
reaches 5 at <= 96 VGPRs, 6 at <= 80, 7 at <= 72, 8 at <= 64.

    python tools/kernel_resources.py                  # the engine (ks_engine*.hip)
    python tools/kernel_resources.py ks_cell.hip      # other sources of csrc/
    python tools/kernel_resources.py --filter 'k_bf_round|k_sweep'
    python tools/kernel_resources.py --all            # library templates (hipCUB) too
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ksched_amd import _build  # noqa: E402

ENGINE = ("ks_engine.hip", "ks_engine_build.hip", "ks_engine_io.hip", "ks_engine_sched.hip")
FIELDS = (("Function Name", "name"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"))
REMARK = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?):\s*(\S+)\s*\[-Rpass-analysis=kernel-resource-usage\]")


def demangle(names: list[str]) -> list[str]:
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if tool and os.path.exists(tool):
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return out.splitlines()
    return names


def short(sig: str) -> str:
    """void k_sweep<true>(DG, int, int) -> k_sweep<true>"""
    sig = sig.removeprefix("void ").replace("(anonymous namespace)::", "").replace("ks::", "")
    depth = 0
    for i, ch in enumerate(sig):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return sig[:i]
    return sig


def resources(src: str, arch: str) -> list[dict]:
    cmd = [_build.hipcc(), *_build._flags(arch), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", src, "-o", os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.stderr.write(p.stderr)
        raise SystemExit(f"{os.path.basename(src)}: the compile failed")
    key = dict(FIELDS)
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = REMARK.search(line)
        if not m or m.group(1) not in key:
            continue
        k = key[m.group(1)]
        if k == "name":
            cur = {"name": m.group(2), "file": os.path.basename(src)}
            rows.append(cur)
        elif cur is not None:
            cur[k] = int(m.group(2))
    for r, d in zip(rows, demangle([r["name"] for r in rows])):
        n = short(d)
        r["name"] = n if len(n) <= 72 else n[:69] + "..."
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("sources", nargs="*", default=list(ENGINE), help="files of ksched_amd/csrc (default: the engine)")
    ap.add_argument("--arch", default=os.environ.get("KS_OFFLOAD_ARCH", "gfx950"))
    ap.add_argument("--filter", default="", help="regular expression on the kernel name")
    ap.add_argument("--all", action="store_true", help="also the kernels of library templates (names not starting k_)")
    a = ap.parse_args()
    rows = []
    for s in a.sources:
        rows += resources(s if os.path.isabs(s) else os.path.join(_build.CSRC, s), a.arch)
    if not a.all:
        rows = [r for r in rows if r["name"].startswith("k_")]
    if a.filter:
        rows = [r for r in rows if re.search(a.filter, r["name"])]
    rows.sort(key=lambda r: (r["file"], r["name"]))
    w = max([len(r["name"]) for r in rows] + [6])
    print(f"# {a.arch}; occupancy in waves/SIMD, scratch in bytes/lane, LDS in bytes/workgroup")
    print(f"{'kernel':<{w}}  {'VGPRs':>5}  {'AGPRs':>5}  {'SGPRs':>5}  {'scratch':>7}  {'occ':>3}  {'LDS':>6}  file")
    for r in rows:
        print(f"{r['name']:<{w}}  {r.get('vgpr', 0):>5}  {r.get('agpr', 0):>5}  {r.get('sgpr', 0):>5}  "
              f"{r.get('scratch', 0):>7}  {r.get('occ', 0):>3}  {r.get('lds', 0):>6}  {r['file']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
