#!/usr/bin/env python3
"""VGPR / scratch / LDS / occupancy of every kernel of one or more of libmghip's units (hipcc -Rpass-analysis=kernel-resource-usage,
device code only), one line each.

    python3 tools/kernel_resources.py [substring-of-mangled-name] [--unit mg_heat.hip ...] [--root other/checkout] [compiler flags]

--unit: the units to compile (default mg_launch.hip; `solvers` stands for the seven units of the solver modules).
--root: the checkout whose csrc/ is compiled (default: this one), to put two trees side by side.
"""
import argparse
import os
import re
import subprocess
import tempfile

SOLVERS = ["mg_pcg.hip", "mg_heat.hip", "mg_rd.hip", "mg_nl.hip", "mg_eig.hip", "mg_ho.hip", "mg_flow.hip"]
ap = argparse.ArgumentParser()
ap.add_argument("filter", nargs="?", default="")
ap.add_argument("--unit", action="append")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args, flags = ap.parse_known_args()
units = [u for name in (args.unit or ["mg_launch.hip"]) for u in (SOLVERS if name == "solvers" else [name])]

rows = {}
for unit in units:
    src = os.path.join(args.root, "mixed_precision_multigrid_solvers_for_pdes_amd", "csrc", unit)
    with tempfile.NamedTemporaryFile(suffix=".o") as obj:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-c", "-o", obj.name, src] + flags
        out = subprocess.run(cmd, capture_output=True, text=True).stderr
    cur = None
    for line in out.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.rsplit(":", 1)
            rows[cur][k.strip()] = v.strip()
for name, r in sorted(rows.items()):
    if args.filter in name:
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        short = re.sub(r"\(.*", "", short)[:110]
        print(f"{short:110s} vgpr {r.get('VGPRs'):>4s} agpr {r.get('AGPRs'):>3s} spill {r.get('VGPRs Spill'):>3s} "
              f"scratch {r.get('ScratchSize [bytes/lane]'):>3s} lds {r.get('LDS Size [bytes/block]'):>6s} occ {r.get('Occupancy [waves/SIMD]')}")
