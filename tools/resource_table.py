#!/usr/bin/env python3
"""The compiler's resource remarks of chosen kernels as one table (no GPU needed).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -c -o /dev/null \\
        -Rpass-analysis=kernel-resource-usage segmminterest_amd/csrc/capi.hip 2> remarks.txt
    python tools/resource_table.py remarks.txt layernorm_fwd colsum splitk_reduce > profiles/row_stream/resource_usage.txt

Every further argument is a substring of the demangled kernel name to keep.  The columns are the remark's own fields;
tests/test_row_stream_cpu.py reads the committed table back (no instance may use scratch, and the LayerNorm forward's grid table in
capi.hip must be 256 CUs x the occupancy listed here)."""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS"), ("VGPRs Spill", "spills")]


def parse(text):
    """-> [(mangled name, {field: int})] in the order of the remarks"""
    out = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            out.append((m.group(1), {}))
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass-analysis", line)
        if m and out:
            out[-1][1][m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True)
        return [re.sub(r"^(void )?segmm::", "", n) for n in r.stdout.splitlines()]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    rows = parse(open(argv[1]).read())
    names = demangle([n for n, _ in rows])
    keep = argv[2:]
    print("# hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -Rpass-analysis=kernel-resource-usage, csrc/capi.hip")
    print("# scratch in bytes per lane, occupancy in waves per SIMD, LDS in bytes per workgroup")
    print("%-44s %6s %6s %6s %8s %10s %6s %7s" % (("kernel",) + tuple(h for _, h in FIELDS)))
    seen = set()
    for name, (_, f) in zip(names, rows):
        if name in seen or (keep and not any(k in name for k in keep)):
            continue
        seen.add(name)
        print("%-44s %6d %6d %6d %8d %10d %6d %7d" % ((name,) + tuple(f.get(k, -1) for k, _ in FIELDS)))


if __name__ == "__main__":
    main(sys.argv)
