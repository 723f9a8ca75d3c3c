#!/usr/bin/env python3
"""Register, scratch and LDS use of every attention kernel the dispatcher can reach at head dims 64, 96 and 128.

Writes one translation unit of explicit instantiations (the instance ladders of attn_launch_fwd / attn_launch_bwd in
csrc/capi.hip), compiles its DEVICE code only for gfx950 with -Rpass-analysis=kernel-resource-usage and prints, per
instantiation: VGPRs, AGPRs, scratch bytes per lane, occupancy (waves per SIMD) and static LDS.  Needs hipcc, no GPU.

    python tools/attn_resource_table.py                 > profiles/attn_wide_heads_resources.txt
    python tools/attn_resource_table.py --dh 64 --csrc OTHER_TREE/segmminterest_amd/csrc      # the DH = 64 rows of another tree
    python tools/attn_resource_table.py --check profiles/attn_wide_heads_resources.txt       # the committed table is current
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 64          # head dims above this take attn_bwd_fused_wide_kernel (att_wide, csrc/attention.h)


def instantiations(dh):
    """(kernel<args>, used on the default model path) for one head dim, in dispatcher order."""
    out = []
    for nt in (4, 10, 12):
        out.append(("attn_fwd_kernel<%d, %d>" % (dh, nt), True))
    if dh <= WIDE:
        for nt in (4, 10, 12):
            out.append(("attn_fwd_lds_kernel<%d, %d>" % (dh, nt), True))
    out.append(("attn_fwd_stream_kernel<%d>" % dh, False))
    out.append(("attn_D_kernel<%d>" % dh, True))
    out.append(("attn_D_stream_kernel<%d>" % dh, False))
    for nt in (4, 10, 12):
        out.append(("attn_bwd_dq_kernel<%d, %d>" % (dh, nt), False))
    out.append(("attn_bwd_dq_stream_kernel<%d>" % dh, False))
    for nqt in (0, 1, 3):
        out.append(("attn_bwd_dkv_kernel<%d, %d>" % (dh, nqt), False))
    fused, waves = ("attn_bwd_fused_kernel", (4, 8, 12)) if dh <= WIDE else ("attn_bwd_fused_wide_kernel", (4, 8))
    for nw in waves:
        out.append(("%s<%d, %d, true, 16>" % (fused, dh, nw), True))
        out.append(("%s<%d, %d, true, 32>" % (fused, dh, nw), True))
        out.append(("%s<%d, %d, true, 48>" % (fused, dh, nw), True))
        out.append(("%s<%d, %d, false, 48>" % (fused, dh, nw), True))
    return out


def translation_unit(dhs, have_wide):
    lines = ['#include "attention.h"', '#include "attention_stream.h"']
    if have_wide:
        lines.append('#include "attention_wide.h"')
    lines.append("namespace segmm {")
    for dh in dhs:
        for inst, _ in instantiations(dh):
            lines.append("template __global__ void %s(const AttnArgs);" % inst)
    lines.append("}")
    return "\n".join(lines) + "\n"


FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"))


def compile_and_parse(csrc, dhs):
    hipcc = shutil.which("hipcc")
    if hipcc is None:
        sys.exit("attn_resource_table: hipcc not found")
    have_wide = os.path.exists(os.path.join(csrc, "attention_wide.h"))
    if not have_wide:
        dhs = [d for d in dhs if d <= WIDE]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "attn_instances.hip")
        with open(src, "w") as f:
            f.write(translation_unit(dhs, have_wide))
        cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-c", "-I", csrc,
               "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "attn_instances.o"), src]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit("attn_resource_table: compile failed\n" + r.stdout[-4000:])
    res, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt")
    names = list(res)
    dem = subprocess.run([filt] + names, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    table = {}
    for mangled, d in zip(names, dem):
        m = re.match(r"void segmm::(\w+<[^>]*>)", d)
        if m:
            table[re.sub(r"\s+", " ", m.group(1))] = res[mangled]
    return table, dhs


def norm(inst):
    """demangled spelling of an instantiation: defaulted QCH spelled out, no space after commas"""
    return inst.replace(", ", ",")


def render(table, dhs):
    byname = {norm(k): v for k, v in table.items()}
    out = ["# attention kernels at head dims %s: hipcc --offload-arch=gfx950 -O3, device code only, -Rpass-analysis=kernel-resource-usage"
           % ", ".join(str(d) for d in dhs),
           "# path: default = taken by a model step with no knob set at <= 192 padded keys; opt = above 192 keys or under a knob",
           "%-50s %-8s %6s %6s %14s %10s %10s" % ("kernel", "path", "VGPR", "AGPR", "scratch B/lane", "waves/SIMD", "LDS B")]
    for dh in dhs:
        for inst, default in instantiations(dh):
            d = byname.get(norm(inst))
            if d is None:
                sys.exit("attn_resource_table: no remark for %s (have: %s)" % (inst, ", ".join(sorted(byname))))
            out.append("%-50s %-8s %6d %6d %14d %10d %10d" % (inst, "default" if default else "opt", d["vgpr"], d["agpr"], d["scratch"],
                                                              d["occ"], d["lds"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "segmminterest_amd", "csrc"), help="directory of the kernel headers")
    ap.add_argument("--dh", type=int, nargs="*", default=[64, 96, 128])
    ap.add_argument("--check", metavar="FILE", help="compare with a committed table instead of printing")
    a = ap.parse_args()
    table, dhs = compile_and_parse(a.csrc, a.dh)
    text = render(table, dhs)
    if a.check:
        with open(a.check) as f:
            if f.read() != text:
                sys.stdout.write(text)
                sys.exit("attn_resource_table: %s is stale" % a.check)
        print("attn_resource_table: %s is current" % a.check)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
