#!/usr/bin/env python
"""The only reader of include/segmm_hip.h.  Generates, from the header's text, the two committed files that mirror the C ABI:

  segmminterest_amd/csrc/cmd_dispatch.inc   the switch that lets segmm_run_phase call any stream-taking entry point from a
                                            recorded command (op id + 8-byte argument slots)
  segmminterest_amd/_abi.py                 plain data for the ctypes binding (hipabi.py): every prototype's parameter names and
                                            type codes, the ABI version, the integer constants, the fields of segmm_attn_planes_t and of the
                                            other descriptor structs (segmm_itable_t)

    python tools/gen_cmd_dispatch.py          # rewrite both files
    python tools/gen_cmd_dispatch.py --check  # fail if either is stale (__graft_entry__.build() and the tests run this)

Op ids are the alphabetical rank of the function name among the dispatchable entry points; the library exports the table
(segmm_cmd_op_name) so that host bindings never hard-code an id."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "segmm_hip.h")
OUT = os.path.join(ROOT, "segmminterest_amd", "csrc", "cmd_dispatch.inc")
OUT_ABI = os.path.join(ROOT, "segmminterest_amd", "_abi.py")

# entry points that are not kernels enqueued on a stream with device / persistent-host arguments
SKIP = {"segmm_step_get", "segmm_probe_mfma_rate", "segmm_run_phase", "segmm_step_begin", "segmm_embed_fwd", "segmm_embed_bwd",
        "segmm_layer_fwd", "segmm_layer_bwd", "segmm_head_loss_fwd", "segmm_head_loss_bwd", "segmm_step_tail"}

# by-value C type -> type code of _abi.py (hipabi.py maps the codes to ctypes); every pointer and segmm_stream_t is "p"
CODES = {"int": "i", "int64_t": "i64", "float": "f", "uint64_t": "u64", "uint32_t": "u32"}

# descriptor structs an entry point takes by pointer, besides segmm_attn_planes_t: their fields go into STRUCT_FIELDS of _abi.py
DESCRIPTORS = ("segmm_itable_t",)


def strip_comments(txt):
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def type_code(ty):
    if ty.endswith("*") or ty == "segmm_stream_t":
        return "p"
    if ty not in CODES:
        raise SystemExit("gen_cmd_dispatch: unhandled type %r" % ty)
    return CODES[ty]


def prototypes(txt):
    """[(name, [(C type, parameter name)])] of every ``int segmm_*(...)`` prototype; ``(void)`` gives an empty list."""
    out = []
    for m in re.finditer(r"\bint\s+(segmm_\w+)\s*\(([^;{]*?)\)\s*;", strip_comments(txt), flags=re.S):
        name, params = m.group(1), " ".join(m.group(2).split())
        ps = []
        for p in ([] if params in ("void", "") else params.split(",")):
            p = p.strip()
            mm = re.match(r"(.*?)(\w+)$", p)
            ty = mm.group(1).strip()
            # "const float *Qa" style declarators: the star belongs to the type
            ty = ty.replace(" *", "*")
            ps.append((ty, mm.group(2)))
        # declarators like "uint16_t *dqa, *dqb" do not occur in prototypes; "float* a, float* b" is the style used
        out.append((name, ps))
    return out


def constants(txt):
    """{name: value} of the integer ``#define SEGMM_*`` lines and of the anonymous enum."""
    txt = strip_comments(txt)
    out = {}
    for m in re.finditer(r"^[ \t]*#define[ \t]+(SEGMM_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", txt, flags=re.M):
        out[m.group(1)] = int(m.group(2))
    for m in re.finditer(r"\benum\s*\{([^}]*)\}\s*;", txt):
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            mm = re.match(r"(SEGMM_\w+)\s*=\s*(-?\d+)$", item)
            if mm is None:
                raise SystemExit("gen_cmd_dispatch: unhandled enum item %r" % item)
            out[mm.group(1)] = int(mm.group(2))
    return out


def struct_fields(txt, name):
    """[(field name, type code)] of ``typedef struct { ... } name;``, multi-declarator lines (``T *a, *b;``) included."""
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % re.escape(name), strip_comments(txt))
    if m is None:
        raise SystemExit("gen_cmd_dispatch: struct %s not found" % name)
    out = []
    for decl in filter(None, (" ".join(s.split()) for s in m.group(1).split(";"))):
        mm = re.match(r"((?:const )?\w+)\s*(.*)$", decl)
        for d in mm.group(2).split(","):
            dm = re.match(r"(\**)\s*(\w+)$", d.strip())
            if dm is None:
                raise SystemExit("gen_cmd_dispatch: unhandled field declaration %r in %s" % (decl, name))
            out.append((dm.group(2), type_code(mm.group(1) + dm.group(1))))
    return out


def cast(ty, k):
    a = "a[%d]" % k
    if ty.endswith("*"):
        return "(%s)%s.p" % (ty, a)
    if ty == "float":
        return "(float)%s.f" % a
    if ty in ("int", "int64_t", "uint64_t", "uint32_t"):
        return "(%s)%s.i" % (ty, a)
    raise SystemExit("gen_cmd_dispatch: unhandled parameter type %r" % ty)


def dispatch_inc(txt):
    """Text of cmd_dispatch.inc for the header text ``txt``."""
    protos = [(n, ps) for n, ps in prototypes(txt) if ps and ps[-1][0] == "segmm_stream_t" and n not in SKIP]
    protos.sort(key=lambda x: x[0])
    lines = ["// GENERATED by tools/gen_cmd_dispatch.py from include/segmm_hip.h -- do not edit.",
             "// op id = alphabetical rank of the entry point; arguments in declaration order, the trailing stream comes from the phase.",
             "static const int SEGMM_N_CMD_OPS = %d;" % len(protos),
             "static const char* const segmm_cmd_names[] = {"]
    lines += ['    "%s",' % n for n, _ in protos]
    lines += ["};", "static const unsigned char segmm_cmd_nargs[] = {" + ", ".join(str(len(ps) - 1) for _, ps in protos) + "};",
              "static int segmm_cmd_dispatch(int op, const segmm_arg_t* a, segmm_stream_t st) {", "    switch (op) {"]
    for i, (n, ps) in enumerate(protos):
        if len(ps) - 1 > 48:
            raise SystemExit("%s has %d arguments (> SEGMM_CMD_MAX_ARGS)" % (n, len(ps) - 1))
        args = [cast(ty, k) for k, (ty, _) in enumerate(ps[:-1])] + ["st"]
        lines.append("        case %d: return %s(%s);" % (i, n, ", ".join(args)))
    lines += ["        default: return -1;", "    }", "}", ""]
    return "\n".join(lines)


def abi_py(txt):
    """Text of _abi.py for the header text ``txt``: literals only."""
    consts = constants(txt)
    if "SEGMM_ABI_VERSION" not in consts:
        raise SystemExit("gen_cmd_dispatch: the header does not define SEGMM_ABI_VERSION")
    lines = ["# GENERATED by tools/gen_cmd_dispatch.py from include/segmm_hip.h -- do not edit.",
             "# Type codes: i int, i64 int64_t, f float, u64 uint64_t, u32 uint32_t, p any pointer or segmm_stream_t.",
             "ABI_VERSION = %d" % consts.pop("SEGMM_ABI_VERSION"),
             "CONSTANTS = {"]
    lines += ['    "%s": %d,' % kv for kv in consts.items()]
    lines += ["}", "ATTN_PLANES_FIELDS = ("]
    lines += ['    ("%s", "%s"),' % f for f in struct_fields(txt, "segmm_attn_planes_t")]
    lines += [")", "# descriptor struct -> ((field name, type code), ...) in declaration order", "STRUCT_FIELDS = {"]
    for name in DESCRIPTORS:
        if re.search(r"\}\s*%s\s*;" % re.escape(name), strip_comments(txt)):
            lines.append('    "%s": (%s),' % (name, "".join('("%s", "%s"), ' % f for f in struct_fields(txt, name)).rstrip()))
    lines += ["}", "# entry point -> ((parameter name, type code), ...) in declaration order", "PROTOTYPES = {"]
    for n, ps in prototypes(txt):
        lines.append('    "%s": (%s),' % (n, "".join('("%s", "%s"), ' % (p, type_code(ty)) for ty, p in ps).rstrip()))
    lines += ["}", ""]
    return "\n".join(lines)


def check(txt, current):
    """--check: exit with a message unless ``current`` ({path: text} of the generated files) is what the header text ``txt`` gives."""
    old = [os.path.basename(path) for path, gen in ((OUT, dispatch_inc), (OUT_ABI, abi_py)) if current.get(path) != gen(txt)]
    if old:
        raise SystemExit("%s stale: run python tools/gen_cmd_dispatch.py" % " and ".join(old))


def main():
    txt = open(HDR).read()
    if "--check" in sys.argv:
        return check(txt, {p: open(p).read() for p in (OUT, OUT_ABI) if os.path.exists(p)})
    for path, gen in ((OUT, dispatch_inc), (OUT_ABI, abi_py)):
        open(path, "w").write(gen(txt))
        print("wrote %s" % path)


if __name__ == "__main__":
    main()
