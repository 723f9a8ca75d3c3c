"""The dynamic-LDS layouts of the fp32 fused and the planes-in attention backward kernels (csrc/attention_lds.h) without a GPU: a stand-alone host program
that includes only that header prints bytes() of every layout over the launcher's whole domain, and checks each layout's regions
(no overlap, 16-byte alignment where the kernels use float4 / uint4, the planes-in kernel's transpose scratch inside its K
image).  Every byte count is compared with the formulas the launcher carried by hand before the header existed, written out
below: the LDS bytes of a launch decide how many workgroups a CU holds, so they must not move."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "segmminterest_amd", "csrc")

PROGRAM = r"""
#include "attention_lds.h"
#include <cstdio>
using namespace segmm;

static int bad = 0;
template <class LAYOUT>
static size_t checked(const char* form, const LAYOUT& L) {
    size_t prev_end = 0;
    const char* prev = "";
    L.regions([&](const char* name, size_t begin, size_t end, int align) {
        if (begin < prev_end || end < begin) { std::printf("BAD %s: '%s' overlaps '%s'\n", form, name, prev); ++bad; }
        if (end > begin && begin % (size_t)align != 0) { std::printf("BAD %s: '%s' at %zu, needs %d\n", form, name, begin, align); ++bad; }
        prev_end = end; prev = name;
    });
    if (prev_end != L.bytes()) { std::printf("BAD %s: bytes() is not the end of the last region\n", form); ++bad; }
    return L.bytes();
}

int main() {
    const int dhs[] = {4, 8, 16, 32, 48, 64, 96, 128};
    for (int dh : dhs)
        for (int qc = 16; qc <= 48; qc += 16)
            for (int nw = 1; nw <= 12; ++nw)
                for (int tp = 16; tp <= 384; tp += 16)
                    for (int merged = 0; merged < 2; ++merged) {
                        if (dh <= 64) std::printf("fused %d %d %d %d %d %zu\n", dh, qc, nw, tp, merged, checked("fused", att_lds_fused(dh, qc, nw, tp, merged != 0)));
                    }
    for (int dh = 16; dh <= 48; dh += 16)
        for (int nw = 1; nw <= 12; ++nw) {
            std::printf("pl %d 48 %d 0 0 %zu\n", dh, nw, checked("pl", att_lds_pl(dh, 48, nw)));
            if (!att_lds_pl_scratch_fits(dh)) { std::printf("BAD pl: transpose scratch outside the K image at dh %d\n", dh); ++bad; }
        }
    return bad ? 1 : 0;
}
"""


# ---- the launcher's formulas as they stood before the header (attn_launch_bwd, attn_bwd_pl_lds_bytes)
def fused_bytes(DH, Lq_p, nw, Tp, merged):
    if merged:
        return (5 * Lq_p * (DH + 4) + 3 * Lq_p + nw * 16 * 20 + 8 + Lq_p * (DH // 4)) * 4 + Lq_p + Tp
    return (3 * Lq_p * (DH + 4) + 3 * Lq_p + nw * 16 * 20 + 4 + Lq_p * (DH // 4)) * 4 + Lq_p + Tp


def pl_bytes(DH, QC, nw):
    return (3 * QC * (DH + 4) + 3 * QC + 4 + 36) * 4 + nw * 2 * 16 * (DH * 2 + 8) + QC


def _host_compiler():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            return path
    rocm = "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(rocm), "no host C++ compiler found"
    return rocm


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("attn_lds")
    src, exe = d / "attn_lds.cpp", d / "attn_lds"
    src.write_text(PROGRAM)
    subprocess.check_call([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    rows = [ln.split() for ln in run.stdout.splitlines()]
    return run.returncode, rows


def test_regions_do_not_overlap_and_are_aligned(table):
    rc, rows = table
    assert [r for r in rows if r[0] == "BAD"] == [] and rc == 0


def test_byte_counts_are_the_hand_written_formulas(table):
    _, rows = table
    seen = {"fused": 0, "pl": 0}
    for form, a, b, c, d, e, got in (r for r in rows if r[0] != "BAD"):
        a, b, c, d, e, got = int(a), int(b), int(c), int(d), int(e), int(got)
        want = fused_bytes(a, b, c, d, bool(e)) if form == "fused" else pl_bytes(a, b, c)
        assert got == want, (form, a, b, c, d, e, got, want)
        seen[form] += 1
    assert seen == {"fused": 6 * 3 * 12 * 24 * 2, "pl": 3 * 12}
