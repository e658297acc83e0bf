"""The paired k-loop of the MLP tile engine (psg_mlp.cuh: tile_mac4x2, deal_pairs), checked on the compiler's device assembly
of psg_pn2.hip: every kernel instantiation that can deal pairs carries the paired loop, runs without scratch and within
128 VGPRs (4 waves per SIMD), and the asm-boundary hazard lint finds nothing in it.  A build with -DPSG_MLP_PAIRS=0 has
no paired loop at all.  CPU test: hipcc cross-compiles gfx950 without a GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instantiations that deal pairs on the PointNet++ path: fp1 + head at 64 points, and the flipped last layer of the SA
# levels with two or more point blocks per workgroup (sa1 at 128 points, sa2 at 64; MSG scales alike)
PAIRED = [
    r"fp_fwd_kernelILi64ELi4ELb0E",
    r"fp_bwd_kernelILi64ELi4ELi2ELb0E",
    r"sa_fwd_kernelILi128ELi4ELi32ELi1ELb0E",
    r"sa_fwd_kernelILi64ELi4ELi32ELi1ELb1E",
]

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="needs hipcc")


def _asm(out_dir, extra=""):
    cmd = subprocess.run(["make", "-n", "-B", "psg_pn2.o"], cwd=CSRC, capture_output=True, text=True, check=True).stdout
    line = next(l for l in cmd.splitlines() if "hipcc" in l and " -c " in l)
    out = os.path.join(out_dir, "psg_pn2.s")
    line = line.replace(" -c ", " %s -S --cuda-device-only -c " % extra).replace("-o psg_pn2.o", "-o " + out)
    subprocess.run(line, shell=True, cwd=CSRC, check=True, capture_output=True)
    return out


def _functions(path):
    """{mangled name: assembly text} of every kernel in the file"""
    text = open(path).read()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_Z\S+):", text, re.M)]
    return {name: text[a:(starts[i + 1][0] if i + 1 < len(starts) else len(text))] for i, (a, name) in enumerate(starts)}


@needs_hipcc
def test_paired_instantiations(tmp_path):
    import check_asm_hazards
    import mlp_asm_table
    path = _asm(str(tmp_path))
    funcs = _functions(path)
    table = mlp_asm_table.scan(path, "|".join(PAIRED))
    for pat in PAIRED:
        names = [n for n in funcs if re.search(pat, n)]
        assert names, pat
        for n in names:
            assert "L_psg_x2_loop_" in funcs[n], "%s: no paired k-loop" % n
            assert table[n]["scratch"] == 0, "%s: scratch %d bytes" % (n, table[n]["scratch"])
            assert table[n]["vgpr"] <= 128, "%s: %d VGPRs" % (n, table[n]["vgpr"])
    bad = check_asm_hazards.scan(path)
    assert not bad, bad[:5]


@needs_hipcc
def test_pairs_switch_off(tmp_path):
    """-DPSG_MLP_PAIRS=0 (tools/build_variant.sh) builds the single-tile engine: no paired loop anywhere"""
    path = _asm(str(tmp_path), "-DPSG_MLP_PAIRS=0")
    assert "L_psg_x2_loop_" not in open(path).read()
