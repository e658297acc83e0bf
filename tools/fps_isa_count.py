"""Instruction mix of the step loop of every fps_kernel instantiation (psg_geometry.hip), from hipcc's device assembly.
Compiles the unit with the Makefile's flags plus -S --cuda-device-only (no GPU needed), finds in each fps_kernel the step
loop - the innermost backward-branch loop that holds the s_barrier, or the only loop left after the prologue when the
kernel has one wave and no barrier - and prints per instantiation the vector-ALU (v_*), s_nop, LDS (ds_*) and other scalar
(s_*) instruction counts of the loop and the kernel's VGPR count and scratch size.  Opcodes are counted by class only.
usage: python tools/fps_isa_count.py [--source FILE.hip] [--asm FILE.s]     (--asm: count an existing listing)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")
# psg_geometry.o's line of the Makefile: COMMON + -ffp-contract=off
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=off"]


def compile_asm(source):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-S", "--cuda-device-only", source, "-o", out])
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True)
        return r.stdout.split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):
        return names


def functions(path):
    """name -> list of lines of every fps_kernel body, and name -> metadata lines that follow it"""
    body, meta, name, where = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\S*fps_kernel\S*):", line)
        if m:
            name, where = m.group(1), "body"
            body[name], meta[name] = [], []
            continue
        if name is None:
            continue
        if where == "body":
            body[name].append(line)
            if line.split(";")[0].strip() == "s_endpgm":
                where = "meta"
        else:
            if re.match(r"^_Z\S+:", line):
                name = None
                continue
            meta[name].append(line)
            if ".end_amdhsa_kernel" in line:
                name = None
    return body, meta


def step_loop(lines):
    """(first, last) line index of the step loop: backward branches give the loops; the one with the s_barrier, else the
    last one (the prologue loops come first), and of nested candidates the innermost"""
    labels, last = {}, {}
    for i, line in enumerate(lines):
        code = line.split(";")[0].strip()
        m = re.match(r"^(\.L\w+):", code)
        if m:
            labels[m.group(1)] = i
        m = re.match(r"^s_c?branch\w*\s+(\.L\w+)", code)
        if m and m.group(1) in labels:
            last[labels[m.group(1)]] = i          # several backward branches to one label: one loop, up to the last
    loops = sorted(last.items())
    if not loops:
        return None
    with_barrier = [l for l in loops if any(x.split(";")[0].strip() == "s_barrier" for x in lines[l[0]:l[1] + 1])]
    cand = with_barrier or [max(loops, key=lambda l: l[1])]
    return min(cand, key=lambda l: l[1] - l[0])


def count(lines):
    c = {"valu": 0, "s_nop": 0, "lds": 0, "salu": 0, "other": 0}
    for line in lines:
        code = line.split(";")[0].strip()
        if not code or code.endswith(":") or code.startswith("."):
            continue
        op = code.split()[0]
        if op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        else:
            c["other"] += 1
    return c


def table(asm):
    body, meta = functions(asm)
    names = sorted(body)
    rows = []
    for name, pretty in zip(names, demangle(names)):
        loop = step_loop(body[name])
        c = count(body[name][loop[0]:loop[1] + 1]) if loop else None
        vgpr = scratch = None
        for line in meta[name]:
            m = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", line)
            if m:
                vgpr = int(m.group(1))
            m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
            if m:
                scratch = int(m.group(1))
        m = re.search(r"fps_kernel<([^>]*)>", pretty)
        rows.append((m.group(0) if m else name, c, vgpr, scratch))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(CSRC, "psg_geometry.hip"))
    ap.add_argument("--asm", default=None)
    a = ap.parse_args()
    rows = table(a.asm or compile_asm(a.source))
    if not rows:
        sys.exit("no fps_kernel in the listing")
    print("%-34s %6s %6s %5s %6s %6s %5s %8s" % ("step loop of", "v_*", "s_nop", "ds_*", "s_*", "other", "VGPR", "scratch"))
    for name, c, vgpr, scratch in rows:
        if c is None:
            print("%-34s no loop found" % name)
            continue
        print("%-34s %6d %6d %5d %6d %6d %5s %8s" % (name, c["valu"], c["s_nop"], c["lds"], c["salu"], c["other"], vgpr, scratch))
