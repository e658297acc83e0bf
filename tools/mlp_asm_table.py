"""Per-kernel instruction table of the MLP kernels from hipcc's device assembly (-S), for DESIGN section 4.

For every kernel whose name matches the filter (default: the PointNet++ module kernels sa_fwd / sa_bwd / fp_fwd / fp_bwd /
pw_bwd): VGPRs, scratch bytes, waves per SIMD, and static instruction counts split into inside the inline-assembly blocks
(the k-loops) and outside them (gathers, epilogues, write-backs, the compiler's K tails):
  mfma      v_mfma_*                       vmem  global_* / buffer_*   lds  ds_*
  valu      other v_* (vector ALU)         salu  s_* except waits / nops / branches   wait  s_waitcnt, s_nop
Static counts: a loop body counts once.  The k-loop MFMAs per tile follow from the kernel's shapes.
usage: mlp_asm_table.py file.s [regex]      (build the .s as tests/test_asm_hazards.py does)"""
import re
import sys

DEFAULT = r"(sa_fwd|sa_bwd|fp_fwd|fp_bwd|pw_bwd)_kernel"


def demangle_short(name):
    """_ZN3psg13sa_fwd_kernelILi128ELi4ELi32ELi1ELb0EEEvNS_9SaFwdArgsE -> sa_fwd_kernel<128,4,32,1,0>"""
    m = re.match(r"_Z(?:N\d+psg)?\d+(\w+?_kernel)I(.*)E", name)
    if not m:
        return name
    args = re.findall(r"L([ib])(\d+)E", m.group(2))
    return "%s<%s>" % (m.group(1), ",".join(v for _, v in args))


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return None


KEYS = ("mfma", "vmem", "lds", "valu", "salu", "wait")


def scan(path, pattern=DEFAULT):
    rx = re.compile(pattern)
    rows, cur, inasm = {}, None, False
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1) if rx.search(m.group(1)) else None
            if cur:
                rows[cur] = {"in": dict.fromkeys(KEYS, 0), "out": dict.fromkeys(KEYS, 0)}
            inasm = False
            continue
        if cur is None:
            continue
        if "ASMSTART" in line:
            inasm = True
            continue
        if "ASMEND" in line:
            inasm = False
            continue
        for key, field in (("; NumVgprs:", "vgpr"), ("; ScratchSize:", "scratch"), ("; Occupancy:", "occ")):
            if line.strip().startswith(key):
                rows[cur][field] = int(line.split(":")[1])
        code = line.split(";")[0].strip()
        if not code or code.endswith(":") or code.startswith("."):
            continue
        c = classify(code.split()[0])
        if c:
            rows[cur]["in" if inasm else "out"][c] += 1
    return rows


def main():
    path = sys.argv[1]
    pattern = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    rows = scan(path, pattern)
    hdr = "| kernel | VGPR | scratch | waves/SIMD | " + " | ".join("asm " + k for k in KEYS[:4]) + " | " + \
        " | ".join("other " + k for k in KEYS) + " |"
    print(hdr)
    print("|" + "---|" * (hdr.count("|") - 1))
    for name in sorted(rows, key=demangle_short):
        r = rows[name]
        print("| %s | %s | %s | %s | %s | %s |" % (
            demangle_short(name), r.get("vgpr", "?"), r.get("scratch", "?"), r.get("occ", "?"),
            " | ".join(str(r["in"][k]) for k in KEYS[:4]), " | ".join(str(r["out"][k]) for k in KEYS)))


if __name__ == "__main__":
    main()
