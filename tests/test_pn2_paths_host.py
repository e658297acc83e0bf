"""The PointNet++ launch decisions (pointsecguard_amd/csrc/psg_pn2_paths.h: the switch set, the table of SA module kernels, the
architecture descriptors and sa_path) compiled for the HOST in a tiny stand-alone program - the pattern of
tests/test_ce_row_host.py: the system compiler, no GPU, no library loaded into Python.

The program prints, for SSG and MSG, every SA level / scale / direction (forward, backward, colour-only backward, and for SSG
the full backward): the kernel family with the template arguments run_sa_fwd / run_sa_bwd instantiate for the scale's row, and
the launch site's variant; and per FP level whether its first layer is split.  Each switch setting runs in a process of its
own (the switches are read once per process).

The table below was derived BY HAND from run_sa_fwd / run_sa_bwd / sa_pack_bwd_level / sa_sparse_spv as they stood before the
decision moved into the header (the four forward and four backward switch tables and their qualifying expressions), not from
the header: _default() is written out in full, every other setting (SETTINGS) as the lines it changes, and ERRORS names three
combinations that are an error at a launch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointsecguard_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "psg_pn2_paths.h"
using namespace psg_pn2;
// the template arguments run_sa_fwd / run_sa_bwd (psg_pn2.hip) give a family at a row
static std::string kernel(SaKernel k, const SaCfg &r)
{
    char b[96];
    const int s = (r.v & V_PACK) != 0;
    switch (k) {
    case SaKernel::fwd_whole: snprintf(b, sizeof b, "sa_fwd_kernel<%d,%d,%d,%d>", r.P, r.NW, r.K, r.maxt_f); break;
    case SaKernel::fwd_split: snprintf(b, sizeof b, "sa_fwd_kernel<%d,%d,%d,%d,true>", r.P, r.NW, r.K, r.maxt_f); break;
    case SaKernel::fwd_packed: snprintf(b, sizeof b, "sa_fwd_packed_kernel<%d,%d,%s>", r.P, r.NW, s ? "true" : "false"); break;
    case SaKernel::fwd_packed_keys: snprintf(b, sizeof b, "sa_fwd_packed_kernel<%d,%d,%s,true>", r.P, r.NW, s ? "true" : "false"); break;
    case SaKernel::bwd_dense: snprintf(b, sizeof b, "sa_bwd_kernel<%d,%d,%d,%d>", r.P, r.NW, r.maxt_b, r.K); break;
    case SaKernel::bwd_sparse: snprintf(b, sizeof b, "sa_bwd_sparse_kernel<%d,%d,%d,%d>", r.P, r.NW, r.maxt_b, r.spv); break;
    case SaKernel::bwd_packed_dense0:
    case SaKernel::bwd_packed_sparse: snprintf(b, sizeof b, "sa_bwd_packed_kernel<%d,%d,1,%d>", r.P, r.NW, r.spv); break;
    case SaKernel::bwd_packed_chan: snprintf(b, sizeof b, "sa_bwd_packed_kernel<%d,%d,1,%d+CHAN>", r.P, r.NW, r.spv); break;
    default: snprintf(b, sizeof b, "error"); break;
    }
    return b;
}
int main()
{
    const Pn2Switches sw = read_switches([](const char *n, int d) { const char *v = getenv(n); return v ? atoi(v) : d; },
                                         [](const char *n) -> const char * { return getenv(n); });
    for (int arch = 0; arch < 2; ++arch) {
        const ArchDesc &A = arch_of(arch);
        const char *an = arch ? "msg" : "ssg";
        for (int l = 0; l < 4; ++l)
            for (int s = 0; s < A.ns; ++s) {
                const SaPath p = sa_path(A, sw, l, s);
                const SaCfg &r = SaRows::cfg[A.sc[l][s].row];
                const SaKernel f = sa_fwd_family(p);
                if (f == SaKernel::error) printf("%s l%d s%d fwd error %s\n", an, l, s, p.fwd_error);
                else printf("%s l%d s%d fwd %s %s\n", an, l, s, kernel(f, r).c_str(), sa_site(r, f, l, false).text);
                const char *dirs[3] = {"bwd", "bwd_colour", "bwd_full"};
                for (int d = 0; d < (arch ? 2 : 3); ++d) {
                    const bool colour = d == 1 && l == 0;       // (a colour-only request stores compact rows at level 0 only)
                    const SaKernel b = sa_bwd_family(p, colour);
                    if (b == SaKernel::error) printf("%s l%d s%d %s error %s\n", an, l, s, dirs[d], p.bwd_error);
                    else printf("%s l%d s%d %s %s %s\n", an, l, s, dirs[d], kernel(b, r).c_str(), sa_site(r, b, l, sa_w1c(p, colour)).text);
                }
            }
        for (int l = 0; l < 4; ++l) printf("%s fp%d split=%d\n", an, l, fp_split(sw, l) ? 1 : 0);
    }
    return 0;
}
"""

# rows of the kernel table as they appear in a site: p<P>w<NW>k<K>f<maxt_f>b<maxt_b>
S1, S2, S3, S4 = "#p128w4k32f1b1", "#p64w4k32f1b2", "#p32w4k32f1b2", "#p32w8k32f1b2"
M1A, M2A, M2B, M3A, M4A, M4B = "#p128w4k16f1b1", "#p64w4k16f1b2", "#p64w8k32f1b1", "#p32w8k16f1b2", "#p32w8k16f1b3", "#p32w8k32f2b3"


def _all_bwd(arch, l, s, kern, site, colour=None):
    """bwd, bwd_colour (and bwd_full for SSG) of a level: the same launch, except a colour-only request where `colour` is given"""
    out = {(arch, l, s, "bwd"): (kern, site), (arch, l, s, "bwd_colour"): colour or (kern, site)}
    if arch == "ssg":
        out[(arch, l, s, "bwd_full")] = (kern, site)
    return out


def _default():
    e = {}
    # SSG as shipped: level 0 whole, levels 1 - 3 split, every forward packed, the backward packed at levels 0 - 2 (so their
    # forwards key the masks by packed workgroup), channel order at levels 1 and 2, level 3's backward the unpacked sparse kernel
    e[("ssg", 0, 0, "fwd")] = ("sa_fwd_packed_kernel<128,4,false,true>", S1 + "#keys#packed")
    e[("ssg", 1, 0, "fwd")] = ("sa_fwd_packed_kernel<64,4,true,true>", S2 + "#keys#packed")
    e[("ssg", 2, 0, "fwd")] = ("sa_fwd_packed_kernel<32,4,true,true>", S3 + "#keys#packed")
    e[("ssg", 3, 0, "fwd")] = ("sa_fwd_packed_kernel<32,8,true>", S4 + "#packed")
    e.update(_all_bwd("ssg", 0, 0, "sa_bwd_packed_kernel<128,4,1,0>", S1 + "#bwd#packed",
                      ("sa_bwd_packed_kernel<128,4,1,0>", S1 + "#colour#bwd#packed")))
    e.update(_all_bwd("ssg", 1, 0, "sa_bwd_packed_kernel<64,4,1,1+CHAN>", S2 + "#chan#sa2#bwd#packed"))
    e.update(_all_bwd("ssg", 2, 0, "sa_bwd_packed_kernel<32,4,1,2+CHAN>", S3 + "#chan#sa3#bwd#packed"))
    e.update(_all_bwd("ssg", 3, 0, "sa_bwd_sparse_kernel<32,8,2,4>", S4 + "#sparse"))
    # MSG: never packed, never sparse; level 0 whole, levels 1 - 3 split
    e[("msg", 0, 0, "fwd")] = ("sa_fwd_kernel<128,4,16,1>", M1A + "#whole")
    e[("msg", 0, 1, "fwd")] = ("sa_fwd_kernel<128,4,32,1>", S1 + "#whole")
    e[("msg", 1, 0, "fwd")] = ("sa_fwd_kernel<64,4,16,1,true>", M2A + "#split")
    e[("msg", 1, 1, "fwd")] = ("sa_fwd_kernel<64,8,32,1,true>", M2B + "#split")
    e[("msg", 2, 0, "fwd")] = ("sa_fwd_kernel<32,8,16,1,true>", M3A + "#split")
    e[("msg", 2, 1, "fwd")] = ("sa_fwd_kernel<32,8,32,1,true>", S4 + "#split")
    e[("msg", 3, 0, "fwd")] = ("sa_fwd_kernel<32,8,16,1,true>", M4A + "#split")
    e[("msg", 3, 1, "fwd")] = ("sa_fwd_kernel<32,8,32,2,true>", M4B + "#split")
    e.update(_all_bwd("msg", 0, 0, "sa_bwd_kernel<128,4,1,16>", M1A + "#dense", ("sa_bwd_kernel<128,4,1,16>", M1A + "#dense#colour")))
    e.update(_all_bwd("msg", 0, 1, "sa_bwd_kernel<128,4,1,32>", S1 + "#dense", ("sa_bwd_kernel<128,4,1,32>", S1 + "#dense#colour")))
    e.update(_all_bwd("msg", 1, 0, "sa_bwd_kernel<64,4,2,16>", M2A + "#dense"))
    e.update(_all_bwd("msg", 1, 1, "sa_bwd_kernel<64,8,1,32>", M2B + "#dense"))
    e.update(_all_bwd("msg", 2, 0, "sa_bwd_kernel<32,8,2,16>", M3A + "#dense"))
    e.update(_all_bwd("msg", 2, 1, "sa_bwd_kernel<32,8,2,32>", S4 + "#dense"))
    e.update(_all_bwd("msg", 3, 0, "sa_bwd_kernel<32,8,3,16>", M4A + "#dense"))
    e.update(_all_bwd("msg", 3, 1, "sa_bwd_kernel<32,8,3,32>", M4B + "#dense"))
    for arch in ("ssg", "msg"):
        for l in range(4):
            e[(arch, "fp", l)] = 1 if l <= 2 else 0
    return e


def _merge(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


# the unpacked / non-key / row-ordered forms of the SSG levels, used by several settings
SSG_DENSE0 = _all_bwd("ssg", 0, 0, "sa_bwd_kernel<128,4,1,32>", S1 + "#dense", ("sa_bwd_kernel<128,4,1,32>", S1 + "#dense#colour"))
SSG_SPARSE = [_all_bwd("ssg", 1, 0, "sa_bwd_sparse_kernel<64,4,2,1>", S2 + "#sparse"),
              _all_bwd("ssg", 2, 0, "sa_bwd_sparse_kernel<32,4,2,2>", S3 + "#sparse"),
              _all_bwd("ssg", 3, 0, "sa_bwd_sparse_kernel<32,8,2,4>", S4 + "#sparse")]
SSG_PACKED_NOKEYS = [("sa_fwd_packed_kernel<128,4,false>", S1 + "#packed"), ("sa_fwd_packed_kernel<64,4,true>", S2 + "#packed"),
                     ("sa_fwd_packed_kernel<32,4,true>", S3 + "#packed"), ("sa_fwd_packed_kernel<32,8,true>", S4 + "#packed")]
SSG_WHOLE = [("sa_fwd_kernel<128,4,32,1>", S1 + "#whole"), ("sa_fwd_kernel<64,4,32,1>", S2 + "#whole"),
             ("sa_fwd_kernel<32,4,32,1>", S3 + "#whole"), ("sa_fwd_kernel<32,8,32,1>", S4 + "#whole")]
SSG_SPLIT = [("sa_fwd_kernel<128,4,32,1,true>", S1 + "#split"), ("sa_fwd_kernel<64,4,32,1,true>", S2 + "#split"),
             ("sa_fwd_kernel<32,4,32,1,true>", S3 + "#split"), ("sa_fwd_kernel<32,8,32,1,true>", S4 + "#split")]
L3_PACKED = _merge({("ssg", 3, 0, "fwd"): ("sa_fwd_packed_kernel<32,8,true,true>", S4 + "#keys#packed")},
                   _all_bwd("ssg", 3, 0, "sa_bwd_packed_kernel<32,8,1,4>", S4 + "#sa4#bwd#packed"))
ROW_ORDER = _merge(_all_bwd("ssg", 1, 0, "sa_bwd_packed_kernel<64,4,1,1>", S2 + "#sa2#bwd#packed"),
                   _all_bwd("ssg", 2, 0, "sa_bwd_packed_kernel<32,4,1,2>", S3 + "#sa3#bwd#packed"))


def _split0():
    # whole first layers everywhere.  SSG: only level 0 still fits the packed forward (without packed keys: its packed
    # backward wants level 1 split); levels 1 - 3 run the whole forward and the unpacked sparse backward.  MSG: whole kernels.
    d = _merge(SSG_DENSE0, *SSG_SPARSE)
    d[("ssg", 0, 0, "fwd")] = SSG_PACKED_NOKEYS[0]
    for l in (1, 2, 3):
        d[("ssg", l, 0, "fwd")] = SSG_WHOLE[l]
    d[("msg", 1, 0, "fwd")] = ("sa_fwd_kernel<64,4,16,1>", M2A + "#whole")
    d[("msg", 1, 1, "fwd")] = ("sa_fwd_kernel<64,8,32,1>", M2B + "#whole")
    d[("msg", 2, 0, "fwd")] = ("sa_fwd_kernel<32,8,16,1>", M3A + "#whole")
    d[("msg", 2, 1, "fwd")] = ("sa_fwd_kernel<32,8,32,1>", S4 + "#whole")
    d[("msg", 3, 0, "fwd")] = ("sa_fwd_kernel<32,8,16,1>", M4A + "#whole")
    d[("msg", 3, 1, "fwd")] = ("sa_fwd_kernel<32,8,32,2>", M4B + "#whole")
    return d


SETTINGS = {
    "default": ({}, {}),
    "split0": ({"PSG_PN2_SPLIT": "0"}, _split0()),
    # the forward of SSG level 0 split as well: it leaves the packed path, and with it the level's packed backward
    "split2": ({"PSG_PN2_SPLIT": "2"}, _merge(SSG_DENSE0, {("ssg", 0, 0, "fwd"): SSG_SPLIT[0]})),
    "fpsplit0": ({"PSG_PN2_FPSPLIT": "0"}, {(a, "fp", l): 0 for a in ("ssg", "msg") for l in range(3)}),
    "pack0": ({"PSG_PN2_PACK": "0"}, _merge(SSG_DENSE0, *SSG_SPARSE, {("ssg", 0, 0, "fwd"): SSG_WHOLE[0]},
                                            {("ssg", l, 0, "fwd"): SSG_SPLIT[l] for l in (1, 2, 3)})),
    "pack_bwd0": ({"PSG_PN2_PACK_BWD": "0"}, _merge(SSG_DENSE0, *SSG_SPARSE, {("ssg", l, 0, "fwd"): SSG_PACKED_NOKEYS[l] for l in range(4)})),
    "pack_bwd_L0": ({"PSG_PN2_PACK_BWD": "L0"}, _merge(SSG_SPARSE[0], SSG_SPARSE[1], {("ssg", l, 0, "fwd"): SSG_PACKED_NOKEYS[l] for l in (1, 2)})),
    "pack_bwd_L0123": ({"PSG_PN2_PACK_BWD": "L0123"}, L3_PACKED),
    "pack_bwd_L3": ({"PSG_PN2_PACK_BWD": "L3"}, _merge(SSG_DENSE0, SSG_SPARSE[0], SSG_SPARSE[1], L3_PACKED,
                                                        {("ssg", l, 0, "fwd"): SSG_PACKED_NOKEYS[l] for l in (0, 1, 2)})),
    "poolt_row": ({"PSG_PN2_POOLT_ORDER": "row"}, ROW_ORDER),
    "poolt_row_L0123": ({"PSG_PN2_POOLT_ORDER": "row", "PSG_PN2_PACK_BWD": "L0123"}, _merge(ROW_ORDER, L3_PACKED)),
    # no sparse stream: levels 1 - 3 no longer fit the packed backward and run the dense unpacked kernels
    "poolt_sparse0": ({"PSG_PN2_POOLT_SPARSE": "0"},
                      _merge(_all_bwd("ssg", 1, 0, "sa_bwd_kernel<64,4,2,32>", S2 + "#dense"), _all_bwd("ssg", 2, 0, "sa_bwd_kernel<32,4,2,32>", S3 + "#dense"),
                             _all_bwd("ssg", 3, 0, "sa_bwd_kernel<32,8,2,32>", S4 + "#dense"), {("ssg", l, 0, "fwd"): SSG_PACKED_NOKEYS[l] for l in (1, 2)})),
    "l1t_colour0": ({"PSG_PN2_L1T_COLOUR": "0"}, {("ssg", 0, 0, "bwd_colour"): ("sa_bwd_packed_kernel<128,4,1,0>", S1 + "#bwd#packed"),
                                                  ("msg", 0, 0, "bwd_colour"): ("sa_bwd_kernel<128,4,1,16>", M1A + "#dense"),
                                                  ("msg", 0, 1, "bwd_colour"): ("sa_bwd_kernel<128,4,1,32>", S1 + "#dense")}),
    "fp1_wave": ({"PSG_FP1_WAVE": "1"}, {("ssg", "fp", 0): 0, ("msg", "fp", 0): 0}),
}

NEEDS_FWD = "the packed backward (PSG_PN2_PACK_BWD) needs the packed forward, which this configuration does not run"
NO_BWD = "PSG_PN2_PACK_BWD names a level without a packed backward kernel in this configuration"
# A level named explicitly that does not fit is an error at its launch, not a fall-back.  From the parent's code:
ERRORS = {
    # level 1 whole: run_sa_fwd's packed branch wants split == (lvl >= 1); the masks cannot be keyed by packed workgroup
    "L1_split0": ({"PSG_PN2_PACK_BWD": "L1", "PSG_PN2_SPLIT": "0"}, ("ssg", 1, 0), "fwd", NEEDS_FWD),
    # level 0 packs its forward, but with level 1 whole its pooled-output gradient comes through ginv lists: no dense0 kernel
    "L0_split0": ({"PSG_PN2_PACK_BWD": "L0", "PSG_PN2_SPLIT": "0"}, ("ssg", 0, 0), "bwd", NO_BWD),
    # level 1 split and packed forward, but without the sparse stream (spv = 0) neither packed backward form fits
    "L1_poolt_sparse0": ({"PSG_PN2_PACK_BWD": "L1", "PSG_PN2_POOLT_SPARSE": "0"}, ("ssg", 1, 0), "bwd", NO_BWD),
}

SWITCHES = ["PSG_PN2_SPLIT", "PSG_PN2_FPSPLIT", "PSG_FP1_WAVE", "PSG_PN2_PACK", "PSG_PN2_PACK_BWD", "PSG_PN2_POOLT_ORDER",
            "PSG_PN2_POOLT_SPARSE", "PSG_PN2_L1T_COLOUR", "PSG_PN2_PW_SIZED", "PSG_PN2_BALL_TABLE", "PSG_PN2_FP1_LOOP",
            "PSG_PN2_PGD_FUSE", "PSG_PN2_GRAPH", "PSG_DIAG"]


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no C++ compiler on this machine"
    tmp = tmp_path_factory.mktemp("pn2_paths")
    src = str(tmp / "main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    exes = []
    for name, flags in (("paths", ["-O2"]), ("paths_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp / name)
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-I", CSRC, src, "-o", exe] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        exes.append(exe)
    return exes


def _run(exe, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = {}
    for line in r.stdout.strip().split("\n"):
        w = line.split(" ", 4)
        if w[1].startswith("fp"):
            got[(w[0], "fp", int(w[1][2:]))] = int(w[2].split("=")[1])
        elif w[4].startswith("error "):
            got[(w[0], int(w[1][1:]), int(w[2][1:]), w[3])] = ("error", w[4][6:])
        else:
            got[(w[0], int(w[1][1:]), int(w[2][1:]), w[3])] = tuple(w[4].split(" "))
    return got


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_every_launch_matches_the_hand_derived_table(programs, setting):
    env, changes = SETTINGS[setting]
    want = _merge(_default(), changes)
    assert len(want) == 16 + 24 + 8
    for exe in programs:      # the plain build and the address + undefined-behaviour sanitizer build
        got = _run(exe, env)
        assert sorted(got, key=str) == sorted(want, key=str)
        wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
        assert not wrong, wrong


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_a_named_level_that_does_not_fit_is_an_error(programs, case):
    env, (arch, l, s), direction, message = ERRORS[case]
    for exe in programs:
        got = _run(exe, env)
        hits = {k: v for k, v in got.items() if isinstance(v, tuple) and v[0] == "error"}
        want_keys = {(arch, l, s, d) for d in (("fwd",) if direction == "fwd" else ("bwd", "bwd_colour", "bwd_full"))}
        assert set(hits) >= want_keys and all(hits[k] == ("error", message) for k in want_keys), hits
        assert all(k[0] == "ssg" and k[1] == l for k in hits), hits      # (MSG has no packed rows: nothing named, nothing fails)


def test_sites_keep_the_suffixes_the_gpu_tests_key_on():
    """#packed / #bwd#packed / #colour / #saN / #chan#saN stay where they were; the row tag introduces none of them"""
    for kern, site in (v for v in _default().values() if isinstance(v, tuple)):
        tag = site.split("#")[1]
        assert not any(t in tag for t in ("packed", "colour", "chan", "sa", "nw", "bwd")), site
        assert site.endswith("#packed") == ("packed_kernel" in kern), (kern, site)
