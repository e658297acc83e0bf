"""The channel-ordered max-pool transpose of the packed SA backward of PointNet++ SSG levels 1 - 3 (psg_pn2_kernels.cuh:
sa_bwd_packed_chan, levels 1 and 2) against the batches of row-ordered item lists it replaces (sa_bwd_packed_sparse, PSG_PN2_POOLT_ORDER=row).
Per (row, column) both run the same fmaf chain from 0 over the row's items in ascending channel order, so every gradient
must agree BYTE for byte - no tolerance is involved.  The switches are read once per process: each setting runs in a fresh child
interpreter (the child of tests/test_gpu_sa_pack_bwd_levels.py, with PSG_TRACE_SYNC=1), all three levels packed
(PSG_PN2_PACK_BWD=L0123).

Rooms: the eight kinds of tests/sa_pack_bwd_levels_rooms.py at its size (B = 2, N = 4096, ITERS = 3, the smallest the network's
level sizes allow).  That their packed workgroups hold the shapes that can go wrong - one group, the cap of 16 groups with
one-row groups, P - 1 rows, an unaligned workgroup of full groups, groups across a 32-row block - and how the groups are dealt
to the waves, and that valid rows exist that win no channel (rows without an item: stored as zeros), is stated on the CPU by
tests/test_sa_poolt_order_host.py.

Checked: the colour-only gradient, psg_pn2_backward, psg_pn2_backward_full and a 3-iteration NB attack of the channel-ordered
child are byte-equal to the row-ordered child's, and to a second channel-ordered run's; the channel-ordered children launch
levels 1 and 2 (the levels the channel-ordered kernel exists for; level 3 runs the batches in every child) at sites tagged
#chan and the row-ordered child launches none of those."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILDREN = (("chan", {}), ("chan2", {}), ("row", {"PSG_PN2_POOLT_ORDER": "row"}))
SWITCHES = ("PSG_PN2_PACK", "PSG_PN2_PACK_BWD", "PSG_PN2_POOLT_ORDER", "PSG_PN2_POOLT_SPARSE")


def _child(tmp_path, tag, switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    env["PSG_PN2_PACK_BWD"] = "L0123"
    env["PSG_TRACE_SYNC"] = "1"
    out = str(tmp_path / ("%s.npz" % tag))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    sites = set(re.findall(r"\[psg trace\] launch \d+ at (\S+) issued", r.stderr + r.stdout))
    return dict(np.load(out)), sites


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sa_poolt_order")
    return {tag: _child(tmp, tag, switches) for tag, switches in CHILDREN}


@pytest.mark.gpu
def test_channel_order_and_row_order_byte_equal(runs):
    import sa_pack_bwd_levels_rooms as lr
    ref = runs["row"][0]
    assert len(ref) == 5 * len(lr.ROOM_KINDS) + 1
    for tag in ("chan", "chan2"):
        other = runs[tag][0]
        assert sorted(other) == sorted(ref)
        for k in sorted(ref):
            assert ref[k].tobytes() == other[k].tobytes(), "%s: PSG_PN2_POOLT_ORDER=row and %s differ" % (k, tag)
    for kind in lr.ROOM_KINDS:
        assert np.abs(ref[kind + "_dcolour"]).max() > 0 and np.abs(ref[kind + "_dx0_full"][..., 0:3]).max() > 0, kind
        assert not np.array_equal(ref[kind + "_adv"], 0 * ref[kind + "_adv"]), kind


@pytest.mark.gpu
def test_the_switch_selects_the_launch_sites(runs):
    def chan_levels(sites):
        return {int(m.group(1)) - 1 for s in sites for m in [re.search(r"#chan#sa([234])#bwd#packed$", s)] if m}

    def packed_levels(sites):
        return {int(m.group(1)) - 1 for s in sites for m in [re.search(r"#sa([234])#bwd#packed$", s)] if m}

    for tag in ("chan", "chan2"):
        assert chan_levels(runs[tag][1]) == {1, 2}, sorted(runs[tag][1])
    assert chan_levels(runs["row"][1]) == set(), sorted(runs["row"][1])
    assert packed_levels(runs["row"][1]) == {1, 2, 3}, sorted(runs["row"][1])


if __name__ == "__main__":
    import test_gpu_sa_pack_bwd_levels as base
    base._child_main(sys.argv[1])
