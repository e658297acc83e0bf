"""Host tests of the one window loop of the lockstep NU attacks (pointsecguard_amd/attacks/nu_windows.py) and of the RandLA-Net
family's `attack._run_windows` in the forms its field callers use: the schedule against the literal list, the mask coercion
and its refusals, and the driver on CPU tensors against a per-step transcription of the reference's control flow."""
import numpy as np
import pytest
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.attacks import nu_windows as nw
from pointsecguard_amd.randla import attack


def test_window_end_is_the_literal_schedule():
    windows = [[0]] + [list(range(a, a + 10)) for a in range(1, 62, 10)]          # [0], [1..10], [11..20], .., [61..70]
    for step in range(62):
        w = next(w for w in windows if step in w)
        assert nw.window_end(step) == w[-1] + 1, step
    assert [nw.window_end(s, 3) for s in range(8)] == [1, 4, 4, 4, 7, 7, 7, 10]


def test_room_masks_coerces_tensors_and_arrays_alike_and_refuses_like_the_loops_did():
    m = np.zeros((3, 8), bool)
    m[0, :2], m[1, 5], m[2, ::2] = True, True, True
    for given in (m, m.astype(np.uint8), torch.from_numpy(m), torch.from_numpy(m.astype(np.float32)), m.tolist()):
        mk, n_mask = nw.room_masks(given, 3, 8, True, "target.py:104")
        assert mk.dtype == bool and np.array_equal(mk, m)
        assert n_mask.dtype == np.float64 and n_mask.tolist() == [2.0, 1.0, 4.0]
    mk, n_mask = nw.room_masks(None, 3, 8, False, "x")
    assert mk is None and n_mask.dtype == np.float64 and n_mask.tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="the targeted variant needs one mask per room"):
        nw.room_masks(None, 3, 8, True, "target.py:104")
    with pytest.raises(ValueError, match=r"masks must be boolean \[3, 8\], got shape \(2, 8\)"):
        nw.room_masks(m[:2], 3, 8, True, "target.py:104")
    m[1] = False
    with pytest.raises(ZeroDivisionError, match=r"tar_NU_attack: rooms \[1\] have an empty mask \(tcolper.py:109: division by the mask count\)"):
        nw.room_masks(torch.from_numpy(m), 3, 8, True, "tcolper.py:109")
    assert nw.room_masks(m, 3, 8, False, "x")[1].tolist() == [2.0, 0.0, 4.0]       # (only the targeted variant divides by the count)


# ------------------------------------------------------------------------------------------------ the driver
G, N, LR0 = 3, 4, 0.01


class State:
    """what the driver touches of a lockstep state, on the CPU"""

    def __init__(self):
        self.hist = torch.zeros(nw.CHUNK, 5, G)
        self.exit = torch.full((G,), -1, dtype=torch.int32)
        self.x0 = torch.zeros(G, N, 9)
        self.out = torch.zeros(G, 9, N)


class Attack:
    def __init__(self, steps):
        self.steps, self.lr = steps, LR0


class Moment:
    def __init__(self, log):
        self.log = log

    def zero_(self):
        self.log.append("zeroed")


def costs_of(cap):
    """room 1's cost rises (it asks for a restart after every 10th step past the 10th), the others' fall"""
    s = np.arange(cap, dtype=np.float64)[:, None]
    return np.where(np.arange(G)[None] == 1, s, 100.0 - s)


def reference(cap, exits, costs):
    """The reference's loop (target.py:92-133), room by room, step by step: -> per room the (Adam index, lr) of every step it
    ran, the steps after which it halved, the steps after which it restarted, its step count, whether it ran to the cap."""
    rooms = []
    for g in range(G):
        lr, adam_t, ran, halved, restarted, prev = LR0, 0, [], [], [], {}
        for step in range(cap):
            adam_t += 1
            ran.append((adam_t, lr))
            prev[step] = costs[step, g]
            if exits[g] == step:
                break
            if step > 0 and step % 50 == 0:
                lr, adam_t = lr / 2, 0
                halved.append(step)
            if step > 10 and step % 10 == 0 and costs[step, g] >= prev[step - 10]:
                restarted.append(step)
        rooms.append(dict(ran=ran, halved=halved, restarted=restarted, steps=len(ran), cap=exits[g] < 0))
    return rooms


def drive(monkeypatch, cap, exits, one_step=False, restore_lr=True):
    S, atk, costs = State(), Attack(cap), costs_of(cap)
    windows, halvings, restarts, tails, log = [], [], [], [], []

    def fake_call(name, src, rows, nine, n, dst, stream):
        assert (name, rows, nine, n) == ("psg_to_channel_major", 1, 9, N)
        tails.append((src.value - S.x0.data_ptr()) // (4 * N * 9))

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(runtime, "stream", lambda: None)

    def enqueue(step, n_run, adam_t):
        windows.append((step, n_run, adam_t, atk.lr))
        if "zeroed" in log:                              # the moments were zeroed since the last window: a halving
            halvings.append(step - 1)
            assert log == ["zeroed", "zeroed"]
            del log[:]
        S.hist.zero_()
        S.hist[:n_run, 2] = torch.from_numpy(costs[step:step + n_run]).float()
        for g, e in enumerate(exits):
            if step <= e < step + n_run:
                S.exit[g] = e

    seen = []

    def on_step(s_i, row, was_active, exited):
        assert row.shape == (5, G) and row.dtype == np.float64 and np.array_equal(row[2], costs[s_i])
        seen.append((s_i, was_active.tolist()))
        on_step.cost, on_step.prev[s_i] = row[2], np.where(was_active, row[2], on_step.prev[s_i])
    on_step.prev = np.full((cap, G), 1e10)

    def between(last, step, active):
        assert step == last + 1
        again = nw.to_restart(last, active, on_step.cost, on_step.prev)
        if len(again):
            restarts.append((last, again.tolist()))

    out, steps_run, step = nw.window_loop(atk, S, 1, enqueue, targeted_variant=True, on_step=on_step, between=between,
                                          one_step=one_step, moments=(Moment(log), Moment(log)), restore_lr=restore_lr)
    assert out is not S.out and tuple(out.shape) == (G, 9, N)
    return dict(windows=windows, halvings=halvings, restarts=restarts, tails=tails, steps_run=steps_run.tolist(), step=step, seen=seen,
                lr=atk.lr)


FULL = [(0, 1)] + [(a, 10) for a in (1, 11, 21, 31, 41, 51)]          # the windows of 61 steps: [0], [1..10], .., [51..60]
CASES = [
    # cap, exits per room (-1: none), one-step windows, the literal windows (first step, steps)
    (1, [-1, -1, -1], False, [(0, 1)]),
    (11, [-1, -1, -1], False, [(0, 1), (1, 10)]),
    (12, [-1, -1, -1], False, [(0, 1), (1, 10), (11, 1)]),
    (61, [-1, -1, -1], False, FULL),
    (61, [0, -1, -1], False, FULL),
    (61, [-1, 17, -1], False, FULL),
    (61, [13, 17, 15], False, FULL[:3]),                               # all leave in [11..20]: nothing is enqueued after it
    (12, [-1, -1, -1], True, [(s, 1) for s in range(12)]),
]


@pytest.mark.parametrize("cap,exits,one_step,want_windows", CASES)
def test_the_driver_runs_the_reference_control_flow(monkeypatch, cap, exits, one_step, want_windows):
    got = drive(monkeypatch, cap, exits, one_step)
    ref = reference(cap, exits, costs_of(cap))
    assert [(w[0], w[1]) for w in got["windows"]] == want_windows
    # every step a room ran had the Adam index and the learning rate the reference gives it
    for step0, n_run, adam_t0, lr in got["windows"]:
        for s in range(step0, step0 + n_run):
            for g in range(G):
                if s < ref[g]["steps"]:
                    assert ref[g]["ran"][s] == (adam_t0 + (s - step0) + 1, lr), (s, g)
    running = [max(r["steps"] for r in ref) > s + 1 for s in range(cap)]          # a room runs on after step s
    assert got["halvings"] == [s for s in (50,) if s < cap and running[s]] == sorted(set(sum((r["halved"] for r in ref), [])) & {
        s for s in range(cap) if running[s]})
    want_restarts = {}
    for g, r in enumerate(ref):
        for s in r["restarted"]:
            want_restarts.setdefault(s, []).append(g)
    assert got["restarts"] == sorted(want_restarts.items())
    if cap == 61 and exits[1] < 0:
        assert got["restarts"] == [(s, [1]) for s in (20, 30, 40, 50, 60)]        # the literal: the rising room, every 10th step
    assert got["steps_run"] == [r["steps"] for r in ref]
    assert got["tails"] == [g for g, r in enumerate(ref) if r["cap"]]             # the cap tail: the rooms still running
    assert got["step"] == sum(n for _, n in want_windows)
    # was_active: a room is still in its loop at its exit step, not after it
    for s_i, was_active in got["seen"]:
        assert was_active == [s_i < r["steps"] for r in ref], s_i
    assert got["lr"] == LR0                                                       # put back, whatever was halved


def test_the_batch_form_keeps_the_halved_rate_and_a_failing_window_still_restores(monkeypatch):
    assert drive(monkeypatch, 61, [-1, -1, -1], restore_lr=False)["lr"] == LR0 / 2           # target.py:123-125 leaves it halved
    atk, S = Attack(61), State()
    monkeypatch.setattr(runtime, "stream", lambda: None)

    def enqueue(step, n_run, adam_t):
        if step == 51:
            raise RuntimeError("window failed")

    with pytest.raises(RuntimeError, match="window failed"):
        nw.window_loop(atk, S, 1, enqueue, targeted_variant=True, moments=())
    assert atk.lr == LR0


def test_the_untargeted_variant_neither_halves_nor_restarts(monkeypatch):
    S, atk, calls = State(), Attack(61), []
    monkeypatch.setattr(_lib, "call", lambda *a: None)
    monkeypatch.setattr(runtime, "stream", lambda: None)
    nw.window_loop(atk, S, 1, lambda step, n_run, adam_t: calls.append((step, n_run, adam_t, atk.lr)), targeted_variant=False,
                   between=lambda *a: pytest.fail("no restarts"), moments=(Moment([]),))
    assert calls[-1] == (51, 10, 51, LR0)


def test_a_limit_cuts_the_window_and_is_asked_before_it(monkeypatch):
    S, atk, calls = State(), Attack(30), []
    monkeypatch.setattr(_lib, "call", lambda *a: None)
    monkeypatch.setattr(runtime, "stream", lambda: None)
    nw.window_loop(atk, S, 1, lambda step, n_run, adam_t: calls.append((step, n_run)), targeted_variant=False,
                   limit=lambda step: min(step + 4, 30) if step >= 11 else 30)
    assert calls[:5] == [(0, 1), (1, 10), (11, 4), (15, 4), (19, 2)]


# ------------------------------------------------------------------------------------ attack._run_windows, field forms
class CloudsState:
    def __init__(self, cols, graphs):
        self.hist = torch.zeros(attack.CHUNK + 1, 2, cols)
        self.exit = torch.full((2,), -1, dtype=torch.int32)
        if graphs:
            self.graph, self.graph_tail = "graph", "graph_tail"


def run_windows(monkeypatch, S, cap, chunk, exits=None, **kw):
    calls, hooks = [], []
    win = _lib.RlaNuFieldWindowArgs()

    def fake_call(*args):
        calls.append(args[:1] + (win.n_steps, win.adam_t0, win.tail_eval) + args[2:])
        S.hist[:] = len(calls)
        if exits and len(calls) in exits:
            S.exit.copy_(torch.tensor(exits[len(calls)], dtype=torch.int32))

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(runtime, "stream", lambda: "stream")

    def set_window(t0, n_run, tail):
        win.n_steps, win.adam_t0, win.tail_eval = n_run, t0, 1 if tail else 0
        return n_run + (1 if tail else 0)

    rows, steps = attack._run_windows("entry", win, S, 1, cap, chunk, set_window,
                                      lambda *a: hooks.append((a[0], a[1], a[2], a[4].shape, float(a[4].min()))), **kw)
    return calls, hooks, rows, steps.tolist()


def test_run_windows_takes_the_column_count_from_the_state_and_passes_no_graph_where_there_is_none(monkeypatch):
    calls, hooks, rows, steps = run_windows(monkeypatch, CloudsState(4, graphs=False), 13, 10, exits={2: [12, -1]})
    assert calls == [("entry", 10, 1, 0, "stream"), ("entry", 3, 11, 1, "stream")]          # (entry, block, stream): no handle
    assert hooks == [(1, 10, False, (10, 2, 4), 1.0), (11, 3, True, (4, 2, 4), 2.0)]
    assert rows == [10, 4] and steps == [12, 13]
    calls, _, _, _ = run_windows(monkeypatch, CloudsState(4, graphs=True), 20, 10)
    assert [c[4:] for c in calls] == [("graph", "stream"), ("graph_tail", "stream")]


def test_run_windows_without_read_back_runs_to_the_cap_and_calls_no_hook(monkeypatch):
    S = CloudsState(3, graphs=False)
    monkeypatch.setattr(torch, "cat", lambda *a, **k: pytest.fail("nothing returns to the host"))
    calls, hooks, rows, steps = run_windows(monkeypatch, S, 7, 3, exits={1: [2, 2]}, read_back=False)
    assert [c[1:4] for c in calls] == [(3, 1, 0), (3, 4, 0), (1, 7, 1)] and hooks == [] and rows == [3, 3, 2]
    assert steps == [7, 7]                               # the exit steps are not read: every cloud takes every step
