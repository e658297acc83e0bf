"""Host tests of the helpers every RandLA-Net attack class shares (pointsecguard_amd/randla/attack.py): the window loop of the
lockstep attacks against a scripted library call, and the two metric tuples against the expressions of the one-cloud loops."""
import numpy as np
import pytest
import torch

from pointsecguard_amd import _lib, runtime
from pointsecguard_amd.randla import attack

G = 2


class State:
    """what the window loop touches of a lockstep state"""

    def __init__(self):
        self.hist = torch.zeros(attack.CHUNK + 1, G, 3)
        self.exit = torch.full((G,), -1, dtype=torch.int32)
        self.graph, self.graph_tail = "graph", "graph_tail"


def run(monkeypatch, kind, cap, chunk, exits=None):
    """The loop as NUattack (steps 1 .. cap, a tail row in the last window) or TBIM (iterations 0 .. cap) drives it, with the
    library call recorded; exits: {call number: exit steps [G]} written by that call.  -> (calls, hooks, rows, steps)"""
    S, calls, hooks = State(), [], []
    win = _lib.RlaNuWindowArgs() if kind == "nu" else _lib.RlaTbimWindowArgs()

    def fake_call(entry, block, graph, stream):
        fields = (win.n_steps, win.adam_t0, win.tail_eval) if kind == "nu" else (win.n_steps, win.it0, win.final)
        calls.append((entry,) + fields + (graph,))
        S.hist[:] = len(calls)
        if exits and len(calls) in exits:
            S.exit.copy_(torch.tensor(exits[len(calls)], dtype=torch.int32))

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(runtime, "stream", lambda: None)

    def set_nu(t0, n_run, tail):
        win.n_steps, win.adam_t0, win.tail_eval = n_run, t0, 1 if tail else 0
        return n_run + (1 if tail else 0)

    def set_tbim(it0, n_run, final):
        win.n_steps, win.it0, win.final = n_run, it0, 1 if final else 0
        return n_run

    def hook(first, n_run, last, state, rows):
        hooks.append((first, n_run, last, state is S, rows.shape, float(rows.min())))

    entry, first, setter = ("psg_rla_nu_window", 1, set_nu) if kind == "nu" else ("psg_rla_tbim_window", 0, set_tbim)
    rows, steps = attack._run_windows(entry, win, S, first, cap, chunk, setter, hook)
    return calls, hooks, rows, steps


def test_windows_are_cut_at_the_cap_and_only_the_last_is_flagged(monkeypatch):
    calls, hooks, rows, steps = run(monkeypatch, "nu", 23, 10)
    assert calls == [("psg_rla_nu_window", 10, 1, 0, "graph"), ("psg_rla_nu_window", 10, 11, 0, "graph"),
                     ("psg_rla_nu_window", 3, 21, 1, None)]
    assert rows == [10, 10, 4]                                  # the tail evaluation is one more history row
    assert hooks == [(1, 10, False, True, (10, G, 3), 1.0), (11, 10, False, True, (10, G, 3), 2.0), (21, 3, True, True, (4, G, 3), 3.0)]
    assert steps.tolist() == [23, 23]                           # no exit: the cap, NU's steps count from 1
    calls, _, rows, steps = run(monkeypatch, "tbim", 22, 10)
    assert calls == [("psg_rla_tbim_window", 10, 0, 0, "graph"), ("psg_rla_tbim_window", 10, 10, 0, "graph"),
                     ("psg_rla_tbim_window", 3, 20, 1, None)]
    assert rows == [10, 10, 3] and steps.tolist() == [23, 23]   # iterations 0 .. 22 are 23 gradient steps


def test_only_full_windows_get_a_graph_and_a_full_last_one_the_tail_graph(monkeypatch):
    calls, _, rows, _ = run(monkeypatch, "nu", 20, 10)
    assert [c[1:] for c in calls] == [(10, 1, 0, "graph"), (10, 11, 1, "graph_tail")] and rows == [10, 11]
    calls, _, _, _ = run(monkeypatch, "tbim", 19, 10)
    assert [c[1:] for c in calls] == [(10, 0, 0, "graph"), (10, 10, 1, "graph_tail")]
    calls, _, _, _ = run(monkeypatch, "nu", 9, 4)                # shortened windows run eagerly
    assert [c[1:] for c in calls] == [(4, 1, 0, None), (4, 5, 0, None), (1, 9, 1, None)]
    calls, _, _, _ = run(monkeypatch, "nu", 12, 99)              # at most CHUNK steps per window
    assert [c[1:] for c in calls] == [(10, 1, 0, "graph"), (2, 11, 1, None)]
    calls, _, _, _ = run(monkeypatch, "tbim", 3, 0)              # and at least one
    assert [c[1:4] for c in calls] == [(1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 1)]


@pytest.mark.parametrize("kind,plus", [("nu", 0), ("tbim", 1)])
def test_the_loop_stops_after_the_window_in_which_the_last_cloud_exits(monkeypatch, kind, plus):
    calls, hooks, _, steps = run(monkeypatch, kind, 40, 10, exits={1: [3, -1], 2: [3, 17]})
    assert len(calls) == 2 and len(hooks) == 2 and not hooks[-1][2]
    assert steps.tolist() == [3 + plus, 17 + plus]              # last_steps: TBIM's iteration index + 1, NU's step index
    calls, _, _, steps = run(monkeypatch, kind, 40, 10, exits={1: [3, -1]})
    assert len(calls) == (4 if kind == "nu" else 5)             # one cloud never exits: to the cap (1 .. 40, or 0 .. 40)
    assert steps.tolist() == [3 + plus, 40 + plus]


def hand_cloud():
    """12 points, classes 0 .. 3; class 2 is the origin (4 points), 5 the target"""
    lab = np.array([0, 1, 2, 2, 3, 1, 2, 0, 2, 3, 1, 0], np.int64)
    pred0 = np.array([0, 1, 2, 1, 3, 1, 2, 0, 0, 3, 3, 0], np.int64)
    pred = np.array([0, 5, 5, 5, 3, 2, 5, 1, 2, 3, 1, 0], np.int64)
    rpred = np.array([0, 1, 2, 2, 0, 1, 1, 0, 2, 3, 1, 3], np.int64)
    return lab, pred0, pred, rpred


class Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


def test_targeted_tuple_equals_the_one_cloud_expressions():
    lab, pred0, pred, _ = hand_cloud()
    n, ori, target, new_dists = 12, 2, 5, 0.375
    # TBIM.batch_attack's expressions
    mask_h = lab == ori
    target_points = float(mask_h.sum())
    ys_target = np.where(mask_h, target, lab).astype(np.int32)
    original_other_accuracy = float(np.sum(pred0[~mask_h] == lab[~mask_h]) / (n - target_points))
    original_other_miou = attack._mean_iou(pred0[~mask_h], lab[~mask_h])
    sr = float(np.sum(pred[mask_h] == ys_target[mask_h]) / target_points)
    other_acc = float(np.sum(pred[~mask_h] == ys_target[~mask_h]) / (n - target_points))
    other_miou = attack._mean_iou(pred[~mask_h], lab[~mask_h])
    want = (target_points, sr, other_acc, original_other_accuracy, new_dists, other_miou, original_other_miou)
    log = Log()
    out = attack._targeted_out(log, pred, pred0, lab, ys_target, mask_h, new_dists)
    assert out == want and all(type(q) is float for q in out)
    assert out[:4] == (4.0, 0.75, 0.625, 0.875)
    assert log.lines == ["points={}, sr={},  other_acc={}, original_other_accuracy={}, new_dists={}, other_mIoU={}, "
                         "original_other_mIoU={}".format(*want)]
    assert attack._targeted_out(None, pred, pred0, lab, ys_target, mask_h, new_dists) == want


def test_untargeted_tuple_equals_the_one_cloud_expressions():
    lab, pred0, pred, rpred = hand_cloud()
    n, dist = 12, 1.25
    # NUattack.batch_attack's expressions
    acc, miou = float(np.sum(pred == lab) / n), attack._mean_iou(pred, lab)
    original_accuracy, original_miou = float(np.sum(pred0 == lab) / n), attack._mean_iou(pred0, lab)
    want = (acc, original_accuracy, dist, miou, original_miou, float(np.sum(rpred == lab) / n), attack._mean_iou(rpred, lab))
    log = Log()
    out = attack._untargeted_out(log, pred, pred0, rpred, lab, dist)
    assert out == want and all(type(q) is float for q in out)
    assert (out[0], out[1], out[5]) == (6 / 12, 9 / 12, 9 / 12)          # by hand: points 0, 4, 8, 9, 10, 11 of pred are right
    assert log.lines == ["acc={}, original_acc={}, new_dists={}, mIoU={}, original_mIoU={}, rand_acc={}, rand_mIoU={}".format(*want)]


def test_settings_and_the_origin_class_check():
    class A:
        pass
    a = A()
    attack._config(a, {"magnitude": np.array([0.5]), "alpha": 2, "iteration": "7", "cs": [3.0], "logger": "L", "other": 1},
                   "magnitude", "alpha", "iteration", "logger")
    assert (a.eps, a.alpha, a.iteration, a.logger) == (0.5, 2.0, 7, "L") and type(a.alpha) is float and not hasattr(a, "cs")
    lab = np.array([[2, 1], [1, 1], [0, 3]])
    with pytest.raises(ValueError, match=r"cloud\(s\) 1, 2 \(tester_S3DIS.py:311-314"):
        attack._origin_points(lab, 2, "311-314")
    with pytest.raises(ValueError, match="in this cloud"):
        attack._origin_points(lab[1], 2, "253-256")
    assert attack._origin_points(lab[:2], 1, "x").tolist() == [[False, True], [True, True]]
