"""The device-side-window loop of the lockstep NU attacks, once, for the four host loops that run it:
PointNet++ / PointNet colours (torchattacks/attacks/nu.py), the PointNet++ coordinate field (nu_field.py there), ResGCN colours
and the ResGCN coordinate field (resgcn/.../attacks/nu.py, nu_field.py).

G one-room attacks (or one batch of `rows` rows) advance together.  The optimiser steps are enqueued window by window - [0],
[1..10], [11..20], .. - and after every window ONE read-back brings its history rows and the exit steps to the host, where the
reference's control flow sits: an attack whose accuracy test fired at step s keeps its step-s image (the device latch holds
the snapshot; what the window ran past s is discarded), the targeted variant halves its learning rate(s) with a fresh
optimiser after every 50th step and may restart between windows.  What differs between the networks comes in as callables
(`window_loop`); the schedule, the read-back, the exit rule, the halving, the cap tail and the step count are here.
"""
import ctypes

import numpy as np
import torch

from pointsecguard_amd import _lib, runtime

CHUNK = 10  # control-flow window: restarts and lr halvings can only follow steps that are multiples of 10


def window_end(step, chunk=CHUNK):
    """The step after the window that `step` lies in: the windows are [0], [1..chunk], [chunk+1..2 chunk], .."""
    return 1 if step == 0 else ((step - 1) // chunk + 1) * chunk + 1


def room_masks(masks, R, N, targeted_variant, cite):
    """masks (tensor or array, [R, N], or None for the non-targeted variant) -> (bool numpy [R, N] or None, mask counts
    float64 [R]).  `cite`: the reference line that divides the hits by the mask count - an empty mask raises there too."""
    if masks is None:
        if targeted_variant:
            raise ValueError("the targeted variant needs one mask per room")
        return None, np.zeros(R)
    mk = masks.detach().to(torch.bool).cpu().numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks).astype(bool)
    if mk.shape != (R, N):
        raise ValueError("masks must be boolean [%d, %d], got shape %s" % (R, N, mk.shape))
    n_mask = mk.sum(axis=1).astype(np.float64)
    if targeted_variant and (n_mask == 0).any():
        raise ZeroDivisionError("tar_NU_attack: rooms %s have an empty mask (%s: division by the mask count)"
                                % (np.nonzero(n_mask == 0)[0].tolist(), cite))
    return mk, n_mask


def _bind(win, S, fields):
    """pointers of the state's tensors into the argument block: `fields` = block field names, `field=attribute` where the
    state calls the tensor otherwise"""
    for item in fields.split():
        field, _, attr = item.partition("=")
        setattr(win, field, getattr(S, attr or field).data_ptr())


def new_graphs(n):
    """n psg_nu_graph handles (one remembers ONE window shape: eager, captured, then replayed)"""
    graphs = [ctypes.c_void_p() for _ in range(n)]
    for g in graphs:
        _lib.call("psg_nu_graph_create", ctypes.byref(g))
    return graphs


def destroy_graphs(graphs):
    """for a __del__: never raises"""
    try:
        for g in graphs:
            if g:
                _lib.load().psg_nu_graph_destroy(g)
    except Exception:
        pass


class RoomsState:
    """Device buffers of one lockstep shape (G attacks of `rows` batch rows, N points, `neighbour` Smooth neighbours), kept with
    the model instance between calls: the addresses stay the same, so a 10-step window captured as a hipGraph by one call is
    replayed by the next (one model instance serves one host thread / stream at a time, like its network workspace).  These
    are the buffers every loop has - `scal` [n_scal, G] the step's sums (f, Smooth, L2, then the coordinate field's two), `hist`
    one window of history rows [n_correct, n_hits, scal..] - and the graph handles; the subclasses add what is theirs."""

    def __init__(self, dev, G, rows, N, neighbour, n_scal=3, n_graphs=1):
        B = G * rows
        f32 = self._f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)        # noqa: E731
        i32 = self._i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)          # noqa: E731
        self.x0, self.ori = f32(B, N, 9), f32(B, N, 3)
        self.w, self.m, self.v = f32(B, N, 3), f32(B, N, 3), f32(B, N, 3)
        self.dx0, self.sgrad = f32(B, N, 9), f32(G, N, 3)
        self.pred, self.labels = i32(B, N), i32(B, N)
        self.mask = torch.empty(G, N, device=dev, dtype=torch.uint8)
        self.scal = f32(n_scal, G)
        self.nn_state = i32(G, N, int(neighbour))                    # Smooth term: last step's neighbours
        self.hist = f32(CHUNK, n_scal + 2, G)
        self.active = torch.empty(G, device=dev, dtype=torch.uint8)
        self.exit, self.n_mask = i32(G), i32(G)
        self.out = f32(B, 9, N)
        self.graphs = new_graphs(n_graphs)
        self.graph = self.graphs[0] if n_graphs else None

    def __del__(self):
        destroy_graphs(getattr(self, "graphs", ()))

    @classmethod
    def of(cls, net, attr, key, *args):
        """the state of `key` in the model instance's cache `attr`, built on first use as cls(*args)"""
        cache = net.__dict__.setdefault(attr, {})
        if key not in cache:
            cache[key] = cls(*args)
        return cache[key]


def to_restart(last, active, cost, prev_cost):
    """target.py:127-132 / tcolper.py:129-132: after every 10th step past the 10th, the running attacks whose cost has not
    fallen below that of ten steps earlier"""
    if last <= 10 or last % 10:
        return np.empty(0, np.int64)
    return np.nonzero(active & (cost >= prev_cost[last - 10]))[0]


def window_loop(atk, S, rows, enqueue, *, targeted_variant, on_step=None, between=None, limit=None, one_step=False,
                lr_names=("lr",), moments=(), restore_lr=True):
    """Runs the attack's `atk.steps` steps on the state S in windows.  -> (out [G * rows, 9, N]: per attack the image of its
    exit step, or the current one where it ran to the cap; steps_run [G] int64: the optimiser steps the reference's loop ran
    per attack; the number of steps enqueued).

    enqueue(step, n_run, adam_t)     enqueues steps step .. step + n_run - 1 (Adam index adam_t + 1 ..) with the learning
                                     rates `atk` holds; they write S.hist[:n_run], S.exit and the latch's S.out
    limit(step) -> int               a window starting at `step` ends before this step (default atk.steps); called before
                                     the window is cut, so a caller that plans ahead (PointNet++ geometry) plans here
    on_step(s_i, row, was_active, exited)   per step of a window after its read-back: row [cols, G] float64, was_active [G] =
                                     the attacks whose loop was still running at s_i, exited [G] = the exit steps read back
                                     with this window (-1: running)
    between(last, step, active)      targeted variant, after a window ending with step `last` while an attack is `active`,
                                     after the halving: restarts
    one_step                         windows of one step (the callers' `trace`, which reads every step back)
    lr_names, moments                the attributes of `atk` halved after every 50th step (None: left) and the optimiser
                                     moments zeroed with them; restore_lr puts the attributes back on every way out -
                                     every lockstep call starts from the object's rates, like a fresh object per room."""
    G, cols, N = S.exit.shape[0], S.hist.shape[1], S.x0.shape[1]
    at_call = [getattr(atk, n) for n in lr_names]
    exited = np.full(G, -1, np.int64)                    # step at which an attack's exit test fired (-1: running)
    step = adam_t = 0
    try:
        while step < atk.steps:
            end = min(window_end(step), atk.steps if limit is None else limit(step))
            n_run = 1 if one_step else end - step
            enqueue(step, n_run, adam_t)
            adam_t += n_run
            last = step + n_run - 1
            # ---- the reference's control flow, per attack, where the reference's host work needs the values (ONE read-back)
            got = torch.cat([S.hist[:n_run].reshape(-1), S.exit.float()]).cpu().numpy().astype(np.float64)
            hrows, exited = got[:-G].reshape(n_run, cols, G), got[-G:].astype(np.int64)
            if on_step is not None:
                for s_i in range(step, last + 1):
                    on_step(s_i, hrows[s_i - step], (exited < 0) | (exited >= s_i), exited)
            step = last + 1
            active = exited < 0                          # after this window's exits
            if not active.any():
                break
            if not targeted_variant:
                continue
            if last > 0 and last % 50 == 0:              # target.py:123-125, tcolper.py:125-127: halve, NEW optimiser
                for n in lr_names:
                    if getattr(atk, n) is not None:
                        setattr(atk, n, getattr(atk, n) / 2)
                adam_t = 0
                for t in moments:
                    t.zero_()
            if between is not None:
                between(last, step, active)
    finally:
        if restore_lr:
            for n, value in zip(lr_names, at_call):
                setattr(atk, n, value)
    out = S.out.clone()                                  # (the caller owns what it gets; the state buffer is reused)
    for g in np.nonzero(exited < 0)[0]:                  # attacks that ran to the cap: the current image
        _lib.call("psg_to_channel_major", runtime.ptr(S.x0[g * rows:(g + 1) * rows]), rows, 9, N,
                  runtime.ptr(out[g * rows:(g + 1) * rows]), runtime.stream())
    return out, np.where(exited >= 0, exited + 1, step).astype(np.int64), step
