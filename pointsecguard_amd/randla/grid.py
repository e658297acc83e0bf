"""Grid sub-sampling and the projection of raw points onto the sub-cloud, on the device (psg_grid.hip).

Mirrors the data preparation of the reference's RandLA-Net pipeline: `DataProcessing.grid_sub_sampling`
(RandLA-Net/helper_tool.py:197-216, over the native utils/cpp_wrappers/cpp_subsampling) turns a raw cloud into the
barycentre cloud the sampler and the network see, and `proj_idx` (utils/data_prepare_s3dis.py: a sklearn
`KDTree(sub_xyz).query(xyz, k=1)`) carries predictions on that sub-cloud back to the raw points.

Barycentres and mean features are bit-equal to the reference's (fp32, its evaluation order, a cell's sums in input order).
Three things are ours, because the reference leaves them to accident:
  * output order: ascending cell key iX + NX * iY + NX * NY * iZ (the reference's is its hash map's iteration order);
  * label ties: of equally frequent labels in a cell the smallest in signed int32 order wins (the reference takes whichever
    its hash map meets first);
  * a cell index of -1 (the grid's origin can exceed the minimum corner by a rounding) counts as 0 (the reference casts the
    negative float to size_t, which is undefined).
The projection is `knn_points(sub[None], query[None], 1)` bit for bit - fp32 distances, ties to the lower index -, where
sklearn's query is float64: the two can differ where two sub-points are equally near within fp32 rounding.

There is no CPU path.  Device tensors in, device tensors out, on the current stream; the number of occupied cells is read
back once, inside psg_grid_assign, to size the outputs.
"""
import ctypes
import math

import torch

from pointsecguard_amd import _lib, runtime


class _Grid(runtime._Handle):
    _destroy = "psg_grid_destroy"

    def __init__(self, device, max_points):
        self.ctx = runtime.context(device)
        self.max_points = max_points
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().psg_grid_create(self.ctx, max_points, ctypes.byref(self.handle)), "psg_grid_create")


_grids = {}


def _grid(device, n):
    """The device's scratch handle, re-created (half as large again) when a cloud outgrows it."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    g = _grids.get(idx)
    if g is None or g.max_points < n:
        _grids[idx] = None
        g = None               # (the old handle is released before the new one is allocated)
        _grids[idx] = g = _Grid(device, max(n, min(max(n + n // 2, 1 << 16), 1 << 30)))
    return g


def _check_grid_size(grid_size):
    g = float(grid_size)
    if not (g > 0.0 and math.isfinite(g)):
        raise ValueError("grid_size must be a positive finite number (got %r)" % (grid_size,))
    return g


def _check_points(t, name):
    runtime.require_cuda(t, name, torch.float32)
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError("%s must be [N, 3] with N >= 1 (got %s)" % (name, tuple(t.shape)))
    return t.shape[0]


def grid_sub_sampling_device(points, features=None, labels=None, grid_size=0.1, return_index=False):
    """points [N,3] float32, features [N,d] float32 (optional), labels [N] or [N,l] int32 (optional), all on the device ->
    (sub_points [M,3], sub_features [M,d] or None, sub_labels [M,l] or None), one row per occupied cell of edge grid_size
    in ascending cell-key order; sub_labels is 2-D even for 1-D labels, like the reference's.  return_index=True appends
    voxel_of_point [N] int32, the output row every input point fell into.

    Label ties go to the smallest label; a cell index of -1 counts as 0 (module docstring).  Shape errors are ValueError;
    non-finite coordinates and a grid of more than 2^20 cells along an axis are PsgError, raised before any output exists."""
    n = _check_points(points, "points")
    grid_size = _check_grid_size(grid_size)
    d = l = 0
    if features is not None:
        runtime.require_cuda(features, "features", torch.float32)
        if features.dim() != 2 or features.shape[0] != n or features.shape[1] < 1:
            raise ValueError("features must be [N=%d, d >= 1] (got %s)" % (n, tuple(features.shape)))
        d = features.shape[1]
    if labels is not None:
        runtime.require_cuda(labels, "labels", torch.int32)
        if labels.dim() not in (1, 2) or labels.shape[0] != n or (labels.dim() == 2 and labels.shape[1] < 1):
            raise ValueError("labels must be [N=%d] or [N, l >= 1] (got %s)" % (n, tuple(labels.shape)))
        l = 1 if labels.dim() == 1 else labels.shape[1]
    dev = points.device
    g = _grid(dev, n)
    vox = torch.empty(n, dtype=torch.int32, device=dev) if return_index else None
    m = ctypes.c_int(0)
    _lib.call("psg_grid_assign", g.handle, runtime.ptr(points), n, grid_size, runtime.ptr(vox), ctypes.byref(m), runtime.stream())
    m = m.value
    sub_points = torch.empty(m, 3, dtype=torch.float32, device=dev)
    sub_features = torch.empty(m, d, dtype=torch.float32, device=dev) if d else None
    sub_labels = torch.empty(m, l, dtype=torch.int32, device=dev) if l else None
    _lib.call("psg_grid_reduce", g.handle, runtime.ptr(points), runtime.ptr(features), d, runtime.ptr(labels), l,
              runtime.ptr(sub_points), runtime.ptr(sub_features), runtime.ptr(sub_labels), runtime.stream())
    out = (sub_points, sub_features, sub_labels)
    return out + (vox,) if return_index else out


def nearest_sub_point(sub_points, query, grid_size=0.1):
    """sub_points [M,3], query [Q,3] float32 on the device -> int32 [Q]: the index of the sub-point nearest to every query
    point, equal to knn_points(sub_points[None], query[None], 1)[0, :, 0] (fp32 distance, ties to the lower index), found
    through a table of the sub-points' cells of edge grid_size instead of a scan of all M.  grid_size only sets the cell size
    of the table (the sub-sampling's own is the natural choice; the library doubles it until the grid has at most 64 cells per
    sub-point, so that a sparse sub-cloud does not make a query walk an empty grid); the answer does not depend on it."""
    m = _check_points(sub_points, "sub_points")
    q = _check_points(query, "query")
    grid_size = _check_grid_size(grid_size)
    if sub_points.device != query.device:
        raise ValueError("sub_points and query are on different devices")
    g = _grid(sub_points.device, m)
    out = torch.empty(q, dtype=torch.int32, device=query.device)
    _lib.call("psg_grid_index", g.handle, runtime.ptr(sub_points), m, grid_size, runtime.stream())
    _lib.call("psg_grid_nearest", g.handle, runtime.ptr(query), q, runtime.ptr(out), runtime.stream())
    return out
