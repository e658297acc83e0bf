"""`DataProcessing.knn_search` and the per-batch index pyramid of the reference's RandLA-Net pipeline, on the device.

Mirrors RandLA-Net/helper_tool.py:158-167 (`DataProcessing.knn_search(support_pts, query_pts, k)`: numpy in, int32
numpy out, like the reference, whose implementation is a nanoflann kd-tree per batch element on the host cores) and
the tf.data map function of main_S3DIS.py:189-214 (`tf_map`: for each of the num_layers encoder levels the points, their
k_n neighbours, the pooling indices of the sub-sampled points and the nearest sub-sampled point of every point).
Both run `psg_knn_points` (exact brute-force k-NN, hand-written HIP); there is no CPU path.

`DataProcessing.grid_sub_sampling` (helper_tool.py:197-216, the reference's native cpp_subsampling) is the numpy face of
`randla/grid.py`, which also holds the projection of raw points onto the sub-cloud (`nearest_sub_point`).

Only the indices are produced here; the network (RandLANet.py) is `randla/network.py`, the tester's attacks are
`randla/attack.py`, and the possibility-based crop sampler of main_S3DIS.py:116-187 is `randla/sampler.py`.
"""
import numpy as np
import torch

from pointsecguard_amd import _lib, runtime


def knn_points(support, query, k):
    """support [B,N1,3], query [B,N2,3] float32 CUDA tensors -> [B,N2,k] int32 neighbour indices into `support`,
    ascending (squared distance, index)."""
    runtime.require_cuda(support, "support", torch.float32)
    runtime.require_cuda(query, "query", torch.float32)
    if support.dim() != 3 or query.dim() != 3 or support.shape[2] != 3 or query.shape[2] != 3 or support.shape[0] != query.shape[0]:
        raise ValueError("expected support [B,N1,3] and query [B,N2,3], got %s and %s" % (tuple(support.shape), tuple(query.shape)))
    B, N1, _ = support.shape
    N2 = query.shape[1]
    out = torch.empty(B, N2, int(k), dtype=torch.int32, device=support.device)
    _lib.call("psg_knn_points", runtime.context(support.device), runtime.ptr(support), runtime.ptr(query), B, N1, N2, int(k),
              runtime.ptr(out), runtime.stream())
    return out


class DataProcessing:
    @staticmethod
    def knn_search(support_pts, query_pts, k):
        """
        :param support_pts: points you have, B*N1*3
        :param query_pts: points you want to know the neighbour index, B*N2*3
        :param k: Number of neighbours in knn search
        :return: neighbor_idx: neighboring points indexes, B*N2*k
        """
        s = torch.from_numpy(np.ascontiguousarray(support_pts, np.float32)).cuda()
        q = torch.from_numpy(np.ascontiguousarray(query_pts, np.float32)).cuda()
        return knn_points(s, q, k).cpu().numpy().astype(np.int32)

    @staticmethod
    def grid_sub_sampling(points, features=None, labels=None, grid_size=0.1, verbose=0):
        """
        Grid sub_sampling on the device (method = barycenter for points and features)
        :param points: (N, 3) matrix of input points
        :param features: optional (N, d) matrix of features (floating number)
        :param labels: optional (N,) or (N, l) matrix of integer labels
        :param grid_size: parameter defining the size of grid voxels
        :param verbose: accepted for the reference's signature; nothing is printed
        :return: sub_sampled points, with features and/or labels depending of the input: points alone, (points, features),
        (points, labels) or (points, features, labels); float32 / int32, labels 2-D (M, l) as the reference's wrapper returns
        them.  Inputs are coerced like the wrapper's: anything -> float32 / int32 (uint8 colours are accepted).

        Barycentres and mean features are bit-equal to the reference's.  Rows come in ascending cell-key order, label ties
        go to the smallest label, a cell index of -1 counts as 0 (randla/grid.py).  Shape errors are ValueError, raised
        before any device work.
        """
        p = np.ascontiguousarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError("Wrong dimensions : points.shape is not (N, 3)")
        f = lab = None
        if features is not None:
            f = np.ascontiguousarray(features, np.float32)
            if f.ndim != 2 or f.shape[0] != p.shape[0] or f.shape[1] < 1:
                raise ValueError("Wrong dimensions : features.shape is not (N, d)")
        if labels is not None:
            lab = np.ascontiguousarray(labels, np.int32)
            if lab.ndim not in (1, 2) or lab.shape[0] != p.shape[0] or (lab.ndim == 2 and lab.shape[1] < 1):
                raise ValueError("Wrong dimensions : classes.shape is not (N,) or (N, d)")
        if not (float(grid_size) > 0.0 and np.isfinite(float(grid_size))):
            raise ValueError("grid_size must be a positive finite number (got %r)" % (grid_size,))
        from pointsecguard_amd.randla.grid import grid_sub_sampling_device
        sp, sf, sl = grid_sub_sampling_device(torch.from_numpy(p).cuda(), None if f is None else torch.from_numpy(f).cuda(),
                                              None if lab is None else torch.from_numpy(lab).cuda(), grid_size)
        out = [t.cpu().numpy() for t in (sp, sf, sl) if t is not None]
        return out[0] if len(out) == 1 else tuple(out)


def tf_map_indices(batch_xyz, num_layers=5, k_n=16, sub_sampling_ratio=(4, 4, 4, 4, 2)):
    """The index part of tf_map (main_S3DIS.py:198-207) for a batch of clouds [B,N,3] resident on the device:
    returns (input_points, input_neighbors, input_pools, input_up_samples), each a list of num_layers tensors.
    Sub-sampling is the reference's: the first N // ratio points (its clouds arrive shuffled)."""
    runtime.require_cuda(batch_xyz, "batch_xyz", torch.float32)
    input_points, input_neighbors, input_pools, input_up_samples = [], [], [], []
    cur = batch_xyz
    for i in range(num_layers):
        neighbour_idx = knn_points(cur, cur, k_n)
        n_sub = cur.shape[1] // sub_sampling_ratio[i]
        sub_points = cur[:, :n_sub, :].contiguous()
        input_points.append(cur)
        input_neighbors.append(neighbour_idx)
        input_pools.append(neighbour_idx[:, :n_sub, :])
        input_up_samples.append(knn_points(sub_points, cur, 1))
        cur = sub_points
    return input_points, input_neighbors, input_pools, input_up_samples


DP = DataProcessing
