"""Thin object layer over the C ABI: PyTorch supplies device memory and the HIP stream, libpsg.so does
all the computing.  Nothing here falls back to PyTorch ops for the hot path.
"""
import ctypes

import numpy as np
import torch

from . import _lib

SA_NPOINT = (1024, 256, 64, 16)   # PointNet/models/pointnet2_sem_seg.py:9-12 (reference)
SA_RADIUS = (0.1, 0.2, 0.4, 0.8)
NSAMPLE = 32
SA_PACK_GROUPS = (4, 2, 1, 1)     # SSG: groups per unpacked SA workgroup (psg_pn2.hip: P / 32); plan_tensor(7, ...)
SA_WIDTH3 = (64, 128, 256, 512)   # SSG: width of each SA level's last layer; plan_tensor(8, ...)
NUM_CLASSES = 13
ARCH_SSG, ARCH_MSG = 0, 1          # PSG_PN2_ARCH_* of include/psg.h
ARCH_LAYERS = {ARCH_SSG: 23, ARCH_MSG: 35}
MSG_NSAMPLE = (16, 32)             # PointNet/models/pointnet2_sem_seg_msg.py:10-13 (reference)
ACT_POINTS = (1024, 256, 64, 16, 64, 256, 1024)
ACT_SHAPES = ((1024, 64), (256, 128), (64, 256), (16, 512), (64, 256), (256, 256), (1024, 128))

_ctx = {}
_hip = None


def ptr(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.PsgError("%s must be a tensor on the MI355X device (got %r); there is no CPU path" % (
            name, getattr(t, "device", type(t))))
    if dtype is not None and t.dtype != dtype:
        raise _lib.PsgError("%s must have dtype %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.PsgError("%s must be contiguous" % name)
    return t


def context(device=None):
    """One psg_ctx per device index, created on first use."""
    if device is None:
        device = torch.cuda.current_device()
    device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _ctx:
        lib = _lib.load()
        torch.cuda.init()
        h = ctypes.c_void_p()
        _lib.check(lib.psg_ctx_create(idx, ctypes.byref(h)), "psg_ctx_create")
        _ctx[idx] = h
    return _ctx[idx]


def _hip_memcpy_d2d(dst_ptr, src_ptr, nbytes):
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        _hip.hipMemcpyAsync.restype = ctypes.c_int
    rc = _hip.hipMemcpyAsync(dst_ptr, src_ptr, nbytes, 3, stream())
    if rc != 0:
        raise _lib.PsgError("hipMemcpyAsync failed with %d" % rc)


class _Handle:
    """Owner of one libpsg handle: `handle` is filled in by the subclass's create call and given to the library's
    `_destroy` symbol when the object goes."""
    _destroy = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                getattr(_lib.load(), self._destroy)(self.handle)
                self.handle = None
        except Exception:
            pass


def _as_ndarray(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v


def _as_f64(sd, key):
    return np.asarray(_as_ndarray(sd[key]), np.float64)


def _fold_conv_bn(sd, conv, bn, eps):
    """Eval-mode BatchNorm `bn` (or None) folded into the conv / linear layer `conv` before it: fp64 (w [out][in], b [out])."""
    w = _as_f64(sd, conv + ".weight")
    w = w.reshape(w.shape[0], -1)
    b = _as_f64(sd, conv + ".bias")
    if bn is not None:
        s = _as_f64(sd, bn + ".weight") / np.sqrt(_as_f64(sd, bn + ".running_var") + eps)
        w = w * s[:, None]
        b = (b - _as_f64(sd, bn + ".running_mean")) * s + _as_f64(sd, bn + ".bias")
    return w, b


def fold_state_dict(sd, eps=1e-5, msg=False):
    """Eval-mode BatchNorm folded into the preceding 1x1 conv, in the layer order of
    psg_pn2_model_create.  sd: mapping name -> tensor/ndarray with the reference's state_dict keys
    (sa{1-4}.mlp_convs.N.weight ..., fp{1-4}..., conv1, bn1, conv2).  fp64 math, fp32 result."""
    def fold(conv, bn):
        w, b = _fold_conv_bn(sd, conv, bn, eps)
        return np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)

    out = []
    if msg:   # sa{l}.conv_blocks.{scale}.{j} / bn_blocks (pointnet_util.py:216-227 of the reference)
        for l in range(1, 5):
            for i in range(2):
                for j in range(3):
                    out.append(fold("sa%d.conv_blocks.%d.%d" % (l, i, j), "sa%d.bn_blocks.%d.%d" % (l, i, j)))
    else:
        for name in ("sa1", "sa2", "sa3", "sa4"):
            for i in range(3):
                out.append(fold("%s.mlp_convs.%d" % (name, i), "%s.mlp_bns.%d" % (name, i)))
    for name, nl in (("fp4", 2), ("fp3", 2), ("fp2", 2), ("fp1", 3)):
        for i in range(nl):
            out.append(fold("%s.mlp_convs.%d" % (name, i), "%s.mlp_bns.%d" % (name, i)))
    out.append(fold("conv1", "bn1"))
    out.append(fold("conv2", None))
    return out


class PN2Model(_Handle):
    """Device-resident MFMA-packed weights of get_model (psg_pn2_model)."""
    _destroy = "psg_pn2_model_destroy"

    def __init__(self, folded, device=None, arch=ARCH_SSG):
        n = ARCH_LAYERS[arch]
        if len(folded) != n:
            raise _lib.PsgError("expected %d folded layers, got %d" % (n, len(folded)))
        self.ctx = context(device)
        self.arch = arch
        lib = _lib.load()
        ws = (ctypes.c_void_p * n)(*[w.ctypes.data_as(ctypes.c_void_p) for w, _ in folded])
        bs = (ctypes.c_void_p * n)(*[b.ctypes.data_as(ctypes.c_void_p) for _, b in folded])
        self._keep = folded
        self.handle = ctypes.c_void_p()
        _lib.check(lib.psg_pn2_model_create_arch(self.ctx, arch, ws, bs, n, ctypes.byref(self.handle)),
                   "psg_pn2_model_create_arch")


class PN2Workspace(_Handle):
    """Geometry plan + activations + gradient buffers for a batch (psg_pn2_ws)."""
    _destroy = "psg_pn2_ws_destroy"

    def __init__(self, batch, n_point, max_forwards, device=None, arch=ARCH_SSG):
        self.ctx = context(device)
        self.batch, self.n_point, self.max_forwards, self.arch = batch, n_point, max_forwards, arch
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().psg_pn2_ws_create_arch(self.ctx, arch, batch, n_point, max_forwards,
                                                      ctypes.byref(self.handle)), "psg_pn2_ws_create_arch")
        self.device = torch.device("cuda", torch.cuda.current_device())

    @property
    def nbytes(self):
        return _lib.load().psg_pn2_ws_bytes(self.handle)

    def plan_build(self, x0, starts, n_forward):
        require_cuda(x0, "x0", torch.float32)
        require_cuda(starts, "starts", torch.int32)
        assert x0.shape == (self.batch, self.n_point, 9) and starts.numel() == n_forward * 4 * self.batch
        _lib.call("psg_pn2_plan_build", self.handle, ptr(x0), ptr(starts), n_forward, stream())

    def forward(self, model, slot, x0, logp=None, l4=None, lean=False):
        """lean=True: the forward the fused attack loops run (no module outputs kept for activation(); l4 not available)."""
        require_cuda(x0, "x0", torch.float32)
        if logp is None:
            logp = torch.empty(self.batch, self.n_point, NUM_CLASSES, device=x0.device, dtype=torch.float32)
        if lean:
            assert l4 is None
            _lib.call("psg_pn2_forward_lean", model.handle, self.handle, slot, ptr(x0), ptr(logp), stream())
        else:
            _lib.call("psg_pn2_forward", model.handle, self.handle, slot, ptr(x0), ptr(logp), ptr(l4), stream())
        return logp

    def backward(self, model, slot, dlogp, dx0=None, colour_only=False, full=False):
        """colour_only=True: the backward of the fused attack loops - channels 3..5 of dx0 only (the rest is zero here).
        full=True: psg_pn2_backward_full - channels 0:3 are the complete derivative, geometric paths included (SSG)."""
        require_cuda(dlogp, "dlogp", torch.float32)
        assert not (colour_only and full)
        if dx0 is None:
            dx0 = (torch.zeros if colour_only else torch.empty)(self.batch, self.n_point, 9, device=dlogp.device, dtype=torch.float32)
        name = "psg_pn2_backward_colour" if colour_only else ("psg_pn2_backward_full" if full else "psg_pn2_backward")
        _lib.call(name, model.handle, self.handle, slot, ptr(dlogp), ptr(dx0), stream())
        return dx0

    def field_attack(self, model, images, labels, starts, eps, alpha, iters, field, coord_eps=None, coord_alpha=None,
                     mask=None, target=None):
        """NB_attack / tar_NB_attack on the coordinate field (field = "coord") or on coordinates and colours together
        ("both"): the reference's loop body (nontarget.py:28-39, target.py:31-43) with the slice 0:3 beside / instead of
        3:6.  Geometry moves with the points, so every iteration rebuilds the plan from the current xyz (starts
        [iters][4][B]: four FPS draws per iteration) - a stream-ordered host loop of plan_build(n_forward = 1), forward,
        psg_ce_logp_grad, psg_pn2_backward_full and one psg_pgd_step_field per field, with no read-back inside.  Like the
        reference, the returned fields are the un-projected last step."""
        require_cuda(images, "images", torch.float32)
        require_cuda(starts, "starts", torch.int32)
        if field not in ("coord", "both"):
            raise _lib.PsgError("field must be 'color', 'coord' or 'both' (got %r)" % (field,))
        B, N = self.batch, self.n_point
        assert images.shape == (B, 9, N) and starts.numel() == iters * 4 * B
        if labels is not None:
            require_cuda(labels, "labels", torch.int32)
        if mask is not None:
            require_cuda(mask, "mask", torch.uint8)
        coord_eps = eps if coord_eps is None else coord_eps
        coord_alpha = alpha if coord_alpha is None else coord_alpha
        dev = images.device
        x0 = torch.empty(B, N, 9, device=dev, dtype=torch.float32)
        _lib.call("psg_to_point_major", ptr(images), B, 9, N, ptr(x0), stream())
        ori_xyz, ori_rgb = x0[:, :, 0:3].contiguous(), x0[:, :, 3:6].contiguous()
        logp = torch.empty(B, N, NUM_CLASSES, device=dev, dtype=torch.float32)
        dlogp = torch.empty_like(logp)
        dx0 = torch.empty_like(x0)
        starts = starts.reshape(iters, 4 * B)
        direction = 1.0 if target is None else -1.0
        for it in range(iters):
            last = 1 if it == iters - 1 else 0
            _lib.call("psg_pn2_plan_build", self.handle, ptr(x0), ptr(starts[it]), 1, stream())
            _lib.call("psg_pn2_forward", model.handle, self.handle, 0, ptr(x0), ptr(logp), None, stream())
            # non-targeted: CE_sum over all rooms / N (nontarget.py:34); targeted: CE_mean of room 0 (target.py:36-39)
            _lib.call("psg_ce_logp_grad", ptr(logp), ptr(labels) if target is None else None, 0 if target is None else int(target),
                      B * N, B * N if target is None else N, NUM_CLASSES, 1.0 / N, ptr(dlogp), None, stream())
            _lib.call("psg_pn2_backward_full", model.handle, self.handle, 0, ptr(dlogp), ptr(dx0), stream())
            _lib.call("psg_pgd_step_field", ptr(x0), ptr(dx0), ptr(ori_xyz), ptr(mask), B, N, 0, float(coord_alpha),
                      float(coord_eps), direction, last, stream())
            if field == "both":
                _lib.call("psg_pgd_step_field", ptr(x0), ptr(dx0), ptr(ori_rgb), ptr(mask), B, N, 3, float(alpha), float(eps),
                          direction, last, stream())
        out = torch.empty_like(images)
        _lib.call("psg_to_channel_major", ptr(x0), B, 9, N, ptr(out), stream())
        return out

    def backward_pgd(self, model, slot, dlogp, x0, ori, alpha, eps, mask=None, descent=False, last=False):
        """The colour-only backward with the NB / tar_NB update applied to x0 in place by the gradient's last gather (what
        psg_pn2_nb_attack runs per iteration; nontarget.py:37-39, target.py:41-43)."""
        require_cuda(dlogp, "dlogp", torch.float32)
        require_cuda(x0, "x0", torch.float32)
        require_cuda(ori, "ori", torch.float32)
        if mask is not None:
            require_cuda(mask, "mask", torch.uint8)
        assert x0.shape == (self.batch, self.n_point, 9) and ori.shape == (self.batch, self.n_point, 3) and x0.is_contiguous() and ori.is_contiguous()
        _lib.call("psg_pn2_backward_colour_pgd", model.handle, self.handle, slot, ptr(dlogp), ptr(x0), ptr(ori), ptr(mask),
                  float(alpha), float(eps), -1.0 if descent else 1.0, 1 if last else 0, stream())
        return x0

    def nb_step(self, model, slot, x0, ori, labels, alpha, eps, mask=None, target=None, last=False):
        """One iteration of nb_attack's loop on plan slot `slot`, exactly as the attack runs it (psg_pn2_nb_step): x0
        [B][N][9] is updated in place.  Afterwards no forward is resident for backward(): call forward() first."""
        require_cuda(x0, "x0", torch.float32)
        require_cuda(ori, "ori", torch.float32)
        if labels is not None:
            require_cuda(labels, "labels", torch.int32)
        if mask is not None:
            require_cuda(mask, "mask", torch.uint8)
        assert x0.shape == (self.batch, self.n_point, 9) and ori.shape == (self.batch, self.n_point, 3) and x0.is_contiguous() and ori.is_contiguous()
        _lib.call("psg_pn2_nb_step", model.handle, self.handle, slot, ptr(x0), ptr(ori), ptr(labels), ptr(mask), float(alpha),
                  float(eps), 0 if target is None else 1, 0 if target is None else int(target), 1 if last else 0, stream())
        return x0

    def fp1_grad(self):
        """fp1's first-layer gradient rows [B][N][128] as the last backward or step left them (parity tests)."""
        src = _lib.load().psg_pn2_fp1_grad_ptr(self.handle)
        out = torch.empty(self.batch, self.n_point, 128, dtype=torch.float32, device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
        return out

    def nb_attack(self, model, images, labels, starts, eps, alpha, iters, mask=None, target=None, out=None):
        require_cuda(images, "images", torch.float32)
        require_cuda(starts, "starts", torch.int32)
        if labels is not None:
            require_cuda(labels, "labels", torch.int32)
        if mask is not None:
            require_cuda(mask, "mask", torch.uint8)
        if out is None:
            out = torch.empty_like(images)
        _lib.call("psg_pn2_nb_attack", model.handle, self.handle, ptr(images), ptr(labels), ptr(starts), ptr(mask),
                  float(eps), float(alpha), int(iters), 0 if target is None else 1, 0 if target is None else int(target),
                  ptr(out), stream())
        return out

    PROF_TAGS = ("sa1_fwd", "sa2_fwd", "sa3_fwd", "sa4_fwd", "fp1_head_fwd", "fp2_fwd", "fp3_fwd", "fp4_fwd",
                 "fp1_head_bwd", "fp2_bwd", "fp3_bwd", "fp4_bwd", "sa1_bwd", "sa2_bwd", "sa3_bwd", "sa4_bwd",
                 "fps", "ball_query", "three_nn", "gather", "ce_grad", "pgd_step", "dx0_gather", "pw_fwd", "pw_bwd",
                 "geom_grel", "geom_wgrad", "geom_gx", "sa_pack_plan", "fp1_head_loop")

    def prof_enable(self, on=True):
        _lib.call("psg_pn2_prof_enable", self.handle, 1 if on else 0)

    def prof_read(self):
        """{kernel tag: (total ms, launches)} measured with HIP events on the launch stream."""
        n = len(self.PROF_TAGS)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int * n)()
        _lib.call("psg_pn2_prof_read", self.handle, n, ms, cnt)
        return {t: (ms[i], cnt[i]) for i, t in enumerate(self.PROF_TAGS) if cnt[i]}

    # ---- read-back helpers (parity tests)
    def plan_tensor(self, what, level, forward, room):
        n_l = (self.n_point,) + SA_NPOINT
        k0 = MSG_NSAMPLE[0] if self.arch == ARCH_MSG else NSAMPLE
        shape, dt = {0: ((SA_NPOINT[level],), torch.int32), 1: ((SA_NPOINT[level], k0), torch.int32),
                     2: ((n_l[level], 3), torch.int32), 3: ((n_l[level], 3), torch.float32),
                     4: ((SA_NPOINT[level], 3), torch.float32),
                     5: ((SA_NPOINT[level], MSG_NSAMPLE[1]), torch.int32),
                     6: ((SA_NPOINT[level],), torch.int32),                              # packed SA forward: valid rows per group
                     7: ((SA_NPOINT[level] // SA_PACK_GROUPS[level] + 2,), torch.int32),  # and the workgroup segmentation
                     8: ((SA_NPOINT[level], SA_WIDTH3[level] // 4), torch.int32),        # arg-max bytes, four to a word
                     9: ((SA_NPOINT[level] // SA_PACK_GROUPS[level], 4), torch.int32)}[what]   # workgroup descriptors
        src = _lib.load().psg_pn2_plan_ptr(self.handle, what, level, forward, room)
        if not src:
            raise _lib.PsgError("psg_pn2_plan_ptr: bad slice")
        out = torch.empty(shape, dtype=dt, device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
        return out

    def activation(self, which):
        n, c = ACT_POINTS[which], _lib.load().psg_pn2_activation_channels(self.handle, which)
        src = _lib.load().psg_pn2_activation_ptr(self.handle, which)
        out = torch.empty(self.batch, n, c, dtype=torch.float32, device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
        return out


# ---- vanilla PointNet sem-seg (pointnet_sem_seg.py + pointnet.py of the reference) ----------------------------------
POINTNET_POINT_TILE = 128   # PSG_POINTNET_POINT_TILE: n_point must be a multiple of it
# (conv / linear, BatchNorm or None, identity size added to the bias) in the layer order of psg_pointnet_model_create
POINTNET_LAYERS = (("feat.stn.conv1", "feat.stn.bn1", 0), ("feat.stn.conv2", "feat.stn.bn2", 0),
                   ("feat.stn.conv3", "feat.stn.bn3", 0), ("feat.stn.fc1", "feat.stn.bn4", 0),
                   ("feat.stn.fc2", "feat.stn.bn5", 0), ("feat.stn.fc3", None, 3),
                   ("feat.conv1", "feat.bn1", 0),
                   ("feat.fstn.conv1", "feat.fstn.bn1", 0), ("feat.fstn.conv2", "feat.fstn.bn2", 0),
                   ("feat.fstn.conv3", "feat.fstn.bn3", 0), ("feat.fstn.fc1", "feat.fstn.bn4", 0),
                   ("feat.fstn.fc2", "feat.fstn.bn5", 0), ("feat.fstn.fc3", None, 64),
                   ("feat.conv2", "feat.bn2", 0), ("feat.conv3", "feat.bn3", 0),
                   ("conv1", "bn1", 0), ("conv2", "bn2", 0), ("conv3", "bn3", 0), ("conv4", None, 0))


def fold_pointnet_state_dict(sd, eps=1e-5, dtype=np.float32):
    """Eval-mode BatchNorm folded into the preceding conv / linear layer of pointnet_sem_seg.get_model, and the STN
    identities of pointnet.py:41-47 / 77-83 added to the fc3 biases, in the layer order of psg_pointnet_model_create.
    sd: the reference's state_dict keys.  fp64 math, `dtype` result (fp32 for the device): [(w [out][in], b [out])] * 19."""
    out = []
    for layer, bn, iden in POINTNET_LAYERS:
        w, b = _fold_conv_bn(sd, layer, bn, eps)
        if iden:
            b = b + np.eye(iden).reshape(-1)
        out.append((np.ascontiguousarray(w, dtype), np.ascontiguousarray(b, dtype)))
    return out


class PointNetModel(_Handle):
    """Device-resident BN-folded weights of pointnet_sem_seg.get_model (psg_pointnet_model)."""
    _destroy = "psg_pointnet_model_destroy"

    def __init__(self, folded, device=None):
        n = len(POINTNET_LAYERS)
        if len(folded) != n:
            raise _lib.PsgError("expected %d folded layers, got %d" % (n, len(folded)))
        self.ctx = context(device)
        folded = [(np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)) for w, b in folded]
        ws = (ctypes.c_void_p * n)(*[w.ctypes.data_as(ctypes.c_void_p) for w, _ in folded])
        bs = (ctypes.c_void_p * n)(*[b.ctypes.data_as(ctypes.c_void_p) for _, b in folded])
        self._keep = folded
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().psg_pointnet_model_create(self.ctx, ws, bs, ctypes.byref(self.handle)), "psg_pointnet_model_create")


class PointNetWorkspace(_Handle):
    """Activations, ReLU bits, pooled arg-max sets and gradient buffers for (batch, n_point) (psg_pointnet_ws)."""
    _destroy = "psg_pointnet_ws_destroy"

    def __init__(self, batch, n_point, device=None):
        if n_point % POINTNET_POINT_TILE:
            raise _lib.PsgError("n_point=%d is not a multiple of the point tile %d" % (n_point, POINTNET_POINT_TILE))
        self.ctx = context(device)
        self.batch, self.n_point = batch, n_point
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().psg_pointnet_ws_create(self.ctx, batch, n_point, ctypes.byref(self.handle)), "psg_pointnet_ws_create")
        self.device = torch.device("cuda", torch.cuda.current_device())

    def forward(self, model, x0, logp=None, extras=False):
        """x0 [B][N][9] point-major -> logp [B][N][13]; extras=True also returns (trans [B,3,3], trans_feat [B,64,64],
        pooled [B,3,1024], arg-max [B,3,1024]) of STN3d, STNkd and the encoder."""
        require_cuda(x0, "x0", torch.float32)
        assert x0.shape == (self.batch, self.n_point, 9)
        dev = x0.device
        if logp is None:
            logp = torch.empty(self.batch, self.n_point, NUM_CLASSES, device=dev, dtype=torch.float32)
        trans = torch.empty(self.batch, 3, 3, device=dev, dtype=torch.float32)
        tf = torch.empty(self.batch, 64, 64, device=dev, dtype=torch.float32)
        pool = torch.empty(self.batch, 3, 1024, device=dev, dtype=torch.float32) if extras else None
        arg = torch.empty(self.batch, 3, 1024, device=dev, dtype=torch.int32) if extras else None
        _lib.call("psg_pointnet_forward", model.handle, self.handle, ptr(x0), ptr(logp), ptr(trans), ptr(tf), ptr(pool), ptr(arg),
                  stream())
        if extras:
            return logp, trans, tf, pool, arg
        return logp, tf

    def backward(self, model, dlogp, dtrans_feat=None, dx0=None):
        """dlogp [B][N][13] (+ optional d trans_feat [B][64][64]) -> dx0 [B][N][9] of the last forward."""
        require_cuda(dlogp, "dlogp", torch.float32)
        if dtrans_feat is not None:
            require_cuda(dtrans_feat, "dtrans_feat", torch.float32)
        if dx0 is None:
            dx0 = torch.empty(self.batch, self.n_point, 9, device=dlogp.device, dtype=torch.float32)
        _lib.call("psg_pointnet_backward", model.handle, self.handle, ptr(dlogp), ptr(dtrans_feat), ptr(dx0), stream())
        return dx0

    # psg_pointnet_debug_ptr codes (include/psg.h)
    DEBUG = {"a1": 0, "a2": 1, "h": 2, "k1": 3, "k2": 4, "e2": 5, "z1": 6, "z2": 7, "z3": 8, "logits": 9, "logp": 10, "x0in": 11,
             "mh": 20, "m1": 21, "m2": 22, "m3": 23, "mf1": 24, "mf2": 25, "mfk1": 26, "mfk2": 27,
             "pool": 30, "pidx": 31, "part_val": 32, "part_idx": 33,
             "f1": 40, "f2": 41, "trans": 42, "fk1": 43, "fk2": 44, "tf": 45, "t1": 46, "w1f": 47, "c2f": 48, "h1pf": 49, "gb": 50,
             "dz4": 60, "dz3": 61, "dz2": 62, "dz1": 63, "s1": 64, "dg": 65, "dpf": 66, "ht": 67, "dpft": 68, "dtf": 69, "dfk2": 70,
             "dfk1": 71, "dgk": 72, "dh": 73, "dxu": 74, "dtrans": 75, "df2": 76, "df1": 77, "dgs": 78}

    def debug(self, what):
        """A workspace buffer by name (tests): a [rows, cols] copy taken on the current stream, float32 except the ReLU bit
        words m* and the arg-max sets pidx / part_idx (int32).  Forward buffers are valid from a forward until the next
        forward, the d* ones, s1, ht from a backward until the next backward."""
        code = self.DEBUG[what]
        rows, cols = ctypes.c_int(), ctypes.c_int()
        src = _lib.load().psg_pointnet_debug_ptr(self.handle, code, ctypes.byref(rows), ctypes.byref(cols))
        if not src:
            raise _lib.PsgError("psg_pointnet_debug_ptr(%s): %s" % (what, _lib.load().psg_last_error().decode()))
        dtype = torch.int32 if (20 <= code < 30 or code in (31, 33)) else torch.float32
        out = torch.empty(rows.value, cols.value, dtype=dtype, device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
        return out

    def nb_attack(self, model, images, labels, eps, alpha, iters, mask=None, target=None, out=None):
        require_cuda(images, "images", torch.float32)
        if labels is not None:
            require_cuda(labels, "labels", torch.int32)
        if mask is not None:
            require_cuda(mask, "mask", torch.uint8)
        if out is None:
            out = torch.empty_like(images)
        _lib.call("psg_pointnet_nb_attack", model.handle, self.handle, ptr(images), ptr(labels), ptr(mask), float(eps),
                  float(alpha), int(iters), 0 if target is None else 1, 0 if target is None else int(target), ptr(out), stream())
        return out


# ---- unit ops -----------------------------------------------------------------------------------
def square_distance(src, dst):
    require_cuda(src, "src", torch.float32)
    require_cuda(dst, "dst", torch.float32)
    B, N, _ = src.shape
    M = dst.shape[1]
    out = torch.empty(B, N, M, dtype=torch.float32, device=src.device)
    _lib.call("psg_square_distance", context(src.device), ptr(src), ptr(dst), B, N, M, ptr(out), stream())
    return out


def fps(xyz, npoint, start):
    """xyz [P,N,3] float32 cuda, start [P] int32 -> idx [P,npoint] int32 (pointnet_util.py:63-84)."""
    require_cuda(xyz, "xyz", torch.float32)
    require_cuda(start, "start", torch.int32)
    P, N, _ = xyz.shape
    out = torch.empty(P, npoint, dtype=torch.int32, device=xyz.device)
    _lib.call("psg_fps", context(xyz.device), ptr(xyz), P, P, N, npoint, ptr(start), ptr(out), stream())
    return out


def gather_points(points, idx):
    require_cuda(points, "points", torch.float32)
    require_cuda(idx, "idx", torch.int32)
    P, N, C = points.shape
    S = idx.shape[1]
    out = torch.empty(P, S, C, dtype=torch.float32, device=points.device)
    _lib.call("psg_gather_points", context(points.device), ptr(points), P, P, N, C, ptr(idx), S, ptr(out), stream())
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    require_cuda(xyz, "xyz", torch.float32)
    require_cuda(new_xyz, "new_xyz", torch.float32)
    P, N, _ = xyz.shape
    S = new_xyz.shape[1]
    out = torch.empty(P, S, nsample, dtype=torch.int32, device=xyz.device)
    r2 = float(np.float32(radius ** 2))
    _lib.call("psg_ball_query", context(xyz.device), ptr(xyz), P, ptr(new_xyz), P, N, S, r2, nsample, ptr(out), stream())
    return out


def three_nn(xyz1, xyz2):
    require_cuda(xyz1, "xyz1", torch.float32)
    require_cuda(xyz2, "xyz2", torch.float32)
    P, N, _ = xyz1.shape
    S = xyz2.shape[1]
    idx = torch.empty(P, N, 3, dtype=torch.int32, device=xyz1.device)
    w = torch.empty(P, N, 3, dtype=torch.float32, device=xyz1.device)
    _lib.call("psg_three_nn", context(xyz1.device), ptr(xyz1), P, ptr(xyz2), P, N, S, ptr(idx), ptr(w), stream())
    return idx, w


def seg_stats(logp, labels, n_cls=NUM_CLASSES, counters=None):
    """Accumulate (seen, inter, union) int64 [3, n_cls]; returns (counters, pred)."""
    require_cuda(logp, "logp", torch.float32)
    require_cuda(labels, "labels", torch.int32)
    rows = labels.numel()
    if counters is None:
        counters = torch.zeros(3, n_cls, dtype=torch.int64, device=logp.device)
    pred = torch.empty(rows, dtype=torch.int32, device=logp.device)
    _lib.call("psg_seg_stats", ptr(logp), ptr(labels), rows, n_cls, ptr(counters), ptr(pred), stream())
    return counters, pred.view(labels.shape)


# ---- whole-scene NB attack (psg_scene.hip) ------------------------------------
def scene_occ_build(point_idx, n_scene, bad):
    """Occurrence lists of every scene point over the block slots: point_idx int32 [rows] (any shape) ->
    (occ_off int32 [n_scene + 1], occ_ent int32 [rows]), the slots of a point ascending; bad: int32 [1] device flag."""
    require_cuda(point_idx, "point_idx", torch.int32)
    require_cuda(bad, "bad", torch.int32)
    rows = point_idx.numel()
    occ_off = torch.empty(n_scene + 1, dtype=torch.int32, device=point_idx.device)
    occ_ent = torch.empty(rows, dtype=torch.int32, device=point_idx.device)
    scratch = torch.empty(n_scene + rows, dtype=torch.int32, device=point_idx.device)
    _lib.call("psg_scene_occ_build", ptr(point_idx), rows, int(n_scene), ptr(occ_off), ptr(occ_ent), ptr(scratch), ptr(bad),
              stream())
    return occ_off, occ_ent


def scene_colour_to_blocks(scene_rgb, point_idx, x, bad):
    """x [.., 9] channels 3:6 of every slot <- scene_rgb [n_scene, 3] of its point, in place."""
    require_cuda(scene_rgb, "scene_rgb", torch.float32)
    require_cuda(point_idx, "point_idx", torch.int32)
    require_cuda(x, "x", torch.float32)
    require_cuda(bad, "bad", torch.int32)
    rows = point_idx.numel()
    assert x.numel() == rows * 9 and scene_rgb.dim() == 2 and scene_rgb.shape[1] == 3
    _lib.call("psg_scene_colour_to_blocks", ptr(scene_rgb), ptr(point_idx), rows, scene_rgb.shape[0], ptr(x), ptr(bad), stream())
    return x


def scene_rows_mask(dlogp, point_idx, scene_mask):
    """dlogp [.., n_cls]: rows of slots whose scene point is not under scene_mask (uint8 [n_scene]) <- +0.0, in place."""
    require_cuda(dlogp, "dlogp", torch.float32)
    require_cuda(point_idx, "point_idx", torch.int32)
    require_cuda(scene_mask, "scene_mask", torch.uint8)
    rows = point_idx.numel()
    assert dlogp.numel() == rows * dlogp.shape[-1]
    _lib.call("psg_scene_rows_mask", ptr(dlogp), ptr(point_idx), ptr(scene_mask), rows, dlogp.shape[-1], scene_mask.numel(),
              stream())
    return dlogp


def _scene_step_common(var, name, scene_mask, occ_off, occ_ent, dx0, gsum_out):
    """The checks of the two step wrappers below: `var` [n_scene, 3] is the array the step moves.  Returns (rows, n_scene)."""
    require_cuda(var, name, torch.float32)
    require_cuda(occ_off, "occ_off", torch.int32)
    require_cuda(occ_ent, "occ_ent", torch.int32)
    require_cuda(dx0, "dx0", torch.float32)
    if scene_mask is not None:
        require_cuda(scene_mask, "scene_mask", torch.uint8)
        assert scene_mask.numel() == var.shape[0]
    if gsum_out is not None:
        require_cuda(gsum_out, "gsum_out", torch.float32)
        assert gsum_out.shape == var.shape
    rows, n_scene = occ_ent.numel(), var.shape[0]
    assert dx0.numel() == rows * 9 and occ_off.numel() == n_scene + 1 and var.shape == (n_scene, 3)
    return rows, n_scene


def scene_pgd_step(scene_rgb, scene_ori, scene_mask, occ_off, occ_ent, dx0, alpha, eps, direction, last, gsum_out=None):
    """One step on the scene's colours [n_scene, 3] (in place) from the block gradients dx0 [rows, 9] summed over every
    point's slots in ascending slot order (psg_scene_pgd_step)."""
    rows, n_scene = _scene_step_common(scene_rgb, "scene_rgb", scene_mask, occ_off, occ_ent, dx0, gsum_out)
    require_cuda(scene_ori, "scene_ori", torch.float32)
    assert scene_ori.shape == scene_rgb.shape
    _lib.call("psg_scene_pgd_step", ptr(scene_rgb), ptr(scene_ori), ptr(scene_mask), ptr(occ_off), ptr(occ_ent), ptr(dx0), rows,
              n_scene, float(alpha), float(eps), float(direction), 1 if last else 0, ptr(gsum_out), stream())
    return scene_rgb


def scene_delta_to_blocks(delta, point_idx, x_clean, x, bad):
    """x [.., 9] channels 0:3 of every slot <- fl32(x_clean [.., 9] channels 0:3 + delta [n_scene, 3] of its point), in
    place on x; x_clean holds the clean blocks (psg_scene_delta_to_blocks)."""
    require_cuda(delta, "delta", torch.float32)
    require_cuda(point_idx, "point_idx", torch.int32)
    require_cuda(x_clean, "x_clean", torch.float32)
    require_cuda(x, "x", torch.float32)
    require_cuda(bad, "bad", torch.int32)
    rows = point_idx.numel()
    assert x.numel() == rows * 9 and x_clean.numel() == rows * 9 and delta.dim() == 2 and delta.shape[1] == 3
    _lib.call("psg_scene_delta_to_blocks", ptr(delta), ptr(point_idx), ptr(x_clean), rows, delta.shape[0], ptr(x), ptr(bad),
              stream())
    return x


def scene_field_step(delta, scene_mask, occ_off, occ_ent, dx0, alpha, eps, direction, last, gsum_out=None):
    """One step on the scene's displacements [n_scene, 3] (in place) from channels 0:3 of the block gradients dx0 [rows, 9]
    summed over every point's slots in ascending slot order; clamp to [-eps, eps], no box (psg_scene_field_step)."""
    rows, n_scene = _scene_step_common(delta, "delta", scene_mask, occ_off, occ_ent, dx0, gsum_out)
    _lib.call("psg_scene_field_step", ptr(delta), ptr(scene_mask), ptr(occ_off), ptr(occ_ent), ptr(dx0), rows, n_scene,
              float(alpha), float(eps), float(direction), 1 if last else 0, ptr(gsum_out), stream())
    return delta


# ---- whole-scene NU attack (psg_scene_nu.hip) ---------------------------------
def _scene_nu_common(scene_mask, active, n_scene):
    require_cuda(active, "active", torch.int32)
    assert active.numel() == 1
    if scene_mask is not None:
        require_cuda(scene_mask, "scene_mask", torch.uint8)
        assert scene_mask.numel() == n_scene


def scene_nu_init(c0, w_out=None):
    """w [n_scene, 3] = inverse_tanh_space(c0 [n_scene, 3]) (psg_scene_nu_init)."""
    require_cuda(c0, "c0", torch.float32)
    assert c0.dim() == 2 and c0.shape[1] == 3
    if w_out is None:
        w_out = torch.empty_like(c0)
    require_cuda(w_out, "w_out", torch.float32)
    assert w_out.shape == c0.shape
    _lib.call("psg_scene_nu_init", ptr(c0), c0.shape[0], ptr(w_out), stream())
    return w_out


def scene_nu_colour(w, scene_mask, occ_off, active, c):
    """c [n_scene, 3] <- 0.5 (tanh(w) + 1) on the moving points while active [1] (int32) is set, in place
    (psg_scene_nu_colour)."""
    require_cuda(w, "w", torch.float32)
    require_cuda(occ_off, "occ_off", torch.int32)
    require_cuda(c, "c", torch.float32)
    n_scene = w.shape[0]
    _scene_nu_common(scene_mask, active, n_scene)
    assert w.shape == c.shape == (n_scene, 3) and occ_off.numel() == n_scene + 1
    _lib.call("psg_scene_nu_colour", ptr(w), ptr(scene_mask), ptr(occ_off), n_scene, ptr(active), ptr(c), stream())
    return c


def scene_nu_step(w, m, v, c, c0, scene_mask, occ_off, occ_ent, dx0, sgrad, cw, lr, beta1, beta2, eps, step, active,
                  gsum_f_out=None, gsum_s_out=None):
    """One Adam step (step >= 1) on w / m / v [n_scene, 3] in place from the block gradients dx0 [rows, 9] (channels 3:6)
    and the per-slot Smooth gradients sgrad [rows, 3], both summed over every point's slots in ascending slot order; the L2
    term once per point (psg_scene_nu_step)."""
    n_scene, rows = w.shape[0], occ_ent.numel()
    for t, name in ((w, "w"), (m, "m"), (v, "v"), (c, "c"), (c0, "c0"), (dx0, "dx0"), (sgrad, "sgrad")):
        require_cuda(t, name, torch.float32)
    require_cuda(occ_off, "occ_off", torch.int32)
    require_cuda(occ_ent, "occ_ent", torch.int32)
    _scene_nu_common(scene_mask, active, n_scene)
    for t, name in ((gsum_f_out, "gsum_f_out"), (gsum_s_out, "gsum_s_out")):
        if t is not None:
            require_cuda(t, name, torch.float32)
            assert t.shape == w.shape
    assert w.shape == m.shape == v.shape == c.shape == c0.shape == (n_scene, 3) and occ_off.numel() == n_scene + 1
    assert dx0.numel() == rows * 9 and sgrad.numel() == rows * 3
    _lib.call("psg_scene_nu_step", ptr(w), ptr(m), ptr(v), ptr(c), ptr(c0), ptr(scene_mask), ptr(occ_off), ptr(occ_ent), ptr(dx0),
              ptr(sgrad), rows, n_scene, float(cw), float(lr), float(beta1), float(beta2), float(eps), int(step), ptr(active),
              ptr(gsum_f_out), ptr(gsum_s_out), stream())
    return w


def scene_nu_field_step(delta, m, v, scene_mask, occ_off, occ_ent, dx0, sgrad_xyz, coord_c, coord_lr, beta1, beta2, eps, step,
                        active, gsum_x_out=None, gsum_s_out=None):
    """One Adam step (step >= 1) on the displacements delta / m / v [n_scene, 3] in place from channels 0:3 of the block
    gradients dx0 [rows, 9] and the per-slot Smooth_xyz gradients sgrad_xyz [rows, 3], both summed over every point's slots in
    ascending slot order; the L2 term once per point, no tanh space (psg_scene_nu_field_step)."""
    n_scene, rows = delta.shape[0], occ_ent.numel()
    for t, name in ((delta, "delta"), (m, "m"), (v, "v"), (dx0, "dx0"), (sgrad_xyz, "sgrad_xyz")):
        require_cuda(t, name, torch.float32)
    require_cuda(occ_off, "occ_off", torch.int32)
    require_cuda(occ_ent, "occ_ent", torch.int32)
    _scene_nu_common(scene_mask, active, n_scene)
    for t, name in ((gsum_x_out, "gsum_x_out"), (gsum_s_out, "gsum_s_out")):
        if t is not None:
            require_cuda(t, name, torch.float32)
            assert t.shape == delta.shape
    assert delta.shape == m.shape == v.shape == (n_scene, 3) and occ_off.numel() == n_scene + 1
    assert dx0.numel() == rows * 9 and sgrad_xyz.numel() == rows * 3
    _lib.call("psg_scene_nu_field_step", ptr(delta), ptr(m), ptr(v), ptr(scene_mask), ptr(occ_off), ptr(occ_ent), ptr(dx0),
              ptr(sgrad_xyz), rows, n_scene, float(coord_c), float(coord_lr), float(beta1), float(beta2), float(eps), int(step),
              ptr(active), ptr(gsum_x_out), ptr(gsum_s_out), stream())
    return delta


def scene_nu_latch(pred, labels, target, point_idx, scene_mask, num, den, step, c, snap, counters, hist_row, exit_step, active):
    """The integer exit test of the whole-scene NU attack over all slots (psg_scene_nu_latch): pred / labels / point_idx int32
    [rows]; scene_mask None = non-targeted (hits: pred == labels, fires when hits * den < num * rows), uint8 [n_scene] =
    targeted (hits: masked slots with pred == target, fires when hits * den > num * masked slots).  counters int32 [2] (zero
    on entry, left zero), hist_row int64 [2], exit_step int32 [1], snap [n_scene, 3] <- c at the firing step."""
    require_cuda(pred, "pred", torch.int32)
    rows, n_scene = pred.numel(), c.shape[0]
    if labels is not None:
        require_cuda(labels, "labels", torch.int32)
        assert labels.numel() == rows
    if point_idx is not None:
        require_cuda(point_idx, "point_idx", torch.int32)
        assert point_idx.numel() == rows
    require_cuda(c, "c", torch.float32)
    require_cuda(snap, "snap", torch.float32)
    require_cuda(counters, "counters", torch.int32)
    require_cuda(hist_row, "hist_row", torch.int64)
    require_cuda(exit_step, "exit_step", torch.int32)
    _scene_nu_common(scene_mask, active, n_scene)
    assert c.shape == snap.shape == (n_scene, 3) and counters.numel() == 2 and hist_row.numel() == 2 and exit_step.numel() == 1
    _lib.call("psg_scene_nu_latch", ptr(pred), ptr(labels), int(target), ptr(point_idx), ptr(scene_mask), rows, n_scene, int(num),
              int(den), int(step), ptr(c), ptr(snap), ptr(counters), ptr(hist_row), ptr(exit_step), ptr(active), stream())


# ---- ResGCN (dense DeepGCN) ------------------------------------------------------------------------
def gcn_tensor_list(sd, n_blocks):
    """state_dict (reference key names, ResGCN/sem_seg_dense/architecture.py) -> the flat fp32 tensor list of
    psg_gcn_model_create."""
    def a(k):
        v = np.ascontiguousarray(_as_ndarray(sd[k]), np.float32)
        return v.reshape(v.shape[0], -1) if v.ndim > 1 else v

    out = []
    for e in range(n_blocks):
        base = "head.gconv.nn" if e == 0 else "backbone.%d.body.gconv.nn" % (e - 1)
        out += [a(base + ".0.weight"), a(base + ".0.bias")]
        out += [a(base + ".2." + k) for k in ("weight", "bias", "running_mean", "running_var")]
    for conv, bn in (("fusion_block.0", "fusion_block.2"), ("prediction.0.0", "prediction.0.2"),
                     ("prediction.1.0", "prediction.1.2")):
        out += [a(conv + ".weight"), a(conv + ".bias")] + [a(bn + "." + k) for k in ("weight", "bias", "running_mean", "running_var")]
    out += [a("prediction.3.0.weight"), a("prediction.3.0.bias")]
    return out


GCN_BLOCK_RES, GCN_BLOCK_PLAIN, GCN_BLOCK_DENSE = 0, 1, 2   # PSG_GCN_BLOCK_* / PSG_GCN_CONV_* of include/psg.h
GCN_CONV_EDGE, GCN_CONV_MR = 0, 1


class GCNModel(_Handle):
    _destroy = "psg_gcn_model_destroy"

    def __init__(self, sd, n_blocks, device=None, block=GCN_BLOCK_RES, conv=GCN_CONV_EDGE):
        self.ctx = context(device)
        self.n_blocks, self.block, self.conv = n_blocks, block, conv
        self._keep = gcn_tensor_list(sd, n_blocks)
        arr = (ctypes.c_void_p * len(self._keep))(*[t.ctypes.data_as(ctypes.c_void_p) for t in self._keep])
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().psg_gcn_model_create_cfg(self.ctx, arr, len(self._keep), n_blocks, block, conv,
                                                        ctypes.byref(self.handle)), "psg_gcn_model_create_cfg")


class GCNWorkspace(_Handle):
    _destroy = "psg_gcn_ws_destroy"

    def __init__(self, batch, n_point, n_blocks, device=None, block=GCN_BLOCK_RES, conv=GCN_CONV_EDGE):
        self.ctx = context(device)
        self.batch, self.n_point, self.n_blocks = batch, n_point, n_blocks
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().psg_gcn_ws_create_cfg(self.ctx, batch, n_point, n_blocks, block, conv,
                                                     ctypes.byref(self.handle)), "psg_gcn_ws_create_cfg")
        self.device = torch.device("cuda", torch.cuda.current_device())

    def knn(self, x, dilation):
        require_cuda(x, "x", torch.float32)
        B, N, C = x.shape
        out = torch.empty(B, N, 16, dtype=torch.int32, device=x.device)
        _lib.call("psg_gcn_knn", self.handle, ptr(x), C, int(dilation), ptr(out), stream())
        return out

    def knn_stats(self, reset=True):
        """Counters of the bf16-prefilter kNN kernel (workspaces created under PSG_GCN_KNN_STATS=1): dict of tiles,
        exact_tiles, rows, finalists, cuts, entries, why (reasons of the exact-path tiles)."""
        buf = (ctypes.c_ulonglong * 8)()
        _lib.call("psg_gcn_knn_stats", self.handle, buf, 1 if reset else 0)
        out = dict(zip(("tiles", "exact_tiles", "rows", "finalists", "cuts", "entries"), [int(v) for v in buf[:6]]))
        # why tiles went to the exact path (a tile can count under several): no threshold from the sample, a row above its
        # buffer, a row short of KK entries, a row short of KK keys below the cut's key, more than 256 finalists, bound broken
        a, b = int(buf[6]), int(buf[7])
        out["why"] = {"cut": a & 0xFFFF, "overflow": (a >> 16) & 0xFFFF, "underflow": (a >> 32) & 0xFFFF,
                      "short": b & 0xFFFF, "finalists": (b >> 16) & 0xFFFF, "bound": (b >> 32) & 0xFFFF}
        return out

    PROF_TAGS = ("knn_fused", "knn_other", "vertex_gemm", "edge_max", "fusion_prediction", "backward")

    def prof_enable(self, on=True):
        _lib.call("psg_gcn_prof_enable", self.handle, 1 if on else 0)

    def prof_read(self):
        """{tag: (total ms, launches, algorithmic FLOPs)} measured with HIP events on the launch stream."""
        n = len(self.PROF_TAGS)
        ms, cnt, fl = (ctypes.c_double * n)(), (ctypes.c_int * n)(), (ctypes.c_double * n)()
        _lib.call("psg_gcn_prof_read", self.handle, n, ms, cnt, fl)
        return {t: (ms[i], cnt[i], fl[i]) for i, t in enumerate(self.PROF_TAGS) if cnt[i]}

    def set_graphs(self, nbr):
        if nbr is not None:
            require_cuda(nbr, "nbr", torch.int32)
        _lib.call("psg_gcn_set_graphs", self.handle, ptr(nbr), stream())

    def forward(self, model, x0, logits=None):
        require_cuda(x0, "x0", torch.float32)
        if logits is None:
            logits = torch.empty(self.batch, self.n_point, NUM_CLASSES, device=x0.device, dtype=torch.float32)
        _lib.call("psg_gcn_forward", model.handle, self.handle, ptr(x0), ptr(logits), stream())
        return logits

    def backward(self, model, dlogits, dx0=None):
        require_cuda(dlogits, "dlogits", torch.float32)
        if dx0 is None:
            dx0 = torch.empty(self.batch, self.n_point, 9, device=dlogits.device, dtype=torch.float32)
        _lib.call("psg_gcn_backward", model.handle, self.handle, ptr(dlogits), ptr(dx0), stream())
        return dx0

    def nb_attack(self, model, images, labels, eps, alpha, iters, out=None):
        require_cuda(images, "images", torch.float32)
        require_cuda(labels, "labels", torch.int32)
        if out is None:
            out = torch.empty_like(images)
        _lib.call("psg_gcn_nb_attack", model.handle, self.handle, ptr(images), ptr(labels), float(eps), float(alpha),
                  int(iters), ptr(out), stream())
        return out

    def nb_attack_field(self, model, images, labels, field, eps, alpha, coord_eps, coord_alpha, iters, out=None):
        """psg_gcn_nb_attack_field: NB_attack on the coordinates (field 1) or on coordinates and colours (field 2)."""
        require_cuda(images, "images", torch.float32)
        require_cuda(labels, "labels", torch.int32)
        if out is None:
            out = torch.empty_like(images)
        _lib.call("psg_gcn_nb_attack_field", model.handle, self.handle, ptr(images), ptr(labels), int(field), float(eps),
                  float(alpha), float(coord_eps), float(coord_alpha), int(iters), ptr(out), stream())
        return out

    def nu_field_window(self, args, graph=None):
        """psg_gcn_nu_field_window: a window of optimiser steps of the coordinate-field NU attacks (args:
        _lib.GcnNuFieldWindowArgs; graph as for nu_window)."""
        _lib.call("psg_gcn_nu_field_window", ctypes.byref(args), graph, stream())

    def nu_window(self, args, graph=None):
        """psg_gcn_nu_window: the optimiser steps args.step0 .. args.step0 + args.n_steps - 1 of the ResGCN NU attacks for
        args.G rooms in lockstep, in one call (args: _lib.GcnNuWindowArgs whose model / ws fields hold the handles; graph:
        a psg_nu_graph handle that lets full windows of one shape be replayed, or None)."""
        _lib.call("psg_gcn_nu_window", ctypes.byref(args), graph, stream())

    def edges(self, block):
        src = _lib.load().psg_gcn_edge_ptr(self.handle, block)
        out = torch.empty(self.batch, self.n_point, 16, dtype=torch.int32, device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
        return out

    def feats(self):
        src = _lib.load().psg_gcn_feats_ptr(self.handle)
        out = torch.empty(self.batch, self.n_point, 64 * self.n_blocks, dtype=torch.float32, device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * 4)
        return out

    # psg_gcn_debug_ptr codes (include/psg.h); 50 and above are the kept copies of debug_keep(True)
    DEBUG = {"xyz": 0, "feats": 1, "nbr": 2, "arg": 3, "arg_mr": 4, "mask_mr": 5, "sq": 6, "xp": 7, "fused": 8, "mask_f": 9,
             "fmax": 10, "farg": 11, "gb1": 12, "h1": 13, "mask1": 14, "h2": 15, "mask2": 16, "logits": 17,
             "g2": 30, "g1": 31, "g1part": 32, "g1sum": 33, "gfvec": 34, "dfeats": 35, "gcur": 36,
             "k_pq": 50, "k_dfeats_head": 51, "k_dfeats_fusion": 52, "k_dpq": 53, "k_gz": 54, "k_state": 55, "k_dx0": 56}
    _DEBUG_DTYPE = {2: torch.int32, 3: torch.uint8, 4: torch.uint8, 5: torch.int32, 9: torch.int32, 11: torch.int32,
                    14: torch.int32, 16: torch.int32}

    def debug(self, what, block=0):
        """A workspace buffer by name (tests): a [rows, cols] copy taken on the current stream; float32 except the arg bytes
        (uint8), the ReLU bit words and the index tables (int32).  Validity windows and layouts: include/psg.h."""
        code = self.DEBUG[what]
        rows, cols = ctypes.c_int(), ctypes.c_int()
        src = _lib.load().psg_gcn_debug_ptr(self.handle, code, int(block), ctypes.byref(rows), ctypes.byref(cols))
        if not src:
            raise _lib.PsgError("psg_gcn_debug_ptr(%s, %d): %s" % (what, block, _lib.load().psg_last_error().decode()))
        out = torch.empty(rows.value, cols.value, dtype=self._DEBUG_DTYPE.get(code, torch.float32), device=self.device)
        _hip_memcpy_d2d(out.data_ptr(), src, out.numel() * out.element_size())
        return out

    def debug_keep(self, on=True):
        """psg_gcn_debug_keep: per-block copies of the buffers the forward / backward loops overwrite (the k_* names of debug)."""
        _lib.call("psg_gcn_debug_keep", self.handle, 1 if on else 0)
