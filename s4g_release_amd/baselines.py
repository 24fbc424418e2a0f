"""The baselines' classifiers: GPD on the close-region projection maps, PointNetGPD on the close-region point sets.

`GPDClassifier` has the parameters of the reference's network of that name
(inference/grasp_proposal/network_models/models/GPD.py: `conv1`, `conv2`, `fc1`, `fc2`; a reference checkpoint loads with
strict=True) and runs torch layers.  `FusedGPD` runs the same network in eval mode through csrc/gpd.hip
(s4g_gpd_forward_f32): one sync-free, graph-capturable chain of launches on the current stream that selects the frames
inside its loader, so `regions.maps` is never gathered into a copy.  There is no CPU fallback.

`PointNetGPDClassifier` is the reference's `PointNetClassifier` (models/PointNetGPD.py: `feat.stn.*`, `feat.*`, `fc1..3`,
`bn1`, `bn2`; strict=True) on torch layers; `FusedPointNetGPD` runs it in eval mode through csrc/pointnet_gpd.hip
(s4g_pngpd_forward_f32) on dense (G, 3, n) sets or on the packed sets of `CloseRegions` at their true sizes.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _cabi

GPD_RESOLUTION = 60          # fc1's 7 200 inputs fix the map size
GPD_MAX_CHANNELS = 12
GPD_MAX_CLASSES = 16
GPD_DEFAULT_CHUNK = 1024     # images per pass of the kernels (csrc/gpd.hip's default)
GPD_MAX_CHUNK = 32768


class GPDClassifier(nn.Module):
    """maps (G, C, 60, 60) or (B, K, C, 60, 60) -> {"grasp_logits": (G or B * K, score_classes)}."""

    def __init__(self, in_channels, score_classes, dropout=False):
        super().__init__()
        self.in_channels = int(in_channels)
        self.out_channels = int(score_classes)
        self.conv1 = nn.Conv2d(self.in_channels, 20, 5)
        self.conv2 = nn.Conv2d(20, 50, 5)
        self.fc1 = nn.Linear(50 * 12 * 12, 500)
        self.fc2 = nn.Linear(500, self.out_channels)
        self.if_dropout = bool(dropout)

    def features(self, maps):
        """-> (pool1, pool2, hidden, logits) of maps (G, C, 60, 60); dropout as in forward."""
        p1 = F.max_pool2d(self.conv1(maps), 2, 2)
        p2 = F.max_pool2d(self.conv2(p1), 2, 2)
        h = F.relu(self.fc1(p2.reshape(-1, 7200)))
        if self.if_dropout and self.training:
            h = F.dropout(h, 0.5, True)
        return p1, p2, h, self.fc2(h)

    def forward(self, data_batch):
        maps = data_batch["close_region_projection_maps"]
        if maps.dim() == 5:
            maps = maps.reshape((-1,) + tuple(maps.shape[2:]))
        elif maps.dim() != 4:
            raise RuntimeError("close_region_projection_maps must be 4-D or 5-D")
        return {"grasp_logits": self.features(maps)[3]}


def build_gpd(in_channels=3, score_classes=3, dropout=False):
    """The GPD baseline's network.  (`model.build_model` keeps to the S4G network and the contact model.)"""
    return GPDClassifier(in_channels, score_classes, dropout)


class FusedGPD:
    """`GPDClassifier` in eval mode on the HIP kernels.  Packs the parameters on first use and again whenever one of
    them changed (tensor version counters) or moved."""

    def __init__(self, net):
        if not isinstance(net, GPDClassifier):
            raise RuntimeError("FusedGPD takes a baselines.GPDClassifier")
        if not (1 <= net.in_channels <= GPD_MAX_CHANNELS):
            raise ValueError("in_channels must be 1..%d, got %d" % (GPD_MAX_CHANNELS, net.in_channels))
        if not (1 <= net.out_channels <= GPD_MAX_CLASSES):
            raise ValueError("score_classes must be 1..%d, got %d" % (GPD_MAX_CLASSES, net.out_channels))
        self.net = net
        self.in_channels, self.classes = net.in_channels, net.out_channels
        self._packed = None
        self._key = None

    def _params(self):
        n = self.net
        return [n.conv1.weight, n.conv1.bias, n.conv2.weight, n.conv2.bias, n.fc1.weight, n.fc1.bias, n.fc2.weight,
                n.fc2.bias]

    def pack(self, device):
        """The packed parameters on `device`, repacked only when a parameter changed."""
        from . import functions as _F
        ps = self._params()
        key = (device,) + tuple((p.data_ptr(), p._version) for p in ps)
        if self._packed is not None and key == self._key:
            return self._packed
        lib = _cabi.lib()
        src = [p.detach().to(device=device, dtype=torch.float32).contiguous() for p in ps]
        nbytes = int(lib.s4g_gpd_pack_bytes(self.in_channels, self.classes))
        packed = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            rc = lib.s4g_gpd_pack_f32(*[t.data_ptr() for t in src], self.in_channels, self.classes, packed.data_ptr(),
                                      _F._stream())
        _cabi.check(rc, "gpd_pack")
        self._packed, self._key = packed, key
        return packed

    def __call__(self, maps, index=None, chunk=None, features=False):
        """maps (G, C, 60, 60) or (B, F, C, 60, 60) fp32 CUDA, C >= in_channels (the first in_channels are read; channel
        slices and frame-strided views are read in place) -> logits (..., classes); with features=True
        (logits, {"pool1", "pool2", "hidden"}).  index (K,), or (B, K) with a 5-D input whose rows index within their own
        scene, int32 or int64, -1 = a zero row.  chunk: images per pass (default 1 024)."""
        from . import functions as _F
        if not isinstance(maps, torch.Tensor) or maps.device.type != "cuda":
            raise RuntimeError("maps must be a CUDA tensor (there is no CPU fallback)")
        if maps.dtype != torch.float32:
            raise RuntimeError("maps must be float32")
        if maps.dim() not in (4, 5):
            raise RuntimeError("maps must be (G, C, 60, 60) or (B, F, C, 60, 60)")
        R = GPD_RESOLUTION
        if tuple(maps.shape[-2:]) != (R, R):
            raise RuntimeError("maps must hold %d x %d planes, got %s" % (R, R, tuple(maps.shape[-2:])))
        if maps.shape[-3] < self.in_channels:
            raise RuntimeError("maps hold %d channels, the network reads %d" % (maps.shape[-3], self.in_channels))
        chunk = GPD_DEFAULT_CHUNK if chunk is None else int(chunk)
        if not (1 <= chunk <= GPD_MAX_CHUNK):
            raise ValueError("chunk must be 1..%d, got %d" % (GPD_MAX_CHUNK, chunk))
        dev = maps.device
        lead = tuple(maps.shape[:-3])
        if maps.stride(-1) != 1 or maps.stride(-2) != R:
            maps = maps.contiguous()
        if maps.dim() == 5 and lead[0] > 1 and lead[1] > 1 and maps.stride(0) != lead[1] * maps.stride(1):
            maps = maps.contiguous()                      # the images are not evenly spaced
        if maps.dim() == 5:
            istride = maps.stride(1) if lead[1] > 1 else maps.stride(0)
            n_img = lead[0] * lead[1]
        else:
            istride, n_img = maps.stride(0), lead[0]
        cstride = maps.stride(-3)
        idx = None
        out_lead = lead
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.device != dev:
                raise RuntimeError("index must be a tensor on the device of maps")
            if index.dtype not in (torch.int32, torch.int64):
                raise RuntimeError("index must be int32 or int64")
            if index.dim() == 2:
                if maps.dim() != 5 or index.shape[0] != lead[0]:
                    raise RuntimeError("a (B, K) index needs (B, F, C, 60, 60) maps of the same B")
                Fr = lead[1]
                base = torch.arange(lead[0], device=dev, dtype=index.dtype)[:, None] * Fr
                idx = torch.where((index >= 0) & (index < Fr), index + base, torch.full_like(index, -1))
            elif index.dim() == 1:
                idx = index
            else:
                raise RuntimeError("index must be (K,) or (B, K)")
            out_lead = tuple(index.shape)
            idx = idx.to(torch.int32).contiguous().reshape(-1)
        G = 1
        for d in out_lead:
            G *= int(d)
        packed = self.pack(dev)
        C, K = self.in_channels, self.classes
        logits = torch.empty(out_lead + (K,), dtype=torch.float32, device=dev)
        feats = None
        if features:
            feats = {"pool1": torch.empty(out_lead + (20, 28, 28), dtype=torch.float32, device=dev),
                     "pool2": torch.empty(out_lead + (50, 12, 12), dtype=torch.float32, device=dev),
                     "hidden": torch.empty(out_lead + (500,), dtype=torch.float32, device=dev)}
        if G == 0:
            return (logits, feats) if features else logits
        lib = _cabi.lib()
        ch = min(chunk, G)
        nbytes = int(lib.s4g_gpd_workspace_bytes(ch, C, K))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.s4g_gpd_forward_f32(maps.data_ptr(), istride, cstride, None if idx is None else idx.data_ptr(), G,
                                         n_img, packed.data_ptr(), C, K, ch,
                                         feats["pool1"].data_ptr() if features else None,
                                         feats["pool2"].data_ptr() if features else None,
                                         feats["hidden"].data_ptr() if features else None, logits.data_ptr(),
                                         ws.data_ptr(), nbytes, _F._stream())
        _cabi.check(rc, "gpd_forward")
        return (logits, feats) if features else logits


PNGPD_MAX_CLASSES = 16
PNGPD_DEFAULT_CHUNK = 1024   # sets per pass of the kernels (csrc/pointnet_gpd.hip's default)
PNGPD_MAX_CHUNK = 32768


class _STN3d(nn.Module):
    def __init__(self, input_chann=3):
        super().__init__()
        self.conv1 = nn.Conv1d(input_chann, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.relu = nn.ReLU()
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

    def levels(self, x):
        """x (G, 3, n) -> (stn_global (G, 1024), trans (G, 3, 3))."""
        h = F.relu(self.bn1(self.conv1(x)))
        h = F.relu(self.bn2(self.conv2(h)))
        h = F.relu(self.bn3(self.conv3(h)))
        g = torch.max(h, 2)[0]
        h = F.relu(self.bn4(self.fc1(g)))
        h = F.relu(self.bn5(self.fc2(h)))
        eye = torch.eye(3, dtype=x.dtype, device=x.device)
        return g, self.fc3(h).view(-1, 3, 3) + eye

    def forward(self, x):
        return self.levels(x)[1]


class _PointNetfeat(nn.Module):
    def __init__(self, input_chann=3):
        super().__init__()
        self.stn = _STN3d(input_chann)
        self.conv1 = nn.Conv1d(input_chann, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)

    def levels(self, x):
        """x (G, 3, n) -> (stn_global, trans, global (G, 1024)); no ReLU before the maximum."""
        sg, trans = self.stn.levels(x)
        y = torch.bmm(x.transpose(2, 1), trans).transpose(2, 1)
        h = F.relu(self.bn1(self.conv1(y)))
        h = F.relu(self.bn2(self.conv2(h)))
        h = self.bn3(self.conv3(h))
        return sg, trans, torch.max(h, 2)[0]

    def forward(self, x):
        _, trans, g = self.levels(x)
        return g, trans


class PointNetGPDClassifier(nn.Module):
    """close_region_points (G, 3, n) or (B, K, 3, n) -> {"grasp_logits": (G or B * K, score_classes)}."""

    def __init__(self, input_chann=3, score_classes=3):
        super().__init__()
        self.input_chann = int(input_chann)
        self.out_channels = int(score_classes)
        self.feat = _PointNetfeat(self.input_chann)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, self.out_channels)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()

    def features(self, points):
        """points (G, 3, n) -> {"stn_global", "trans", "global", "hidden", "logits"}."""
        sg, trans, g = self.feat.levels(points)
        h = F.relu(self.bn1(self.fc1(g)))
        h = F.relu(self.bn2(self.fc2(h)))
        return {"stn_global": sg, "trans": trans, "global": g, "hidden": h, "logits": self.fc3(h)}

    def forward(self, data_batch):
        pts = data_batch["close_region_points"]
        if pts.dim() == 4:
            pts = pts.reshape((-1,) + tuple(pts.shape[2:]))
        elif pts.dim() != 3:
            raise RuntimeError("close_region_points must be 3-D or 4-D")
        return {"grasp_logits": self.features(pts)["logits"]}


def build_pointnetgpd(score_classes=3):
    """The PointNetGPD baseline's network.  (`model.build_model` keeps to the S4G network and the contact model.)"""
    return PointNetGPDClassifier(3, score_classes)


def _fold(layer, bn):
    """(weight (out, in), bias) of `layer` followed by eval-mode `bn`, folded in float64 -> fp32 CPU tensors."""
    w = layer.weight.detach().double().cpu().reshape(layer.weight.shape[0], -1)
    b = layer.bias.detach().double().cpu()
    if bn is not None:
        k = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
        w = w * k[:, None]
        b = (b - bn.running_mean.detach().double().cpu()) * k + bn.bias.detach().double().cpu()
    return w.float().contiguous(), b.float().contiguous()


class FusedPointNetGPD:
    """`PointNetGPDClassifier` in eval mode on the HIP kernels (csrc/pointnet_gpd.hip); there is no CPU fallback.  Every
    BatchNorm is folded into its layer in float64 on the host.  Packs on first use and again whenever a parameter or a
    running statistic changed (tensor version counters) or moved."""

    def __init__(self, net):
        if not isinstance(net, PointNetGPDClassifier):
            raise RuntimeError("FusedPointNetGPD takes a baselines.PointNetGPDClassifier")
        if net.input_chann != 3:
            raise ValueError("input_chann must be 3, got %d" % net.input_chann)
        if not (1 <= net.out_channels <= PNGPD_MAX_CLASSES):
            raise ValueError("score_classes must be 1..%d, got %d" % (PNGPD_MAX_CLASSES, net.out_channels))
        self.net = net
        self.classes = net.out_channels
        self._packed = None
        self._key = None

    def _pairs(self):
        n, f, s = self.net, self.net.feat, self.net.feat.stn
        return [(s.conv1, s.bn1), (s.conv2, s.bn2), (s.conv3, s.bn3), (s.fc1, s.bn4), (s.fc2, s.bn5), (s.fc3, None),
                (f.conv1, f.bn1), (f.conv2, f.bn2), (f.conv3, f.bn3), (n.fc1, n.bn1), (n.fc2, n.bn2), (n.fc3, None)]

    def pack(self, device):
        """The packed parameters on `device`, repacked only when a parameter or running statistic changed."""
        from . import functions as _F
        if self.net.training:
            raise RuntimeError("FusedPointNetGPD runs the network in eval mode only (call net.eval())")
        pairs = self._pairs()
        ts = []
        for layer, bn in pairs:
            ts += [layer.weight, layer.bias]
            if bn is not None:
                ts += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        key = (device,) + tuple((p.data_ptr(), p._version) for p in ts) + tuple(bn.eps for _, bn in pairs if bn is not None)
        if self._packed is not None and key == self._key:
            return self._packed
        lib = _cabi.lib()
        folded = [_fold(layer, bn) for layer, bn in pairs]
        src = [(w.to(device), b.to(device)) for w, b in folded]
        wp = (ctypes.c_void_p * 12)(*[w.data_ptr() for w, _ in src])
        bp = (ctypes.c_void_p * 12)(*[b.data_ptr() for _, b in src])
        nbytes = int(lib.s4g_pngpd_pack_bytes(self.classes))
        packed = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            rc = lib.s4g_pngpd_pack_f32(ctypes.cast(wp, ctypes.c_void_p), ctypes.cast(bp, ctypes.c_void_p), self.classes,
                                        packed.data_ptr(), _F._stream())
        _cabi.check(rc, "pngpd_pack")
        self._packed, self._key, self._src = packed, key, src      # the sources outlive the pack kernels
        return packed

    def __call__(self, points, offset=None, count=None, flags=None, index=None, chunk=None, features=False):
        """Two input forms, both fp32 CUDA and read in place:
          dense   points (G, 3, n) or (B, K, 3, n): the reference's input;
          packed  points (B, 3, capacity), offset (B, F + 1) int64, count (B, F) int32, optional flags (B, F): the fields
                  of `CloseRegions`.  Frame f's set is columns offset[b, f] .. offset[b, f] + count[b, f]: the whole set
                  at its true size, no gathered copy and no sampling.  index (K,) (over the B * F sets) or (B, K) (within
                  each scene), int32 or int64, -1 = a zero row.
        -> logits (..., classes); with features=True (logits, {"stn_global" (..., 1024), "trans" (..., 3, 3), "global"
        (..., 1024), "hidden" (..., 256), "status" (...) int32}).  status 0: scored; 1: the set holds a NaN or an infinity
        (a NaN row; no other row changes); 2: not scored -- index -1 or out of range, count 0, or flags bit 0 (the set
        did not fit the capacity) -- a zero row.  The reference would raise on an empty set; the zero row with status 2
        is this project's decision.  chunk: sets per pass (default 1 024)."""
        from . import functions as _F
        if not isinstance(points, torch.Tensor) or points.device.type != "cuda":
            raise RuntimeError("points must be a CUDA tensor (there is no CPU fallback)")
        if points.dtype != torch.float32:
            raise RuntimeError("points must be float32")
        chunk = PNGPD_DEFAULT_CHUNK if chunk is None else int(chunk)
        if not (1 <= chunk <= PNGPD_MAX_CHUNK):
            raise ValueError("chunk must be 1..%d, got %d" % (PNGPD_MAX_CHUNK, chunk))
        dev = points.device
        packed_form = offset is not None or count is not None
        idx = None
        if packed_form:
            if offset is None or count is None:
                raise RuntimeError("offset and count go together")
            if points.dim() != 3 or points.shape[1] != 3:
                raise RuntimeError("packed points must be (B, 3, capacity)")
            B, _, cap = points.shape
            for name, t, dt in (("offset", offset, torch.int64), ("count", count, torch.int32),
                                ("flags", flags, torch.int32)):
                if t is None:
                    continue
                if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or t.dim() != 2 or t.shape[0] != B:
                    raise RuntimeError("%s must be a (B, .) %s tensor on the device of points" % (name, dt))
            Fr = count.shape[1]
            if offset.shape[1] != Fr + 1 or (flags is not None and flags.shape[1] != Fr):
                raise RuntimeError("offset must be (B, F + 1) and flags (B, F) for count (B, F)")
            if cap >= 2 ** 31 or B * Fr >= 2 ** 31:
                raise ValueError("capacity and B * F must be below 2^31")
            points = points.contiguous()
            offset, count = offset.contiguous(), count.contiguous()
            flags = None if flags is None else flags.contiguous()
            sstride, cstride, npts, n_sets = 3 * cap, cap, 0, B * Fr
            out_lead = (B, Fr)
            if index is not None:
                if not isinstance(index, torch.Tensor) or index.device != dev:
                    raise RuntimeError("index must be a tensor on the device of points")
                if index.dtype not in (torch.int32, torch.int64):
                    raise RuntimeError("index must be int32 or int64")
                if index.dim() == 2:
                    if index.shape[0] != B:
                        raise RuntimeError("a (B, K) index needs the B of points")
                    base = torch.arange(B, device=dev, dtype=index.dtype)[:, None] * Fr
                    idx = torch.where((index >= 0) & (index < Fr), index + base, torch.full_like(index, -1))
                elif index.dim() == 1:
                    idx = index
                else:
                    raise RuntimeError("index must be (K,) or (B, K)")
                out_lead = tuple(index.shape)
                idx = idx.to(torch.int32).contiguous().reshape(-1)
            if Fr == 0:
                Fr, n_sets = 1, 0
        else:
            if flags is not None or index is not None:
                raise RuntimeError("flags and index belong to the packed form (offset, count)")
            if points.dim() not in (3, 4) or points.shape[-2] != 3:
                raise RuntimeError("points must be (G, 3, n) or (B, K, 3, n)")
            if points.shape[-1] >= 2 ** 31:
                raise ValueError("a set must hold fewer than 2^31 points")
            out_lead = tuple(points.shape[:-2])
            points = points.contiguous()
            npts = points.shape[-1]
            sstride, cstride, Fr, cap = 3 * npts, npts, 0, 0
            n_sets = 1
            for d in out_lead:
                n_sets *= int(d)
        G = 1
        for d in out_lead:
            G *= int(d)
        if G >= 2 ** 31:
            raise ValueError("the number of sets must be below 2^31")
        packed = self.pack(dev)
        K = self.classes
        logits = torch.empty(out_lead + (K,), dtype=torch.float32, device=dev)
        feats = None
        if features:
            feats = {"stn_global": torch.empty(out_lead + (1024,), dtype=torch.float32, device=dev),
                     "trans": torch.empty(out_lead + (3, 3), dtype=torch.float32, device=dev),
                     "global": torch.empty(out_lead + (1024,), dtype=torch.float32, device=dev),
                     "hidden": torch.empty(out_lead + (256,), dtype=torch.float32, device=dev),
                     "status": torch.empty(out_lead, dtype=torch.int32, device=dev)}
        if G == 0:
            return (logits, feats) if features else logits
        lib = _cabi.lib()
        ch = min(chunk, G)
        nbytes = int(lib.s4g_pngpd_workspace_bytes(ch, K))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        f = feats or {}
        with torch.cuda.device(dev):
            rc = lib.s4g_pngpd_forward_f32(points.data_ptr(), sstride, cstride, npts,
                                           ptr(offset) if packed_form else None, ptr(count) if packed_form else None,
                                           ptr(flags), Fr, cap, ptr(idx), G, n_sets, packed.data_ptr(), K, ch,
                                           ptr(f.get("stn_global")), ptr(f.get("trans")), ptr(f.get("global")),
                                           ptr(f.get("hidden")), ptr(f.get("status")), logits.data_ptr(),
                                           ws.data_ptr(), nbytes, _F._stream())
        _cabi.check(rc, "pngpd_forward")
        return (logits, feats) if features else logits
