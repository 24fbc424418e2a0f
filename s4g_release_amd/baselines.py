"""The GPD baseline's classifier on the close-region projection maps.

`GPDClassifier` has the parameters of the reference's network of that name
(inference/grasp_proposal/network_models/models/GPD.py: `conv1`, `conv2`, `fc1`, `fc2`; a reference checkpoint loads with
strict=True) and runs torch layers.  `FusedGPD` runs the same network in eval mode through csrc/gpd.hip
(s4g_gpd_forward_f32): one sync-free, graph-capturable chain of launches on the current stream that selects the frames
inside its loader, so `regions.maps` is never gathered into a copy.  There is no CPU fallback.
"""
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
