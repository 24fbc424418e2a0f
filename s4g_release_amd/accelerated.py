"""`s4g_release_amd.accelerate(net)`: every SharedMLP and every set-abstraction max-pool of ANY PointNet++ graph on the matrix cores.

`FusedPointNet2` knows one graph shape.  This converts, in place, the modules of whatever network it is given -- the
default-argument 4-level `PointNet2` (a group-all SA level, an FP level without 3-NN), K = 8 or 48, channel widths that
are not multiples of 4, a 2-D `SharedMLP` head on (B, C, N, 1), or a network assembled by hand -- recognised by
STRUCTURE, so the reference's own instances qualify too:

  * SharedMLP-shaped: an `nn.ModuleList` of blocks, each with a `.conv` (1x1 `Conv1d` / `Conv2d`, groups 1), a `.bn`
    (BatchNorm1d / 2d with running statistics, or None) and a `.relu` (`nn.ReLU` or None);
  * SA-module-shaped: `num_centroids`, `sampler`, `grouper`, `use_xyz` and a SharedMLP-shaped `mlp` whose last block has
    a ReLU (`PointNetSAAvgModule` shares those attributes but not the forward: left alone).  An `EdgeSAModule` -- a
    grouper whose forward takes the centroids' features -- qualifies: it groups through its own grouper (the
    (B, 2C+3, M, K) tensor [xyz | f_j | f_j - f_c] exists on this path; `FusedPointNet2` never forms it).

A converted module's class becomes a generated subclass of its own class, so identity, hooks, parent references,
`isinstance` and the `state_dict` stay exactly as they were.  Its forward runs the fast path only in eval mode, on a
float32 HIP input, when autograd is not needed (`torch.no_grad()` / `torch.inference_mode()`, or nothing requires
grad); otherwise the original class's forward runs, bit for bit as before.

Launches (csrc/mlp_gemm.hip, BatchNorm folded into the weights on the first fast call and re-folded when a parameter
or buffer changes -- `load_state_dict`, in-place edits):
  * SharedMLP: layer 0 reads the (B, C, *S) input through the channels-first loader; interior activations are
    channels-last (P, C) fp32; the last layer writes (B, Cout, *S) through the channels-first store;
  * SA: `modules.sample_and_group`, then the same chain on the grouped (B, C, M, K) tensor with the max over the K
    neighbours inside the last launch's epilogue (the (B, Cout, M, K) tensor and `torch.max` are gone).
With "f16x2" every launch needs a per-scene bound of |A|: the first one takes it from the source features (one small
reduction, `s4g_amax_per_scene_f32`; twice that for an edge module, whose columns f_j - f_c reach 2 max|f|) plus the
ball radius for the centred xyz columns, the next ones from the previous launch's `out_amax`.  No host synchronisation.  The logit `Conv1d`s and the sigmoid stay torch.
"""
import ctypes
import inspect

import torch
from torch import nn

from . import _cabi
from . import functions as _F
from .fused import _Layer, _pad_k, fold_conv_bn
from .modules import edge_sample_and_group, sample_and_group

PRECISIONS = {"f16x2": 3, "fp32": 0}
LOAD_PLAIN, LOAD_CHANNEL_FIRST = 0, 6
EPI_STORE, EPI_CHANNEL_FIRST, EPI_MAX_CHANNEL_FIRST = 0, 2, 3


def _is_block(b):
    conv, bn = getattr(b, "conv", None), getattr(b, "bn", False)
    if not isinstance(conv, (nn.Conv1d, nn.Conv2d)) or conv.groups != 1 or not hasattr(b, "relu"):
        return False
    if any(v != 1 for v in tuple(conv.kernel_size) + tuple(conv.stride) + tuple(conv.dilation)):
        return False
    if conv.padding not in ("valid", (0,), (0, 0)):
        return False
    two_d = isinstance(conv, nn.Conv2d)
    if bn is not None and not (isinstance(bn, nn.BatchNorm2d if two_d else nn.BatchNorm1d) and
                               bn.running_mean is not None and bn.running_var is not None):
        return False
    return b.relu is None or isinstance(b.relu, nn.ReLU)


def _is_shared_mlp(m):
    if not isinstance(m, nn.ModuleList) or len(m) == 0 or not all(_is_block(b) for b in m):
        return False
    if len({type(b.conv) for b in m}) != 1:
        return False
    return all(a.conv.out_channels == b.conv.in_channels for a, b in zip(m, list(m)[1:]))


def _is_sa(m):
    if not all(hasattr(m, a) for a in ("num_centroids", "sampler", "grouper", "use_xyz", "mlp")):
        return False
    name = getattr(type(m), "_s4g_base", type(m)).__name__
    if "Avg" in name:
        return False
    return (_is_shared_mlp(m.mlp) and isinstance(m.mlp[0].conv, nn.Conv2d) and m.mlp[-1].relu is not None and
            (m.num_centroids == 0 or hasattr(m.grouper, "radius")))


class _State:
    """Precision and the folded-weight cache of one converted module."""

    def __init__(self, precision):
        self.precision = precision
        self.key = None
        self.layers = None

    def folded(self, mlp, dev):
        blocks = list(mlp)
        key = (dev, tuple((t._version, t.data_ptr(), t.device) for b in blocks
                          for t in list(b.parameters()) + list(b.buffers())))
        if key != self.key:
            layers = []
            for b in blocks:
                w, bias = fold_conv_bn(b)
                layers.append((_Layer(_pad_k(w.to(dev)), bias.to(dev), w.shape[1]), b.relu is not None))
            self.layers, self.key = layers, key
        return self.layers


def _fast(mod, *xs):
    """Eval mode, float32 HIP inputs, parameters float32 on the same device, no autograd needed."""
    if mod.training:
        return False
    dev = xs[0].device
    for x in xs:
        if x is not None and (not x.is_cuda or x.dtype != torch.float32 or x.device != dev):
            return False
    params = list(mod.parameters())
    if any(p.device != dev or p.dtype != torch.float32 for p in params):
        return False
    if torch.is_grad_enabled() and (any(x is not None and x.requires_grad for x in xs) or
                                    any(p.requires_grad for p in params)):
        return False
    return True


def _slots(B, dev):
    return torch.zeros((B, 64), dtype=torch.int32, device=dev)


def _amax(x, B):
    """(B, 64) slot rows bounding |x| per scene (x contiguous, B equal blocks)."""
    s = _slots(B, x.device)
    _cabi.check(_cabi.lib().s4g_amax_per_scene_f32(x.data_ptr(), B, x.numel() // B, s.data_ptr(), _F._stream()),
                "amax_per_scene")
    return s


def _launch(layer, prec, relu, loader, epi, P, cin, A, out, rps, lda=0, a_L=0, a_amax=None, a_amax2=None, floor=0.0,
            out_amax=None, ldc=0, M=0, K=0, cf_N=0):
    d = _cabi.GemmDesc()
    d.loader, d.epilogue, d.groups, d.relu = loader, epi, 1, int(relu)
    d.P, d.Cin, d.Kpad, d.Cout = P, cin, layer.kpad, layer.cout
    d.W, d.bias = layer.W.data_ptr(), layer.bias.data_ptr()
    d.w_gstride, d.b_gstride = layer.cout * layer.kpad, layer.cout
    d.precision, d.Kpad16, d.W_bf16x3 = prec, layer.kpad16, layer.W3.data_ptr()
    d.W_f16x2, d.w_inv_scale = layer.Wh2.data_ptr(), layer.w_inv_scale.data_ptr()
    if layer.Wfrag is not None:
        d.W_f16x2_frag = layer.Wfrag.data_ptr()
    d.A, d.lda, d.a_L, d.rows_per_scene = A.data_ptr(), lda, a_L, rps
    if a_amax is not None:
        d.a_amax = a_amax.data_ptr()
    if a_amax2 is not None:
        d.a_amax2 = a_amax2.data_ptr()
    d.a_amax_floor = floor
    if out_amax is not None:
        d.out_amax = out_amax.data_ptr()
    d.out, d.ldc, d.M, d.K = out.data_ptr(), ldc, M, K
    d.cf_ptr[0] = out.data_ptr()
    for i in range(5):
        d.cf_start[i] = 0 if i == 0 else layer.cout
    d.cf_sigmoid_from, d.cf_N = layer.cout, cf_N
    _cabi.check(_cabi.lib().s4g_mlp_gemm_f32(ctypes.byref(d), _F._stream()), "mlp_gemm (accelerate)")


def _chain(mlp, st, x, bound=None, M=0, K=0):
    """The SharedMLP `mlp` on x (B, C, *S): (B, Cout, *S), or with M / K (S = (M, K)) the max over K: (B, Cout, M).
    bound: (a_amax, a_amax2, floor) of x for f16x2, or None to reduce x itself."""
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    spatial = tuple(x.shape[2:])
    L = x[0, 0].numel()
    P = B * L
    dev = x.device
    prec = PRECISIONS[st.precision]
    h2 = prec == PRECISIONS["f16x2"]
    layers = st.folded(mlp, dev)
    if h2 and bound is None:
        bound = (_amax(x, B), None, 0.0)
    amax = bound if h2 else (None, None, 0.0)
    cur, lda = x, 0
    for i, (layer, relu) in enumerate(layers):
        last = i == len(layers) - 1
        loader = LOAD_CHANNEL_FIRST if i == 0 else LOAD_PLAIN
        cin = C if i == 0 else lda
        kw = dict(a_amax=amax[0], a_amax2=amax[1], floor=amax[2], lda=lda, a_L=L)
        if last and K:
            out = torch.zeros((B, layer.cout, M), dtype=torch.float32, device=dev)   # merged by atomicMax
            _launch(layer, prec, relu, loader, EPI_MAX_CHANNEL_FIRST, P, cin, cur, out, L, M=M, K=K, **kw)
        elif last:
            out = torch.empty((B, layer.cout) + spatial, dtype=torch.float32, device=dev)
            _launch(layer, prec, relu, loader, EPI_CHANNEL_FIRST, P, cin, cur, out, L, cf_N=L, **kw)
        else:
            ldc = (layer.cout + 3) // 4 * 4     # the next PLAIN loader reads 4-channel chunks: zero pad columns
            out = (torch.zeros if ldc != layer.cout else torch.empty)((P, ldc), dtype=torch.float32, device=dev)
            out_amax = _slots(B, dev) if h2 else None
            _launch(layer, prec, relu, loader, EPI_STORE, P, cin, cur, out, L, out_amax=out_amax, ldc=ldc, **kw)
            amax, lda = (out_amax, None, 0.0), ldc
        cur = out
    return cur


def _mlp_forward(self, x):
    base = type(self)._s4g_base
    st = self.__dict__.get("_s4g")
    if st is None or x.dim() < 3 or x.shape[1] != self[0].conv.in_channels or not _fast(self, x):
        return base.forward(self, x)
    return _chain(self, st, x)


def _is_edge(sa):
    """An edge SA module by structure: its grouper's forward takes the centroids' features (reference modules.py:70)."""
    g = getattr(sa, "grouper", None)
    return g is not None and "centroid_feature" in inspect.signature(type(g).forward).parameters


def _sa_forward(self, xyz, feature=None):
    base = type(self)._s4g_base
    st = self.__dict__.get("_s4g")
    if st is None or not _fast(self, xyz, feature):
        return base.forward(self, xyz, feature)
    edge = _is_edge(self) and feature is not None and self.num_centroids != 0
    new_xyz, group = (edge_sample_and_group if _is_edge(self) else sample_and_group)(self, xyz, feature)
    if group.shape[1] != self.mlp[0].conv.in_channels:
        return base.forward(self, xyz, feature)
    B, _, M, K = group.shape
    bound = None
    if st.precision == "f16x2":
        # |A| per scene: the source features, and for the xyz columns the ball radius (centred coordinates) or,
        # grouping all points, the coordinates themselves -- the grouped tensor is not reduced a second time
        a = _amax(feature.contiguous(), B) if feature is not None else None
        if edge:
            # |f_j| <= a and |f_j - f_c| <= 2 a: this loader JOINS its bounds by the maximum, so the feature columns'
            # bound is 2 a (an exact doubling of the slots on the device)
            a = a.view(torch.float32) * 2.0
        a2, floor = None, 0.0
        if self.use_xyz:
            if self.num_centroids == 0:
                a2 = _amax(xyz.contiguous(), B)
            else:
                floor = float(self.grouper.radius)
        if a is not None or a2 is not None or floor > 0.0:
            bound = (a, a2, floor)
    return new_xyz, _chain(self.mlp, st, group, bound, M=M, K=K)


_SUBCLASSES = {}


def _convert(m, forward, precision):
    base = getattr(type(m), "_s4g_base", type(m))
    key = (base, forward)
    sub = _SUBCLASSES.get(key)
    if sub is None:
        sub = _SUBCLASSES[key] = type("Accelerated" + base.__name__, (base,),
                                      {"forward": forward, "_s4g_base": base, "__module__": base.__module__})
    m.__class__ = sub
    m._s4g = _State(precision)


def accelerate(net, precision="f16x2"):
    """Convert in place every SharedMLP-shaped and SA-module-shaped module of `net` (see the module docstring) and
    return their qualified names.  precision: "f16x2" (default; two scaled fp16 planes per operand, three products,
    fp32 accumulate: fp32-class, as in `FusedPointNet2`) or "fp32" (fp32-input MFMA).  Call it after `net.eval()`
    and run inference under `torch.no_grad()` / `torch.inference_mode()`: with autograd live, in train mode, on the
    CPU or in float64 the original forwards run.  The MLP inside a converted SA module is run by the SA module and
    is not listed on its own."""
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, not %r" % (sorted(PRECISIONS), precision))
    names, owned = [], []
    for name, m in net.named_modules():
        if any(name.startswith(o + ".") for o in owned):
            continue
        if _is_sa(m):
            _convert(m, _sa_forward, precision)
        elif _is_shared_mlp(m):
            _convert(m, _mlp_forward, precision)
        else:
            continue
        names.append(name)
        owned.append(name)
    return names
