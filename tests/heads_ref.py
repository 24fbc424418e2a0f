"""What the heads-kernel tests share (s4g_heads_chain_f32, csrc/mlp_heads.hip): the layer builder, the descriptor
filler, the float64 restatement of PointNet2_tcls.py:83-95,126-140 (optionally rounded to bf16 at the layer inputs), the
feature-propagation tail in front of the heads (PRE) with its reference, the per-tile error scale, guarded output
buffers and the input sets of tests/test_heads_edges_gpu.py -- which tests/test_heads_ref.py proves discriminating on
the CPU.  Everything is built on the CPU generator, so a CPU test sees the very tensors a GPU test uploads."""
import ctypes

import torch

CH = (3, 9, 4, 5)
MAGS = (1.0, 40.0, 0.02)              # per-scene magnitudes of X, cycled over the scenes
PRE_MAGS = (1.0, 25.0, 0.05)          # ... of the sparse features in front of the tail
# bf16 is compared with a restatement ROUNDED at the same points, and that yardstick is only as steady as its rounding
# decisions: noise of 1e-7 (below fp32 round-off) on the hidden layers moves it by 1e-3 .. 3e-3 of scale at unit
# magnitude -- and by 5e-3 .. 1.5e-2 on the sigmoid head of a 40 x scene, whose logits grow with X while its scale
# stays 1 (one flipped bf16 ulp of a hidden value ~100 moves a logit by ~0.015).  The bf16 bounds (3e-3 / 6e-3 max)
# are the project's for unit-magnitude X (tests/test_heads_gpu.py), so the bf16 cases keep every scene of X at or below
# 1 and the tail's sparse features within 4 (a dense addend of 1; smaller features let permuted neighbour weights pass
# at 84 x).  Measured with 1 / 40 / 0.02 in bf16: sigmoid head 3.76e-3 at (B, N) = (3, 63) and 6.46e-3 with 32 channels
# at (2, 100) against 3e-3; with the tail at 1 / 25 sparse features and a dense addend of 2, head 0 6.39e-3 against 6e-3;
# every mean 10 x inside its bound, every f16x2 case and every guard / bit-identity check passing.
BF16_MAGS = (1.0, 0.25, 0.02)
BF16_PRE_MAGS = (4.0, 1.0, 0.25)
TILE = {3: 64, 2: 128}                # rows a workgroup owns: f16x2 (S4G_GEMM_F16X2 = 3), bf16 (S4G_GEMM_BF16 = 2)
# the project's bounds (tests/test_heads_gpu.py): f16x2 against float64, (max,); bf16 against the reference rounded at
# the same points, (max, mean); each without / with the tail in front
BOUND = {(3, False): (2e-5,), (3, True): (3e-5,), (2, False): (3e-3, 5e-5), (2, True): (6e-3, 1e-4)}
SENTINEL_BITS = 0x7FC0BEEF            # a quiet NaN no kernel produces: "not finite" and "bit pattern intact" both test it

f64 = lambda t: t.double()                            # noqa: E731
bf16 = lambda t: t.to(torch.bfloat16).double()        # noqa: E731


def x_mags(precision):
    return BF16_MAGS if precision == 2 else MAGS


def pre_mags(precision):
    return BF16_PRE_MAGS if precision == 2 else PRE_MAGS


def pre_dense_mag(precision):
    return 1.0 if precision == 2 else PRE_DENSE_MAG


def _cycle(mags, B):
    return torch.tensor([mags[i % len(mags)] for i in range(B)])


# ---------------------------------------------------------------------------------------------------------- layers

def make_weights(seed, ch=CH):
    """The five layers' fp32 weights and biases on the CPU: heads.0 (2048, 256) stacked over the heads, heads.1 .. 3
    and the logits grouped by head (the logits padded to 32 channels with zeros)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    W0 = r(2048, 256) / 16
    W1 = r(4, 256, 512) / 512 ** 0.5
    W2 = r(4, 256, 256) / 16
    W3 = r(4, 128, 256) / 16
    WL = torch.zeros(4, 32, 128)
    bL = torch.zeros(4, 32)
    for h, c in enumerate(ch):
        WL[h, :c] = r(c, 128) / 128 ** 0.5
        bL[h, :c] = r(c)
    b = [r(2048), r(4, 256), r(4, 256), r(4, 128), bL]
    return [W0, W1, W2, W3, WL], b


def pack_layers(Ws, b, dev):
    """(Ws, b, layers) on `dev`: the tensors of make_weights and their packed `_Layer`s (fragment order, both forms)."""
    from s4g_release_amd.fused import _Layer
    Ws = [w.to(dev) for w in Ws]
    b = [x.to(dev) for x in b]
    layers = [_Layer(Ws[0], b[0], 256)] + [_Layer(Ws[i], b[i], Ws[i].shape[-1], groups=4) for i in range(1, 5)]
    return Ws, b, layers


def build_layers(dev, seed, ch=CH):
    return pack_layers(*make_weights(seed, ch), dev)


def with_bias(b, layers, l, new_bias):
    """The layer set with layer l's bias replaced (biases are not packed: the fragments are shared)."""
    import copy
    b, layers = list(b), list(layers)
    b[l] = new_bias.contiguous()
    layers[l] = copy.copy(layers[l])
    layers[l].bias = b[l]
    return b, layers


def with_logits(Ws, b, layers, ch, seed):
    """The layer set with another logits layer (channel counts `ch`, up to 32 per head); the rest is shared."""
    from s4g_release_amd.fused import _Layer
    dev = Ws[0].device
    g = torch.Generator(device="cpu").manual_seed(seed)
    WL = torch.zeros(4, 32, 128)
    bL = torch.zeros(4, 32)
    for h, c in enumerate(ch):
        WL[h, :c] = torch.randn(c, 128, generator=g) / 128 ** 0.5
        bL[h, :c] = torch.randn(c, generator=g)
    Ws, b, layers = list(Ws), list(b), list(layers)
    Ws[4], b[4] = WL.to(dev), bL.to(dev)
    layers[4] = _Layer(Ws[4], b[4], 128, groups=4)
    return Ws, b, layers


# ------------------------------------------------------------------------------------------------------- the launch

def fill_desc(d, layers, precision, pre_layers=None):
    """Widths and the weight / bias / scale pointers of the five layers (and of the tail's two)."""
    d.precision = precision
    d.C, d.H0, d.H1, d.H2, d.H3 = 256, 512, 256, 256, 128
    pick = (lambda l: l.Wfrag_bf16) if precision == 2 else (lambda l: l.Wfrag)
    for l, layer in enumerate(layers):
        d.W_frag[l], d.bias[l], d.w_inv_scale[l] = pick(layer).data_ptr(), layer.bias.data_ptr(), layer.w_inv_scale.data_ptr()
    for l, layer in enumerate(pre_layers or ()):
        d.pre_W_frag[l], d.pre_bias[l] = pick(layer).data_ptr(), layer.bias.data_ptr()
        d.pre_w_inv_scale[l] = layer.w_inv_scale.data_ptr()


def launch(dev, layers, X, B, N, precision, amax=None, floor=0.0, *, outs, ch=CH, sigmoid_head=3, head_mask=0,
           out_batch_stride=0, ldx=None, rows_per_scene=None, pre=None, P=None, x_ptr=None):
    """One s4g_heads_chain_f32 call; returns its status.  X (rows, ldx) fp32 or None with `pre`; outs[h] a tensor whose
    first element is scene 0 / channel 0 / point 0 of head h, or None (a NULL pointer); pre = pre_setup's tuple + (N2,).
    amax: (scenes, 64) slot rows of X (PRE: of the sparse features; the dense addend's are derived here)."""
    from s4g_release_amd import _cabi
    d = _cabi.HeadsDesc()
    keep = []
    fill_desc(d, layers, precision, None if pre is None else pre[5])
    d.P, d.N = (B * N if P is None else P), N
    if pre is None:
        d.X = X.data_ptr() if x_ptr is None else x_ptr
        d.ldx = X.shape[1] if ldx is None else ldx
    else:
        S, nidx, nw, dense, lbias, _, N2 = pre
        d.pre_nidx, d.pre_nw, d.pre_sparse, d.pre_N2 = nidx.data_ptr(), nw.data_ptr(), S.data_ptr(), N2
        d.pre_dense = None if dense is None else dense.data_ptr()
        d.pre_lbias = lbias.data_ptr()
        if amax is None:
            amax = torch.zeros((B, 64), device=dev)
            amax[:, 9] = S.view(B, -1).abs().amax(dim=1)
            if rows_per_scene == 0:
                amax = amax.amax(dim=0, keepdim=True).contiguous()
        if dense is not None:
            amax2 = torch.zeros((B, 64), device=dev)
            amax2[:, 1] = dense.view(B, -1).abs().amax(dim=1)
            if rows_per_scene == 0:
                amax2 = amax2.amax(dim=0, keepdim=True).contiguous()
            d.pre_a_amax2 = amax2.data_ptr()
            keep.append(amax2)
        floor = float(lbias.abs().max())
    d.a_amax = None if amax is None else amax.data_ptr()
    d.a_amax_floor = floor
    d.rows_per_scene = N if rows_per_scene is None else rows_per_scene
    for h in range(4):
        d.out[h] = None if outs[h] is None else outs[h].data_ptr()
        d.channels[h] = ch[h]
    d.sigmoid_head, d.head_mask, d.out_batch_stride = sigmoid_head, head_mask, out_batch_stride
    rc = _cabi.lib().s4g_heads_chain_f32(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    return rc


def run(dev, layers, X, B, N, precision, amax=None, floor=0.0, *, outs=None, ch=CH, **kw):
    """launch() that must succeed; without `outs` the four (B, c, N) tensors are made here, NaN-filled."""
    from s4g_release_amd import _cabi
    if outs is None:
        outs = [torch.full((B, c, N), float("nan"), device=dev) for c in ch]
    _cabi.check(launch(dev, layers, X, B, N, precision, amax, floor, outs=outs, ch=ch, **kw), "heads")
    return outs


# --------------------------------------------------------------------------------------------------- the yardsticks

def _act(rnd):
    """A hidden layer's values as the next layer reads them: float64 stays float64 (the yardstick rounds nowhere); a
    rounded form rounds the fp32 value the kernel holds."""
    return rnd if rnd is f64 else (lambda y: rnd(y.float()))


def reference(Ws, b, X, B, N, rnd=f64, ch=CH, sigmoid_head=3, rowmap=None):
    """The layers restated in float64: per head relu(W x + b) four times, the logits, the sigmoid on one head; `rnd`
    rounds every layer's inputs (weights and activations; biases are added in fp32 by the kernel).  rowmap (P,) long:
    output row r takes the value computed for row rowmap[r] (only the sabotage tests pass one)."""
    outs = []
    x = rnd(X)
    act = _act(rnd)
    for h, c in enumerate(ch):
        y = (x @ rnd(Ws[0][h * 512:(h + 1) * 512]).t() + b[0][h * 512:(h + 1) * 512].double()).clamp_min(0)
        for l in (1, 2, 3):
            y = (act(y) @ rnd(Ws[l][h]).t() + b[l][h].double()).clamp_min(0)
        o = act(y) @ rnd(Ws[4][h, :c]).t() + b[4][h, :c].double()
        if h == sigmoid_head:
            o = torch.sigmoid(o)
        if rowmap is not None:
            o = o[rowmap]
        outs.append(o.view(B, N, c).permute(0, 2, 1))
    return outs


def pre_setup(dev, B, N, N2, seed, with_dense, dense_mag=0.5, mags=PRE_MAGS):
    """Inputs of the feature-propagation tail in front of the heads (s4g_heads_desc_t.pre_*):
    sparse features (B N2, 256), three neighbour indices + weights per point, an optional dense
    addend, the first layer's bias, and the two 256 -> 256 layers."""
    from s4g_release_amd.fused import _Layer
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    S = (r(B * N2, 256) * _cycle(mags, B)[:, None].repeat_interleave(N2, dim=0)).to(dev)
    nidx = torch.randint(0, N2, (B * N, 3), generator=g, dtype=torch.int32).to(dev)
    w = torch.rand(B * N, 3, generator=g)
    nw = (w / w.sum(dim=1, keepdim=True)).to(dev)
    dense = (r(B * N, 256) * dense_mag).to(dev) if with_dense else None
    lbias = r(256).to(dev)
    pl = [_Layer((r(256, 256) / 16).to(dev), r(256).to(dev), 256) for _ in range(2)]
    return S, nidx, nw, dense, lbias, pl


def pre_reference(S, nidx, nw, dense, lbias, pl, B, N, N2, rnd=f64, scene_of_row=None):
    """X as the tail produces it: relu(sum_k w_k S[idx_k] (+ dense) + bias), then the two layers.  scene_of_row (P,):
    the scene whose sparse rows a position reads (only the sabotage tests pass one)."""
    scene = torch.arange(B, device=S.device).repeat_interleave(N) if scene_of_row is None else scene_of_row
    base = (scene * N2).view(-1, 1)
    rows = S.double()[(base + nidx.long())]                       # (P, 3, 256)
    x = (rows * nw.double().unsqueeze(-1)).sum(dim=1) + lbias.double()
    if dense is not None:
        x = x + dense.double()
    x = x.clamp_min(0)
    for layer in pl:
        w = layer.W[0] if layer.W.dim() == 3 else layer.W
        x = (_act(rnd)(x) @ rnd(w).t() + layer.bias.double()).clamp_min(0)
    return x if rnd is f64 else x.float()


def tile_scale(ref_h, B, N, tile):
    """(B, 1, N): per row, max(1, max |ref|) of this head over every scene with a row in the row's workgroup tile --
    the f16x2 form scales a tile by the largest a_amax among the scenes it touches.  Per scene where tile | N."""
    P = B * N
    smax = ref_h.abs().amax(dim=(1, 2)).clamp_min(1.0)
    rows = torch.arange(P, device=ref_h.device)
    t = rows // tile
    tmax = torch.zeros(int(t[-1]) + 1, dtype=smax.dtype, device=ref_h.device)
    tmax = tmax.scatter_reduce(0, t, smax[rows // N], "amax", include_self=True)
    return tmax[t].view(B, 1, N)


def rel_err(out_h, ref_h, B, N, tile):
    """|out - ref| / tile_scale, (B, c, N) float64."""
    return (out_h.double() - ref_h).abs() / tile_scale(ref_h, B, N, tile)


def per_block(err, B, N):
    """Worst error of each 32-row block of the launch ((B, c, N) -> list over blocks of 32 positions)."""
    flat = err.permute(0, 2, 1).reshape(B * N, -1).amax(dim=1)
    return [float(flat[i:i + 32].max()) for i in range(0, B * N, 32)]


# ------------------------------------------------------------------------------------------------- guarded outputs

class GuardedOuts:
    """The output tensors of one call carved out of ONE sentinel-filled buffer, >= 256 guard floats before and after
    each tensor and -- wherever the layout has a batch stride -- between scenes.  Layouts:
      "plain"    four contiguous (B, c, N) tensors, out_batch_stride 0
      "strided"  four tensors sharing the batch stride max(c) N + 256 (a gap after every scene of every head)
      "packed"   one (B, sum c, N) tensor, heads as channel slices, out_batch_stride = sum(c) N (+ `gap`)"""
    GUARD = 256

    def __init__(self, dev, B, N, ch=CH, layout="plain", gap=0, null=()):
        G = self.GUARD
        self.B, self.N, self.ch, self.null = B, N, tuple(ch), tuple(null)
        if layout == "plain":
            self.stride = [c * N for c in ch]
            self.obs = 0
            span = [max(B, 1) * c * N for c in ch]
        elif layout == "strided":
            s = max(ch) * N + G
            self.stride, self.obs = [s] * 4, s
            span = [max(B, 1) * s] * 4
        else:
            s = sum(ch) * N + gap
            self.stride, self.obs = [s] * 4, s
            span = None
        if span is not None:
            self.off, o = [], G
            for h in range(4):
                self.off.append(o)
                o += span[h] + G
            total = o
        else:
            self.off = [G + sum(ch[:h]) * N for h in range(4)]
            total = G + max(B, 1) * s + G
        self.buf = torch.full((total,), SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)
        self.outs = [None if h in self.null else self.buf[self.off[h]:] for h in range(4)]

    def head(self, h):
        """(B, c, N) view of head h."""
        return self.buf.as_strided((self.B, self.ch[h], self.N), (self.stride[h], self.N, 1), self.off[h])

    def check(self, written_heads, P=None):
        """Every row < P of the written heads is finite; every other word of the buffer still holds the sentinel."""
        P = self.B * self.N if P is None else P
        bits = self.buf.view(torch.int32)
        expect = torch.ones_like(bits, dtype=torch.bool)           # True: must still be the sentinel
        for h in written_heads:
            assert h not in self.null
            m = expect.as_strided((self.B, self.ch[h], self.N), (self.stride[h], self.N, 1), self.off[h])
            live = (torch.arange(self.B * self.N, device=bits.device) < P).view(self.B, 1, self.N)
            m[live.expand(-1, self.ch[h], -1)] = False
            assert torch.isfinite(self.head(h)[live.expand(-1, self.ch[h], -1)]).all(), "head %d: a row below P is not finite" % h
        stray = (bits != SENTINEL_BITS) & expect
        assert not stray.any(), "written outside the outputs at word(s) %s" % stray.nonzero().flatten()[:8].tolist()

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENTINEL_BITS).all())


# ------------------------------------------------------------------------------------------------------- input sets

LAYER_SEED = 1234                         # the one layer set of tests/test_heads_edges_gpu.py
SCENE_SHAPES = [(130, 1), (19, 7), (7, 20), (3, 63), (3, 65), (5, 33)]      # (B, N): scenes inside a tile
PRE_SCENE_SHAPES = [(19, 7), (3, 65)]                                        # ... the two that also run with the tail


def x_seed(B, N):
    return 1000 * B + N


PRE_DENSE_MAG = 2.0        # the dense addend of the edge tests (0.5 went unnoticed next to a 25 x scene: 93 x the bf16 bound)


def pre_seed(B, N, N2):
    return 7 + 1000 * B + 10 * N + N2


def make_x(B, N, seed, mags=MAGS):
    """X (B N, 256) on the CPU, scene s scaled by mags[s mod len], and its true per-scene maxima as (B, 64) slot rows."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn(B * N, 256, generator=g) * _cycle(mags, B)[:, None].repeat_interleave(N, dim=0)
    amax = torch.zeros((B, 64))
    if B:
        amax[:, 5] = X.view(B, -1).abs().amax(dim=1)
    return X, amax


def straddle_rowmap(B, N, tile):
    """Sabotage: rows of a tile that straddles scenes, beyond the tile's first scene, take scene - 1 (row - N)."""
    rows = torch.arange(B * N)
    first_scene = (rows // tile * tile) // N
    return torch.where(rows // N != first_scene, rows - N, rows)


def swap_rowmap(P, tile, half):
    """Sabotage: within every `tile` rows, rows [0, half) and [half, 2 half) exchanged (where both exist)."""
    rows = torch.arange(P)
    r = rows % tile
    m = torch.where(r < half, rows + half, torch.where(r < 2 * half, rows - half, rows))
    return torch.where(m < P, m, rows)
