"""What the chain-kernel tests share (mlp_chain_kernel behind s4g_mlp_gemm_f32, csrc/mlp_gemm.hip): problem builders for
every loader the chain has (PLAIN, GATHER_MLP1 on gidx, GATHER_MLP1 on rel_xyz4, GATHER_ADD, INTERP_ADD), both precisions,
two- and three-layer chains; the float64 restatement of the layers (`nn_utils/conv.py:24-34,64-74` stacks, the max over
neighbours of `pointnet2_utils/modules.py:242-243`), optionally rounded to bf16 where the bf16 form rounds (inputs,
weights, every hidden activation); the kernel's geometry; the per-tile error scale; guarded output buffers; and the
sabotage transforms tests/test_chain_ref.py proves the GPU tests' inputs discriminating with.  Everything is built on
the CPU generator, so a CPU test sees the very tensors a GPU test uploads."""
import ctypes
import functools
import types

import torch

from tests.heads_ref import BF16_MAGS, MAGS, SENTINEL_BITS

F16X2, BF16 = 3, 2                    # S4G_GEMM_F16X2, S4G_GEMM_BF16
PLAIN, GIDX, REL4, GADD, IADD = "plain", "gidx", "rel4", "gadd", "iadd"
LOADER_CODE = {PLAIN: 0, GIDX: 3, REL4: 3, GADD: 4, IADD: 5}
STORE, MAX = 0, 1
KN = 64                               # neighbours per centroid of the chain's max epilogue
# rows a workgroup owns (the kernel's header comment: RW = 2 / 1 / 8, two 32-row blocks per wave in the f16x2 form, four
# in the single-plane form) and the final layer's channels per strip (64 per wave column: 2, 4 and 8 of them)
TILE = {(F16X2, 128): 128, (F16X2, 256): 64, (F16X2, 512): 64, (BF16, 128): 256, (BF16, 256): 128, (BF16, 512): 128}
STRIP = {128: 128, 256: 256, 512: 512}
WAVE_ROWS = {F16X2: 64, BF16: 128}
NPTS = 50                             # points per scene the gathering loaders index

f64 = lambda t: t.double()                            # noqa: E731
bf16 = lambda t: t.to(torch.bfloat16).double()        # noqa: E731


def mags(precision):
    """Per-scene magnitudes: 1 / 40 / 0.02, and 1 / 0.25 / 0.02 for bf16 (tests/heads_ref.py, BF16_MAGS: the rounded
    yardstick is only steady at or below unit magnitude)."""
    return BF16_MAGS if precision == BF16 else MAGS


def bounds(precision, layers, deep=False, mlp1=False):
    """The project's bounds (tests/test_fused_gpu.py, tests/test_bf16_chain_gpu.py), as fractions of the row's tile scale.
    f16x2: {"max"} against float64.  bf16: {"max", "mean"} against the restatement rounded at the same points and
    {"exact"} (max) against un-rounded float64."""
    if precision == F16X2:
        return {"max": 4e-5 if (layers == 3 or deep) else 3e-5}
    return {"max": 2e-3, "mean": 3e-5 if mlp1 else 2e-5, "exact": 5e-2}


# ----------------------------------------------------------------------------------------------------------- problems

def _scene_col(m, B, rows_per_scene):
    return torch.tensor([m[i % len(m)] for i in range(B)]).repeat_interleave(rows_per_scene)[:, None]


def make_problem(loader, precision, C, widths, epi, B, n, *, groups=1, K1=None, relus=None, N2=40, dense=True, seed=0,
                 scene_mags=None, bias_mag=1.0):
    """One launch's tensors on the CPU.  widths: the layers behind the first ([Cout2] or [C, Cout3]).  n: rows per scene
    (STORE) or centroids per scene (MAX, 64 rows each).  K1: the first layer's depth (PLAIN: C, 2 C or 4 C)."""
    K1 = C if K1 is None else K1
    g = torch.Generator(device="cpu").manual_seed(1000003 * seed + 7919 * C + 31 * sum(widths) + 7 * B + n + groups)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    pr = types.SimpleNamespace(loader=loader, precision=precision, C=C, widths=list(widths), epi=epi, B=B, n=n,
                               groups=groups, K1=K1, N2=N2, tile=TILE.get((precision, C), 64))
    pr.relus = tuple(relus) if relus is not None else (1,) * (1 + len(widths))
    pr.rps = n * KN if epi == MAX else n              # rows per scene
    pr.P = B * pr.rps
    pr.out_rows = B * n
    pr.coutF = widths[-1]
    m = mags(precision) if scene_mags is None else scene_mags
    ins, outs = [K1] + [C] * len(widths), [C] + list(widths)
    pr.Ws = [r(groups, o, i) / i ** 0.5 for o, i in zip(outs, ins)]
    pr.bs = [r(groups, o) * bias_mag for o in outs]
    col = _scene_col(m, B, pr.rps)
    pr.amax = pr.amax2 = None
    pr.floor = 0.0
    if loader == PLAIN:
        pr.A = r(pr.P, groups * K1) * col
        pr.amax = _slots(pr.A, B, 5)
    elif loader in (GIDX, REL4, GADD):
        assert epi == MAX and groups == 1
        cmag = torch.tensor([m[i % len(m)] for i in range(B)])[:, None, None] if loader != GADD else 1.0
        pr.xyz = torch.rand(B, 3, NPTS, generator=g) * 0.2 * cmag
        cidx = torch.randint(0, NPTS, (B, n), generator=g)
        pr.ctr = torch.stack([pr.xyz[b][:, cidx[b]] for b in range(B)]).contiguous()
        pr.gidx = torch.randint(0, NPTS, (B, n, KN), generator=g).int()
        rel = torch.stack([pr.xyz[b][:, pr.gidx[b].long()] - pr.ctr[b][:, :, None] for b in range(B)])    # fp32, one rounding
        pr.rel = rel.permute(0, 2, 3, 1).reshape(pr.P, 3).contiguous()
        pr.rel4 = torch.cat([pr.rel, torch.zeros(pr.P, 1)], dim=1).contiguous()
        pr.w1 = r(C, 4)
        relmax = float(pr.rel.abs().max()) if pr.P else 0.0
        pr.floor = float((pr.w1[:, :3].abs().sum(1) * max(relmax, 1e-30) + pr.w1[:, 3].abs()).max())
        if loader == GADD:
            pr.F = r(B * NPTS, C) * _scene_col(m, B, NPTS)
            pr.amax = _slots(pr.F, B, 17)
    elif loader == IADD:
        assert epi == STORE and groups == 1
        pr.S = r(B * N2, C) * _scene_col(m, B, N2)
        pr.dense = r(pr.P, C) * col if dense else None
        pr.lbias = r(C)
        pr.nidx = torch.randint(0, N2, (B, n, 3), generator=g).int()
        w = torch.rand(B, n, 3, generator=g)
        pr.nw = (w / w.sum(dim=2, keepdim=True)).contiguous()
        pr.amax = _slots(pr.S, B, 9)
        pr.amax2 = _slots(pr.dense, B, 1) if dense else None
        pr.floor = float(pr.lbias.abs().max())
    else:
        raise ValueError(loader)
    return pr


def _slots(x, B, slot):
    """(B, 64) slot rows holding the true per-scene maxima of x (rows [scene][...]); the slot position is arbitrary."""
    row = torch.zeros(max(B, 1), 64)
    if B and x.numel():
        row[:B, slot] = x.reshape(B, -1).abs().amax(dim=1)
    return row


def loader_rows(pr, exact=True, no_xyz=False):
    """The first layer's input rows (P, groups K1) as the loader forms them: float64 from the fp32 inputs, or (exact =
    False) in fp32 like the loader itself (fma order aside) -- what the bf16 form then rounds."""
    t = (lambda x: x.double()) if exact else (lambda x: x)
    if pr.loader == PLAIN:
        return t(pr.A)
    if pr.loader in (GIDX, REL4, GADD):
        a = t(pr.w1[:, 3]).expand(pr.P, -1)
        if not no_xyz:
            a = a + t(pr.rel) @ t(pr.w1[:, :3]).t()
        if pr.loader == GADD:
            rows = torch.cat([pr.F.view(pr.B, NPTS, pr.C)[b][pr.gidx[b].long().reshape(-1)] for b in range(pr.B)])
            a = a + t(rows)
        return a.clamp_min(0)
    rows = torch.stack([pr.S.view(pr.B, pr.N2, pr.C)[b][pr.nidx[b].long()] for b in range(pr.B)])       # (B, n, 3, C)
    a = (t(rows) * t(pr.nw)[..., None]).sum(dim=2).view(pr.P, pr.C)
    if pr.dense is not None:
        a = a + t(pr.dense)
    return (a + t(pr.lbias)).clamp_min(0)


def chain(A, Ws, bs, relus, groups=1, rnd=f64, K=0, group_shift=0, final_bias=None, k_rows=None):
    """The layers restated in float64: per group act_l(W_l x + b_l), the groups side by side, then (K > 0) the maximum
    over every K consecutive rows.  `rnd` rounds each layer's inputs (weights and activations; the kernel adds the
    biases in fp32 and the bf16 form rounds the fp32 value it holds).  Sabotage only: group_shift (group g takes group
    g + shift's weights), final_bias (another bias for the last layer), k_rows (the maximum over the first k_rows of K)."""
    K1 = Ws[0].shape[-1]
    act = rnd if rnd is f64 else (lambda y: rnd(y.float()))
    cols = []
    for gi in range(groups):
        h = A[:, gi * K1:(gi + 1) * K1]
        gw = (gi + group_shift) % groups
        for l, (W, b) in enumerate(zip(Ws, bs)):
            bias = final_bias[gi] if (final_bias is not None and l == len(Ws) - 1) else b[gi]
            h = act(h) @ rnd(W[gw]).t() + bias.double()
            if relus[l]:
                h = h.clamp_min(0)
        cols.append(h)
    o = torch.cat(cols, dim=1)
    if K:
        o = o.view(-1, K, o.shape[1])[:, :(K if k_rows is None else k_rows)].amax(dim=1)
    return o


def reference(pr, rounded=False, **sab):
    """The launch's expected output (out_rows, groups coutF), float64.  rounded: the bf16 yardstick."""
    no_xyz = sab.pop("no_xyz", False)
    relus = sab.pop("relus", pr.relus)
    A = sab.pop("A", None)
    if A is None:
        A = loader_rows(pr, exact=not rounded, no_xyz=no_xyz)
    return chain(A, pr.Ws, pr.bs, relus, pr.groups, bf16 if rounded else f64, KN if pr.epi == MAX else 0, **sab)


def pad_row_value(pr):
    """max |out| of a row past P: the loaders hand such a row over as zeros, so it carries the activated biases."""
    if pr.P % pr.tile == 0:
        return 0.0
    z = torch.zeros(1, pr.groups * pr.K1, dtype=torch.float64)
    return float(chain(z, pr.Ws, pr.bs, pr.relus, pr.groups).abs().max())


# --------------------------------------------------------------------------------------------------------- error scale

def row_geometry(pr):
    """(scene, tile) of every output row: a STORE row is its own loader row, a MAX row stands for 64 of them."""
    rows = torch.arange(pr.out_rows) * (KN if pr.epi == MAX else 1)
    return rows // max(pr.rps, 1), rows // pr.tile


def tile_scale(ref, scene, tile, groups=1):
    """(rows, groups, 1): per row and group, max(1, max |ref|) over every scene with a row in the row's workgroup tile --
    the f16x2 form scales a tile by the largest a_amax among the scenes it touches (tests/heads_ref.tile_scale)."""
    rows = ref.shape[0]
    r3 = ref.reshape(rows, groups, -1).abs().amax(dim=2)                       # (rows, groups)
    ns, nt = int(scene.max()) + 1, int(tile.max()) + 1
    smax = torch.zeros(ns, groups, dtype=ref.dtype).scatter_reduce(0, scene[:, None].expand(-1, groups), r3, "amax")
    smax = smax.clamp_min(1.0)
    tmax = torch.zeros(nt, groups, dtype=ref.dtype).scatter_reduce(0, tile[:, None].expand(-1, groups), smax[scene], "amax")
    return tmax[tile][:, :, None]


def rel_err(out, ref, pr):
    """|out - ref| / tile scale, (rows, groups coutF) float64; non-finite differences count as infinite."""
    if ref.shape[0] == 0:
        return torch.zeros_like(ref)
    scene, tile = row_geometry(pr)
    d = (out.double() - ref).abs().reshape(ref.shape[0], pr.groups, -1) / tile_scale(ref, scene, tile, pr.groups)
    return torch.nan_to_num(d, nan=float("inf")).reshape(ref.shape)


# ------------------------------------------------------------------------------------------------------ guarded output

class GuardedOut:
    """One launch's output carved out of a sentinel-filled buffer (tests/heads_ref.GuardedOuts' idea and sentinel):
    >= 256 guard floats before and behind, ldc = cout groups + 8 and c_coff = 4, so every row has sentinel columns on
    both sides.  zero_payload (the distinct-row MAX form merges with atomicMax into zeros, as its ABI requires): the
    rows x ldc payload is zero-filled, the guards stay sentinels."""
    GUARD = 256

    def __init__(self, dev, rows, cout, groups=1, zero_payload=False):
        G = self.GUARD
        self.rows, self.cout, self.groups, self.zero = rows, cout, groups, zero_payload
        self.ldc, self.c_coff, self.c_gcol = cout * groups + 8, 4, cout
        self.n = rows * self.ldc
        bits = torch.full((2 * G + self.n,), SENTINEL_BITS, dtype=torch.int32, device=dev)
        if zero_payload:
            bits[G:G + self.n] = 0
        self.want = bits.clone()
        self.buf = bits.view(torch.float32)
        self.out = self.buf[G:]

    def values(self):
        """(rows, groups cout) view of the owed elements."""
        G = self.GUARD
        return self.buf[G:G + self.n].view(self.rows, self.ldc)[:, self.c_coff:self.c_coff + self.cout * self.groups]

    def check(self, rows_owed=None):
        """Every owed element is finite; every other word of the buffer still holds what it was filled with."""
        G = self.GUARD
        owed = self.rows if rows_owed is None else rows_owed
        bits = self.buf.view(torch.int32)
        free = torch.ones_like(bits, dtype=torch.bool)           # True: must be untouched
        free[G:G + self.n].view(self.rows, self.ldc)[:owed, self.c_coff:self.c_coff + self.cout * self.groups] = False
        stray = (bits != self.want) & free
        assert not stray.any(), "written outside the output at word(s) %s" % stray.nonzero().flatten()[:8].tolist()
        assert torch.isfinite(self.values()[:owed]).all(), "an owed element is not finite (never written?)"

    def untouched(self):
        return bool((self.buf.view(torch.int32) == self.want).all())


# ------------------------------------------------------------------------------------------------------------ launches

def f16x2_fields(w, *tensors, floor=0.0):
    """Descriptor fields of the f16x2 mode for a first layer (.., Cout, K): scaled fp16 planes of W (K padded to 16),
    per-channel inverse scales, the planes in fragment order where Cout allows it, one 64-slot amax row per input
    tensor (the slot position is arbitrary) and a zeroed out_amax row."""
    from s4g_release_amd.fused import fragment_order, split_f16x2
    k = w.shape[-1]
    kp = (k + 15) // 16 * 16
    w16 = w.new_zeros(w.shape[:-1] + (kp,))
    w16[..., :k] = w
    planes, inv = split_f16x2(w16)
    kw = dict(W_f16x2=planes, w_inv_scale=inv, a_amax_floor=float(floor), out_amax=torch.zeros(64, device=w.device))
    if w.shape[-2] % 32 == 0:     # enables the chain kernel's single-layer form where the shape qualifies
        kw["W_f16x2_frag"] = fragment_order(planes)
    for name, t in zip(("a_amax", "a_amax2"), [t for t in tensors if t is not None]):
        row = torch.zeros(64, device=w.device)
        row[17] = t.abs().max()
        kw[name] = row
    return kw


def f16x2_second(W2):
    """(W2_f16x2_frag, w2_inv_scale) of a layer fused behind the first (groups leading)."""
    from s4g_release_amd.fused import fragment_order, split_f16x2
    planes, inv = split_f16x2(W2.contiguous())
    return fragment_order(planes), inv


def bf16_frag(w):
    """(G, Cout, K16) or (Cout, K16) fp32 -> (the bf16 plane in fragment order, the bf16x3 planes)."""
    from s4g_release_amd.fused import fragment_order, split_bf16x3
    w3 = split_bf16x3(w)
    return fragment_order(w3[:1])[:, :, :, 0].contiguous(), w3


def _weights(pr, dev):
    """Descriptor fields of the layers for pr.precision; cached on the problem per device."""
    key = "_w_%s" % dev
    if hasattr(pr, key):
        return getattr(pr, key)
    from s4g_release_amd.fused import fragment_order, split_bf16x3, split_f16x2
    Ws = [w.to(dev) for w in pr.Ws]
    bs = [b.to(dev).contiguous() for b in pr.bs]
    kw = dict(W=Ws[0].contiguous(), bias=bs[0], bias2=bs[1], Cout2=pr.widths[0])
    names = [("W_f16x2_frag", "w_inv_scale"), ("W2_f16x2_frag", "w2_inv_scale"), ("W3_f16x2_frag", "w3_inv_scale")]
    if len(Ws) == 3:
        kw.update(bias3=bs[2], Cout3=pr.widths[1])
    for l, W in enumerate(Ws):
        if pr.precision == F16X2:
            planes, inv = split_f16x2(W.contiguous())
            kw[names[l][0]], kw[names[l][1]] = fragment_order(planes), inv
            if l == 0:
                kw["W_f16x2"] = planes
        else:
            w3 = split_bf16x3(W.contiguous())
            kw[names[l][0]] = fragment_order(w3[:1])[:, :, :, 0].contiguous()
            if l == 0:
                kw["W_bf16x3"] = w3
    setattr(pr, key, kw)
    return kw


def descriptor(pr, dev, out, ldc, c_coff, c_gcol, out_amax=None, **over):
    """The s4g_gemm_desc_t fields of the problem as a dict of ints / floats / device tensors."""
    C, K1, G = pr.C, pr.K1, pr.groups
    kw = dict(loader=LOADER_CODE[pr.loader], epilogue=pr.epi, groups=G, P=pr.P, Cin=K1 if pr.loader == PLAIN else C, Kpad=K1, Kpad16=K1, Cout=C,
              w_gstride=C * K1, b_gstride=C, out=out, ldc=ldc, c_coff=c_coff, c_gcol=c_gcol, precision=pr.precision,
              relu=pr.relus[0], relu2=pr.relus[1], K=KN, rows_per_scene=pr.rps, a_amax_floor=pr.floor)
    if len(pr.widths) == 2:
        kw["relu3"] = pr.relus[2]
    kw.update(_weights(pr, dev))
    up = lambda x: x.to(dev).contiguous()             # noqa: E731
    if pr.loader == PLAIN:
        kw.update(A=up(pr.A), lda=G * K1, a_gcol=K1)
    elif pr.loader == IADD:
        kw.update(nidx=up(pr.nidx), nw=up(pr.nw), sparse=up(pr.S), C2=C, N2=pr.N2, N1=pr.n, loader_bias=up(pr.lbias))
        if pr.dense is not None:
            kw["dense"] = up(pr.dense)
    else:
        kw.update(N=NPTS, M=pr.n, mlp1_w=up(pr.w1))
        if pr.loader == REL4:
            kw.update(rel_xyz4=up(pr.rel4), N=999)
        else:
            kw.update(gidx=up(pr.gidx), xyz=up(pr.xyz), ctr=up(pr.ctr))
        if pr.loader == GADD:
            kw.update(feat=up(pr.F), Cf=C)
    if pr.precision == F16X2:
        if pr.amax is not None:
            kw["a_amax"] = up(pr.amax)
        if pr.amax2 is not None:
            kw["a_amax2"] = up(pr.amax2)
        if out_amax is not None:
            kw["out_amax"] = out_amax
    kw.update(over)
    return kw


def call(kw):
    """One s4g_mlp_gemm_f32 call from a field dict; returns its status (tensors stay alive across the call)."""
    from s4g_release_amd import _cabi
    d = _cabi.GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = _cabi.lib().s4g_mlp_gemm_f32(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def launch(pr, dev, out_amax=None, zero_payload=False, **over):
    """(status, GuardedOut) of the problem's launch into a guarded buffer."""
    go = GuardedOut(dev, pr.out_rows, pr.coutF, pr.groups, zero_payload)
    rc = call(descriptor(pr, dev, go.out, go.ldc, go.c_coff, go.c_gcol, out_amax, **over))
    return rc, go


def compare(pr, out, what=""):
    """Position by position against the yardstick(s) of pr.precision; prints the worst error next to its bound and
    returns {name: (worst, bound)}.  `out`: (out_rows, groups coutF), any device."""
    out = out.detach().cpu()
    layers, deep = 1 + len(pr.widths), pr.K1 > pr.C
    bd = bounds(pr.precision, layers, deep, pr.loader in (GIDX, REL4, GADD))
    exact = reference_cached(pr, False)
    res = {}
    if pr.precision == F16X2:
        res["max"] = (float(rel_err(out, exact, pr).max()) if out.numel() else 0.0, bd["max"])
    else:
        e = rel_err(out, reference_cached(pr, True), pr)
        res["max"] = (float(e.max()) if out.numel() else 0.0, bd["max"])
        res["mean"] = (float(e.mean()) if out.numel() else 0.0, bd["mean"])
        res["exact"] = (float(rel_err(out, exact, pr).max()) if out.numel() else 0.0, bd["exact"])
    print("%s %s" % (what, "  ".join("%s %.3e / %.1e" % (k, v[0], v[1]) for k, v in res.items())))
    return res


def reference_cached(pr, rounded):
    key = "_ref_%d" % rounded
    if not hasattr(pr, key):
        setattr(pr, key, reference(pr, rounded))
    return getattr(pr, key)


@functools.lru_cache(maxsize=None)
def problem(loader, precision, C, widths, epi, B, n, groups=1, K1=None, relus=None, N2=40, dense=True, seed=0):
    """make_problem, one object per argument set: its references are computed once and shared."""
    return make_problem(loader, precision, C, list(widths), epi, B, n, groups=groups, K1=K1, relus=relus, N2=N2,
                        dense=dense, seed=seed)


# ---------------------------------------------------------------------------------------------------- distinct-row form

def seg_problem(precision, C, cout2, rps, seed=0):
    """Hand-built distinct-row layouts (seg4 / seg_rows, include/s4g_ops.h) on rel_xyz4: scenes of rps rows (rps / 64
    output rows each).  rps = 512: scene 0 compact in 256 rows -- centroids that continue across the half-wave (row 32),
    wave (64) and tile (128; 192) boundaries, filler in the middle of the run and at its end, two centroids no group
    names --, scene 1 in the plain layout (seg_rows == rps), scene 2 with seg_rows = 0, scene 3 compact again with
    other cuts.  rps = 256: a compact scene would need seg_rows < 256, so the scenes are plain / empty / plain.  Rows
    behind seg_rows hold NaN: the kernel must not read them.  (The single-plane form's 256-row tile at C = 128 has no
    tile boundary inside 256 rows: its waves' 128-row boundary is crossed instead.)"""
    M = rps // KN
    if rps == 512:
        B = 4
        cuts = {0: [(0, 0, 40), (1, 40, 80), (2, 80, 100), (-1, 100, 108), (3, 108, 140), (4, 140, 204), (5, 204, 232),
                    (-1, 232, 256)],
                3: [(7, 0, 28), (-1, 28, 36), (2, 36, 132), (0, 132, 136), (5, 136, 196), (6, 196, 256)]}
        seg_rows = [256, 512, 0, 256]
    else:
        B, cuts, seg_rows = 3, {}, [256, 0, 256]
    pr = make_problem(REL4, precision, C, [cout2], MAX, B, M, seed=100 + seed)
    seg4 = torch.full((pr.P // 4,), -1, dtype=torch.int32)
    owner = torch.full((pr.P,), -1, dtype=torch.long)            # output row of every loader row, -1: none
    for b in range(B):
        base = b * rps
        if seg_rows[b] == rps:
            owner[base:base + rps] = b * M + torch.arange(rps) // KN
        elif seg_rows[b]:
            for m, lo, hi in cuts[b]:
                owner[base + lo:base + hi] = -1 if m < 0 else b * M + m
                if m < 0:
                    pr.rel4[base + lo:base + hi] = 0.0
            pr.rel4[base + seg_rows[b]:base + rps] = float("nan")
        else:
            pr.rel4[base:base + rps] = float("nan")
        seg4[base // 4:(base + rps) // 4] = owner[base:base + rps:4].int()
    pr.rel = pr.rel4[:, :3].contiguous()
    pr.seg4, pr.seg_rows, pr.owner = seg4, torch.tensor(seg_rows, dtype=torch.int32), owner
    return pr


def seg_reference(pr, rounded=False):
    """Per output row the maximum over ITS rows of the final activations; rows no group names stay 0."""
    live = pr.owner >= 0
    rel = torch.where(live[:, None], pr.rel, torch.zeros_like(pr.rel))
    t = (lambda x: x.double()) if not rounded else (lambda x: x)
    A = (t(rel) @ t(pr.w1[:, :3]).t() + t(pr.w1[:, 3])).clamp_min(0)
    rows = chain(A, pr.Ws, pr.bs, pr.relus, 1, bf16 if rounded else f64)
    out = torch.zeros(pr.out_rows, pr.coutF, dtype=torch.float64)
    idx = pr.owner[live][:, None].expand(-1, pr.coutF)
    return out.scatter_reduce(0, idx, rows[live], "amax", include_self=True)


# ------------------------------------------------------------------------------------------------------------ sabotage

def swap_row_blocks(ref, wave_rows=64, block=32):
    """Two 32-row blocks of every wave exchanged (where both exist)."""
    P = ref.shape[0]
    rows = torch.arange(P)
    r = rows % wave_rows
    m = torch.where(r < block, rows + block, torch.where(r < 2 * block, rows - block, rows))
    return ref[torch.where(m < P, m, rows)]


def swap_wave_slices(ref, strip):
    """The first two 64-channel wave slices of every strip exchanged."""
    cols = torch.arange(ref.shape[1])
    c = cols % strip
    m = torch.where(c < 64, cols + 64, torch.where(c < 128, cols - 64, cols))
    return ref[:, torch.where(m < ref.shape[1], m, cols)]


def drop_last_partial_strip(ref, strip):
    """The last, partial strip never computed (modelled as zeros; in a guarded buffer it stays a sentinel)."""
    out = ref.clone()
    out[:, ref.shape[1] // strip * strip:] = 0.0
    return out


def previous_strip_bias(pr, strip):
    """The final layer's bias with every strip behind the first reading the strip before it."""
    b = pr.bs[-1]
    out = b.clone()
    out[:, strip:] = b[:, :b.shape[1] - strip]
    return out


def merge_into_neighbour(ref):
    """Every even output row's maximum merged into the odd row behind it (a single-plane wave owns two centroids)."""
    out = ref.clone()
    n = ref.shape[0] // 2 * 2
    out[1:n:2] = torch.maximum(ref[0:n:2], ref[1:n:2])
    return out


def f16x2_planes(x, amax):
    """x as the f16x2 form holds it: scaled by the power of two that puts `amax` (per row) in [2^14, 2^15), split into
    two fp16 numbers, scaled back.  A bound below the row's true maximum overflows the high plane (inf - inf = NaN
    behind it), one far above it pushes the low plane into fp16's subnormals."""
    _, ex = torch.frexp(amax.clamp_min(2.0 ** -112))
    s = torch.ldexp(torch.ones_like(amax), 15 - ex)[:, None]
    xs = x.float() * s
    hi = xs.to(torch.float16)
    lo = (xs - hi.float()).to(torch.float16)
    return (hi.double() + lo.double()) / s.double()


def previous_scene_scale(pr):
    """The loader's rows split with the PREVIOUS scene's maximum (scene 0 with the last scene's)."""
    smax = pr.A.view(pr.B, -1).abs().amax(dim=1)
    return f16x2_planes(pr.A, smax.roll(1).repeat_interleave(pr.rps))
