"""What the tests of the tiled single-layer kernels share (mlp_gemm_kernel, mlp_gemm_bf16x3_kernel and mlp_gemm_f16x2_kernel
behind s4g_mlp_gemm_f32, csrc/mlp_gemm.hip): problem builders for every (loader, epilogue) pair of the S4G_GEMM_CASE /
S4G_GEMM_CASE_CF lists in every precision the pair supports; the float64 restatement of one layer and its epilogue
(`nn_utils/conv.py:24-34,64-74`, the grouping of `pointnet2_utils/modules.py:42-50`, the interpolation of `:118-127`, the
max over neighbours of `:242-243`), optionally rounded to bf16 where the one-plane form rounds (the A and W hi planes); the
kernels' geometry READ out of csrc/mlp_gemm.hip; the per-tile-and-scene error scale; guarded outputs; and the sabotage
transforms tests/test_tiled_ref.py proves the GPU tests' inputs discriminating with.  GuardedOut, f16x2_fields, the bf16
rounding helpers, loader_rows, tile_scale's rule and the row / strip / scene-scale sabotages come from tests/chain_ref.py
by import.  Everything is built on the CPU generator: a CPU test sees the very tensors a GPU test uploads.

Every result is handled as a (rows, groups Cout) matrix, whatever the epilogue stores: EPI_MAX / EPI_MAX_CF rows are
groups of K loader rows, the channels-first tensors are read back position by position."""
import ctypes
import functools
import os
import re
import types

import torch

from tests.chain_ref import (GADD, GIDX, IADD, NPTS, PLAIN, REL4, GuardedOut, _slots, bf16, call,  # noqa: F401
                             drop_last_partial_strip, f16x2_fields, f64, loader_rows, mags, previous_scene_scale,
                             swap_row_blocks, tile_scale)
from tests.heads_ref import SENTINEL_BITS

FP32, BF16X3, BF16, F16X2 = 0, 1, 2, 3               # S4G_GEMM_FP32 ... S4G_GEMM_F16X2
PNAME = {FP32: "fp32", BF16X3: "bf16x3", BF16: "bf16", F16X2: "f16x2"}
GATHER, INTERP, CFIRST = "gather", "interp", "cfirst"
LOADER_CODE = {PLAIN: 0, GATHER: 1, INTERP: 2, GIDX: 3, REL4: 3, GADD: 4, IADD: 5, CFIRST: 6}
STORE, MAX, CF, MAXCF = 0, 1, 2, 3                   # S4G_GEMM_EPI_*
GATHERS = (GATHER, GIDX, REL4, GADD)
# the S4G_GEMM_CASE list (every precision) and the S4G_GEMM_CASE_CF list (f16x2 and fp32 only) of s4g_mlp_gemm_f32
PAIRS_ALL = [(PLAIN, STORE), (PLAIN, MAX), (PLAIN, CF), (GATHER, STORE), (GATHER, MAX), (INTERP, STORE), (GIDX, STORE),
             (GIDX, MAX), (REL4, STORE), (REL4, MAX), (GADD, STORE), (GADD, MAX), (IADD, STORE)]
PAIRS_CF = [(CFIRST, STORE), (CFIRST, CF), (CFIRST, MAXCF), (PLAIN, MAXCF)]
PRECS_ALL, PRECS_CF = (F16X2, BF16, BF16X3, FP32), (F16X2, FP32)


def precisions(loader, epi):
    return PRECS_CF if (loader, epi) in PAIRS_CF else PRECS_ALL


# ----------------------------------------------------------------------------------------------------------- geometry

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "s4g_release_amd", "csrc", "mlp_gemm.hip")


@functools.lru_cache(maxsize=None)
def geometry():
    """The tile sizes and the wide-tile predicate as csrc/mlp_gemm.hip states them."""
    src = open(_SRC).read()
    g = types.SimpleNamespace()
    for name in ("GM_BM", "GM_BN", "GM_BK"):
        setattr(g, name, int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)))
    body = src[src.index("void mlp_gemm_f16x2_kernel("):]
    g.H2_BK = int(re.search(r"constexpr int RPT = \d+, RS = \d+, WPT = BN / 64, WRS = 64, BK = (\d+);", body).group(1))
    g.H2_BN = [int(re.search(r"constexpr int BN = (\d+) \* NCB;", body).group(1)) * ncb for ncb in (2, 4)]
    m = re.search(r"wide_wgs = \(int64_t\)\(\(p\.P \+ GM_BM - 1\) / GM_BM\) \* \(\(p\.Cout \+ (\d+)\) / (\d+)\) \* groups;", src)
    assert int(m.group(1)) + 1 == int(m.group(2)) == g.H2_BN[1]
    m = re.search(r"p\.Cout > (\d+) && wide_wgs >= (\d+) &&\s*\(LOADER == LOAD_PLAIN \|\| LOADER == LOAD_GATHER_MLP1 \|\| "
                  r"LOADER == LOAD_GATHER_ADD\)", src)
    g.WIDE_COUT, g.WIDE_WGS = int(m.group(1)), int(m.group(2))
    return g


def wide_wgs(P, Cout, groups=1):
    g = geometry()
    return -(-P // g.GM_BM) * -(-Cout // g.H2_BN[1]) * groups


def wide(pr):
    """launch_gemm_f16x2's choice of the 128 x 256 tile."""
    g = geometry()
    return (pr.precision in (F16X2, BF16) and pr.loader in (PLAIN, GIDX, REL4, GADD) and pr.Cout > g.WIDE_COUT and
            wide_wgs(pr.P, pr.Cout, pr.groups) >= g.WIDE_WGS)


def col_tile(pr):
    g = geometry()
    return g.H2_BN[1] if wide(pr) else g.GM_BN


# the ladders the GPU suite walks; tests/test_tiled_ref.py holds them against geometry()
ROWS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
COLS = [1, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 132, 255, 256, 260]
DEPTH16 = [(k16, cin) for k16 in (16, 32, 48, 64, 80) for cin in range(k16 - 12, k16 + 1, 4)]     # (Kpad16, Cin)
DEPTH8 = [8, 24, 32, 40, 72]                                                                       # fp32: Kpad = Cin
WIDE_COLS = [260, 320, 512, 516]
WIDE_GROUPS, WIDE_MT = 8, 32          # PLAIN + STORE: 32 row tiles x 2 column tiles x 8 groups = 512 workgroups
WIDE_GATHER_COUT, WIDE_GATHER_NC = 1028, 205       # 103 row tiles x 5 column tiles = 515 workgroups (204: 510)
WIDE_SPLIT = (768, 256, 171)          # Cout, split_n, row tiles: 171 x 3 = 513 workgroups (170: 510)


# ----------------------------------------------------------------------------------------------------------- problems

def _ceil(x, m):
    return -(-x // m) * m


def _scene_col(m, B, rows):
    return torch.tensor([m[i % len(m)] for i in range(B)], dtype=torch.float32).repeat_interleave(rows)[:, None]


def make(loader, epi, precision, Cin=16, Cout=32, *, B=1, n=1, K=0, groups=1, relu=1, C1=0, N2=40, dense=True,
         heads=None, sigmoid_from=None, split_n=0, seed=0, scene_mags=None, lda_pad=8, a_coff=4):
    """One launch's tensors on the CPU.  n: rows per scene, or with K > 0 the centroids / groups per scene (K loader
    rows each; the GATHER family's neighbours, the max epilogues' group).  Cin: the loader's feature width (GATHER:
    Cf, the row is [feat | xyz]; INTERP: C2, the row is [interpolated | dense C1])."""
    g = torch.Generator(device="cpu").manual_seed(1000003 * seed + 7919 * Cin + 31 * Cout + 7 * B + 3 * n + K + 131 * groups)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    pr = types.SimpleNamespace(loader=loader, epi=epi, precision=precision, C=Cin, Cin=Cin, Cout=Cout, B=B, n=n, K=K,
                               groups=groups, relu=relu, C1=C1, N2=N2, split_n=split_n, lda_pad=lda_pad, a_coff=a_coff)
    assert (loader, epi) in PAIRS_ALL + PAIRS_CF and precision in precisions(loader, epi)
    assert (K > 0) == (epi in (MAX, MAXCF) or loader in GATHERS), "K: grouped loader rows or a max epilogue"
    pr.rps = n * K if K else n
    pr.P = B * pr.rps
    pr.out_rows = B * n if epi in (MAX, MAXCF) else pr.P
    pr.kw = Cin + 3 if loader == GATHER else (Cin + C1 if loader == INTERP else Cin)        # logical width of an A row
    pr.Kpad, pr.Kpad16 = _ceil(pr.kw, 8), _ceil(pr.kw, 16)
    m = mags(precision) if scene_mags is None else scene_mags
    pr.scene_mags = [m[i % len(m)] for i in range(B)]
    pr.W = r(groups, Cout, pr.kw) / pr.kw ** 0.5
    pr.bias = r(groups, Cout)
    if epi in (MAX, MAXCF):
        pr.bias[:, ::3] -= 6.0          # channels whose maximum stays negative in the unit and the quiet scenes
    pr.heads = list(heads) if heads else [Cout]
    assert sum(pr.heads) == Cout and len(pr.heads) <= 4
    pr.sigmoid_from = Cout if sigmoid_from is None else sigmoid_from
    col = _scene_col(m, B, pr.rps)
    pr.amax = pr.amax2 = None
    pr.floor = 0.0
    if loader == PLAIN:
        pr.A = r(pr.P, groups * Cin) * col
        pr.amax = _slots(pr.A, B, 5)
    elif loader == CFIRST:
        assert groups == 1
        pr.A = r(pr.P, Cin) * col                     # uploaded as (B, Cin, aL)
        pr.amax = _slots(pr.A, B, 23)
    elif loader in GATHERS:
        assert groups == 1
        cmag = torch.tensor(pr.scene_mags)[:, None, None] if loader in (GIDX, REL4) else 1.0
        pr.xyz = torch.rand(B, 3, NPTS, generator=g) * 0.2 * cmag
        cidx = torch.randint(0, NPTS, (B, n), generator=g)
        pr.ctr = torch.stack([pr.xyz[b][:, cidx[b]] for b in range(B)]).contiguous() if B else torch.zeros(0, 3, n)
        pr.gidx = torch.randint(0, NPTS, (B, n, K), generator=g).int()
        rel = torch.stack([pr.xyz[b][:, pr.gidx[b].long()] - pr.ctr[b][:, :, None] for b in range(B)])   # fp32, one rounding
        pr.rel = rel.permute(0, 2, 3, 1).reshape(pr.P, 3).contiguous()
        pr.rel4 = torch.cat([pr.rel, torch.zeros(pr.P, 1)], dim=1).contiguous()
        relmax = max(float(pr.rel.abs().max()), 1e-30)
        if loader == GATHER:
            pr.F = r(B * NPTS, Cin) * _scene_col(m, B, NPTS)
            pr.amax = _slots(pr.F, B, 17) if Cin else None
            pr.floor = relmax
        else:
            pr.w1 = r(Cin, 4)
            pr.floor = float((pr.w1[:, :3].abs().sum(1) * relmax + pr.w1[:, 3].abs()).max())
            if loader == GADD:
                pr.F = r(B * NPTS, Cin) * _scene_col(m, B, NPTS)
                pr.amax = _slots(pr.F, B, 17)
    else:                                             # INTERP, IADD: n points per scene, three of N2 sparse rows each
        assert groups == 1
        pr.S = r(B * N2, Cin) * _scene_col(m, B, N2)
        pr.nidx = torch.randint(0, N2, (B, n, 3), generator=g).int()
        w = torch.rand(B, n, 3, generator=g)
        pr.nw = (w / w.sum(dim=2, keepdim=True)).contiguous()
        pr.amax = _slots(pr.S, B, 9) if Cin else None
        if loader == IADD:
            pr.dense = r(pr.P, Cin) * col if dense else None
            pr.lbias = r(Cin)
            pr.floor = float(pr.lbias.abs().max())
            pr.amax2 = _slots(pr.dense, B, 1) if dense else None
        else:
            pr.dense = r(pr.P, C1) * col if C1 else None
            pr.amax2 = _slots(pr.dense, B, 1) if C1 else None
            pr.floor = 0.0 if Cin else 1e-30
    return pr


@functools.lru_cache(maxsize=16)
def problem(loader, epi, precision, Cin=16, Cout=32, **kw):
    """make(), one object per argument set: its references are computed once and shared (leave them unchanged).  The
    cache is small: the wide-tile problems hold a few hundred MB of float64 each."""
    return make(loader, epi, precision, Cin, Cout, **kw)


def row_scene(pr):
    return torch.arange(pr.P) // max(pr.rps, 1)


def rows(pr, exact=True, scene=None, xyz_at=None, no_xyz=False, no_dense=False, nw=None):
    """The layer's input rows (P, groups kw) as the loader forms them: float64 from the fp32 inputs, or (exact = False)
    in fp32 like the loader itself (fma order aside) -- what the one-plane bf16 form then rounds.  Sabotage only: scene
    (the scene each GATHER row takes its feature row from), xyz_at (GATHER's xyz columns placed at another column),
    no_xyz, no_dense, nw (other interpolation weights)."""
    t = (lambda x: x.double()) if exact else (lambda x: x)
    if pr.loader in (PLAIN, CFIRST):
        return t(pr.A)
    if pr.loader in (GIDX, REL4, GADD, IADD):
        return loader_rows(pr, exact=exact, no_xyz=no_xyz)
    if pr.loader == GATHER:
        sc = row_scene(pr) if scene is None else scene
        a = torch.zeros(pr.P, pr.kw + 4, dtype=torch.float64 if exact else torch.float32)
        a[:, :pr.C] = t(pr.F[sc * NPTS + pr.gidx.reshape(-1).long()])
        if not no_xyz:
            at = pr.C if xyz_at is None else xyz_at
            a[:, at:at + 3] = t(pr.rel)
        return a[:, :pr.kw]
    w = t(pr.nw if nw is None else nw)
    srows = torch.stack([pr.S.view(pr.B, pr.N2, pr.C)[b][pr.nidx[b].long()] for b in range(pr.B)])     # (B, n, 3, C2)
    if exact:
        a = (t(srows) * w[..., None]).sum(dim=2)
    else:                                             # the loader's order: ((f0 w0 + f1 w1) + f2 w2), products rounded
        a = (srows[:, :, 0] * w[:, :, 0:1] + srows[:, :, 1] * w[:, :, 1:2]) + srows[:, :, 2] * w[:, :, 2:3]
    a = a.reshape(pr.P, pr.C)
    if pr.C1:
        a = torch.cat([a, torch.zeros_like(t(pr.dense)) if no_dense else t(pr.dense)], dim=1)
    return a


def product(pr, A, rnd=f64):
    """(P, groups Cout): per group A_g W_g^T in float64, the operands rounded by `rnd` first."""
    act = rnd if rnd is f64 else (lambda y: rnd(y.float()))
    return torch.cat([act(A[:, g * pr.kw:(g + 1) * pr.kw]) @ rnd(pr.W[g]).t() for g in range(pr.groups)], dim=1)


def epilogue(pr, y, bias=None, group_shift=0, one_side=False, sigmoid_from=None):
    """The epilogue on the pre-bias products y: STORE / CHANNEL_FIRST act(y + b) (sigmoid from a channel on), MAX /
    MAX_CF the maximum over K consecutive rows FIRST, then bias and ReLU.  Sabotage only: group_shift (every group
    starts that many rows late), one_side (a group that straddles row tiles keeps the rows of its first tile)."""
    b = (pr.bias if bias is None else bias).double().reshape(1, -1)
    if pr.epi in (MAX, MAXCF):
        if group_shift:
            y = y.roll(-group_shift, dims=0)
        y3 = y.view(-1, pr.K, y.shape[1])
        if one_side:
            p = torch.arange(pr.P).view(-1, pr.K)
            keep = (p // geometry().GM_BM) == (p[:, :1] // geometry().GM_BM)
            y3 = torch.where(keep[:, :, None], y3, torch.full_like(y3, -float("inf")))
        v = y3.amax(dim=1) + b
        return v.clamp_min(0) if (pr.relu or pr.epi == MAXCF) else v
    v = y + b
    if pr.relu:
        v = v.clamp_min(0)
    if pr.epi == CF:
        s = pr.sigmoid_from if sigmoid_from is None else sigmoid_from
        v = torch.cat([v[:, :s], torch.sigmoid(v[:, s:])], dim=1)
    return v


def reference(pr, rounded=False, A=None, **sab):
    """The launch's expected result as a (out_rows, groups Cout) float64 matrix.  rounded: the one-plane yardstick."""
    if A is None:
        A = rows(pr, exact=not rounded)
    return epilogue(pr, product(pr, A, bf16 if rounded else f64), **sab)


def epilogue_pre_activation(pr):
    """A max epilogue's values in front of its ReLU: max over the group + bias, float64."""
    y = product(pr, rows(pr))
    return y.view(-1, pr.K, y.shape[1]).amax(dim=1) + pr.bias.double().reshape(1, -1)


def reference_cached(pr, rounded=False):
    key = "_ref_%d" % rounded
    if not hasattr(pr, key):
        setattr(pr, key, reference(pr, rounded))
    return getattr(pr, key)


def fp32_cpu(pr):
    """The same case as a plain fp32 product on the CPU (torch, k-ordered): the yardstick of the fp32 MFMA kernel's bound."""
    A = rows(pr, exact=False).float()
    ys = []
    for g in range(pr.groups):            # k-ordered, every product and sum rounded: the same on every CPU and BLAS
        acc = torch.zeros(pr.P, pr.Cout)
        for k in range(pr.kw):
            acc = acc + A[:, g * pr.kw + k, None] * pr.W[g, :, k][None, :]
        ys.append(acc)
    y = torch.cat(ys, dim=1)
    b = pr.bias.reshape(1, -1)
    if pr.epi in (MAX, MAXCF):
        v = y.view(-1, pr.K, y.shape[1]).amax(dim=1) + b
        return v.clamp_min(0) if (pr.relu or pr.epi == MAXCF) else v
    v = y + b
    if pr.relu:
        v = v.clamp_min(0)
    if pr.epi == CF:
        v = torch.cat([v[:, :pr.sigmoid_from], torch.sigmoid(v[:, pr.sigmoid_from:])], dim=1)
    return v


# --------------------------------------------------------------------------------------------------------- error scale

def row_span(pr):
    """(first, last) loader row of every output row."""
    k = pr.K if pr.epi in (MAX, MAXCF) else 1
    first = torch.arange(pr.out_rows) * k
    return first, first + k - 1


def scale(pr, ref):
    """(out_rows, groups Cout): per element max(1, max |ref|) over its scene's rows and its column tile's columns,
    joined over every scene with a row in a 128-row tile the element's loader rows lie in -- tests/chain_ref.tile_scale's
    rule (the f16x2 form scales a tile by the largest a_amax among the scenes it touches) per COLUMN TILE, so that a
    small channel block is not measured against a large one."""
    geo = geometry()
    R, G, Co, bn = ref.shape[0], pr.groups, pr.Cout, col_tile(pr)
    nct = -(-Co // bn)
    a = torch.zeros(R, G, nct * bn, dtype=torch.float64)
    a[:, :, :Co] = ref.abs().reshape(R, G, Co)
    a = a.view(R, G * nct, bn).amax(dim=2)                                                   # (R, G nct)
    first, last = row_span(pr)
    scene = first // pr.rps
    smax = torch.zeros(pr.B, G * nct, dtype=torch.float64).scatter_reduce(0, scene[:, None].expand(-1, G * nct), a, "amax")
    smax = smax.clamp_min(1.0)
    nt = -(-pr.P // geo.GM_BM)
    tmax = torch.stack([smax[t * geo.GM_BM // pr.rps:(min((t + 1) * geo.GM_BM, pr.P) - 1) // pr.rps + 1].amax(dim=0)
                        for t in range(nt)])
    t0, t1 = first // geo.GM_BM, last // geo.GM_BM
    s = tmax[t0]
    for j in range(1, int((t1 - t0).max()) + 1):
        s = torch.maximum(s, tmax[torch.minimum(t0 + j, t1)])
    return s[:, :, None].expand(-1, -1, bn).reshape(R, G, nct * bn)[:, :, :Co].reshape(R, G * Co)


def rel_err(out, ref, pr):
    """|out - ref| / scale, every element; non-finite differences count as infinite."""
    if ref.numel() == 0:
        return torch.zeros_like(ref)
    d = (out.double() - ref).abs() / scale(pr, ref)
    return torch.nan_to_num(d, nan=float("inf"))


# fp32 MFMA: four times the distance of the plain fp32 CPU product (torch) of the same cases from float64 at the same
# scale (the summation order differs).  The distance is measured over every fp32 case of the GPU suite by
# tests/test_tiled_ref.py, which fails if a case exceeds the figure written here.
FP32_CPU_DISTANCE = 6.0e-7                      # measured: 5.66e-7 (PLAIN + EPI_MAX_CF, K = 31, Cout = 129)
# f16x2 and bf16x3: tests/test_fused_gpu.py's 2e-5; one-plane bf16: 2e-3 max / 2e-5 mean against the restatement rounded
# where the kernel rounds, 5e-2 against float64 (tests/chain_ref.bounds)
BOUNDS = {F16X2: {"max": 2e-5}, BF16X3: {"max": 2e-5}, FP32: {"max": 4 * FP32_CPU_DISTANCE},
          BF16: {"max": 2e-3, "mean": 2e-5, "exact": 5e-2}}


def bounds(precision):
    return BOUNDS[precision]


def compare(pr, out, what=""):
    """Element by element against the yardstick(s) of pr.precision; prints the worst error next to its bound and
    returns {name: (worst, bound)}.  `out`: the (out_rows, groups Cout) matrix, any device."""
    out = out.detach().cpu()
    bd, exact, res = bounds(pr.precision), reference_cached(pr, False), {}
    worst = lambda e: float(e.max()) if e.numel() else 0.0        # noqa: E731
    if pr.precision == BF16:
        e = rel_err(out, reference_cached(pr, True), pr)
        res["max"] = (worst(e), bd["max"])
        res["mean"] = (float(e.mean()) if e.numel() else 0.0, bd["mean"])
        res["exact"] = (worst(rel_err(out, exact, pr)), bd["exact"])
    else:
        res["max"] = (worst(rel_err(out, exact, pr)), bd["max"])
    print("%s %s" % (what, "  ".join("%s %.3e / %.1e" % (k, v[0], v[1]) for k, v in res.items())))
    return res


# ------------------------------------------------------------------------------------------------------ guarded outputs

class Guard(GuardedOut):
    """tests/chain_ref.GuardedOut with the layout chosen by the case: ldc, c_coff, c_gcol, and `shift` floats in front
    of the output pointer (1: the pointer is not 16-byte aligned)."""

    def __init__(self, dev, rows, cout, groups=1, zero_payload=False, ldc=None, c_coff=4, c_gcol=None, shift=0):
        self.GUARD = G = GuardedOut.GUARD + shift
        self.rows, self.cout, self.groups, self.zero = rows, cout, groups, zero_payload
        self.c_gcol = cout if c_gcol is None else c_gcol
        width = self.c_gcol * (groups - 1) + cout
        self.ldc = _ceil(width, 4) + 8 if ldc is None else ldc
        self.c_coff = c_coff
        assert self.ldc >= c_coff + width
        self.n = rows * self.ldc
        bits = torch.full((G + self.n + GuardedOut.GUARD,), SENTINEL_BITS, dtype=torch.int32, device=dev)
        if zero_payload:
            bits[G:G + self.n] = 0
        self.want = bits.clone()
        self.buf = bits.view(torch.float32)
        self.out = self.buf[G:]

    def _owed(self, bits_like):
        """(rows, groups, cout) view of the owed elements of a buffer-shaped tensor."""
        G = self.GUARD
        v = bits_like[G:G + self.n].view(self.rows, self.ldc)[:, self.c_coff:]
        return v.as_strided((self.rows, self.groups, self.cout), (self.ldc, self.c_gcol, 1))

    def values(self):
        return self._owed(self.buf).reshape(self.rows, self.groups * self.cout)

    def check(self, rows_owed=None):
        owed = self.rows if rows_owed is None else rows_owed
        bits = self.buf.view(torch.int32)
        free = torch.ones_like(bits, dtype=torch.bool)
        self._owed(free)[:owed] = False
        stray = (bits != self.want) & free
        assert not stray.any(), "written outside the output at word(s) %s" % stray.nonzero().flatten()[:8].tolist()
        assert torch.isfinite(self._owed(self.buf)[:owed]).all(), "an owed element is not finite (never written?)"


class Outs:
    """The guarded output tensor(s) of one launch and their reading as the (out_rows, groups Cout) matrix."""

    def __init__(self, pr, dev, ldc=None, c_coff=4, shift=0, c_gcol=None):
        self.pr = pr
        if pr.epi == CF:             # one (B, ch, cf_N) tensor per head, guards around each
            self.g = [Guard(dev, 1, pr.B * ch * pr.rps, c_coff=0, ldc=pr.B * ch * pr.rps) for ch in pr.heads]
        elif pr.epi == MAXCF:        # (B, Cout, M), merged by atomicMax into zeros
            self.g = [Guard(dev, 1, pr.B * pr.Cout * pr.n, zero_payload=True, c_coff=0, ldc=pr.B * pr.Cout * pr.n)]
        elif pr.split_n:             # two row-major tensors, c_coff = 0 as the form requires
            self.g = [Guard(dev, pr.out_rows, pr.split_n, c_coff=0), Guard(dev, pr.out_rows, pr.Cout - pr.split_n, c_coff=0)]
        else:
            self.g = [Guard(dev, pr.out_rows, pr.Cout, pr.groups, ldc=ldc, c_coff=c_coff, shift=shift, c_gcol=c_gcol)]

    def fields(self):
        pr, g0 = self.pr, self.g[0]
        if pr.epi == CF:
            starts = [0]
            for ch in pr.heads:
                starts.append(starts[-1] + ch)
            starts += [pr.Cout] * (5 - len(starts))
            from s4g_release_amd import _cabi
            ptrs = (_cabi._vp * 4)(*([x.out.data_ptr() for x in self.g] + [0] * (4 - len(self.g))))
            return dict(cf_ptr=ptrs, cf_start=(_cabi._i32 * 5)(*starts), cf_sigmoid_from=pr.sigmoid_from, cf_N=pr.rps)
        if pr.epi == MAXCF:
            return dict(out=g0.out)
        kw = dict(out=g0.out, ldc=g0.ldc, c_coff=g0.c_coff, c_gcol=g0.c_gcol)
        if pr.split_n:
            kw.update(out2=self.g[1].out, ldc2=self.g[1].ldc, split_n=pr.split_n)
        return kw

    def matrix(self):
        pr = self.pr
        if pr.epi == CF:
            return torch.cat([x.values().view(pr.B, ch, pr.rps).permute(0, 2, 1).reshape(pr.P, ch)
                              for x, ch in zip(self.g, pr.heads)], dim=1)
        if pr.epi == MAXCF:
            return self.g[0].values().view(pr.B, pr.Cout, pr.n).permute(0, 2, 1).reshape(pr.out_rows, pr.Cout)
        return torch.cat([x.values() for x in self.g], dim=1)

    def check(self):
        for x in self.g:
            x.check()

    def untouched(self):
        return all(x.untouched() for x in self.g)


# ------------------------------------------------------------------------------------------------------------ launches

def _weights(pr, dev):
    """Descriptor fields of the layer for pr.precision (W padded to Kpad / Kpad16, group strides with a gap); cached."""
    key = "_w_%s" % dev
    if hasattr(pr, key):
        return getattr(pr, key)
    from s4g_release_amd.fused import split_bf16x3
    G, Co = pr.groups, pr.Cout
    bstride = Co + 5                                  # b_gstride: bias and w_inv_scale rows with a gap behind them
    bias = torch.full((G, bstride), 1e30)
    bias[:, :Co] = pr.bias
    kw = dict(bias=bias.to(dev), b_gstride=bstride, Kpad=pr.Kpad, Kpad16=pr.Kpad16)
    if pr.precision == FP32:
        wstride = Co * pr.Kpad + 8                    # w_gstride: a gap between the groups' matrices
        W = torch.full((G, wstride), 1e30)
        Wv = W.as_strided((G, Co, pr.Kpad), (wstride, pr.Kpad, 1))
        Wv.zero_()
        Wv[:, :, :pr.kw] = pr.W
        kw.update(W=W.to(dev), w_gstride=wstride)
    else:
        w16 = torch.zeros(G, Co, pr.Kpad16)
        w16[:, :, :pr.kw] = pr.W
        kw["w_gstride"] = Co * pr.Kpad16
        if pr.precision == F16X2:
            h2 = f16x2_fields(w16.to(dev), floor=pr.floor)
            inv = torch.full((G, bstride), 1e30, device=dev)
            inv[:, :Co] = h2["w_inv_scale"]
            kw.update(W_f16x2=h2["W_f16x2"], w_inv_scale=inv, a_amax_floor=h2["a_amax_floor"])   # W_f16x2_frag stays unset
        else:
            kw["W_bf16x3"] = split_bf16x3(w16.to(dev))
    setattr(pr, key, kw)
    return kw


def descriptor(pr, dev, outs, out_amax=None, out_amax2=None, **over):
    """The s4g_gemm_desc_t fields of the problem as a dict of ints / floats / ctypes arrays / device tensors."""
    kw = dict(loader=LOADER_CODE[pr.loader], epilogue=pr.epi, groups=pr.groups, P=pr.P, Cin=pr.kw, Cout=pr.Cout,
              precision=pr.precision, relu=pr.relu, K=pr.K, rows_per_scene=pr.rps)
    kw.update(_weights(pr, dev))
    kw.update(outs.fields())
    if pr.epi == MAXCF:
        kw["M"] = pr.n
    up = lambda x: x.to(dev).contiguous()             # noqa: E731
    if pr.loader == PLAIN:                            # lda > Cin, a_coff > 0; the columns around the rows hold 1e30
        lda = pr.a_coff + pr.groups * pr.Cin + pr.lda_pad
        A = torch.full((max(pr.P, 1), lda), 1e30)
        A[:pr.P, pr.a_coff:pr.a_coff + pr.groups * pr.Cin] = pr.A
        kw.update(A=up(A), lda=lda, a_coff=pr.a_coff, a_gcol=pr.Cin)
    elif pr.loader == CFIRST:
        kw.update(A=up(pr.A.view(pr.B, pr.rps, pr.Cin).permute(0, 2, 1)), a_L=pr.rps)
    elif pr.loader in GATHERS:
        kw.update(N=NPTS, M=pr.n, gidx=up(pr.gidx), xyz=up(pr.xyz), ctr=up(pr.ctr))
        if pr.loader == GATHER:
            kw.update(Cf=pr.C, Cin=pr.kw)
            if pr.C:
                kw["feat"] = up(pr.F)
        else:
            kw.update(mlp1_w=up(pr.w1), Cin=pr.C)
            if pr.loader == REL4:                     # pre-gathered rows: gidx / xyz / ctr are not read
                kw.update(rel_xyz4=up(pr.rel4), gidx=0, xyz=0, ctr=0)
            if pr.loader == GADD:
                kw.update(feat=up(pr.F), Cf=pr.C)
    else:
        kw.update(nidx=up(pr.nidx), nw=up(pr.nw), C2=pr.C, N2=pr.N2, N1=pr.n)
        if pr.C or pr.loader == IADD:
            kw["sparse"] = up(pr.S)
        else:
            kw["sparse"] = torch.zeros(4, device=dev)  # C2 = 0: required non-NULL, never read
        if pr.dense is not None:
            kw["dense"] = up(pr.dense)
        if pr.loader == IADD:
            kw.update(loader_bias=up(pr.lbias), Cin=pr.C)
        else:
            kw.update(C1=pr.C1)
    if pr.precision == F16X2:
        if pr.amax is not None:
            kw["a_amax"] = up(pr.amax)
        if pr.amax2 is not None:
            kw["a_amax2"] = up(pr.amax2)
        if out_amax is not None:
            kw["out_amax"] = out_amax
        if out_amax2 is not None:
            kw["out_amax2"] = out_amax2
    kw.update(over)
    return kw


def launch(pr, dev, out_amax=None, out_amax2=None, layout=None, **over):
    """(status, Outs) of the problem's ONE s4g_mlp_gemm_f32 call into guarded buffers.  layout: Outs' keywords."""
    outs = Outs(pr, dev, **(layout or {}))
    kw = descriptor(pr, dev, outs, out_amax, out_amax2, **over)
    from s4g_release_amd import _cabi
    d = _cabi.GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = _cabi.lib().s4g_mlp_gemm_f32(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del kw
    return rc, outs


# ------------------------------------------------------------------------------------------------------------ sabotage
# (swap_row_blocks, drop_last_partial_strip and previous_scene_scale are tests/chain_ref.py's)

def neighbour_block_bias(pr, block=32):
    """Every 32-column block read with the bias of the block before it (the first with the second's)."""
    return pr.bias.roll(block if pr.Cout > block else 1, dims=1)


def drop_half_step(pr):
    """The loader rows with the last 16 columns of Kpad16 zeroed (the half-deep last K step never run)."""
    A = rows(pr).clone()
    lo = pr.Kpad16 - 16
    for g in range(pr.groups):
        A[:, g * pr.kw + lo:(g + 1) * pr.kw] = 0.0
    return A


def first_row_scene(pr):
    """The scene of every row taken from its tile's first row."""
    p = torch.arange(pr.P)
    return (p // geometry().GM_BM * geometry().GM_BM) // pr.rps


def out2_off_by_a_tile(pr, ref):
    """out2's columns shifted by one 256-column tile (what lands past the tensor's width is lost)."""
    out = ref.clone()
    w = geometry().H2_BN[1]
    out[:, pr.split_n:] = 0.0
    out[:, pr.split_n:pr.Cout - w] = ref[:, pr.split_n + w:]
    return out


def cf_point_not_reduced(pr, ref):
    """Channels-first stores at point index `row` instead of `row - scene cf_N`: every element lands scene * cf_N
    floats late in its head's tensor, or past its end (lost; the place it owed keeps its sentinel, modelled as 0)."""
    out, N, c0 = torch.zeros_like(ref), pr.rps, 0
    p = torch.arange(pr.P)
    b, pt = p // N, p % N
    for ch in pr.heads:
        flat = torch.zeros(pr.B * ch * N, dtype=ref.dtype)
        idx = ((b[:, None] * ch + torch.arange(ch)[None, :]) * N + b[:, None] * N + pt[:, None]).reshape(-1)
        ok = idx < flat.numel()
        flat[idx[ok]] = ref[:, c0:c0 + ch].reshape(-1)[ok]
        out[:, c0:c0 + ch] = flat.view(pr.B, ch, N).permute(0, 2, 1).reshape(pr.P, ch)
        c0 += ch
    return out


def head_boundary_off(pr, ref, h=1):
    """cf_start[h] one channel late: the channel at the boundary goes to the end of the head before it and never
    reaches its own tensor (modelled as 0)."""
    out = ref.clone()
    out[:, sum(pr.heads[:h])] = 0.0
    return out
