"""The GATHER_ADD layer pairs of SA levels 2 and 3 as ONE launch whose loader has no vector arithmetic of its own:
the gathered rows F[b N + gidx] are copied into LDS, the xyz term w1 . (xyz_j - ctr_m, 1) is one 16-deep step on
the matrix cores (scaled fp16 planes, the wave's measured coordinate maximum and each channel's own weight scale),
and relu(F + term) is split into the panel in place.  Driven alone through s4g_mlp_gemm_f32 against a float64
evaluation of the same formula on the same indices.

Bound: 3e-5 x max(1, max|ref|), the bound of test_fused_gpu.py::test_gemm_gather_add_loader (the same loader's
formula on the tiled kernel)."""
import pytest
import torch

from tests.test_fused_gpu import _h2, _h2_second, _run, _w3

pytestmark = pytest.mark.gpu
K = 64
REL_TOL = 3e-5


def _problem(seed, B, N, M, C, Cin, Cout2, scale, bias_scale):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xyz = torch.rand(B, 3, N, generator=g) * scale
    cidx = torch.randint(0, N, (B, M), generator=g)
    ctr = torch.stack([xyz[b][:, cidx[b]] for b in range(B)]).contiguous()
    gidx = torch.randint(0, N, (B, M, K), generator=g).int()
    F = torch.randn(B * N, Cin, generator=g)
    w1 = torch.randn(Cin, 4, generator=g)
    w1[:, 3] *= bias_scale
    w1[3] = 0.0                                  # a channel without an xyz term
    W = torch.zeros(C, C)
    W[:, :Cin] = torch.randn(C, Cin, generator=g) / Cin ** 0.5
    b = torch.randn(C, generator=g)
    W2 = torch.randn(Cout2, C, generator=g) / C ** 0.5
    b2 = torch.randn(Cout2, generator=g)
    return dict(xyz=xyz, ctr=ctr, gidx=gidx, F=F, w1=w1, W=W, b=b, W2=W2, b2=b2)


def _rel64(t, scenes):
    rel = torch.stack([t["xyz"][bi][:, t["gidx"][bi].long()] - t["ctr"][bi][:, :, None] for bi in scenes])
    return rel.permute(0, 2, 3, 1).reshape(-1, 3).double()            # fp32 subtraction, as the kernel's


def _ref64(t, scenes, N, with_xyz=True):
    Cin = t["F"].shape[1]
    rows = torch.cat([t["F"].view(-1, N, Cin)[bi][t["gidx"][bi].long().reshape(-1)] for bi in scenes]).double()
    A = rows + t["w1"][:, 3].double()
    if with_xyz:
        A = A + _rel64(t, scenes) @ t["w1"][:, :3].double().t()
    A = A.clamp_min(0)
    h = (A @ t["W"][:, :Cin].double().t() + t["b"].double()).clamp_min(0)
    o = (h @ t["W2"].double().t() + t["b2"].double()).clamp_min(0)
    return o.view(-1, K, o.shape[1]).max(dim=1)[0]


def _launch(t, dev, scenes, N, M, per_scene=False):
    """The launch on the given scenes of the problem (their tensors sliced: a solo run sees nothing of the others)."""
    B = len(scenes)
    C, Cin, Cout2 = t["W"].shape[0], t["F"].shape[1], t["W2"].shape[0]
    d = {k: v.to(dev) for k, v in t.items()}
    xyz = d["xyz"][scenes].contiguous()
    ctr = d["ctr"][scenes].contiguous()
    gidx = d["gidx"][scenes].contiguous()
    F = d["F"].view(-1, N, Cin)[scenes].reshape(B * N, Cin).contiguous()
    relmax = max(float(_rel64(t, [s]).abs().max()) for s in scenes if torch.isfinite(t["xyz"][s]).all())
    bound = float((t["w1"][:, :3].abs().sum(1) * max(relmax, 1e-30) + t["w1"][:, 3].abs()).max())
    k16, w3 = _w3(d["W"])
    h2 = _h2(d["W"], floor=bound)
    if per_scene:       # one 64-slot row of maxima per scene, as the network runs it
        am = torch.zeros(B, 64, device=dev)
        am[:, 17] = F.view(B, -1).abs().max(dim=1)[0]
        h2.update(a_amax=am, out_amax=torch.zeros(B, 64, device=dev), rows_per_scene=M * K)
    else:
        am = torch.zeros(64, device=dev)
        am[17] = F.abs().max()
        h2.update(a_amax=am)
    frag2, inv2 = _h2_second(d["W2"])
    P = B * M * K
    out = torch.full((B * M, Cout2), float("nan"), device=dev)
    _run(dict(loader=4, epilogue=1, groups=1, relu=1, P=P, Cin=Cin, Kpad=C, Cout=C, W=d["W"], bias=d["b"],
              gidx=gidx, feat=F, Cf=Cin, xyz=xyz, ctr=ctr, N=N, M=M, K=K, mlp1_w=d["w1"], out=out, ldc=Cout2,
              precision=3, Kpad16=k16, W_bf16x3=w3, W2_f16x2_frag=frag2, w2_inv_scale=inv2, bias2=d["b2"],
              Cout2=Cout2, relu2=1, **h2), dev)
    return out


def _check(out, ref, what):
    tol = REL_TOL * max(1.0, ref.abs().max().item())
    err = (out.double().cpu() - ref).abs().max().item()
    print("%s: max error %.3e, bound %.3e, max|ref| %.3e" % (what, err, tol, ref.abs().max().item()))
    assert torch.isfinite(out).all()
    assert err < tol, (what, err, tol)
    return err, tol


# C: the pair's width (128 -> RW = 2, 256 -> RW = 1, 512 -> the eight-wave form); Cin == C unless given
@pytest.mark.parametrize("C,Cout2,B,M,Cin", [
    (128, 256, 2, 24, 128),      # the shipped shapes: 128 -> 128 -> 256 ...
    (256, 512, 2, 9, 256),       # ... and 256 -> 256 -> 512
    (512, 512, 2, 5, 512),       # the eight-wave form at its own width
    (128, 256, 1, 23, 128),      # P = 23 x 64: not a multiple of the 128-row tile
    (128, 128, 3, 5, 128),       # tiles that straddle two scenes, ragged last tile
    (256, 512, 3, 3, 256),       # B M odd at 64-row tiles
    (128, 256, 2, 7, 64),        # Cin below the panel width
    (256, 256, 2, 4, 192),
    (512, 1024, 1, 3, 260),      # ... and not a multiple of a 32-column piece
    (256, 512, 1, 11, 256),      # B = 1
    (512, 512, 1, 2, 512),
])
def test_gather_add_pair_against_float64(dev, C, Cout2, B, M, Cin):
    N = 300
    t = _problem(C + Cout2 + 7 * M + Cin, B, N, M, C, Cin, Cout2, 0.2, 1.0)
    out = _launch(t, dev, list(range(B)), N, M)
    _check(out, _ref64(t, list(range(B)), N), "C=%d Cin=%d B=%d M=%d" % (C, Cin, B, M))


# ONE (the position operand's bias slot) and the channel scale are measured in the kernel: coordinates and biases
# over several decades (test_fused_gpu.py::test_chain_first_layer_on_the_matrix_cores' sweep)
@pytest.mark.parametrize("C,Cout2", [(256, 512), (512, 512), (128, 256)])
@pytest.mark.parametrize("scale,bias_scale", [(0.2, 1.0), (0.03, 1.0), (1e-6, 40.0), (300.0, 1e-3), (0.0, 1.0),
                                              (5.0, 40.0), (1e-3, 1e-3)])
def test_gather_add_pair_operand_ranges(dev, C, Cout2, scale, bias_scale):
    B, N, M = 2, 200, 4
    t = _problem(C + int(bias_scale * 1000) + 3, B, N, M, C, C, Cout2, scale, bias_scale)
    out = _launch(t, dev, [0, 1], N, M)
    _check(out, _ref64(t, [0, 1], N), "C=%d scale=%g bias_scale=%g" % (C, scale, bias_scale))


@pytest.mark.parametrize("C,Cout2", [(256, 512), (512, 512), (128, 256)])
def test_gather_add_pair_sees_a_dropped_xyz_term(dev, C, Cout2):
    """Sabotage: against the same formula WITHOUT the xyz term the launch's output must miss the bound by >= 100 x
    (the comparison above would catch a kernel that lost the term)."""
    B, N, M = 2, 300, 6
    t = _problem(C + 11, B, N, M, C, C, Cout2, 0.2, 1.0)
    out = _launch(t, dev, [0, 1], N, M)
    err, tol = _check(out, _ref64(t, [0, 1], N), "C=%d" % C)
    bad = _ref64(t, [0, 1], N, with_xyz=False)
    miss = (out.double().cpu() - bad).abs().max().item()
    print("without the xyz term: %.3e = %.0f x the bound" % (miss, miss / tol))
    assert miss >= 100 * tol, (miss, tol)


@pytest.mark.parametrize("C,Cout2,M", [(256, 512, 5), (512, 512, 3), (128, 256, 4)])
def test_gather_add_pair_nonfinite_scene_stays_in_its_rows(dev, C, Cout2, M):
    """A scene with NaN / inf coordinates between two clean scenes: no fault, and the clean scenes' rows are
    bit-identical to their solo runs (per-scene maxima, a wave's rows are one centroid of one scene)."""
    B, N = 3, 250
    t = _problem(C + 5, B, N, M, C, C, Cout2, 0.2, 1.0)
    t["xyz"][1, 0, 5] = float("nan")
    t["xyz"][1, 2, 7] = float("inf")
    t["xyz"][1, 1, 9] = float("-inf")
    t["gidx"][1, :, 3] = 5                     # every centroid of the scene meets them
    t["gidx"][1, :, 4] = 7
    t["gidx"][1, :, 5] = 9
    out = _launch(t, dev, [0, 1, 2], N, M, per_scene=True)
    torch.cuda.synchronize()
    for s in (0, 2):
        solo = _launch(t, dev, [s], N, M, per_scene=True)
        assert torch.equal(out[s * M:(s + 1) * M], solo), s
        _check(solo, _ref64(t, [s], N), "clean scene %d" % s)
