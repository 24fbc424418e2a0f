"""s4g_heads_chain_f32: the four per-point heads (PointNet2_tcls.py:83-95,126-140 -- four
SharedMLP stacks 256 -> 512 -> 256 -> 256 -> 128 on a shared input, Conv1d logits, sigmoid on
the movable head) as one launch, against an fp64 restatement of the same layers."""
import ctypes

import pytest
import torch

from tests import golden_util as GU
from tests import heads_ref as H

pytestmark = pytest.mark.gpu
CH = H.CH


@pytest.fixture(scope="module")
def layer_set(dev):
    """The packed layer sets of this module, built once per seed (`_Layer` / `fragment_order` are the expensive part)."""
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = H.build_layers(dev, seed)
        return cache[seed]
    return get


@pytest.mark.parametrize("B,N", [(2, 100), (1, 64), (3, 171)])
def test_heads_chain_f16x2_is_fp32_class(dev, layer_set, B, N):
    Ws, b, layers = layer_set(7 + N)
    g = torch.Generator(device="cpu").manual_seed(N)
    X = (torch.randn(B * N, 256, generator=g) * torch.tensor([1.0, 40.0, 0.02])[:B, None]
         .repeat_interleave(N, dim=0)).to(dev)      # scenes of very different magnitude
    amax = torch.zeros((B, 64), device=dev)
    amax[:, 5] = X.view(B, -1).abs().amax(dim=1)
    outs = H.run(dev, layers, X, B, N, 3, amax=amax)
    ref = H.reference(Ws, b, X, B, N)
    for h in range(4):
        assert torch.isfinite(outs[h]).all()
        err = (outs[h].double() - ref[h]).abs()
        scale = ref[h].abs().amax(dim=(1, 2), keepdim=True).clamp_min(1.0)     # per scene
        assert (err / scale).max().item() < 2e-5, (h, (err / scale).max().item())


def test_heads_chain_bf16_matches_a_reference_rounded_at_the_same_points(dev, layer_set):
    B, N = 2, 150
    Ws, b, layers = layer_set(3)
    X = torch.randn(B * N, 256, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    outs = H.run(dev, layers, X, B, N, 2)
    ref = H.reference(Ws, b, X, B, N, rnd=lambda t: t.to(torch.bfloat16).double())
    exact = H.reference(Ws, b, X, B, N)
    for h in range(4):
        scale = max(1.0, ref[h].abs().max().item())
        assert torch.isfinite(outs[h]).all()
        assert (outs[h].double() - ref[h]).abs().max().item() < 3e-3 * scale
        assert (outs[h].double() - ref[h]).abs().mean().item() < 5e-5 * scale
        assert (outs[h].double() - exact[h]).abs().max().item() < 8e-2 * scale


def test_heads_chain_rejects_other_widths_and_bad_arguments(dev):
    from s4g_release_amd import _cabi
    X = torch.randn(64, 256, device=dev)
    d = _cabi.HeadsDesc()
    d.precision, d.P, d.N, d.ldx = 3, 64, 64, 256
    d.C, d.H0, d.H1, d.H2, d.H3 = 256, 512, 256, 256, 64          # not the shipped widths
    d.X = X.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert _cabi.lib().s4g_heads_chain_f32(ctypes.byref(d), st) != 0
    d.H3 = 128
    assert _cabi.lib().s4g_heads_chain_f32(ctypes.byref(d), st) != 0     # no weights / outputs given


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("B,N,N2,with_dense", [(2, 100, 40, False), (3, 171, 64, True), (1, 64, 3, False)])
def test_heads_chain_with_fp_tail_in_front(dev, layer_set, precision, B, N, N2, with_dense):
    """ABI 6: interpolate + add + ReLU in the loader, two 256 -> 256 layers inside LDS, then the
    heads -- against fp64 (f16x2: fp32-class) / a reference rounded to bf16 at the layer inputs."""
    Ws, b, layers = layer_set(11 + N)
    S, nidx, nw, dense, lbias, pl = H.pre_setup(dev, B, N, N2, 5 + N, with_dense)
    outs = H.run(dev, layers, None, B, N, precision, pre=(S, nidx, nw, dense, lbias, pl, N2))
    if precision == 3:
        X = H.pre_reference(S, nidx, nw, dense, lbias, pl, B, N, N2)
        ref = H.reference(Ws, b, X, B, N)
        for h in range(4):
            assert torch.isfinite(outs[h]).all()
            err = (outs[h].double() - ref[h]).abs()
            scale = ref[h].abs().amax(dim=(1, 2), keepdim=True).clamp_min(1.0)
            assert (err / scale).max().item() < 3e-5, (h, (err / scale).max().item())
    else:
        rb = lambda t: t.to(torch.bfloat16).double()
        X = H.pre_reference(S, nidx, nw, dense, lbias, pl, B, N, N2, rnd=rb)
        ref = H.reference(Ws, b, X, B, N, rnd=rb)
        for h in range(4):
            scale = max(1.0, ref[h].abs().max().item())
            assert torch.isfinite(outs[h]).all()
            assert (outs[h].double() - ref[h]).abs().max().item() < 6e-3 * scale
            assert (outs[h].double() - ref[h]).abs().mean().item() < 1e-4 * scale


def test_fused_model_with_and_without_the_tail_in_the_heads_launch(dev, monkeypatch):
    """The whole network at a small size: S4G_HEADS_PRE=0 (separate fp2 chain launch) and the default
    (tail inside the heads launch) agree to fp32 round-off, and the launch list shrinks by one."""
    from s4g_release_amd import functions as F, synth
    from s4g_release_amd.fused import FusedPointNet2
    from s4g_release_amd.model import S4GConfig, build_pointnet2_cls, randomize_bn_
    net = GU.shipped_net(dev)
    pts = torch.from_numpy(synth.make_batch([0, 1], 25600)).to(dev)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("S4G_HEADS_PRE", flag)
        run = FusedPointNet2(net)
        F.OpTimer.reset(enabled=True)
        with torch.no_grad():
            out = run({"scene_points": pts})
        torch.cuda.synchronize()
        F.OpTimer.enabled = False
        res[flag] = ({k: v.clone() for k, v in out.items()}, sorted(F.OpTimer.summary()))
    a, b = res["0"], res["1"]
    assert any("fp2.1+fp2.2+heads" in n for n in b[1]) and not any("fp2.1+fp2.2+heads" in n for n in a[1])
    assert len([n for n in a[1] if n.startswith("gemm[")]) == len([n for n in b[1] if n.startswith("gemm[")]) + 1
    for k in a[0]:
        assert (a[0][k] - b[0][k]).abs().max().item() < 2e-5, k


def test_fused_model_fp1_chain_into_the_next_levels_first_layer(dev, monkeypatch):
    """S4G_FP_CHAIN_NEXT: FP level 1's (interpolate + add) -> 512 -> 512 layer and level 2's linear
    first layer as one chain launch (level 1's own output never written) against the separate
    launches: same outputs to fp32 round-off, two launches (interp_add + fp2.0s) fewer."""
    from s4g_release_amd import functions as F, synth
    from s4g_release_amd.fused import FusedPointNet2
    from s4g_release_amd.model import S4GConfig, build_pointnet2_cls, randomize_bn_
    net = GU.shipped_net(dev)
    pts = torch.from_numpy(synth.make_batch([2, 3], 25600)).to(dev)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("S4G_FP_CHAIN_NEXT", flag)
        run = FusedPointNet2(net)
        F.OpTimer.reset(enabled=True)
        with torch.no_grad():
            out = run({"scene_points": pts})
        torch.cuda.synchronize()
        F.OpTimer.enabled = False
        res[flag] = ({k: v.clone() for k, v in out.items()}, sorted(F.OpTimer.summary()))
    a, b = res["0"], res["1"]
    assert any("fp1.1+fp2.0s" in n for n in b[1]) and not any("fp1.1+fp2.0s" in n for n in a[1])
    assert any(n.startswith("gemm[fp2.0s") for n in a[1]) and not any(n.startswith("gemm[fp2.0s") for n in b[1])
    assert len([n for n in a[1] if n.startswith("interp_add")]) == len([n for n in b[1] if n.startswith("interp_add")]) + 1
    for k in a[0]:
        assert (a[0][k] - b[0][k]).abs().max().item() < 2e-5, k
