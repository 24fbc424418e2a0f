"""GPU tests of `s4g_release_amd.accelerate`: the new contraction forms against float64 products on the host (the
channels-first loader, the any-K max epilogue with channels-first output, the channels-first store, the per-scene amax
kernel), then converted networks -- the calibrated fixtures, graphs `FusedPointNet2` refuses, determinism, the
fallbacks and the folded-weight cache.  f16x2 is held to 1e-4 of the tensor's scale, fp32 to fp32 round-off."""
import copy

import pytest
import torch
import torch.nn.functional as F

import s4g_release_amd
from s4g_release_amd import _cabi
from s4g_release_amd import accelerated as A
from s4g_release_amd.fused import FusedPointNet2, _Layer, _pad_k
from s4g_release_amd.model import PointNet2, randomize_bn_
from s4g_release_amd.modules import sample_and_group
from s4g_release_amd.nn_utils import SharedMLP
from tests import golden_util as GU
from tests.test_calib_gpu import _check_small, _hook_levels, _np, _small_net

pytestmark = pytest.mark.gpu
TOL = {"f16x2": 1e-4, "fp32": 2e-6}


def _rel(a, ref):
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((a - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _layer(cout, cin, dev, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dev)
    b = (torch.randn(cout, generator=g) * 0.1).to(dev)
    return _Layer(_pad_k(w), b, cin), w.double(), b.double()


def _ref_rows(x, w, b, relu):
    """float64 Y[b][n][l] = act(sum_c W[n][c] x[b][c][l] + bias[n]) of a (B, C, L) tensor."""
    y = torch.einsum("nc,bcl->bnl", w, x.double()) + b[None, :, None]
    return y.clamp_min(0) if relu else y


def _bound(prec, x, B):
    return (A._amax(x.contiguous(), B), None, 0.0) if prec == "f16x2" else (None, None, 0.0)


@pytest.mark.parametrize("prec", ["f16x2", "fp32"])
@pytest.mark.parametrize("cin", [3, 7, 131, 259])
def test_channel_first_loader_and_store(dev, prec, cin):
    B, L, cout = 3, 37, 40                        # odd L, P = 111: ragged against the 128-row tile
    x = torch.randn(B, cin, L, device=dev) * 3.0
    layer, w, b = _layer(cout, cin, dev, cin)
    a = _bound(prec, x, B)
    P = B * L
    out = torch.full((B, cout, L), float("nan"), device=dev)     # every element must be written
    A._launch(layer, A.PRECISIONS[prec], False, A.LOAD_CHANNEL_FIRST, A.EPI_CHANNEL_FIRST, P, cin, x, out, L,
              a_L=L, a_amax=a[0], cf_N=L)
    ref = _ref_rows(x, w, b, False)
    assert _rel(out, ref) < TOL[prec], (prec, cin, _rel(out, ref))
    # ... and channels-last STORE, the interior layers' layout, with a padded row stride
    ldc = (cout + 3) // 4 * 4 + 4
    cl = torch.zeros((P, ldc), device=dev)
    A._launch(layer, A.PRECISIONS[prec], True, A.LOAD_CHANNEL_FIRST, A.EPI_STORE, P, cin, x, cl, L,
              a_L=L, a_amax=a[0], ldc=ldc)
    ref_cl = ref.clamp_min(0).permute(0, 2, 1).reshape(P, cout)
    assert _rel(cl[:, :cout], ref_cl) < TOL[prec]
    assert torch.count_nonzero(cl[:, cout:]) == 0


@pytest.mark.parametrize("prec", ["f16x2", "fp32"])
@pytest.mark.parametrize("K", [1, 5, 16, 48, 64, 100, "N"])
def test_max_epilogue_any_k(dev, prec, K):
    B, M, cin, cout = 2, 7, 19, 72
    if K == "N":
        M, K = 1, 1000                            # group-all: one group of every point
    x = torch.randn(B, cin, M, K, device=dev)
    layer, w, b = _layer(cout, cin, dev, K)
    a = _bound(prec, x, B)
    out = torch.zeros((B, cout, M), device=dev)
    A._launch(layer, A.PRECISIONS[prec], True, A.LOAD_CHANNEL_FIRST, A.EPI_MAX_CHANNEL_FIRST, B * M * K, cin, x, out,
              M * K, a_L=M * K, a_amax=a[0], M=M, K=K)
    ref = _ref_rows(x.reshape(B, cin, M * K), w, b, True).reshape(B, cout, M, K).amax(dim=3)
    assert _rel(out, ref) < TOL[prec], (prec, K, _rel(out, ref))
    again = torch.zeros_like(out)
    A._launch(layer, A.PRECISIONS[prec], True, A.LOAD_CHANNEL_FIRST, A.EPI_MAX_CHANNEL_FIRST, B * M * K, cin, x, again,
              M * K, a_L=M * K, a_amax=a[0], M=M, K=K)
    assert torch.equal(out, again)                # atomicMax merge: order-independent


def test_max_epilogue_needs_relu(dev):
    x = torch.randn(1, 4, 2, 8, device=dev)
    layer, _, _ = _layer(8, 4, dev, 0)
    with pytest.raises(RuntimeError, match="code -1"):
        A._launch(layer, A.PRECISIONS["fp32"], False, A.LOAD_CHANNEL_FIRST, A.EPI_MAX_CHANNEL_FIRST, 16, 4, x,
                  torch.zeros(1, 8, 2, device=dev), 16, a_L=16, M=2, K=8)
    assert _cabi.S4G_EINVAL == -1


def test_amax_per_scene(dev):
    x = torch.randn(5, 3, 1001, device=dev)
    x[3, 1, 17] = -40.0
    s = A._amax(x, 5)
    got = s.view(torch.float32).amax(dim=1)
    assert torch.equal(got, x.abs().flatten(1).amax(dim=1))


def test_abi_version(dev):
    assert _cabi.S4G_ABI_VERSION == 14 and _cabi.lib().s4g_abi_version() == 14
    assert _cabi.GemmDesc._fields_[-1][0] == "a_L"


# ----------------------------------------------------------------------------------------------- module level
@pytest.mark.parametrize("prec", ["f16x2", "fp32"])
def test_small_calibrated(dev, prec):
    g, net = _small_net()
    net = net.to(dev)
    assert len(s4g_release_amd.accelerate(net, precision=prec)) == 10
    feats = {}
    _hook_levels(net, feats)
    with torch.no_grad():
        pred = net({"scene_points": torch.from_numpy(g["points"]).to(dev)})
    _check_small(g, _np(pred), _np(feats))


@pytest.fixture(scope="module")
def full():
    g = GU.load("pn2_calib_full.npz")
    return g, GU.calib_full_model(g), GU.calib_scenes(g)


@pytest.mark.parametrize("prec", ["f16x2", "fp32"])
@pytest.mark.parametrize("scene", ["tabletop", "real"])
def test_full_calibrated(dev, full, scene, prec):
    g, net, scenes = full
    net = copy.deepcopy(net).to(dev)
    s4g_release_amd.accelerate(net, precision=prec)
    feats = {}
    _hook_levels(net, feats)
    with torch.no_grad():
        pred = net({"scene_points": torch.from_numpy(scenes[scene]).to(dev)})
    GU.calib_compare_full(g, scene, _np(pred), _np(feats))


GRAPHS = {
    # (every graph here has a feature FusedPointNet2 refuses: group-all / FP without 3-NN, or K outside {16, 32, 64})
    # the default-argument PointNet2 (group-all SA level, FP num_neighbours=0) at reduced centroid counts
    "default4": dict(score_classes=3, num_centroids=(512, 128, 32, 0)),
    "k8": dict(score_classes=3, num_centroids=(256, 64, 16), radius=(0.1, 0.2, 0.4), num_neighbours=(8, 8, 8),
               sa_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128)), fp_channels=((64, 64), (32, 32), (32, 32)),
               num_fp_neighbours=(3, 3, 3), seg_channels=(32,)),
    "k48": dict(score_classes=3, num_centroids=(256, 64, 16), radius=(0.1, 0.2, 0.4), num_neighbours=(48, 48, 48),
                sa_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128)), fp_channels=((64, 64), (32, 32), (32, 32)),
                num_fp_neighbours=(3, 3, 3), seg_channels=(32,)),
    "odd_widths": dict(score_classes=3, num_centroids=(256, 64, 16), radius=(0.1, 0.2, 0.4),
                       num_neighbours=(16, 12, 16), sa_channels=((13, 7, 33), (21, 35, 67), (45, 66, 131)),
                       fp_channels=((59, 37), (23, 29), (17, 19, 25)), num_fp_neighbours=(3, 3, 3),
                       seg_channels=(30, 11)),
}


def _graph_net(dev, cfg, seed, pts):
    torch.manual_seed(seed)
    net = PointNet2(**cfg).to(dev).eval()
    return GU.calibrated(net, seed, pts)


def _check_modules(net, pts):
    """Every converted module within 1e-4 of scale of a float64 evaluation on its captured fp32 input."""
    caps = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: caps.append((mod, args)))
             for m in net.modules() if hasattr(type(m), "_s4g_base")]
    with torch.no_grad():
        net({"scene_points": pts})
    for h in hooks:
        h.remove()
    assert caps
    for mod, args in caps:
        base = type(mod)._s4g_base
        with torch.no_grad():
            got = mod(*args)
            if hasattr(mod, "num_centroids"):
                _, group = sample_and_group(mod, *args)
                mlp64 = copy.deepcopy(mod.mlp).double()
                ref = mlp64(group.double()).amax(dim=3)
                got = got[1]
            else:
                m64 = copy.deepcopy(mod)
                m64.__class__ = base
                ref = m64.double()(args[0].double())
        assert _rel(got, ref) < 1e-4, (base.__name__, _rel(got, ref))


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_graphs_the_fused_path_refuses(dev, graph):
    from s4g_release_amd import synth
    cfg = GRAPHS[graph]
    pts = torch.from_numpy(synth.make_batch([0, 1], 2048)).to(dev)
    net = _graph_net(dev, cfg, 7, pts)
    with pytest.raises((NotImplementedError, ValueError)):
        FusedPointNet2(net)
    ref = copy.deepcopy(net)
    s4g_release_amd.accelerate(net)
    _check_modules(net, pts)
    with torch.no_grad():
        got, want = net({"scene_points": pts}), ref({"scene_points": pts})
    # The float64 bar is the per-module 1e-4 check above (tests/ref64.py has no group-all / FP-without-3-NN form for an
    # end-to-end float64 run).  End to end, two fp32-class paths on a freshly calibrated network: the 4-level default
    # graph compounds both paths' round-off through 11 re-normalised layers to 4.5e-4 .. 6.7e-4 of scale (measured on
    # two boxes); the 3-level graphs stay inside WIRING_TOL64.  A wiring error shows at >= 1e-2
    tol = 1e-3 if graph == "default4" else GU.WIRING_TOL64
    for k in GU.HEADS:
        assert _rel(got[k], want[k]) < tol, (graph, k, _rel(got[k], want[k]))


def test_two_d_head_on_n_by_1(dev):
    """The PointNet2_local shape: a 2-D SharedMLP grasp-evaluation head on (B, C, N, 1)."""
    torch.manual_seed(3)
    mlp = randomize_bn_(SharedMLP(37, (64, 32, 5), ndim=2), 4).to(dev).eval()
    x = torch.randn(2, 37, 1000, 1, device=dev)
    ref = copy.deepcopy(mlp).double()
    assert s4g_release_amd.accelerate(mlp) == [""]
    with torch.no_grad():
        got = mlp(x)
        want = ref(x.double())
    assert got.shape == (2, 5, 1000, 1)
    assert _rel(got, want) < 1e-4


def test_deterministic_and_batch_invariant(dev):
    """Two calls bit-identical; scene b of a 3-scene batch bit-identical to that scene alone (per-scene scales) -- at the
    output of every converted module (the logit Conv1d layers stay torch, whose kernels may pick another algorithm
    for another batch size)."""
    g, net = _small_net()
    net = net.to(dev)
    s4g_release_amd.accelerate(net)
    outs = []
    for name, m in net.named_modules():
        if hasattr(type(m), "_s4g_base"):
            m.register_forward_hook(lambda mod, a, out, name=name: outs.append((name, out[1] if isinstance(out, tuple)
                                                                               else out)))
    one = torch.from_numpy(g["points"][:1]).to(dev)
    from s4g_release_amd import synth
    n = one.shape[2]
    batch = torch.cat([torch.from_numpy(synth.make_batch([5], n)).to(dev), one,
                       torch.from_numpy(synth.make_batch([9], n)).to(dev)], dim=0)
    runs = []
    with torch.no_grad():
        for pts in (batch, batch, one):
            outs.clear()
            net({"scene_points": pts})
            runs.append(list(outs))
    assert len(runs[0]) == 10
    for (name, a), (_, b), (_, s) in zip(*runs):
        assert torch.equal(a, b), name
        assert torch.equal(a[1:2], s), name


def test_fallbacks_and_cache(dev):
    g, net = _small_net()
    net = net.to(dev)
    ref = copy.deepcopy(net)
    s4g_release_amd.accelerate(net)
    pts = torch.from_numpy(g["points"][:1]).to(dev)
    sa, mlp = net.sa_modules[1], net.mlp_seg
    rsa, rmlp = ref.sa_modules[1], ref.mlp_seg
    x = torch.randn(1, mlp.in_channels, 300, device=dev)
    # grad-enabled input, float64 and train(): the original forwards, bit for bit
    xg = x.clone().requires_grad_()
    assert torch.equal(mlp(xg), rmlp(xg))
    assert torch.equal(mlp.double()(x.double()), rmlp.double()(x.double()))
    mlp.float()
    rmlp.float()
    feat = torch.randn(1, sa.in_channels, pts.shape[2], device=dev)
    assert torch.equal(sa(pts, feat.clone().requires_grad_())[1], rsa(pts, feat)[1])
    net.train()
    ref.train()
    torch.manual_seed(0)
    y = mlp(x)
    torch.manual_seed(0)
    assert torch.equal(y, rmlp(x))
    with torch.no_grad():
        assert torch.equal(sa(pts, feat)[1], rsa(pts, feat)[1])
    net.eval()
    ref.eval()
    # load_state_dict of other weights: the outputs follow
    torch.manual_seed(11)
    other = PointNet2(**GU.small_config(g)).to(dev)
    randomize_bn_(other, 12)
    with torch.no_grad():
        net({"scene_points": pts})                # fold the old weights first
        net.load_state_dict(other.state_dict())
        ref.load_state_dict(other.state_dict())
        got, want = net({"scene_points": pts}), ref({"scene_points": pts})
    for k in GU.HEADS:
        assert _rel(got[k], want[k]) < GU.WIRING_TOL64, k


def test_no_torch_conv_bn_or_max_on_the_fast_path(dev, monkeypatch):
    g, net = _small_net()
    net = net.to(dev)
    s4g_release_amd.accelerate(net)
    pts = torch.from_numpy(g["points"]).to(dev)
    with torch.no_grad():
        xyz1, f1 = net.sa_modules[0](pts)
        xyz2, f2 = net.sa_modules[1](xyz1, f1)
        xyz3, f3 = net.sa_modules[2](xyz2, f2)

    def boom(*a, **k):
        raise AssertionError("torch library op on the accelerated path")
    for mod, name in ((F, "conv1d"), (F, "conv2d"), (F, "batch_norm"), (torch, "max")):
        monkeypatch.setattr(mod, name, boom)
    with torch.no_grad():
        _, f3b = net.sa_modules[2](xyz2, f2)
        out = net.fp_modules[0](xyz2, xyz3, f2, f3b)
    assert out.shape == (pts.shape[0], net.fp_modules[0].out_channels, xyz2.shape[2]) and torch.equal(f3b, f3)
