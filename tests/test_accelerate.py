"""CPU tests of `s4g_release_amd.accelerate`: which modules it converts (by structure), that the conversion keeps
identity, `isinstance` and the `state_dict`, and that a converted module off the fast path (here: the CPU) computes
bit for bit what the unconverted one does.  The fast path itself is tested on the GPU (test_accelerate_gpu.py)."""
import copy
import os
import sys

import pytest
import torch

import s4g_release_amd
from s4g_release_amd.model import ContactPointNet2, PointNet2, S4GConfig, randomize_bn_
from s4g_release_amd.nn_utils import SharedMLP

SHIPPED = ["sa_modules.0", "sa_modules.1", "sa_modules.2", "fp_modules.0.mlp", "fp_modules.1.mlp",
           "fp_modules.2.mlp", "mlp_seg", "mlp_R", "mlp_t", "mlp_movable"]


def _same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("cls", [PointNet2, ContactPointNet2])
def test_converts_the_shipped_network(cls):
    torch.manual_seed(0)
    net = randomize_bn_(cls(**S4GConfig().model_kwargs()), 1).eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    mods = dict(net.named_modules())
    names = s4g_release_amd.accelerate(net)
    assert names == SHIPPED
    _same_state(before, net.state_dict())
    after = dict(net.named_modules())
    assert all(after[k] is mods[k] for k in mods)          # identity: the same objects, in place
    for n in names:
        base = type(mods[n]).__mro__[1]
        assert isinstance(after[n], base) and type(after[n]) is not base
    assert isinstance(net.sa_modules[0], s4g_release_amd.modules.PointNetSAModule)
    assert isinstance(net.mlp_seg, SharedMLP) and isinstance(net.sa_modules[0].mlp, SharedMLP)
    assert type(net.sa_modules[0].mlp) is SharedMLP          # run by its SA module, not converted on its own
    # converting again changes nothing and names the same modules
    assert s4g_release_amd.accelerate(net, precision="fp32") == SHIPPED
    _same_state(before, net.state_dict())


def test_converts_the_default_argument_network():
    net = PointNet2(score_classes=3).eval()
    names = s4g_release_amd.accelerate(net)
    assert names == (["sa_modules.%d" % i for i in range(4)] + ["fp_modules.%d.mlp" % i for i in range(4)] +
                     ["mlp_seg", "mlp_R", "mlp_t", "mlp_movable"])


@pytest.mark.parametrize("ndim,shape", [(1, (2, 7, 33)), (2, (2, 7, 5, 9))])
def test_converted_shared_mlp_is_bit_identical_off_the_fast_path(ndim, shape):
    torch.manual_seed(1)
    mlp = randomize_bn_(SharedMLP(7, (13, 6), ndim=ndim), 2).eval()
    ref = copy.deepcopy(mlp)
    assert s4g_release_amd.accelerate(mlp) == [""]
    x = torch.randn(shape)
    with torch.no_grad():
        assert torch.equal(mlp(x), ref(x))                  # CPU input: the original forward
    assert torch.equal(mlp.double()(x.double()), ref.double()(x.double()))   # float64: the original forward too
    mlp.train()
    ref.train()
    torch.manual_seed(3)
    y = mlp.float()(x)
    torch.manual_seed(3)
    assert torch.equal(y, ref.float()(x))


def test_bad_precision_raises():
    with pytest.raises(ValueError):
        s4g_release_amd.accelerate(SharedMLP(3, (4,)), precision="bf16")
    with pytest.raises(ValueError):
        s4g_release_amd.accelerate(SharedMLP(3, (4,)), precision="f16")


def test_unrecognised_modules_are_left_alone():
    seq = torch.nn.ModuleList([torch.nn.Conv1d(3, 4, 1)])          # blocks without .conv / .bn / .relu
    grouped = SharedMLP(4, (8,))
    grouped[0].conv = torch.nn.Conv1d(4, 8, 1, groups=2, bias=False)
    wide = SharedMLP(4, (8,))
    wide[0].conv = torch.nn.Conv1d(4, 8, 3, bias=False)
    for m in (seq, grouped, wide):
        assert s4g_release_amd.accelerate(m) == []


REF = "/root/reference/inference"
EXT = "grasp_proposal.network_models.models.pointnet2_utils.pn2_ext"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_reference_instance_converts_the_same_set():
    """The reference's own PointNet2_tcls.PointNet2, imported over our extension shim as tests/test_reference_dropin.py
    does."""
    from s4g_release_amd import pn2_ext as ours
    saved = {k: v for k, v in sys.modules.items() if k.startswith("grasp_proposal")}
    for k in saved:
        del sys.modules[k]
    sys.modules[EXT] = ours
    sys.path.insert(0, REF)
    try:
        from grasp_proposal.network_models.models import PointNet2_tcls
        torch.manual_seed(0)
        net = randomize_bn_(PointNet2_tcls.PointNet2(**S4GConfig().model_kwargs()), 1).eval()
        before = {k: v.clone() for k, v in net.state_dict().items()}
        sa_cls = type(net.sa_modules[0])
        assert s4g_release_amd.accelerate(net) == SHIPPED
        _same_state(before, net.state_dict())
        assert isinstance(net.sa_modules[0], sa_cls) and type(net.sa_modules[0]) is not sa_cls
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k.startswith("grasp_proposal")]:
            del sys.modules[k]
        sys.modules.update(saved)
