"""CPU: the edge network (`MODEL.TYPE: "EDGEPN2D"`, reference network_models/models/EdgePointNet2Down.py) -- model
layer, the fast path's fold of an edge level, and the calibrated fixture tests/golden/pn2_edge_calib_small.npz
(tools/gen_golden_edge.py) against the float64 forward of tests/edge64.py and its sabotaged variants.  The tests marked
for the reference tree run in the build container only (the reference is imported in a child process, over the oracle
stand-in)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from s4g_release_amd import model as M
from tests import edge64 as E
from tests import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/inference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
FIXTURE = "pn2_edge_calib_small.npz"
HEADS = ("scene_score_logits", "frame_R", "frame_t", "movable_logits")


def _fixture_net():
    g = GU.load(FIXTURE)
    net = M.EdgePointNet2Down(**GU.small_config(g))
    net.load_state_dict(GU.small_state_dict(g), strict=True)
    return g, net.eval()


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.fixture(scope="module")
def honest():
    g = GU.load(FIXTURE)
    return g, E.edge_forward64(GU.small_state_dict(g), g["points"], GU.small_config(g))


def test_build_model_edge():
    net = M.build_model("EDGEPN2D")
    assert type(net) is M.EdgePointNet2Down and isinstance(net, M.ContactPointNet2)
    sd = net.state_dict()
    assert len(sd) == 200
    # level 0 has no features; from level 1 on the first conv takes [xyz | f_j | f_j - f_c] = 2 C + 3 inputs
    assert [tuple(sd["sa_modules.%d.mlp.0.conv.weight" % i].shape) for i in range(3)] == \
        [(128, 3, 1, 1), (256, 2 * 256 + 3, 1, 1), (512, 2 * 512 + 3, 1, 1)]
    contact = M.build_model("PN2").state_dict()
    assert list(contact) == list(sd)
    # every other entry has the contact model's shape
    edge_convs = {"sa_modules.1.mlp.0.conv.weight", "sa_modules.2.mlp.0.conv.weight"}
    assert {k for k in sd if contact[k].shape != sd[k].shape} == edge_convs
    assert tuple(sd["R_logit.weight"].shape) == (6, 128, 1) and float(sd["t_logit.weight"].abs().max()) == 0.0
    for bad in ("EDGEPN2DU", "PN2_LOCAL", "edgepn2d"):
        with pytest.raises(ValueError):
            M.build_model(bad)


def test_edge_sa_module_constructor_variants():
    from s4g_release_amd.modules import EdgeQueryGrouper, EdgeSAModule
    m = EdgeSAModule(16, (8, 8), 4, 0.1, 16, True)
    assert m.mlp[0].conv.in_channels == 35 and isinstance(m.grouper, EdgeQueryGrouper) and m.sampler.num_centroids == 4
    assert EdgeSAModule(16, (8,), -1, 0.1, 16, False).mlp[0].conv.in_channels == 32     # every point its own centroid
    g = EdgeSAModule(16, (8,), 0, -1.0, -1, True)                                         # group all: no edge term
    assert g.mlp[0].conv.in_channels == 19 and g.grouper is None and g.sampler is None
    assert EdgeSAModule(0, (8,), 4, 0.1, 16, True).mlp[0].conv.in_channels == 3


@needs_ref
def test_state_dict_layout_equals_the_reference_edge_network():
    code = ("import sys, json; sys.path.insert(0, %r); from tools import gen_golden_edge as C; "
            "from tools.gen_golden import FULL; Net, _ = C.setup(); "
            "print(json.dumps({k: list(v.shape) for k, v in Net(**FULL).state_dict().items()}))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    ref = json.loads(out.stdout.strip().splitlines()[-1])
    ours = {k: list(v.shape) for k, v in M.build_model("EDGEPN2D").state_dict().items()}
    assert list(ours) == list(ref)
    assert ours == ref


@needs_ref
def test_committed_edge_fixture_is_what_the_reference_network_produces(tmp_path):
    """Provenance: tools/gen_golden_edge.py re-run here (child process) gives the committed fixture array for array."""
    code = ("import sys; sys.path.insert(0, %r); from tools import gen_golden_edge as C; C.gen_small(%r)"
            % (ROOT, str(tmp_path)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    new = np.load(os.path.join(str(tmp_path), FIXTURE), allow_pickle=False)
    old = GU.load(FIXTURE)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if old[k].dtype.kind in "fc":
            assert np.allclose(new[k], old[k], rtol=0, atol=2e-6 * max(1.0, float(np.abs(old[k]).max()))), k
        else:
            assert np.array_equal(new[k], old[k]), k


@needs_ref
def test_fast_path_packs_the_reference_edge_instance_like_ours():
    """The reference's own `EdgePointNet2Down` object (it keeps no `in_channels` on its SA modules) folds and packs to
    the very tensors `model.EdgePointNet2Down` with the same state_dict gives."""
    code = """
import sys, torch
sys.path.insert(0, %r)
from tools import gen_golden_edge as C
from tools.gen_golden import SMALL
from s4g_release_amd.fused import FusedPointNet2
from s4g_release_amd.model import EdgePointNet2Down, calibrate_bn_
from s4g_release_amd import synth
Net, _ = C.setup()
torch.manual_seed(5)
ref = Net(**SMALL)
calibrate_bn_(ref, 6, {"scene_points": torch.from_numpy(synth.make_batch([1], 2048))})
ours = EdgePointNet2Down(**SMALL)
ours.load_state_dict(ref.state_dict(), strict=True)
a, b = FusedPointNet2(ref, fold_only=True), FusedPointNet2(ours.eval(), fold_only=True)
assert a.kind == b.kind == "PN2" and [s["edge"] for s in a.sa] == [s["edge"] for s in b.sa] == [False, True, True]
wa, wb = a.packed_weights(), b.packed_weights()
assert sorted(wa) == sorted(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
assert "sa1.pre.lc.W" in wa and "sa0.pre.lc.W" not in wa
print("OK", len(wa))
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1].startswith("OK")


def test_fixture_is_not_degenerate():
    """Per-point spread as tools/gen_golden_calib.spread_check: every channel's std over the points >= 0.05 of its own
    magnitude (outputs, raw logits) -- and the stored SA slices, where the edge term lives, likewise in the median."""
    g = GU.load(FIXTURE)
    for k in ("out/scene_score_logits", "out/frame_R", "out/movable_logits", "raw/R6", "raw/t"):
        a = g[k].astype(np.float64)
        assert (a.std(axis=2) / np.abs(a).max(axis=2)).min() >= 0.05, k
    for li in range(3):
        a = g["feat/sa%d" % li].astype(np.float64)
        mag = np.abs(a).max(axis=2)
        assert np.median((a.std(axis=2) / np.where(mag > 0, mag, 1.0))[mag > 0]) >= 0.05, li
    assert np.abs(g["raw/t"]).max() > 0.05          # the t head was re-seeded: frame_t != points
    assert os.path.getsize(os.path.join(GU.GOLDEN, FIXTURE)) < 1 << 20


def test_float64_forward_is_within_tolerance_of_the_fixture(honest):
    """The honest float64 forward against the reference network's own fp32 outputs: within GU.CALIB_TOL of scale."""
    g, ref = honest
    for k in ("scene_score_logits", "movable_logits", "frame_t"):
        e = _rel(g["out/" + k], ref[k])
        print("fixture (torch fp32) vs float64, %-20s %.2e of scale" % (k, e))
        assert e < GU.CALIB_TOL, (k, e)
    for k in ("raw/R6", "raw/t"):
        e = _rel(g[k], ref[k])
        print("fixture (torch fp32) vs float64, %-20s %.2e of scale" % (k, e))
        assert e < GU.CALIB_TOL, (k, e)
    for li in range(3):
        lv = "sa%d" % li
        want = ref["feat/" + lv][:, g["featch/" + lv]][:, :, g["featpos/" + lv]]
        e = _rel(g["feat/" + lv], want)
        print("fixture (torch fp32) vs float64, feat/%-15s %.2e of scale" % (lv, e))
        assert e < GU.CALIB_TOL, (lv, e)


@pytest.mark.parametrize("name", sorted(E.SABOTAGES))
def test_every_sabotage_misses_the_fixture(honest, name):
    """A forward that is wrong in one way (tests/edge64.SABOTAGES) is at least 100 x GU.CALIB_TOL of scale away from
    the fixture in some output: the fixture can tell each of these mistakes from the honest forward."""
    g, _ = honest
    bad = E.edge_forward64(GU.small_state_dict(g), g["points"], GU.small_config(g), sabotage=name)
    errs = {k: _rel(g["out/" + k], bad[k]) for k in ("scene_score_logits", "movable_logits")}
    errs["raw/R6"] = _rel(g["raw/R6"], bad["raw/R6"])
    print(name, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) >= 100 * GU.CALIB_TOL, (name, errs)


def test_the_fold_of_an_edge_level_is_an_identity_in_float64():
    """W . [rel | f_j | f_j - f_c] + b == W_x . rel + (W_a + W_b) . f_j + (b - W_b . f_c): the three pieces
    `FusedPointNet2(..., fold_only=True)` makes, applied in float64 to random rows, against the unfused first layer
    (conv -> eval BatchNorm, float64) to 1e-12 of scale; the launched fp32 tensors are those pieces rounded ONCE."""
    from s4g_release_amd.fused import FusedPointNet2, fold_conv_bn
    g, net = _fixture_net()
    f = FusedPointNet2(net, fold_only=True)
    assert f.kind == "PN2" and [s["edge"] for s in f.sa] == [False, True, True]
    rng = np.random.default_rng(9)
    for li in (1, 2):
        sa, blk = f.sa[li], net.sa_modules[li].mlp[0]
        cf = sa["cf"]
        assert blk.conv.in_channels == 2 * cf + 3
        rows = 257
        rel = torch.from_numpy(rng.uniform(-1, 1, (rows, 3)) * sa["radius"])
        fj = torch.from_numpy(rng.standard_normal((rows, cf)) * 3.0)
        fc = torch.from_numpy(rng.standard_normal((rows, cf)) * 3.0)
        # the unfused layer, as the module computes it: conv, then eval BatchNorm, in float64
        x = torch.cat([rel, fj, fj - fc], dim=1)
        y = x @ blk.conv.weight.detach().double().flatten(1).T
        bn = blk.bn
        y = (y - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.detach().double() \
            + bn.bias.detach().double()
        p64 = sa["pre"]["fold64"]
        z = rel @ p64["w1"][:, :3].T + fj @ p64["la"].T + (fc @ p64["lc"].T + p64["w1"][:, 3])
        scale = float(y.abs().max())
        assert float((y - z).abs().max()) <= 1e-12 * scale, (li, float((y - z).abs().max()), scale)
        # what the launches read: each piece rounded once from float64
        pre = sa["pre"]
        assert torch.equal(pre["la"].W[:, :cf], p64["la"].float()) and float(pre["la"].bias.abs().max()) == 0.0
        assert torch.equal(pre["lc"].W[:, :cf], p64["lc"].float())
        assert torch.equal(pre["lc"].bias, p64["w1"][:, 3].float())
        assert torch.equal(pre["w1"], p64["w1"].float())
        w32, b32 = fold_conv_bn(blk)
        assert torch.equal(pre["w1"][:, :3], w32[:, :3]) and torch.equal(pre["w1"][:, 3], b32)
        # the loader's floor is the xyz term alone
        assert sa["pre"]["bound"] == float((pre["w1"][:, :3].abs().sum(dim=1) * sa["radius"]).max())


def test_fast_path_limits_on_an_edge_level(monkeypatch):
    from s4g_release_amd.fused import FusedPointNet2
    cfg = dict(GU.small_config(GU.load(FIXTURE)), sa_channels=((16, 16, 30), (32, 32, 64), (64, 64, 128)))
    net = M.EdgePointNet2Down(**cfg).eval()
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        FusedPointNet2(net, fold_only=True)
    _, net = _fixture_net()
    monkeypatch.setenv("S4G_TEST_KNOBS", "1")
    monkeypatch.setenv("S4G_SA_LINEAR_FIRST", "0")
    with pytest.raises(NotImplementedError, match="linear-first"):
        FusedPointNet2(net, fold_only=True)
