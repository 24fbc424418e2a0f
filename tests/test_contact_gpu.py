"""GPU: the contact network (`MODEL.TYPE: "PN2"`) end to end -- the output-tail kernel `s4g_contact_heads_f32` against
float64, the calibrated small fixture (tests/golden/pn2_contact_calib_small.npz: the reference's own PointNet2.py) through
the modules path and the fast path in three precisions, the shipped configuration (fused heads, batch invariance, graph
replay, top-K), and the decode / detector on its predictions."""
import ctypes

import numpy as np
import pytest
import torch

from tests import golden_util as GU
from tests.contact64 import contact_forward64, rot6d_to_matrix64, shipped_contact_net

pytestmark = pytest.mark.gpu
HEADS = ("scene_score_logits", "frame_R", "frame_t", "movable_logits")


def _contact_heads(raw, xyz, index=None):
    from s4g_release_amd import _cabi
    B, _, M = raw.shape
    out = torch.full((B, 20, M), -7.0, dtype=torch.float32, device=raw.device)
    rc = _cabi.lib().s4g_contact_heads_f32(raw.data_ptr(), xyz.data_ptr(), None if index is None else index.data_ptr(),
                                           B, xyz.shape[2], M, out.data_ptr(), ctypes.c_void_p(0))
    _cabi.check(rc, "contact_heads")
    torch.cuda.synchronize()
    return out


def _random_raw(B, M, seed):
    """(B, 17, M) raw logits: 6-D rotation logits of magnitudes 1e-3 .. 1e3 (per point), offsets, score, movable."""
    g = np.random.default_rng(seed)
    raw = g.standard_normal((B, 17, M)).astype(np.float32)
    mag = 10.0 ** g.uniform(-3, 3, (B, 2, M))
    raw[:, 3:6] *= mag[:, :1]
    raw[:, 6:9] *= mag[:, 1:]
    raw[:, 9:12] *= 0.05
    raw[:, 12:17] = 1 / (1 + np.exp(-raw[:, 12:17]))
    return raw.astype(np.float32)


def _check_rotations(R, R64, pre, a2n, tol=2e-6):
    """R (B, 9, M) fp32 against float64.  The map amplifies the fp32 rounding of its inputs where a2 is nearly parallel
    to a1: b2 = a2 - (a2.b1) b1 cancels, so b2's error grows as |a2| / |b2 before normalising|.  Points where that
    pre-norm is below 0.05 |a2| are left out (and counted); elsewhere the bounds hold as stated up to pre-norm |a2| / 4
    and scale with |a2| / (4 pre-norm) below it (a float32 emulation of the kernel's arithmetic: error 1.2e-6,
    |R^T R - I| 1.2e-6, |det R - 1| 4.4e-7 after that scaling)."""
    mask = pre >= 0.05 * a2n
    amp = np.maximum(1.0, 0.25 * a2n / pre)[mask]
    err = np.abs(R.astype(np.float64) - R64).max(axis=1)[mask]
    assert (err / amp).max() <= tol, (err / amp).max()
    Rm = R.astype(np.float64).transpose(0, 2, 1).reshape(-1, 3, 3)[mask.reshape(-1)]      # R[i][j] = channel 3i + j
    orth = np.abs(np.einsum("kji,kjl->kil", Rm, Rm) - np.eye(3)).max(axis=(1, 2))
    det = np.abs(np.linalg.det(Rm) - 1)
    assert (orth / amp).max() < 2e-6 and det.max() < 1e-6, ((orth / amp).max(), det.max())
    return 1 - mask.mean()


@pytest.mark.parametrize("with_index", [False, True])
def test_contact_heads_kernel_against_float64(dev, with_index):
    B, M = 3, 40000 - 13
    N = M if not with_index else 50000
    raw = _random_raw(B, M, 11 + with_index)
    xyz = np.random.default_rng(3).uniform(-1, 1, (B, 3, N)).astype(np.float32)
    idx = None
    if with_index:
        idx = np.stack([np.random.default_rng(20 + b).choice(N, M, replace=False) for b in range(B)]).astype(np.int64)
    out = _contact_heads(torch.from_numpy(raw).to(dev), torch.from_numpy(xyz).to(dev),
                         None if idx is None else torch.from_numpy(idx).to(dev)).cpu().numpy()
    assert np.array_equal(out[:, :3], raw[:, :3]) and np.array_equal(out[:, 15:], raw[:, 12:])     # bit copies
    p = xyz if idx is None else np.stack([xyz[b][:, idx[b]] for b in range(B)])
    assert np.array_equal(out[:, 12:15], (torch.from_numpy(p) + torch.from_numpy(raw[:, 9:12])).numpy())   # fp32 add
    R64, pre = rot6d_to_matrix64(raw[:, 3:9])
    frac = _check_rotations(out[:, 3:12], R64, pre, np.linalg.norm(raw[:, 6:9].astype(np.float64), axis=1))
    print("near-parallel points left out: %.4f" % frac)
    assert frac < 0.01


def test_contact_heads_degenerate_rows_are_nan_and_contained(dev):
    B, M = 1, 300
    raw = _random_raw(B, M, 5)
    xyz = np.random.default_rng(6).uniform(-1, 1, (B, 3, M)).astype(np.float32)
    clean = _contact_heads(torch.from_numpy(raw).to(dev), torch.from_numpy(xyz).to(dev)).cpu().numpy()
    bad = raw.copy()
    bad[0, 3:9, 10] = 0.0                                         # zero a1
    bad[0, 3:9, 77] = [3.0, 0.0, 0.0, -5.0, 0.0, 0.0]             # a2 parallel to a1: b2 = 0 exactly
    bad[0, 3:9, 78] = [0.0, 4.0, 0.0, 0.0, 7.0, 0.0]
    out = _contact_heads(torch.from_numpy(bad).to(dev), torch.from_numpy(xyz).to(dev)).cpu().numpy()
    for m in (10, 77, 78):
        assert np.isnan(out[0, 3:12, m]).any(), m
        assert np.array_equal(out[0, :3, m], clean[0, :3, m]) and np.array_equal(out[0, 12:, m], clean[0, 12:, m])
    keep = np.setdiff1d(np.arange(M), [10, 77, 78])
    assert np.array_equal(out[..., keep], clean[..., keep])
    # torch's toRotMatrix gives NaN at the same points
    from s4g_release_amd.model import to_rot_matrix
    t = to_rot_matrix(torch.from_numpy(bad[:, 3:9]).to(dev)).cpu().numpy()
    assert np.array_equal(np.isnan(t).any(axis=1), np.isnan(out[:, 3:12]).any(axis=1))


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.fixture(scope="module")
def small():
    from s4g_release_amd.model import ContactPointNet2
    g = GU.load("pn2_contact_calib_small.npz")
    cfg = GU.small_config(g)
    sd = GU.small_state_dict(g)
    net = ContactPointNet2(**cfg)
    net.load_state_dict(sd, strict=True)
    return g, net.eval(), contact_forward64(sd, g["points"], cfg)


@pytest.mark.parametrize("path", ["modules", "f16x2", "bf16x3", "fp32"])
def test_small_fixture_four_routes(dev, small, path):
    from s4g_release_amd.fused import FusedPointNet2, PackedPred
    g, net, ref = small
    net = net.to(dev)
    pts = torch.from_numpy(g["points"]).to(dev)
    inter = None
    with torch.no_grad():
        if path == "modules":
            pred = net({"scene_points": pts})
        else:
            pred, inter = FusedPointNet2(net, precision=path)({"scene_points": pts}, return_intermediates=True)
            assert isinstance(pred, PackedPred) and pred.packed.shape == (2, 20, 2048)
    torch.cuda.synchronize()
    assert sorted(pred) == sorted(HEADS)
    got = {k: pred[k].cpu().numpy() for k in HEADS}
    if inter is not None:
        for li in range(3):
            for n in ("fps", "ball", "cnt", "nn"):
                assert np.array_equal(inter["%s%d" % (n, li)].cpu().numpy().astype(np.int64),
                                      g["%s%d" % (n, li)].astype(np.int64)), (n, li)
    # score / movable: as tests/test_calib_gpu.py -- within 1e-4 of scale of float64, and of the fixture within 1e-4 +
    # the fixture's own distance from float64
    for k in ("scene_score_logits", "movable_logits"):
        e64, efx = _rel(got[k], ref[k]), _rel(got[k], g["out/" + k])
        margin = _rel(g["out/" + k], ref[k])
        print(path, k, "vs float64 %.1e, vs fixture %.1e (fixture %.1e)" % (e64, efx, margin))
        assert e64 < GU.CALIB_TOL and efx < GU.CALIB_TOL + margin, (k, e64, efx)
    et = _rel(got["frame_t"], ref["frame_t"])
    assert et < GU.CALIB_TOL, et
    # frame_R: against float64 toRotMatrix of the float64 6-D logits.  Where b2 before normalising is >= 0.05 |a2|,
    # the error may be the 6-D logits' error (<= 1e-4 of their scale) times the map's sensitivity there
    # kappa = 1/|a1| + (1 + |a2|/|a1|) / |b2 pre-norm|
    a1n = np.linalg.norm(ref["raw/R6"][:, :3], axis=1)
    a2n = np.linalg.norm(ref["raw/R6"][:, 3:6], axis=1)
    mask = ref["b2_prenorm"] >= 0.05 * a2n
    kappa = 1 / a1n + (1 + a2n / a1n) / ref["b2_prenorm"]
    delta = GU.CALIB_TOL * max(1.0, float(np.abs(ref["raw/R6"]).max()))
    err = np.abs(got["frame_R"].astype(np.float64) - ref["frame_R"]).max(axis=1)
    ratio = err[mask] / (delta * kappa[mask])
    print(path, "frame_R: masked fraction %.4f, max err %.1e, max err / bound %.2f" % (1 - mask.mean(), err[mask].max(),
                                                                                      ratio.max()))
    assert ratio.max() < 1.0 and 1 - mask.mean() < 0.01


def _fused_route_net(dev):
    from s4g_release_amd.fused import FusedPointNet2
    run = FusedPointNet2(shipped_contact_net(dev))
    assert run.kind == "PN2" and run.heads_fused is not None          # the one-launch heads (shipped widths)
    return run


def test_shipped_config_batch_invariance_and_graph_replay(dev):
    from s4g_release_amd import synth
    run = _fused_route_net(dev)
    pts = torch.from_numpy(synth.make_batch(list(range(16)), 25600)).to(dev)
    full = run({"scene_points": pts})
    assert full.packed.shape == (16, 20, 25600)
    # every scene equals itself alone (as tests/test_batch_invariance_gpu.py: <= 1e-6, bit-identical in practice;
    # frame_R is the 6-D map of such logits, which amplifies a difference by up to ~1/|a1|)
    for b in (0, 9, 15):
        one = run({"scene_points": pts[b:b + 1].contiguous()})
        for k in HEADS:
            assert (one[k][0] - full[k][b]).abs().max().item() <= (1e-4 if k == "frame_R" else 1e-6), (b, k)
    R = full["frame_R"].double().permute(0, 2, 1).reshape(-1, 3, 3)
    assert torch.isfinite(R).all()
    assert (torch.linalg.det(R) - 1).abs().max().item() < 1e-5
    t = full["frame_t"] - pts
    assert t.abs().max().item() > 0.01                                  # the t head is live
    gr = run.graph({"scene_points": pts})
    rep = gr({"scene_points": pts})
    torch.cuda.synchronize()
    for k in HEADS:
        assert torch.equal(rep[k], full[k]), k


def test_shipped_config_topk_equals_the_full_forward_at_the_kept_points(dev):
    from s4g_release_amd import synth
    run = _fused_route_net(dev)
    pts = torch.from_numpy(synth.make_batch([3, 4], 25600)).to(dev)
    full = run({"scene_points": pts})
    K = 1024
    kept = run({"scene_points": pts}, topk=K)
    assert kept.packed.shape == (2, 20, K) and kept["index"].shape == (2, K)
    idx = kept["index"]
    # the kept points' values are the full forward's up to the hidden layers' per-tile scales (as
    # tests/test_sparse_heads_gpu.py: 2e-5 of scale); frame_R is the 6-D map of such logits (sensitivity ~1/|a1|)
    for k in HEADS:
        want = torch.gather(full[k], 2, idx.unsqueeze(1).expand(-1, full[k].shape[1], -1))
        err = (kept[k] - want).abs().max().item()
        assert err < (1e-3 if k == "frame_R" else 2e-5) * max(1.0, want.abs().max().item()), (k, err)
    assert torch.equal(kept["scene_score_logits"],
                       torch.gather(full["scene_score_logits"], 2, idx.unsqueeze(1).expand(-1, 3, -1)))
    # pipelined submissions give what the sequential calls give
    hs = [run.submit({"scene_points": pts}, topk=K) for _ in range(2)]
    for h in hs:
        r = h.result()
        for k in HEADS:
            assert torch.equal(r[k], kept[k]), k


def test_detect_poses_equals_a_float64_host_composition(dev):
    from s4g_release_amd import postprocess as PP, synth
    run = _fused_route_net(dev)
    pts = torch.from_numpy(synth.make_batch([5, 6], 25600)).to(dev)
    pred = run({"scene_points": pts})
    es = PP.expected_score(pred["scene_score_logits"].contiguous(), "detector")
    thr = float(torch.sort(es, dim=1, descending=True)[0][:, 500].max())
    A = np.linalg.qr(np.random.default_rng(4).standard_normal((3, 3)))[0]
    vthr = 0.0
    H, score, index, count = PP.detect_poses(pred, pts, score_threshold=thr, verticalness_threshold=vthr,
                                             direction_matrix=A, max_poses=1024)
    assert int(count.min()) > 0
    host = {k: v.cpu().numpy().astype(np.float64) for k, v in pred.items()}
    es_h = es.cpu().numpy()
    fr = np.asarray(PP.TRAIN2REAL, dtype=np.float64)
    for b in range(2):
        R = host["frame_R"][b].reshape(3, 3, -1)                       # R[i][j][n]
        vert = (-(A @ R[:, 0, :])).T @ np.array([0.0, 0.0, 1.0])
        ok = (es_h[b] > thr) & (vert > vthr)
        # (the device's verticalness is an fp32 dot product: keep only points clear of the threshold)
        n = int(count[b])
        sel = index[b, :n].cpu().numpy()
        assert set(sel.tolist()) <= set(np.nonzero(ok | (np.abs(vert - vthr) < 1e-5))[0].tolist())
        assert abs(n - int(ok.sum())) <= int((np.abs(vert - vthr) < 1e-5).sum())
        assert np.all(np.diff(es_h[b][sel]) <= 0)                       # best first
        for j, p in enumerate(sel[:200]):
            Rm = R[:, :, p]
            x = Rm[:, 0] / np.linalg.norm(Rm[:, 0])
            y = Rm[:, 1] - (x @ Rm[:, 1]) * x
            y /= np.linalg.norm(y)
            Hh = np.eye(4)
            Hh[:3, 0], Hh[:3, 1], Hh[:3, 2], Hh[:3, 3] = x, y, np.cross(x, y), host["frame_t"][b][:, p]
            Hh = fr @ Hh
            assert np.abs(H[b, j].cpu().numpy() - Hh).max() < 2e-5, (b, j)
        assert float(score[b, :n].cpu().numpy().max()) <= 1.0
    # decode_top_poses takes the same translation
    Ht, _, st = PP.decode_top_poses(pred, pts, 20)
    p = st[0, 0].item()
    assert torch.equal(Ht[0, 0, :3, 3], pred["frame_t"][0, :, p])


def test_grasp_detector_on_the_contact_network(dev):
    from s4g_release_amd import synth
    from s4g_release_amd.detector import GraspDetector
    t = synth.make_batch([8], 30000)[0]
    cloud = np.stack([t[1], t[0], -t[2]], axis=0).T                   # (n, 3), REAL frame
    cl = torch.from_numpy(np.ascontiguousarray(cloud.T[None])).float().to(dev)
    # (the importance sampling's draws passed in: without them every call draws its own)
    kw = dict(num_selected=5, score_threshold=0.5, verticalness_threshold=-1.0,
              uniforms=np.random.default_rng(2).random(5))
    cls = GraspDetector(GU.shipped_net(dev), topk=2048, seed=1)      # a curvature-model detector in the same process
    before = [x.clone() for x in cls.detect_device(cl, **kw)]
    det = GraspDetector(shipped_contact_net(dev), topk=2048, seed=1)
    for collision_check in (True, False):
        poses, scores = det.detect(cloud, num_selected=5, score_threshold=0.5, verticalness_threshold=-1.0,
                                   collision_check=collision_check)
        torch.cuda.synchronize()
        P = poses.double().cpu().numpy()
        assert P.shape[1:] == (4, 4) and P.shape[0] == scores.shape[0] <= 5
        if not collision_check:                  # (whether any pose survives the collision check depends on the net)
            assert P.shape[0] == 5
        R = P[:, :3, :3]
        assert np.abs(np.einsum("kji,kjl->kil", R, R) - np.eye(3)).max(initial=0) < 1e-5
        assert np.abs(np.linalg.det(R) - 1).max(initial=0) < 1e-5
        assert np.array_equal(P[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (P.shape[0], 1)))
    # graph capture of the whole call replays the eager result
    eager = det.detect_device(cl, **kw)
    gr = det.graph(cl, **kw)
    rep = gr(cl)
    torch.cuda.synchronize()
    assert torch.equal(rep[2], eager[2]) and torch.equal(rep[0], eager[0])
    # the curvature-model detector is unaffected: same detections as before the contact one ran
    assert cls.run.kind == "PN2_CLS"
    after = cls.detect_device(cl, **kw)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    pred = cls.run({"scene_points": cls.pre_processing(cl)}, topk=2048)
    assert "score" in pred and pred.packed.shape[1] == 21
