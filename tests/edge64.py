"""float64 yardstick of the EDGE network (`MODEL.TYPE: "EDGEPN2D"`) -- TEST INFRASTRUCTURE ONLY.

Written from the reference's statements (pointnet2_utils/modules.py:63-93, 407-475), NOT from the fast path's fold:
the grouped tensor of a level with features is the explicit concatenation [xyz_j - c_m | f_j | f_j - f_c(m)], with
f_c = the feature of the point FPS picked (`gather_points(feature, index)`), and the level's whole first conv is
applied to it.  Everything else is tests/ref64.py (float64 arithmetic on fp32 geometry through the C oracle, so the
indices are the reference's) and tests/contact64.py (toRotMatrix and points + offsets in float64).

`SABOTAGES` are forwards that are wrong in ONE way each -- the mistakes an implementation of the per-centroid term can
make; tests require the fixture to tell every one of them from the honest forward."""
import numpy as np
import torch

from oracle import oracle as O
from tests.contact64 import rot6d_to_matrix64
from tests.ref64 import _mlp

# name -> what is wrong
SABOTAGES = {
    "edge_dropped": "the edge block f_j - f_c replaced by zeros",
    "fc_next_centroid": "f_c taken from centroid m + 1 of the same scene",
    "fc_neighbour_row": "f_c taken from the neighbour's own row (f_c = f_j)",
    "sign_flipped": "the edge block is f_c - f_j",
    "blocks_swapped": "the weight blocks W_a and W_b swapped",
    "order_swapped": "channel order [xyz | f_j - f_c | f_j]",
    "fc_previous_level": "f_c read from the previous level's feature tensor (its channels tiled to the width)",
    "edge_level1_only": "the edge term applied at level 0's successor only, zeros at the deeper levels",
    "fc_next_scene": "the per-centroid term taken across the scene boundary (f_c of scene b + 1)",
}


def _heads64(sd, x):
    out = {}
    for name, mlp, logit in (("score", "mlp_seg", "seg_logit"), ("frame_R", "mlp_R", "R_logit"),
                             ("frame_t", "mlp_t", "t_logit"), ("movable_logits", "mlp_movable", "movable_logit.0")):
        h = _mlp(x, sd, mlp)
        o = sd[logit + ".weight"].double().flatten(1) @ h + sd[logit + ".bias"].double()[:, None]
        out[name] = (torch.sigmoid(o) if name == "movable_logits" else o).numpy()
    return out


def edge_forward64(state_dict, points, cfg, sabotage=None):
    """points (B, 3, N) float32 numpy -> {"scene_score_logits", "frame_R", "frame_t", "movable_logits", "raw/R6",
    "raw/t", "b2_prenorm", "feat/sa{l}" (B, C, M)} float64 numpy.  sabotage: a key of `SABOTAGES` or None."""
    assert sabotage is None or sabotage in SABOTAGES
    sd = {k: v.detach().cpu() for k, v in state_dict.items()}
    if sabotage == "blocks_swapped":
        sd = dict(sd)
        for li in range(1, len(cfg["num_centroids"])):
            k = "sa_modules.%d.mlp.0.conv.weight" % li
            w = sd[k]
            c = (w.shape[1] - 3) // 2
            sd[k] = torch.cat([w[:, :3], w[:, 3 + c:], w[:, 3:3 + c]], dim=1)
    B = points.shape[0]
    xyz = [np.ascontiguousarray(points[b:b + 1], dtype=np.float32) for b in range(B)]
    feat = [None] * B                                  # per scene (C, n) float64
    prev = [None] * B                                  # the level before's input features
    lv_xyz, lv_feat = [xyz], [feat]
    out = {}
    with torch.no_grad():
        for li, (M, r, K) in enumerate(zip(cfg["num_centroids"], cfg["radius"], cfg["num_neighbours"])):
            geo = []
            for b in range(B):
                idx = O.fps(xyz[b], M)
                ctr = O.gather_points(xyz[b], idx)
                gidx, _ = O.ball_query(xyz[b], ctr, r, K)
                geo.append((torch.from_numpy(idx[0].astype(np.int64)), ctr,
                            torch.from_numpy(gidx[0].reshape(-1).astype(np.int64))))
            new_feat = []
            for b in range(B):
                fidx, ctr, j = geo[b]
                # group_xyz -= new_xyz: ONE fp32 subtraction in the reference (modules.py:77)
                gx = (torch.from_numpy(xyz[b][0])[:, j].reshape(3, M, K) - torch.from_numpy(ctr[0])[:, :, None]).double()
                if feat[b] is None:
                    g = gx                                                           # modules.py:88
                else:
                    f = feat[b]
                    gf = f[:, j].reshape(-1, M, K)                                  # group_points(feature, index)
                    fc = f[:, fidx]                                                  # gather_points(feature, fps index)
                    if sabotage == "fc_next_centroid":
                        fc = torch.roll(fc, -1, dims=1)
                    elif sabotage == "fc_next_scene":
                        fc = feat[(b + 1) % B][:, geo[(b + 1) % B][0]]
                    elif sabotage == "fc_previous_level" and prev[b] is not None:
                        p = prev[b][:, :f.shape[1]][:, fidx]                         # same point, the level before's tensor
                        fc = p.repeat((f.shape[0] + p.shape[0] - 1) // p.shape[0], 1)[:f.shape[0]]
                    gf2 = gf - fc[:, :, None]                                        # modules.py:82
                    if sabotage == "fc_neighbour_row":
                        gf2 = gf - gf
                    elif sabotage == "sign_flipped":
                        gf2 = -gf2
                    elif sabotage == "edge_dropped" or (sabotage == "edge_level1_only" and li > 1):
                        gf2 = torch.zeros_like(gf2)
                    parts = [gx, gf2, gf] if sabotage == "order_swapped" else [gx, gf, gf2]
                    g = torch.cat(parts, dim=0)                                      # modules.py:84
                y = _mlp(g.reshape(g.shape[0], M * K), sd, "sa_modules.%d.mlp" % li)
                new_feat.append(y.reshape(-1, M, K).max(dim=2)[0])
            prev = feat
            feat = new_feat
            xyz = [geo[b][1] for b in range(B)]
            lv_xyz.append(xyz)
            lv_feat.append(feat)
            out["feat/sa%d" % li] = np.stack([f.numpy() for f in feat])
        heads = []
        for b in range(B):
            sparse_xyz, sparse = lv_xyz[-1][b], lv_feat[-1][b]
            for fi in range(len(cfg["num_centroids"])):
                dense_xyz, dense = lv_xyz[-2 - fi][b], lv_feat[-2 - fi][b]
                nidx, d2 = O.three_nn(dense_xyz, sparse_xyz)
                w = torch.from_numpy(O.interp_weights(d2, 1e-10)[0]).double()
                ni = torch.from_numpy(nidx[0].astype(np.int64))
                interp = (sparse[:, ni[:, 0]] * w[:, 0] + sparse[:, ni[:, 1]] * w[:, 1]) + sparse[:, ni[:, 2]] * w[:, 2]
                x = interp if dense is None else torch.cat([interp, dense], dim=0)
                sparse = _mlp(x, sd, "fp_modules.%d.mlp" % fi)
                sparse_xyz = dense_xyz
            heads.append(_heads64(sd, sparse))
    raw = {k: np.stack([h[k] for h in heads]) for k in heads[0]}
    R, pre = rot6d_to_matrix64(raw["frame_R"])
    out.update({"scene_score_logits": raw["score"], "frame_R": R,
                "frame_t": points.astype(np.float64) + raw["frame_t"], "movable_logits": raw["movable_logits"],
                "raw/R6": raw["frame_R"], "raw/t": raw["frame_t"], "b2_prenorm": pre})
    return out


# the shipped widths, radii and K = 64 (so the fused chain kernel runs at every SA level) over clouds of 4 096 points;
# every level's rows per scene a multiple of the tallest tile (128), so no launch's tile holds rows of two scenes
SHIPPED_SMALL_CLOUD = dict(num_centroids=(1024, 256, 128))


def shipped_edge_net(dev, pts, seed=78):
    """(net, cfg): the edge network with the shipped widths on `pts` (B, 3, 4096) device clouds, trained-like BatchNorm
    parameters with running statistics calibrated on `pts` through the reference-shaped modules over the HIP operators
    (tests/golden_util.calibrated), t_logit re-seeded to offsets of a few cm as `tests/contact64.shipped_contact_net`
    does (the reference zero-initialises it)."""
    from s4g_release_amd.model import EdgePointNet2Down
    from tests import golden_util as GU
    cfg = dict(GU.FULL, **SHIPPED_SMALL_CLOUD)
    torch.manual_seed(seed)
    net = EdgePointNet2Down(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        net.t_logit.weight.copy_(torch.randn(net.t_logit.weight.shape, generator=g) * 0.01)
        net.t_logit.bias.copy_(torch.randn(net.t_logit.bias.shape, generator=g) * 0.01)
    return GU.calibrated(net.to(dev), seed + 2, pts), cfg
