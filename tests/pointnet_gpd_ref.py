"""Float64 numpy yardstick of the PointNetGPD classifier (inference/grasp_proposal/network_models/models/PointNetGPD.py,
`PointNetClassifier` in eval mode), the closed-form weights and point sets the fixture and the GPU tests share, and the
sabotaged variants that show the fixture can tell the network from its near misses.  No torch, no RNG streams.

Per set x (3, n), BN = eval-mode BatchNorm1d (eps 1e-5):
    stn_global = max_j relu(BN3(W3 relu(BN2(W2 relu(BN1(W1 x_j))))))            feat.stn.conv1..3, bn1..3
    trans      = fc3(relu(BN5(fc2(relu(BN4(fc1(stn_global))))))) + I            feat.stn.fc1..3, bn4, bn5      (3, 3)
    y_j        = trans^T x_j                                                    (x^T trans, as torch.bmm has it)
    global     = max_j BN3(V3 relu(BN2(V2 relu(BN1(V1 y_j)))))                  feat.conv1..3, bn1..3: NO ReLU at the end
    hidden     = relu(BN2(fc2(relu(BN1(fc1(global))))))                         fc1, fc2, bn1, bn2
    logits     = fc3(hidden)
"""
import os

import numpy as np

from tests.gpd_ref import _unit, distance  # noqa: F401  (distance: max |got - want| / max |want|)

EPS = 1e-5
LEVELS = ("stn_global", "trans", "global", "hidden", "logits")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet_gpd.npz")
SABOTAGES = ("relu_feat3", "no_relu_stn3", "trans_transposed", "no_identity", "mean_pool", "bn_mean_sign",
             "head_bn_swapped", "xyz_reversed", "untransformed", "no_bn_beta", "bn_no_eps")

# (prefix, layer, out, in, its BatchNorm or None); out None = score_classes
_LAYERS = (("feat.stn.", "conv1", 64, 3, "bn1"), ("feat.stn.", "conv2", 128, 64, "bn2"),
           ("feat.stn.", "conv3", 1024, 128, "bn3"), ("feat.stn.", "fc1", 512, 1024, "bn4"),
           ("feat.stn.", "fc2", 256, 512, "bn5"), ("feat.stn.", "fc3", 9, 256, None),
           ("feat.", "conv1", 64, 3, "bn1"), ("feat.", "conv2", 128, 64, "bn2"), ("feat.", "conv3", 1024, 128, "bn3"),
           ("", "fc1", 512, 1024, "bn1"), ("", "fc2", 256, 512, "bn2"), ("", "fc3", None, 256, None))


def hashed_state(classes, salt=0):
    """name -> array in torch's shapes for every key of the reference's state dict: weights uniform in
    +-sqrt(3 / fan_in), biases and BN beta in +-0.1, BN gamma in [0.5, 1.5), running mean in +-0.1, running variance in
    [0.5, 1.5), num_batches_tracked 0.  The fixture replaces the running statistics by calibrated ones
    (`fixture_state`)."""
    out = {}
    stream = 1 + 64 * salt
    for prefix, name, cout, cin, bn in _LAYERS:
        cout = classes if cout is None else cout
        shape = (cout, cin, 1) if name.startswith("conv") else (cout, cin)
        out[prefix + name + ".weight"] = (_unit(cout * cin, stream) * np.sqrt(3.0 / cin)).astype(np.float32).reshape(shape)
        out[prefix + name + ".bias"] = (_unit(cout, stream + 1) * 0.1).astype(np.float32)
        if bn:
            out[prefix + bn + ".weight"] = (1.0 + 0.5 * _unit(cout, stream + 2)).astype(np.float32)
            out[prefix + bn + ".bias"] = (0.1 * _unit(cout, stream + 3)).astype(np.float32)
            out[prefix + bn + ".running_mean"] = (0.1 * _unit(cout, stream + 4)).astype(np.float32)
            out[prefix + bn + ".running_var"] = (1.0 + 0.5 * _unit(cout, stream + 5)).astype(np.float32)
            out[prefix + bn + ".num_batches_tracked"] = np.zeros((), np.int64)
        stream += 6
    return out


def fixture_state(fx, classes=3):
    """`hashed_state(classes)` with the fixture's calibrated running statistics."""
    st = hashed_state(classes)
    for k in fx:
        if k.startswith("stat/"):
            st[k[5:]] = fx[k]
    return st


def hashed_set(n, salt=0, amp=0.05):
    """(3, n) fp32, uniform in +-amp."""
    return (_unit(3 * n, 2000 + salt) * amp).astype(np.float32).reshape(3, n)


def hashed_subset(real, n, salt=0, jitter=0.002):
    """(3, n) fp32: points of the real set `real` (3, m) picked by a hashed index (with replacement), each coordinate
    moved by a hashed +-jitter: a set of any size that lies where the real sets lie."""
    pick = np.minimum(((_unit(n, 3000 + salt) + 1.0) * 0.5 * real.shape[1]).astype(np.int64), real.shape[1] - 1)
    return (real[:, pick].astype(np.float64) + jitter * _unit(3 * n, 4000 + salt).reshape(3, n)).astype(np.float32)


def real_sets():
    """The 26 close-region sets of tests/golden/baseline_regions.npz: the scene points set_index[set_offset[i] :
    set_offset[i + 1]] taken through `baseline_frame` of the i-th valid frame (rotation and translation, formed in
    float64 and rounded to fp32 once) -> list of (3, n) fp32."""
    path = os.path.join(os.path.dirname(GOLDEN), "baseline_regions.npz")
    with np.load(path) as z:
        cloud, frames = z["cloud"].astype(np.float64), z["baseline_frame"][z["valid"]].astype(np.float64)
        off, idx = z["set_offset"], z["set_index"]
    out = []
    for i in range(len(off) - 1):
        p = cloud[:, idx[off[i]:off[i + 1]]]
        out.append(np.ascontiguousarray((frames[i][:3, :3] @ p + frames[i][:3, 3:4]).astype(np.float32)))
    return out


def fixture_sets():
    """The fixture's sets: the 26 real ones, then hashed sets of 1, 2 and 1 024 points (`hashed_subset` of real sets 3,
    11 and 20)."""
    real = real_sets()
    return real + [hashed_subset(real[3], 1, 1), hashed_subset(real[11], 2, 2), hashed_subset(real[20], 1024, 3)]


def _bn(p, name, x, sab, eps=EPS):
    """x (C, n) or (C,)."""
    mean, var = p[name + ".running_mean"], p[name + ".running_var"]
    g, b = p[name + ".weight"], p[name + ".bias"]
    if sab == "bn_mean_sign":
        mean = -mean
    if sab == "no_bn_beta":
        b = 0.0 * b
    if sab == "bn_no_eps":
        eps = 0.0
    k = g / np.sqrt(var + eps)
    sh = (-1,) + (1,) * (x.ndim - 1)
    return (x - mean.reshape(sh)) * k.reshape(sh) + np.reshape(b, sh)


def _lin(p, name, x):
    w = p[name + ".weight"]
    w = w.reshape(w.shape[0], -1)
    return w @ x + p[name + ".bias"].reshape((-1,) + (1,) * (x.ndim - 1))


def forward_one(p, x, sab=None, eps=EPS):
    """p: float64 state, x (3, n) float64 -> dict of LEVELS."""
    relu = lambda v: np.maximum(v, 0.0)   # noqa: E731
    pool = (lambda v: v.mean(axis=1)) if sab == "mean_pool" else (lambda v: v.max(axis=1))
    if sab == "xyz_reversed":
        x = x[::-1]
    bn4, bn5, bn1, bn2 = "feat.stn.bn4", "feat.stn.bn5", "bn1", "bn2"
    if sab == "head_bn_swapped":
        bn4, bn5, bn1, bn2 = bn1, bn2, bn4, bn5
    s = "feat.stn."
    h = relu(_bn(p, s + "bn1", _lin(p, s + "conv1", x), sab, eps))
    h = relu(_bn(p, s + "bn2", _lin(p, s + "conv2", h), sab, eps))
    h = _bn(p, s + "bn3", _lin(p, s + "conv3", h), sab, eps)
    if sab != "no_relu_stn3":
        h = relu(h)
    sg = pool(h)
    h = relu(_bn(p, bn4, _lin(p, s + "fc1", sg), sab, eps))
    h = relu(_bn(p, bn5, _lin(p, s + "fc2", h), sab, eps))
    trans = _lin(p, s + "fc3", h).reshape(3, 3)
    if sab != "no_identity":
        trans = trans + np.eye(3)
    y = x if sab == "untransformed" else ((trans @ x) if sab == "trans_transposed" else (trans.T @ x))
    h = relu(_bn(p, "feat.bn1", _lin(p, "feat.conv1", y), sab, eps))
    h = relu(_bn(p, "feat.bn2", _lin(p, "feat.conv2", h), sab, eps))
    h = _bn(p, "feat.bn3", _lin(p, "feat.conv3", h), sab, eps)
    if sab == "relu_feat3":
        h = relu(h)
    g = pool(h)
    h = relu(_bn(p, bn1, _lin(p, "fc1", g), sab, eps))
    h = relu(_bn(p, bn2, _lin(p, "fc2", h), sab, eps))
    return {"stn_global": sg, "trans": trans, "global": g, "hidden": h, "logits": _lin(p, "fc3", h)}


def forward64(state, sets, sabotage=None, eps=EPS):
    """state: name -> array (the reference's state dict), sets: list of (3, n) -> dict level -> float64 (len(sets), ...).
    `sabotage`: one of SABOTAGES, a deliberately wrong network."""
    assert sabotage is None or sabotage in SABOTAGES
    p = {k: np.asarray(v, np.float64) for k, v in state.items()}
    rows = [forward_one(p, np.asarray(x, np.float64), sabotage, eps) for x in sets]
    return {k: np.stack([r[k] for r in rows]) for k in LEVELS}


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
