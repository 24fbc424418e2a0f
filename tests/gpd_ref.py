"""Float64 numpy yardstick of the GPD classifier (inference/grasp_proposal/network_models/models/GPD.py, eval mode), the
closed-form weights and images the fixture and the GPU tests share, and the sabotaged variants that show the fixture can
tell the network from its near misses.  No torch, no RNG streams: `hashed_state` and `hashed_images` are functions of the
element index alone, so fc1's 3.6 M weights need no storage.

    p1 = maxpool2x2(conv1(x) + b1)      Cin -> 20, 5x5 valid cross-correlation      (20, 28, 28)   no ReLU
    p2 = maxpool2x2(conv2(p1) + b2)     20 -> 50                                     (50, 12, 12)   no ReLU
    h  = relu(fc1(flatten(p2)) + c1)    flatten order (c, y, x), 7200 -> 500
    logits = fc2(h) + c2
"""
import os

import numpy as np

SHAPES = (("conv1.weight", lambda c, k: (20, c, 5, 5)), ("conv1.bias", lambda c, k: (20,)),
          ("conv2.weight", lambda c, k: (50, 20, 5, 5)), ("conv2.bias", lambda c, k: (50,)),
          ("fc1.weight", lambda c, k: (500, 7200)), ("fc1.bias", lambda c, k: (500,)),
          ("fc2.weight", lambda c, k: (k, 500)), ("fc2.bias", lambda c, k: (k,)))
SABOTAGES = ("relu1", "relu2", "flip", "pool_offset", "avg_pool", "flatten_yxc", "transpose", "channels_reversed",
             "no_conv_bias")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpd_classifier.npz")


def _unit(n, stream):
    """n values in [-1, 1): a splitmix64-style hash of (stream, element index) in wrapping uint64 arithmetic."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(stream) * np.uint64(0x632BE59BD9B4E019)
        z = (z + np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def hashed_state(in_channels, classes, salt=0):
    """name -> fp32 array in torch's shapes: weights uniform in +-sqrt(3 / fan_in), biases in +-0.1."""
    out = {}
    for t, (name, shape) in enumerate(SHAPES):
        s = shape(in_channels, classes)
        n = int(np.prod(s))
        u = _unit(n, 1 + t + 16 * salt)
        amp = 0.1 if name.endswith("bias") else np.sqrt(3.0 / int(np.prod(s[1:])))
        out[name] = (u * amp).astype(np.float32).reshape(s)
    return out


def hashed_images(n, channels, salt=0):
    """(n, channels, 60, 60) fp32, dense, uniform in [-1, 1)."""
    return _unit(n * channels * 3600, 1000 + salt).astype(np.float32).reshape(n, channels, 60, 60)


def maps_of_baseline_fixture():
    """(26, 12, 60, 60) fp32: the maps of the valid frames of tests/golden/baseline_regions.npz."""
    path = os.path.join(os.path.dirname(GOLDEN), "baseline_regions.npz")
    with np.load(path) as z:
        R, V = int(z["resolution"][0]), int(z["valid"].sum())
        maps = np.zeros(V * 12 * R * R, np.float32)
        maps[z["map_nz_index"]] = z["map_nz_value"]
    return maps.reshape(V, 12, R, R)


def fixture_images(in_channels):
    """The fixture's images for a network of `in_channels`: the real maps (their first channels), 6 dense hashed images
    and one all-zero image -> (33, in_channels, 60, 60) fp32."""
    real = maps_of_baseline_fixture()[:, :in_channels]
    return np.concatenate([real, hashed_images(6, in_channels, salt=in_channels),
                           np.zeros((1, in_channels, 60, 60), np.float32)]).astype(np.float32)


def _conv5(x, w, flip=False):
    """x (G, C, H, W), w (O, C, 5, 5) float64 -> valid cross-correlation (G, O, H - 4, W - 4)."""
    if flip:
        w = w[:, :, ::-1, ::-1]
    win = np.lib.stride_tricks.sliding_window_view(x, (5, 5), axis=(2, 3))      # (G, C, H-4, W-4, 5, 5)
    return np.einsum("gcyxij,ocij->goyx", win, w, optimize=True)


def _pool(x, offset=0, avg=False):
    x = x[:, :, offset:, offset:]
    h, w = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * h, :2 * w].reshape(x.shape[0], x.shape[1], h, 2, w, 2)
    return x.mean(axis=(3, 5)) if avg else x.max(axis=(3, 5))


def forward64(state, images, sabotage=None):
    """-> dict(pool1, pool2, hidden, logits) in float64.  `sabotage`: one of SABOTAGES, a deliberately wrong network."""
    assert sabotage is None or sabotage in SABOTAGES
    p = {k: np.asarray(v, np.float64) for k, v in state.items()}
    x = np.asarray(images, np.float64)
    if sabotage == "transpose":
        x = x.transpose(0, 1, 3, 2)
    if sabotage == "channels_reversed":
        x = x[:, ::-1]
    b1 = 0.0 if sabotage == "no_conv_bias" else p["conv1.bias"][None, :, None, None]
    b2 = 0.0 if sabotage == "no_conv_bias" else p["conv2.bias"][None, :, None, None]
    off, avg, flip = int(sabotage == "pool_offset"), sabotage == "avg_pool", sabotage == "flip"
    c1 = _conv5(x, p["conv1.weight"], flip) + b1
    if sabotage == "relu1":
        c1 = np.maximum(c1, 0.0)
    p1 = _pool(c1, off, avg)
    if off:                                  # keep the shapes of the true network: pad back to 28 x 28
        p1 = np.pad(p1, ((0, 0), (0, 0), (0, 28 - p1.shape[2]), (0, 28 - p1.shape[3])))
    c2 = _conv5(p1, p["conv2.weight"], flip) + b2
    if sabotage == "relu2":
        c2 = np.maximum(c2, 0.0)
    p2 = _pool(c2, off, avg)
    if off:
        p2 = np.pad(p2, ((0, 0), (0, 0), (0, 12 - p2.shape[2]), (0, 12 - p2.shape[3])))
    flat = (p2.transpose(0, 2, 3, 1) if sabotage == "flatten_yxc" else p2).reshape(len(x), 7200)
    h = np.maximum(flat @ p["fc1.weight"].T + p["fc1.bias"], 0.0)
    return {"pool1": p1, "pool2": p2, "hidden": h, "logits": h @ p["fc2.weight"].T + p["fc2.bias"]}


def distance(got, want64):
    """max |got - want| as a fraction of the tensor's scale (max |want|)."""
    want64 = np.asarray(want64, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want64))) / max(float(np.abs(want64).max()), 1e-30)


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
