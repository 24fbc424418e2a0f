"""s4g_heads_chain_f32 alone at its tile, scene, mask and output edges (csrc/mlp_heads.hip): every position of every
case against the float64 restatement of tests/heads_ref.py (f16x2) or the restatement rounded to bf16 at the layer inputs
(bf16), at the project's own bounds (tests/test_heads_gpu.py: 2e-5 / 3e-5 with the tail of scale; 3e-3 max + 5e-5 mean /
6e-3 + 1e-4).  The scale of a row is max(1, max |ref|) of its head over the scenes that share its workgroup tile (64
rows f16x2, 128 rows bf16): the per-scene rule wherever the tile divides N.  Every call writes into slices of one
sentinel-filled buffer with >= 256 guard floats round each tensor (and between scenes where the layout has a stride):
afterwards the guards are intact, every row below P is finite and nothing else was written.  tests/test_heads_ref.py
proves on the CPU that these inputs tell a mis-wired kernel from a right one by >= 100 x the bounds.

Each case prints its worst error per head next to the bound (pytest -s / -rA)."""
import pytest
import torch

from tests import heads_ref as H

pytestmark = pytest.mark.gpu
PREC = {3: "f16x2", 2: "bf16"}
RND = {3: H.f64, 2: H.bf16}


@pytest.fixture(scope="module")
def hs(dev):
    """The one packed layer set of this module (Ws, b, layers)."""
    return H.build_layers(dev, H.LAYER_SEED)


@pytest.fixture(scope="module")
def memo():
    """Module-wide store for what several cases share (a reference, the mask-15 outputs): computed once, never changed."""
    return {}


def _x(dev, B, N, precision, mags=None):
    X, amax = H.make_x(B, N, H.x_seed(B, N), mags or H.x_mags(precision))
    return X.to(dev), amax.to(dev)


def _pre(dev, B, N, N2, with_dense, precision):
    return H.pre_setup(dev, B, N, N2, H.pre_seed(B, N, N2), with_dense, H.pre_dense_mag(precision), H.pre_mags(precision)) + (N2,)


def _ref(hs, X, B, N, precision, pre=None, **kw):
    Ws, b, _ = hs
    if pre is not None:
        X = H.pre_reference(*pre[:6], B, N, pre[6], rnd=RND[precision])
    return H.reference(Ws, b, X, B, N, rnd=RND[precision], **kw)


def _go(dev, hs, X, amax, B, N, precision, layout="plain", gap=0, null=(), ch=H.CH, **kw):
    """One guarded call that must succeed; returns the GuardedOuts after the guard check."""
    from s4g_release_amd import _cabi
    g = H.GuardedOuts(dev, B, N, ch=ch, layout=layout, gap=gap, null=null)
    rc = H.launch(dev, hs[2], X, B, N, precision, amax, kw.pop("floor", 0.0), outs=g.outs, ch=ch,
                  out_batch_stride=g.obs, **kw)
    _cabi.check(rc, "heads")
    mask = kw.get("head_mask", 0) or 15
    g.check([h for h in range(4) if mask >> h & 1])
    return g


def _close(g, ref, B, N, precision, pre, label, heads=range(4), blocks=False):
    """Every position of `heads` within the bound; prints the worst figure per head (and per 32-row block)."""
    bound = H.BOUND[(precision, pre)]
    bad = []
    for h in heads:
        e = H.rel_err(g.head(h), ref[h], B, N, H.TILE[precision])
        fig = [float(e.max())] + ([float(e.mean())] if len(bound) > 1 else [])
        line = "%s %s head %d: %s (bound %s)" % (label, PREC[precision], h, " / ".join("%.2e" % f for f in fig),
                                                 " / ".join("%.0e" % x for x in bound))
        if blocks:
            line += "  per 32-row block: " + " ".join("%.1e" % v for v in H.per_block(e, B, N))
        print(line)
        if any(not f < x for f, x in zip(fig, bound)):      # (a NaN fails)
            bad.append(line)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------- a. the tile ladder

LADDER = {3: (1, 31, 32, 33, 63, 64, 65, 127, 128, 129), 2: (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257)}


@pytest.mark.parametrize("precision,P", [(p, n) for p in (3, 2) for n in LADDER[p]])
def test_tile_ladder(dev, hs, precision, P):
    """B = 1, N = P round the 32-row blocks and the tile edge: which block a wave owns in heads.3 (`row3`) and in the
    logits (`wv < NRBT`), the ragged last tile.  The worst error is reported per 32-row block."""
    X, amax = _x(dev, 1, P, precision)
    g = _go(dev, hs, X, amax, 1, P, precision)
    _close(g, _ref(hs, X, 1, P, precision), 1, P, precision, False, "ladder P=%d" % P, blocks=True)


@pytest.mark.parametrize("precision", [3, 2])
def test_no_positions_is_ok_and_writes_nothing(dev, hs, precision):
    """P = 0 returns S4G_OK without a launch (N stays positive: the entry refuses N <= 0 before it looks at P)."""
    X, amax = _x(dev, 1, 64, precision)
    g = H.GuardedOuts(dev, 1, 64)
    assert H.launch(dev, hs[2], X, 1, 64, precision, amax, outs=g.outs, P=0) == 0
    assert g.untouched()


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("with_dense", [False, True])
@pytest.mark.parametrize("N2", [3, 40])
@pytest.mark.parametrize("P", [1, 63, 65, 129])
def test_tile_ladder_with_the_tail(dev, hs, precision, P, N2, with_dense):
    pre = _pre(dev, 1, P, N2, with_dense, precision)
    g = _go(dev, hs, None, None, 1, P, precision, pre=pre)
    _close(g, _ref(hs, None, 1, P, precision, pre), 1, P, precision, True,
           "ladder+tail P=%d N2=%d dense=%d" % (P, N2, with_dense), blocks=True)


# --------------------------------------------------------------------------------------------- b. scenes inside a tile

@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("B,N", H.SCENE_SHAPES)
def test_scenes_inside_a_tile(dev, hs, precision, B, N):
    """Tiles shared by up to 128 scenes whose X magnitudes cycle through 1, 40, 0.02 (bf16: 1, 0.25, 0.02 -- the
    rounded yardstick is not steady to 3e-3 on the sigmoid head of a 40 x scene, see heads_ref.BF16_MAGS: measured
    3.76e-3 at (3, 63)) with true per-scene a_amax; each
    row against its own scene's reference, each scene's block of every head behind a gap of sentinels (batch stride
    max(c) N + 256): a row read from, or written to, the neighbouring scene shows (`row / N`, `obs`, `amax_rows`)."""
    X, amax = _x(dev, B, N, precision)
    g = _go(dev, hs, X, amax, B, N, precision, layout="strided")
    _close(g, _ref(hs, X, B, N, precision), B, N, precision, False, "scenes (%d, %d)" % (B, N))


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("B,N", H.PRE_SCENE_SHAPES)
def test_scenes_inside_a_tile_with_the_tail(dev, hs, precision, B, N):
    """... with the tail: the sparse rows come from `bq * N2` of the row's own scene."""
    pre = _pre(dev, B, N, 40, True, precision)
    g = _go(dev, hs, None, None, B, N, precision, layout="strided", pre=pre)
    _close(g, _ref(hs, None, B, N, precision, pre), B, N, precision, True, "scenes+tail (%d, %d)" % (B, N))


@pytest.mark.parametrize("precision", [3, 2])
def test_rows_per_scene_zero_reads_one_global_slot_row(dev, hs, precision):
    """rows_per_scene = 0: a_amax is ONE slot row for the whole launch (the scene index must not be applied to it: a
    second row does not exist).  The outputs are still addressed per scene."""
    B, N = 3, 65
    X, amax = _x(dev, B, N, precision)
    glob = amax.amax(dim=0, keepdim=True).contiguous()
    g = _go(dev, hs, X, glob, B, N, precision, layout="strided", rows_per_scene=0)
    _close(g, _ref(hs, X, B, N, precision), B, N, precision, False, "rows_per_scene=0 (3, 65)")


# ----------------------------------------------------------------------------------------------------- c. head masks

MB, MN = 2, 100


def _mask_inputs(dev, hs, memo, precision, with_tail):
    """Inputs, reference and the mask-15 outputs of the mask cases: made once per (precision, tail)."""
    key = ("mask", precision, with_tail)
    if key not in memo:
        if with_tail:
            X, amax, pre = None, None, _pre(dev, MB, MN, 40, True, precision)
        else:
            (X, amax), pre = _x(dev, MB, MN, precision), None
        ref = _ref(hs, X, MB, MN, precision, pre)
        g = _go(dev, hs, X, amax, MB, MN, precision, layout="strided", pre=pre, head_mask=15)
        memo[key] = (X, amax, pre, ref, [g.head(h).clone() for h in range(4)])
    return memo[key]


def _mask_case(dev, hs, memo, precision, mask, null, with_tail):
    X, amax, pre, ref, full = _mask_inputs(dev, hs, memo, precision, with_tail)
    run = [h for h in range(4) if mask >> h & 1]
    nul = tuple(h for h in range(4) if h not in run) if null else ()
    # the guard check inside _go: every masked-out tensor (handed in, or NULL) and every gap still hold the sentinel
    g = _go(dev, hs, X, amax, MB, MN, precision, layout="strided", null=nul, pre=pre, head_mask=mask)
    _close(g, ref, MB, MN, precision, with_tail, "mask %d%s" % (mask, " +tail" if with_tail else ""), heads=run)
    for h in run:
        assert torch.equal(g.head(h), full[h]), "head %d under mask %d differs from the same head under mask 15" % (h, mask)


@pytest.mark.parametrize("null", [False, True], ids=["given", "null"])
@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("mask", range(1, 16))
def test_every_head_mask(dev, hs, memo, precision, mask, null):
    """All fifteen masks: each takes its own `g_first` / `gn` / `gnx` path through the W ring's prefetch.  Every
    evaluated head is within the bound AND bit-identical to the same head of the mask-15 run on the same inputs, which is
    what the code promises: each head restarts from panel A with `inv_sa`, its hidden layers' scales are its own tile
    maxima, and only the ring prefetch crosses heads -- a head's outputs do not depend on which other heads run.  The
    masked-out tensors keep their sentinel; "null" hands NULL pointers in for them."""
    _mask_case(dev, hs, memo, precision, mask, null, False)


@pytest.mark.parametrize("null", [False, True], ids=["given", "null"])
@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("mask", [1, 2, 8, 5, 10, 14, 15])
def test_head_masks_with_the_tail(dev, hs, memo, precision, mask, null):
    """... with the tail in front, whose last strip prefetches the FIRST evaluated head (`w0(g_first, 0)`)."""
    _mask_case(dev, hs, memo, precision, mask, null, True)


@pytest.mark.parametrize("precision", [3, 2])
def test_mask_zero_is_mask_fifteen(dev, hs, memo, precision):
    X, amax, pre, ref, full = _mask_inputs(dev, hs, memo, precision, False)
    g = _go(dev, hs, X, amax, MB, MN, precision, layout="strided", head_mask=0)
    for h in range(4):
        assert torch.equal(g.head(h), full[h]), h


# ------------------------------------------------------------------- d. output addressing and the input stride

@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("gap", [0, 64])
def test_packed_payload(dev, hs, precision, gap):
    """The four heads as channel slices of one (B, 21, N) tensor, out_batch_stride = 21 N, and the same with a stride
    of 21 N + 64 whose gap stays sentinel -- against the reference."""
    B, N = 2, 100
    X, amax = _x(dev, B, N, precision)
    g = _go(dev, hs, X, amax, B, N, precision, layout="packed", gap=gap)
    assert g.obs == 21 * N + gap
    _close(g, _ref(hs, X, B, N, precision), B, N, precision, False, "packed stride 21 N + %d" % gap)


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("ch", [(1, 32, 4, 5), (32, 32, 32, 32)])
def test_channel_counts_one_and_thirty_two(dev, hs, memo, precision, ch):
    if ("logits", ch) not in memo:
        memo[("logits", ch)] = H.with_logits(*hs, ch, 77 + sum(ch))
    hs2 = memo[("logits", ch)]
    B, N = 2, 100
    X, amax = _x(dev, B, N, precision)
    g = _go(dev, hs2, X, amax, B, N, precision, layout="strided", ch=ch)
    _close(g, _ref(hs2, X, B, N, precision, ch=ch), B, N, precision, False, "channels %s" % (ch,))


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("sig", [-1, 0, 3])
def test_sigmoid_head(dev, hs, precision, sig):
    B, N = 2, 100
    X, amax = _x(dev, B, N, precision)
    g = _go(dev, hs, X, amax, B, N, precision, layout="strided", sigmoid_head=sig)
    ref = _ref(hs, X, B, N, precision, sigmoid_head=sig)
    for h in range(4):          # the reference itself tells the sigmoid head from the others
        assert (float(ref[h].min()) >= 0 and float(ref[h].max()) <= 1) == (h == sig)
    _close(g, ref, B, N, precision, False, "sigmoid_head %d" % sig)


@pytest.mark.parametrize("precision", [3, 2])
def test_x_as_a_column_slice_of_a_wider_tensor(dev, hs, precision):
    """ldx = 320: X is [:, :256] of a (P, 320) tensor whose other columns are NaN."""
    B, N = 2, 100
    X, amax = _x(dev, B, N, precision)
    wide = torch.full((B * N, 320), float("nan"), device=dev)
    wide[:, :256] = X
    g = _go(dev, hs, wide, amax, B, N, precision, layout="strided")
    _close(g, _ref(hs, X, B, N, precision), B, N, precision, False, "ldx 320")


@pytest.mark.parametrize("precision", [3, 2])
def test_refusals_return_nonzero_and_write_nothing(dev, hs, precision):
    B, N = 2, 100
    X, amax = _x(dev, B, N, precision)
    big = torch.zeros(B * N * 256 + 8, device=dev)
    g = H.GuardedOuts(dev, B, N, layout="strided")
    call = lambda Xc=X, **kw: H.launch(dev, hs[2], Xc, B, N, precision, kw.pop("amax", amax), kw.pop("floor", 0.0),   # noqa: E731
                                       outs=g.outs, out_batch_stride=g.obs, **kw)
    assert call(ldx=258) != 0
    assert call(ldx=252) != 0
    assert call(big, ldx=256, x_ptr=big.data_ptr() + 4) != 0          # X misaligned by 4 bytes
    assert call(ch=(0, 9, 4, 5)) != 0
    assert call(ch=(3, 33, 4, 5)) != 0
    if precision == 3:
        assert call(amax=None, floor=0.0) != 0                        # f16x2: neither a_amax nor a positive floor
    assert g.untouched()
    assert call() == 0 and not g.untouched()                          # ... and the very same call, unspoilt, runs


# ------------------------------------------------------------------------- e. operand ranges and a dead tile

def _dead(hs, memo, head):
    """The layer set with head `head` dead from heads.2 on: heads.2 bias -1e4 (its 256 channels are zero after ReLU in
    every tile: the `exh < 15` clamp), heads.3 bias -|b| (relu(W 0 + b) is zero too), so the logits are their bias."""
    if ("dead", head) not in memo:
        Ws, b, layers = hs
        b2, b3 = b[2].clone(), b[3].clone()
        b2[head] = -1e4
        b3[head] = -b3[head].abs()
        bb, ll = H.with_bias(b, layers, 2, b2)
        bb, ll = H.with_bias(bb, ll, 3, b3)
        memo[("dead", head)] = (Ws, bb, ll)
    return memo[("dead", head)]


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("dead", [1, 3])
@pytest.mark.parametrize("mags", [(1e-6, 300.0), (0.03, 1.0), (0.0, 1.0)])
def test_operand_ranges_and_a_dead_head(dev, hs, memo, precision, dead, mags):
    """B = 2, N = 128 with scenes of magnitudes (1e-6, 300), (0.03, 1) and (0, 1) -- the last an all-zero scene with
    a_amax 0 and a positive floor.  One head is dead from heads.2 on (see _dead): its logits equal its logits bias
    EXACTLY -- fma(0, scale, bias) -- and on the sigmoid head 1 / (1 + expf(-bias)): the same value in every row, within
    4 fp32 ulps of 1 of the float64 sigmoid (expf, the sum, the quotient: <= 1 ulp each, of values <= 1 after the
    quotient).  The other heads stay within the bound, and a second run is bit-identical."""
    B, N = 2, 128
    hs2 = _dead(hs, memo, dead)
    X, amax = _x(dev, B, N, precision, mags)
    kw = dict(floor=1e-3) if mags[0] == 0.0 else {}
    g = _go(dev, hs2, X, amax, B, N, precision, **dict(kw))
    g2 = _go(dev, hs2, X, amax, B, N, precision, **dict(kw))
    assert torch.equal(g.buf.view(torch.int32), g2.buf.view(torch.int32))
    ref = _ref(hs2, X, B, N, precision)
    _close(g, ref, B, N, precision, False, "ranges %s dead head %d" % (mags, dead))
    bias = hs2[1][4][dead, :H.CH[dead]].view(1, -1, 1).expand(B, -1, N)
    if dead == 3:
        assert torch.equal(g.head(3), g.head(3)[:1, :, :1].expand(B, -1, N))
        assert float((g.head(3).double() - torch.sigmoid(bias.double())).abs().max()) <= 4 * 2.0 ** -24
    else:
        assert torch.equal(g.head(dead), bias)


# ----------------------------------------------------------------- f. a non-finite scene stays in its tiles

@pytest.mark.parametrize("precision", [3, 2])
def test_a_non_finite_scene_stays_in_its_tiles(dev, hs, precision):
    """B = 3, N = 128 (a multiple of both tiles): scene 1's X is NaN and inf and its a_amax NaN.  The call returns, and
    scenes 0 and 2 are bit-identical to the same call made without scene 1.  (Scene 1's own outputs are unspecified.)"""
    B, N = 3, 128
    X, amax = _x(dev, B, N, precision)
    X = X.clone()
    X[N:2 * N] = float("nan")
    X[N:2 * N:2, ::3] = float("inf")
    X[N + 1:2 * N:2, 1::3] = float("-inf")
    amax = amax.clone()
    amax[1] = float("nan")
    outs = H.run(dev, hs[2], X, B, N, precision, amax)
    keep = torch.cat([X[:N], X[2 * N:]]).contiguous()
    outs2 = H.run(dev, hs[2], keep, 2, N, precision, amax[[0, 2]].contiguous())
    ref = _ref(hs, keep, 2, N, precision)
    for h in range(4):
        assert torch.isfinite(outs2[h]).all()
        assert torch.equal(outs[h][0], outs2[h][0]) and torch.equal(outs[h][2], outs2[h][1]), h
        e = H.rel_err(outs2[h], ref[h], 2, N, H.TILE[precision])
        assert float(e.max()) < H.BOUND[(precision, False)][0], h
