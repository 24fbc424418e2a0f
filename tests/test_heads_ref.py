"""CPU: the yardstick of the heads-kernel tests (tests/heads_ref.py) and the inputs of tests/test_heads_edges_gpu.py can
discriminate.  The float64 restatement is checked against an independent formulation of the same layers -- grouped
`conv1d` on (B, C, N) tensors, the way PointNet2_tcls.py:83-95,126-140 builds the heads -- and every wiring error a
rewrite of csrc/mlp_heads.hip can make is applied to the restatement ON THE GPU TESTS' INPUTS: it must miss the
unsabotaged restatement by >= 100 x the bound the GPU test asserts (the convention of tests/test_golden_calib.py).

For bf16 the GPU test asserts a maximum AND a mean; a kernel fails it when either is missed, so a sabotage counts as
found at 100 x when either is missed by 100 x (a logits bias is a constant offset of one head: its mean error is the
robust figure, its maximum need not reach 0.3 of the head's range)."""
import pytest
import torch
import torch.nn.functional as F

from tests import heads_ref as H

_cache = {}


def _weights(ch=H.CH):
    if ch not in _cache:
        _cache[ch] = H.make_weights(H.LAYER_SEED, ch)
    return _cache[ch]


def _conv_heads(Ws, b, X, B, N, ch, sigmoid_head):
    """The four heads as the reference network lays them out: channel-first tensors, 1 x 1 convolutions; the four
    stacks side by side as the groups of one convolution."""
    x = X.double().view(B, N, 256).permute(0, 2, 1)
    y = F.relu(F.conv1d(x, Ws[0].double().unsqueeze(-1), b[0].double()))
    for l, cin in ((1, 512), (2, 256), (3, 256)):
        y = F.relu(F.conv1d(y, Ws[l].double().reshape(-1, cin, 1), b[l].double().reshape(-1), groups=4))
    o = F.conv1d(y, Ws[4].double().reshape(128, 128, 1), b[4].double().reshape(-1), groups=4)
    outs = [o[:, 32 * h:32 * h + c] for h, c in enumerate(ch)]
    return [torch.sigmoid(t) if h == sigmoid_head else t for h, t in enumerate(outs)]


@pytest.mark.parametrize("B,N,ch,sig", [(2, 100, H.CH, 3), (3, 63, H.CH, 0), (19, 7, (1, 32, 4, 5), -1),
                                        (1, 129, (32, 32, 32, 32), 3)])
def test_restatement_equals_grouped_conv1d(B, N, ch, sig):
    Ws, b = _weights(ch)
    X, _ = H.make_x(B, N, H.x_seed(B, N))
    ref = H.reference(Ws, b, X, B, N, ch=ch, sigmoid_head=sig)
    ind = _conv_heads(Ws, b, X, B, N, ch, sig)
    for h in range(4):
        assert ref[h].shape == ind[h].shape == (B, ch[h], N)
        scale = max(1.0, float(ind[h].abs().max()))
        assert float((ref[h] - ind[h]).abs().max()) <= 1e-12 * scale, h


def test_tile_scale_is_the_per_scene_rule_where_the_tile_divides_n():
    ref = torch.randn(3, 5, 128, dtype=torch.float64) * torch.tensor([1.0, 40.0, 0.02]).view(3, 1, 1)
    per_scene = ref.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1.0).expand(3, 1, 128)
    for tile in (64, 128):
        assert torch.equal(H.tile_scale(ref, 3, 128, tile), per_scene)
    # ... and a tile shared by scenes takes the largest of them: rows 0 .. 63 of (B, N) = (3, 40) see scenes 0 and 1
    ref = torch.ones(3, 1, 40, dtype=torch.float64) * torch.tensor([2.0, 7.0, 3.0]).view(3, 1, 1)
    s = H.tile_scale(ref, 3, 40, 64).flatten()
    assert s[:64].eq(7.0).all() and s[64:].eq(7.0).all()          # tile 1 = rows 64 .. 119: scenes 1 and 2
    s = H.tile_scale(ref, 3, 40, 32).flatten()
    assert s[:32].eq(2.0).all() and s[32:64].eq(7.0).all() and s[64:96].eq(7.0).all() and s[96:].eq(3.0).all()


@pytest.mark.parametrize("layout,gap", [("plain", 0), ("strided", 0), ("packed", 0), ("packed", 64)])
def test_guarded_outputs_notice_every_stray_or_missing_word(layout, gap):
    """The guard check itself: clean when exactly the rows below P of the written heads are filled; it fires for a word
    in a guard, in the gap between scenes, in a masked-out head, in a row at or beyond P, and for a row left unwritten."""
    B, N, P = 3, 10, 25
    cpu = torch.device("cpu")

    def filled():
        g = H.GuardedOuts(cpu, B, N, layout=layout, gap=gap)
        live = (torch.arange(B * N) < P).view(B, 1, N)
        for h in (0, 1, 3):
            g.head(h)[live.expand(-1, H.CH[h], -1)] = 1.0
        return g
    filled().check((0, 1, 3), P=P)
    pokes = [0, H.GuardedOuts.GUARD - 1, -1]
    g = filled()
    pokes.append(g.off[2])                                  # the masked-out head
    pokes.append(g.off[0] + 2 * g.stride[0] + 7)            # scene 2, point 7: row 27 >= P
    if layout == "strided":
        pokes.append(g.off[3] + g.stride[3] - 1)            # the gap after scene 0
    if gap:
        pokes.append(H.GuardedOuts.GUARD + sum(H.CH) * N + 3)
    for w in pokes:
        g = filled()
        g.buf[w] = 0.0
        with pytest.raises(AssertionError):
            g.check((0, 1, 3), P=P)
    g = filled()
    g.head(1).view(torch.int32)[1, 4, 3] = H.SENTINEL_BITS          # a row below P left unwritten
    with pytest.raises(AssertionError):
        g.check((0, 1, 3), P=P)
    assert not filled().untouched() and H.GuardedOuts(cpu, B, N, layout=layout, gap=gap).untouched()


# ------------------------------------------------------------------------------------------------------- sabotage

def _swap_heads2(Ws, b):
    Ws, b = [w.clone() for w in Ws], [x.clone() for x in b]
    Ws[2][[1, 2]] = Ws[2][[2, 1]]
    b[2][[1, 2]] = b[2][[2, 1]]
    return Ws, b


def _swap_heads1_halves(Ws, b):
    Ws = [w.clone() for w in Ws]
    Ws[1] = torch.cat([Ws[1][..., 256:], Ws[1][..., :256]], dim=-1)
    return Ws, b


def _drop_heads0_second_half(Ws, b):
    Ws = [w.clone() for w in Ws]
    Ws[1][..., 256:] = 0                 # heads.1 never sees channels 256 .. 511 of heads.0
    return Ws, b


def _logits_bias_of_the_previous_head(Ws, b):
    b = [x.clone() for x in b]
    b[4] = torch.roll(b[4], 1, dims=0)
    return Ws, b


WEIGHT_SABOTAGE = {
    "heads.2-of-heads-1-and-2-swapped": _swap_heads2,
    "heads.1-input-halves-swapped": _swap_heads1_halves,
    "heads.0-second-half-dropped": _drop_heads0_second_half,
    "logits-bias-of-head-g-for-g+1": _logits_bias_of_the_previous_head,
    "sigmoid-on-the-wrong-head": None,
}


def _miss(sab, ref, B, N, precision, pre):
    """How far `sab` misses `ref` in units of the GPU test's bound(s): the largest factor over bounds and heads."""
    bound = H.BOUND[(precision, pre)]
    worst = 0.0
    for h in range(4):
        e = H.rel_err(sab[h], ref[h], B, N, H.TILE[precision])
        worst = max(worst, float(e.max()) / bound[0])
        if len(bound) > 1:
            worst = max(worst, float(e.mean()) / bound[1])
    return worst


RND = {3: H.f64, 2: H.bf16}


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("B,N", [(2, 100), (1, 129), (2, 128)])          # the mask, ladder and range cases' shapes
@pytest.mark.parametrize("name", sorted(WEIGHT_SABOTAGE))
def test_wiring_sabotage_misses_by_100x(name, B, N, precision):
    Ws, b = _weights()
    X, _ = H.make_x(B, N, H.x_seed(B, N), H.x_mags(precision))
    ref = H.reference(Ws, b, X, B, N, rnd=RND[precision])
    if WEIGHT_SABOTAGE[name] is None:
        sab = H.reference(Ws, b, X, B, N, rnd=RND[precision], sigmoid_head=0)
    else:
        sab = H.reference(*WEIGHT_SABOTAGE[name](Ws, b), X, B, N, rnd=RND[precision])
    miss = _miss(sab, ref, B, N, precision, False)
    print("miss / bound: %.3g" % miss)
    assert miss >= 100, (name, miss)


@pytest.mark.parametrize("precision,P,half", [(3, 33, 32), (3, 64, 32), (3, 65, 32), (3, 129, 32), (2, 33, 32), (2, 64, 32),
                                              (2, 97, 32), (2, 127, 64), (2, 128, 64), (2, 129, 64), (2, 257, 64),
                                              (2, 65, 64)])
def test_exchanged_row_blocks_miss_by_100x(precision, P, half):
    """Rows 0-31 / 32-63 of a tile exchanged (which 32-position block a wave owns in the logits), rows 0-63 / 64-127
    of the bf16 tile exchanged (`row3`'s two halves), on the ladder's own inputs."""
    Ws, b = _weights()
    X, _ = H.make_x(1, P, H.x_seed(1, P), H.x_mags(precision))
    ref = H.reference(Ws, b, X, 1, P, rnd=RND[precision])
    rowmap = H.swap_rowmap(P, H.TILE[precision], half)
    assert (rowmap != torch.arange(P)).any()
    sab = H.reference(Ws, b, X, 1, P, rnd=RND[precision], rowmap=rowmap)
    miss = _miss(sab, ref, 1, P, precision, False)
    print("miss / bound: %.3g" % miss)
    assert miss >= 100, miss


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("B,N", H.SCENE_SHAPES)
def test_scene_index_off_by_one_misses_by_100x(B, N, precision):
    """Rows of a tile that straddles scenes, attributed to the scene before their own."""
    Ws, b = _weights()
    X, _ = H.make_x(B, N, H.x_seed(B, N), H.x_mags(precision))
    ref = H.reference(Ws, b, X, B, N, rnd=RND[precision])
    rowmap = H.straddle_rowmap(B, N, H.TILE[precision])
    assert (rowmap != torch.arange(B * N)).any()
    sab = H.reference(Ws, b, X, B, N, rnd=RND[precision], rowmap=rowmap)
    miss = _miss(sab, ref, B, N, precision, False)
    print("miss / bound: %.3g" % miss)
    assert miss >= 100, miss


_TAIL_LADDER = [(1, 1, 3), (1, 129, 40), (1, 63, 3), (1, 65, 40)]
_TAIL_SCENES = [s + (40,) for s in H.PRE_SCENE_SHAPES]
_TAIL_CASES = ([(n, c) for n in ("neighbour-weights-permuted", "dense-addend-dropped") for c in _TAIL_LADDER + _TAIL_SCENES] +
               [("sparse-rows-of-the-scene-before", c) for c in _TAIL_SCENES])


@pytest.mark.parametrize("precision", [3, 2])
@pytest.mark.parametrize("name,shape", _TAIL_CASES)
def test_tail_sabotage_misses_by_100x(name, shape, precision):
    B, N, N2 = shape
    Ws, b = _weights()
    cpu = torch.device("cpu")
    rnd = RND[precision]
    S, nidx, nw, dense, lbias, pl = H.pre_setup(cpu, B, N, N2, H.pre_seed(B, N, N2), True, H.pre_dense_mag(precision), H.pre_mags(precision))
    ref = H.reference(Ws, b, H.pre_reference(S, nidx, nw, dense, lbias, pl, B, N, N2, rnd=rnd), B, N, rnd=rnd)
    scene = None
    if name == "neighbour-weights-permuted":
        nw = nw[:, [1, 2, 0]].contiguous()
    elif name == "dense-addend-dropped":
        dense = None
    else:
        scene = H.straddle_rowmap(B, N, H.TILE[precision]) // N
        assert (scene != torch.arange(B * N) // N).any()
    sab = H.reference(Ws, b, H.pre_reference(S, nidx, nw, dense, lbias, pl, B, N, N2, rnd=rnd, scene_of_row=scene),
                      B, N, rnd=rnd)
    miss = _miss(sab, ref, B, N, precision, True)
    print("miss / bound: %.3g" % miss)
    assert miss >= 100, (name, miss)
