"""CPU: the derived layer graphs of dvc_amd/arch.py as literals, the WarpNet trunk geometry against a restatement of the
reference's rule, and the launch sequences of the three layer walks (tests/launch_recorder.py) against the records taken at the
commit named in tests/golden/cvn_launch_sequence.json — before the walks read the graphs."""
import json
import os
import sys

import pytest

from dvc_amd import arch

G = arch.CVN_GRAPH
SS = {"c1_2": "conv1_2norm_ss", "c2_2": "conv2_2norm_ss", "c3_3": "conv3_3norm_ss"}
PLAIN_NORMED = ("c4_3", "c5_3", "c6_3", "c7_3", "c8_3", "c9_2")


def test_arch_imports_no_torch():
    import subprocess
    code = "import sys; import dvc_amd.arch; assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(arch.__file__)))


def test_cvn_graph_facts():
    assert dict(G.norm_pair) == SS
    assert dict(G.ss_of) == SS
    assert dict(G.norm_variants) == {**{a: (k, None) for a, k in SS.items()}, **{a: (None,) for a in PLAIN_NORMED}}
    assert G.norm_only == frozenset(SS) | frozenset(PLAIN_NORMED)
    assert dict(G.dual) == {"conv8_1.1": "conv3_3_short", "conv9_1.1": "conv2_2_short", "conv10_1.1": "conv1_2_short"}
    assert G.skip_keys == {"conv3_3_short", "conv2_2_short", "conv1_2_short"}
    assert dict(G.adder) == {"s3": "c8_1", "s2": "c9_1", "s1": "c10_1"}
    assert dict(G.grad_kind) == {None: "raw", "norm": "full", "norm_ss": "ss", "up": "up"}
    assert arch.CVN_OUT["src"] == "c10_2"
    # 30 convolutions, three of them the linear skips
    assert len(G.saved_acts) == len(set(G.saved_acts)) == 27 and not {"s1", "s2", "s3"} & set(G.saved_acts)
    assert set(G.by_key) == {c["key"] for c in arch.CVN_CONVS} and set(G.by_dst) == {c["dst"] for c in arch.CVN_CONVS}
    assert all(G.by_key[c["key"]] == c and G.by_dst[c["dst"]] == c for c in arch.CVN_CONVS)


def test_vgg_tables():
    assert arch.VGG_POOL_AFTER == {"r12", "r22", "r34", "r44", "r54"}
    assert arch.VGG_CONV_OF["r12"] == "conv1_2" and arch.VGG_CONV_OF["r54"] == "conv5_4"
    assert list(arch.VGG_CONV_OF) == [k for k in arch.VGG_KEYS if k[0] == "r"]
    assert list(arch.VGG_CONV_OF.values()) == [n for n, _, _ in arch.VGG_CONVS]


def test_graphs_reject_mutation():
    with pytest.raises(AttributeError):
        G.dual = {}
    for field in G._fields:
        v = getattr(G, field)
        if isinstance(v, (tuple, frozenset)):
            assert not hasattr(v, "add") and not hasattr(v, "append")
        else:
            with pytest.raises(TypeError):
                v["c1_2"] = None
    with pytest.raises(TypeError):
        G.by_key["conv1_2"]["dil"] = 2
    with pytest.raises(TypeError):
        arch.VGG_CONV_OF["r12"] = "conv1_1"
    assert isinstance(arch.VGG_POOL_AFTER, frozenset) and isinstance(arch.WARP_HEAD_PLAN, tuple)
    with pytest.raises(AttributeError):
        arch.WARP_HEAD_PLAN[0].stride_b = 1


def test_warp_head_plan():
    assert [tuple(hd) for hd in arch.WARP_HEAD_PLAN] == [
        (0, "layer2_1", 1, 3, 5, 2, 7, False, False), (1, "layer3_1", 1, 3, 5, 1, 7, False, False),
        (2, "layer4_1", 1, 3, 5, 1, 7, False, True), (3, "layer5_1", 1, 3, 6, 1, 8, True, True)]


def _head_inputs(H, W):
    """(H, W) of relu2_1 .. relu5_1 of an H x W frame: /2, /4, /8, /16, each a floor-halving pool."""
    out = []
    for _ in range(4):
        H, W = H // 2, W // 2
        out.append((H, W))
    return out


def _reference_head_sizes(shapes_in):
    """The reference's rule, head by head (NonlocalNet.py:364-410): 3x3 convolutions behind a reflection pad keep the size."""
    (h2, w2), (h3, w3), (h4, w4), (h5, w5) = shapes_in
    return [((h2 + 1) // 2, (w2 + 1) // 2),     # layer2_1: stride-2 second convolution
            (h3, w3),                           # layer3_1
            (2 * h4, 2 * w4),                   # layer4_1: x2 behind the head
            (4 * h5, 4 * w5)]                   # layer5_1: x2 between the convolutions, x2 behind


@pytest.mark.parametrize("H,W,rpad5", [(48, 80, 0), (96, 160, 0), (64, 96, 0), (40, 64, 1), (216, 384, 1)])
def test_warp_trunk_geometry(H, W, rpad5):
    """(216 x 384, the production frame, takes the replicate-pad branch: relu5_1 is 13 rows, 52 after the two upsamples, against
    layer2_1's 54.)"""
    shapes_in = _head_inputs(H, W)
    ref = _reference_head_sizes(shapes_in)
    assert [arch.warp_head_out_hw(n, *s) for n, s in zip(arch.WARP_HEAD_ORDER, shapes_in)] == ref
    assert (ref[3] != ref[0]) == bool(rpad5)
    assert ref[1] == ref[2] == ref[0] and (ref[3][0] + 2 * rpad5, ref[3][1]) == ref[0]
    assert arch.warp_trunk_geometry(shapes_in) == (H // 4, W // 4, rpad5)


def test_warp_trunk_geometry_mismatch():
    with pytest.raises(RuntimeError) as e:      # 72 columns: relu5_1 has 4, 16 after the upsamples; layer2_1 gives 18
        arch.warp_trunk_geometry(_head_inputs(40, 72))
    assert str(e.value) == "Sizes of tensors must match except in dimension 1: layer5_1 gives (10, 16), layer2_1 gives (10, 18)"
    with pytest.raises(RuntimeError) as e:      # 44 rows: relu4_1 has 5, 10 after the upsample; layer2_1 gives 11
        arch.warp_trunk_geometry(_head_inputs(44, 80))
    assert str(e.value) == "Sizes of tensors must match except in dimension 1: layer4_1 gives (10, 20), layer2_1 gives (11, 20)"


# ================================================================================================ launch sequences
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cvn_launch_sequence.json")) as _f:
    GOLDEN = json.load(_f)
SEQUENCES = [k for k in GOLDEN if k != "_commit"]


@pytest.fixture(scope="module")
def recorded():
    import launch_recorder
    with pytest.MonkeyPatch.context() as mp:
        return launch_recorder.record_all(mp)


def test_every_sequence_is_pinned(recorded):
    assert list(recorded) == SEQUENCES and len(SEQUENCES) == 11


@pytest.mark.parametrize("name", SEQUENCES)
def test_launch_sequence_unchanged(recorded, name):
    got, want = recorded[name], GOLDEN[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i} differs"
    assert len(got) == len(want)
