"""The image pipeline without a GPU: the torch fallback of ``ops.image.preprocess`` against the float64
reference, the host-side box samplers, and the CPU path of ``ops.metrics.TopK``."""
import numpy as np
import pytest
import torch

from image_ref import GEOMETRIES, INCEPTION, RESNET, assert_close, box_tables, pixels, reference


@pytest.mark.parametrize("norm", [INCEPTION, RESNET], ids=["inception", "resnet"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1][0]}x{g[1][1]}-{g[2][0]}x{g[2][1]}")
def test_cpu_fallback_matches_float64_reference(geo, norm):
    from tony_amd.ops.image import preprocess

    N, (H, W), size = geo
    src = pixels(N, H, W)
    for i, boxes in enumerate(box_tables(N, H, W)):
        ref = reference(src, boxes, size, *norm)
        got = preprocess(src, boxes, size, torch.float32, *norm)
        assert got.shape == ref.shape and got.permute(0, 2, 3, 1).is_contiguous()
        assert_close(got, ref, *norm, f"fp32 table {i}")
        assert_close(preprocess(src, boxes, size, torch.bfloat16, *norm), ref, *norm, f"bf16 table {i}")


def test_cpu_fallback_identity_flip_and_out():
    from tony_amd.ops.image import preprocess

    src = pixels(2, 9, 11, seed=3)
    full = torch.tensor([[0, 0, 9, 11, 0]] * 2, dtype=torch.int32)
    got = preprocess(src, full, (9, 11), torch.float32, 1.0, 0.0)
    assert torch.equal(got, src.permute(0, 3, 1, 2).float())
    flipped = full.clone()
    flipped[:, 4] = 1
    out = torch.empty((2, 9, 11, 3)).permute(0, 3, 1, 2)
    assert preprocess(src, flipped, (9, 11), torch.float32, 1.0, 0.0, out=out) is out
    assert torch.equal(out, got.flip(-1))
    with pytest.raises(ValueError):
        preprocess(src, full, (9, 11), torch.float32, out=torch.empty(2, 3, 9, 11))  # not channels_last
    with pytest.raises(TypeError):
        preprocess(src.float(), full, (9, 11), torch.float32)


@pytest.mark.parametrize("sampler,lo", [("inception_train_boxes", 0.05), ("resnet_train_boxes", 0.08)])
def test_train_boxes_contract(sampler, lo):
    from tony_amd.ops import image

    H, W, n = 346, 300, 4000
    t = getattr(image, sampler)(np.random.default_rng(5), n, H, W)
    assert t.dtype == np.int32 and t.shape == (n, 5)
    y0, x0, h, w, flip = (t[:, i].astype(np.float64) for i in range(5))
    assert (y0 >= 0).all() and (x0 >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    # h and w are each rounded to an integer (at most 1/2 off): the ranges widen by exactly that much
    assert ((h + 0.5) * (w + 0.5) >= lo * H * W).all() and ((h - 0.5) * (w - 0.5) <= H * W).all()
    assert ((w + 0.5) / (h - 0.5) >= 3 / 4).all() and ((w - 0.5) / (h + 0.5) <= 4 / 3).all()
    assert set(np.unique(flip)) == {0.0, 1.0} and abs(flip.mean() - 0.5) < 0.05  # 4000 draws: sigma 0.008
    assert (h * w < 0.5 * H * W).any() and (h * w > 0.5 * H * W).any()  # the area range is used
    again = getattr(image, sampler)(np.random.default_rng(5), n, H, W)
    assert np.array_equal(t, again)
    assert not np.array_equal(t, getattr(image, sampler)(np.random.default_rng(6), n, H, W))


def test_train_boxes_fall_back_to_whole_image():
    from tony_amd.ops.image import inception_train_boxes, resnet_train_boxes

    # 2 x 200: the smallest crop (5% of 400 pixels, as wide as 4/3 allows) is 4 rows high: no attempt fits
    for fn in (inception_train_boxes, resnet_train_boxes):
        t = fn(np.random.default_rng(0), 16, 2, 200)
        assert (t[:, :4] == np.array([0, 0, 2, 200])).all()
        assert set(np.unique(t[:, 4])) <= {0, 1}


def test_central_boxes_exact_and_validation():
    from tony_amd.ops.image import central_boxes, validate_boxes

    assert central_boxes(2, 346, 346, 0.875).tolist() == [[21, 21, 304, 304, 0]] * 2
    assert central_boxes(1, 64, 64, 0.875).tolist() == [[4, 4, 56, 56, 0]]
    assert central_boxes(1, 320, 360, 0.875).tolist() == [[20, 22, 280, 316, 0]]
    assert central_boxes(3, 5, 7, 1.0).tolist() == [[0, 0, 5, 7, 0]] * 3
    ok = np.array([[0, 0, 5, 7, 1], [4, 6, 1, 1, 0]], dtype=np.int32)
    assert validate_boxes(ok, 5, 7) is ok
    for bad in ([0, 0, 6, 7, 0], [1, 0, 5, 7, 0], [0, 1, 5, 7, 0], [-1, 0, 2, 2, 0], [0, 0, 0, 2, 0], [0, 0, 2, 2, 2]):
        with pytest.raises(ValueError):
            validate_boxes(np.array([bad], dtype=np.int32), 5, 7)


def test_topk_cpu_hand_count():
    from tony_amd.ops.metrics import TopK

    x = torch.tensor([[5., 4., 3., 2., 1., 0.],   # target 0: rank 1            -> top1, top3
                      [5., 4., 3., 2., 1., 0.],   # target 2: 2 greater         -> top3
                      [5., 4., 3., 2., 1., 0.],   # target 3: 3 greater         -> miss
                      [5., 3., 3., 3., 3., 0.],   # target 4: 1 greater, a tie that straddles k -> top3
                      [1., 1., 1., 1., 1., 1.],   # target 5: all tied          -> top1, top3
                      [0., float("-inf"), 0., 0., 0., 0.],  # target 1: -inf    -> miss
                      [0., float("inf"), 0., 0., 0., 0.],   # target 1: +inf    -> miss (not finite)
                      [0., float("nan"), 0., 0., 0., 0.],   # target 1: NaN     -> miss
                      [float("nan"), 1., 0., 0., 0., 0.]])  # target 1: a NaN elsewhere is not greater -> top1, top3
    y = torch.tensor([0, 2, 3, 4, 5, 1, 1, 1, 1])
    m = TopK(3, "cpu")
    m.update(x, y)
    assert m.counters.tolist() == [3, 5, 9]
    m.update(x.bfloat16()[:2], y[:2])  # accumulates
    assert m.counters.tolist() == [4, 7, 11]
    top1, top3, seen = m.result()
    assert (top1, top3, seen) == (4 / 11, 7 / 11, 11)
    m.reset()
    assert m.result() == (0.0, 0.0, 0)
