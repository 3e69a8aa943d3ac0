"""Colour distortion without a GPU: the CPU path of ``ops.image.preprocess(..., colour=table)`` against the
float64 reference within the derived bound (tests/image_colour_ref.py), rows of order -1 exactly as without a table,
the parameter sampler, ``validate_colour``, and ``ImageBatches.plan_colour``."""
import functools

import numpy as np
import pytest
import torch

from image_colour_ref import (B_HI, B_LO, F_HI, F_LO, H_HI, H_LO, adversarial_pixels, assert_close, colour_tables,
                              reference)
from image_ref import GEOMETRIES, INCEPTION, RESNET, box_tables, pixels

NORMS = {"inception": INCEPTION, "resnet": RESNET}


@functools.lru_cache(maxsize=None)
def _case(gi):
    N, (H, W), _ = GEOMETRIES[gi]
    return adversarial_pixels(pixels(N, H, W, seed=gi)), box_tables(N, H, W, seed=gi), colour_tables(N, seed=gi)


@pytest.mark.parametrize("norm", list(NORMS))
@pytest.mark.parametrize("gi", range(3), ids=lambda i: "geo%d" % i)
def test_cpu_path_matches_float64_reference(gi, norm):
    from tony_amd.ops.image import preprocess

    size = GEOMETRIES[gi][2]
    src, boxes, tables = _case(gi)
    worst = 0.0
    for i, colour in enumerate(tables):
        b = boxes[i % len(boxes)]
        ref = reference(src, b, colour, size, *NORMS[norm])
        got = preprocess(src, b, size, torch.float32, *NORMS[norm], colour=colour)
        assert got.shape == ref.shape and got.dtype == torch.float32
        worst = max(worst, assert_close(got, ref, colour, *NORMS[norm], f"geo{gi} {norm} table {i}"))
    print(f"geo{gi} {norm}: worst error / bound {worst:.4f}")


def test_rows_without_an_order_equal_the_call_without_a_table():
    from tony_amd.ops.image import preprocess

    N, (H, W), size = GEOMETRIES[0]
    src, boxes, _ = _case(0)
    colour = torch.tensor([[-1, 0.1, 1.3, 0.1, 0.7], [2, 0.1, 1.3, 0.1, 0.7], [-1, 0, 1, 0, 1]], dtype=torch.float32)
    plain = preprocess(src, boxes[0], size, torch.float32, *RESNET)
    got = preprocess(src, boxes[0], size, torch.float32, *RESNET, colour=colour)
    assert torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32))
    assert torch.equal(got[2].view(torch.int32), plain[2].view(torch.int32))
    assert not torch.equal(got[1], plain[1])
    with pytest.raises(ValueError, match="colour must be"):
        preprocess(src, boxes[0], size, torch.float32, colour=colour[:2])
    with pytest.raises(ValueError, match="colour must be"):
        preprocess(src, boxes[0], size, torch.float32, colour=colour.double())


def test_sampler_ranges_codes_and_determinism():
    from tony_amd.ops.image import inception_colour_params

    full = inception_colour_params(np.random.default_rng(3), 4000)
    assert full.dtype == np.float32 and full.shape == (4000, 5)
    assert set(full[:, 0].tolist()) == {0.0, 1.0, 2.0, 3.0}
    for col, lo, hi in ((1, B_LO, B_HI), (2, F_LO, F_HI), (3, H_LO, H_HI), (4, F_LO, F_HI)):
        assert full[:, col].min() >= np.float32(lo) and full[:, col].max() < np.float32(hi), col
        span = float(hi - lo)  # 4000 uniform draws leave the outer 2 % empty with probability 1e-35
        assert full[:, col].min() < lo + 0.02 * span and full[:, col].max() > hi - 0.02 * span, col
    fast = inception_colour_params(np.random.default_rng(3), 500, fast=True)
    assert set(fast[:, 0].tolist()) == {4.0}
    assert (fast[:, 3] == 0).all() and (fast[:, 4] == 1).all()
    assert fast[:, 1].min() >= np.float32(B_LO) and fast[:, 1].max() < np.float32(B_HI)
    assert fast[:, 2].min() >= np.float32(F_LO) and fast[:, 2].max() < np.float32(F_HI)
    assert np.array_equal(full, inception_colour_params(np.random.default_rng(3), 4000))
    assert not np.array_equal(full, inception_colour_params(np.random.default_rng(4), 4000))


def test_validate_colour_refusals():
    from tony_amd.ops.image import validate_colour

    good = np.array([[-1, 0, 1, 0, 1], [5, -0.1, 0.5, 0.2, 1.5]], dtype=np.float32)
    assert validate_colour(good) is good
    for r, c, v in ((0, 0, 6), (0, 0, -2), (1, 0, 2.5), (0, 1, np.nan), (1, 3, np.inf), (0, 2, 0.0), (1, 4, -1.0),
                    (0, 0, np.nan)):
        bad = good.copy()
        bad[r, c] = v
        with pytest.raises(ValueError, match=f"colour row {r}"):
            validate_colour(bad)
    with pytest.raises(ValueError, match=r"float32 \[N, 5\]"):
        validate_colour(good.astype(np.float64))
    with pytest.raises(ValueError, match=r"float32 \[N, 5\]"):
        validate_colour(good[:, :4])


@pytest.fixture(scope="module")
def shard_dir(tmp_path_factory):
    from tony_amd.data.images import write_shards

    d = str(tmp_path_factory.mktemp("shards"))
    rng = np.random.default_rng(4)
    images = rng.integers(0, 256, (24, 40, 44, 3), dtype=np.uint8)
    write_shards(d, images, np.arange(24) % 10, per_shard=7)
    return d, images


def test_plan_boxes_do_not_depend_on_colour_and_plan_colour_is_pure(shard_dir):
    from tony_amd.data.images import ImageBatches
    from tony_amd.ops.image import preprocess

    d, images = shard_dir
    kw = dict(train=True, model="inception", seed=5, rank=1, world=2)
    with ImageBatches(d, 4, 35, **kw) as none, ImageBatches(d, 4, 35, colour="fast", **kw) as fast, \
            ImageBatches(d, 4, 35, colour="full", **kw) as full:
        assert none.plan_colour(0) is None
        for t in (0, 1, 5):
            idx, boxes = none.plan(t)
            for other in (fast, full):
                i2, b2 = other.plan(t)
                assert np.array_equal(idx, i2) and np.array_equal(boxes, b2)
            assert set(fast.plan_colour(t)[:, 0].tolist()) == {4.0}
            assert set(full.plan_colour(t)[:, 0].tolist()) <= {0.0, 1.0, 2.0, 3.0}
            assert full.plan_colour(t).shape == (4, 5) and full.plan_colour(t).dtype == np.float32
        tables = [full.plan_colour(t).copy() for t in range(4)]
        assert not np.array_equal(tables[0], tables[1])
        # the loader's batches are preprocess on plan(t) / plan_colour(t), before and after a seek
        seen = {}
        for t in range(3):
            x, _ = full.next()
            idx, boxes = full.plan(t)
            want = preprocess(torch.from_numpy(images[idx]), torch.from_numpy(boxes), 35, torch.float32, full.scale,
                              full.bias, colour=torch.from_numpy(full.plan_colour(t)))
            assert torch.equal(x, want), t
            seen[t] = x.clone()
        full.seek(1)
        assert np.array_equal(full.plan_colour(1), tables[1]) and np.array_equal(full.plan_colour(3), tables[3])
        x, _ = full.next()
        assert torch.equal(x, seen[1])
    with ImageBatches(d, 4, 35, colour="full", **dict(kw, rank=0)) as other_rank:
        assert not np.array_equal(other_rank.plan_colour(0), tables[0])
    with ImageBatches(d, 4, 35, train=False, colour="full") as ev:  # evaluation never distorts
        assert ev.plan_colour(0) is None
    with pytest.raises(ValueError, match="colour"):
        ImageBatches(d, 4, 35, colour="slow")
