"""tony_amd/data/images.py on CPU: shard reading, rank sharding, seeking, the evaluation mode and shutdown."""
import threading

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    """24 random images of 12 x 10 in shards of 5: a shard boundary falls inside a batch of 4."""
    from tony_amd.data.images import write_shards

    d = str(tmp_path_factory.mktemp("shards"))
    images = np.random.default_rng(1).integers(0, 256, (24, 12, 10, 3), dtype=np.uint8)
    labels = np.arange(24, dtype=np.int64) * 7 % 1000
    assert write_shards(d, images, labels, per_shard=5) == 5
    return d, images, labels


def test_one_epoch_covers_every_index_once_across_ranks(shards):
    from tony_amd.data.images import ImageBatches

    d, images, labels = shards
    seen = []
    for rank in (0, 1):
        with ImageBatches(d, 4, 8, train=True, device="cpu", seed=3, rank=rank, world=2) as b:
            assert len(b) == 3
            for t in range(len(b)):
                idx, boxes = b.plan(t)
                x, y = b.next()
                assert x.shape == (4, 3, 8, 8) and x.dtype == torch.float32 and y.dtype == torch.int64
                assert torch.equal(y, torch.from_numpy(labels[idx]))  # labels follow the samples across shards
                seen.extend(idx.tolist())
            nxt, _ = b.plan(len(b))  # the next epoch is another permutation
            assert len(nxt) == 4
    assert sorted(seen) == list(range(24))


def test_batches_are_the_preprocessed_samples(shards):
    from tony_amd.data.images import ImageBatches
    from tony_amd.ops.image import normalisation, preprocess

    d, images, _ = shards
    with ImageBatches(d, 4, 9, train=True, model="resnet", device="cpu", seed=0) as b:
        b.seek(1)  # indices 4..7 of the permutation: spans shards
        idx, boxes = b.plan(1)
        x, _ = b.next()
        want = preprocess(torch.from_numpy(images[idx]), torch.from_numpy(boxes), 9, torch.float32,
                          *normalisation("resnet"))
        assert torch.equal(x, want)


def test_seek_reproduces_a_batch_bit_for_bit(shards):
    from tony_amd.data.images import ImageBatches

    d, _, _ = shards
    with ImageBatches(d, 4, 8, train=True, device="cpu", seed=9) as b:
        got = [tuple(t.clone() for t in b.next()) for _ in range(8)]  # into the second epoch (6 batches each)
        for t in (5, 0, 7, 2):
            b.seek(t)
            x, y = b.next()
            assert torch.equal(x, got[t][0]) and torch.equal(y, got[t][1]), t
            assert b.t == t + 1
    with ImageBatches(d, 4, 8, train=True, device="cpu", seed=9) as fresh:  # a resumed job: a new loader, seek
        fresh.seek(6)
        x, y = fresh.next()
        assert torch.equal(x, got[6][0]) and torch.equal(y, got[6][1])
    with ImageBatches(d, 4, 8, train=True, device="cpu", seed=10) as other:
        assert not torch.equal(other.next()[0], got[0][0])


def test_eval_mode_is_the_central_crop_in_file_order(shards):
    from tony_amd.data.images import ImageBatches
    from tony_amd.ops.image import central_boxes, normalisation, preprocess

    d, images, labels = shards
    with ImageBatches(d, 5, 6, train=False, device="cpu", rank=1, world=2) as b:
        assert len(b) == 3  # 12 samples: 5 + 5 + 2
        xs, ys = zip(*[(x.clone(), y.clone()) for x, y in b])
        assert [len(y) for y in ys] == [5, 5, 2]
        mine = np.arange(1, 24, 2)
        assert torch.equal(torch.cat(ys), torch.from_numpy(labels[mine]))
        boxes = central_boxes(12, 12, 10, 0.875)
        assert boxes[0].tolist() == [0, 0, 12, 10, 0]  # int(0.75) = int(0.625) = 0
        want = preprocess(torch.from_numpy(images[mine]), torch.from_numpy(boxes), 6, torch.float32,
                          *normalisation("inception"))
        assert torch.equal(torch.cat(xs), want)
        assert isinstance(b.wait_ms, float) and b.wait_ms >= 0.0


def test_close_joins_every_thread(shards):
    from tony_amd.data.images import ImageBatches

    d, _, _ = shards
    before = set(threading.enumerate())
    b = ImageBatches(d, 8, 8, train=True, device="cpu")
    b.next()
    assert any(t.name.startswith("tony-image") for t in threading.enumerate())
    b.close()
    b.close()  # idempotent
    assert set(threading.enumerate()) <= before
    with pytest.raises(RuntimeError):
        b.next()


def test_refuses_what_it_cannot_serve(shards, tmp_path):
    from tony_amd.data.images import ImageBatches, write_shards

    d, _, _ = shards
    with pytest.raises(FileNotFoundError):
        ImageBatches(str(tmp_path), 4, 8)
    with pytest.raises(ValueError):
        ImageBatches(d, 16, 8, train=True, world=2)  # 12 samples per rank do not fill a batch of 16
    with pytest.raises(ValueError):
        write_shards(str(tmp_path), np.zeros((2, 4, 4, 3), dtype=np.float32), [0, 1], 2)
