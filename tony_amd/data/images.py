"""Image shards and the loader that feeds the image jobs.

Shard format: a directory of ``images_00000.npy`` (uint8 ``[n, H, W, 3]``, one ``H x W`` per directory) and
``labels_00000.npy`` (int64 ``[n]``), read with ``numpy.load(mmap_mode="r")``; ``write_shards`` produces them.
Nothing is decoded and nothing is downloaded.

``ImageBatches`` yields ``(x, y)``: ``x`` the channels_last ``[batch, 3, size, size]`` model input made by
``ops.image.preprocess`` (random crop + flip for training, with ``colour="fast" | "full"`` followed by Inception's
colour distortion from a per-sample table; the 0.875 central crop for evaluation, never distorted), ``y`` int64
labels.  Batch ``t``'s sample indices and boxes are a pure function of ``(seed, rank, world, t)``: the epoch
permutation comes from ``(seed, epoch)`` and is dealt to the ranks round-robin, the boxes from
``(seed, rank, world, t)``, the colour table from a stream of its own keyed ``(seed, rank, world, t, 1)``, so
``seek(t)`` is all a resumed job needs and checkpoints do not change.

A background thread gathers batch ``t+1`` from the memory-mapped shards into one of two staging slots (pinned on
a GPU) while the step of batch ``t`` runs; on a GPU the slot and its box table go host-to-device on a copy stream
with an event, and ``next()`` makes the current stream wait for the event and launches the preprocess kernel.
``wait_ms`` accumulates the host time ``next()`` spent blocked on the filler thread while the filler was working:
about 0 when the input keeps up.  With two slots the filler cannot refill a slot before the GPU has taken its
previous batch, so a host that runs ahead of the GPU (a replayed step) also blocks in ``next()``; that time is the
GPU's back-pressure, not the input's, and is accumulated apart in ``backpressure_ms``.

ONE persistent output tensor: every ``next()`` writes the same ``x`` (and ``y``), so the graph-mode ``Trainer``
adopts it as its static input and never copies.  This is safe because ``Trainer.step`` joins the weight-gradient
side stream and the branch streams back into the caller's stream before it returns (``ops/streams.py`` ``end()``,
called from ``Trainer._body``; the stem's weight gradient, the last reader of ``x``, runs there), and the native
plan replays the captured joins: the next preprocess launch, on the caller's stream, is ordered after every reader
of the previous batch.  A caller that keeps a batch across ``next()`` must clone it.
"""
from __future__ import annotations

import collections
import glob
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import image

FILL_WORKERS = 4  # threads that gather one batch from the shards (a constant: never the machine's CPU count)
EVAL_FRACTION = 0.875


def write_shards(directory: str, images: np.ndarray, labels: Sequence[int], per_shard: int) -> int:
    """Write ``images`` (uint8 ``[n, H, W, 3]``) and ``labels`` as shards of ``per_shard`` samples; returns the
    number of shards."""
    images = np.asarray(images)
    labels = np.asarray(labels, dtype=np.int64)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError(f"images must be uint8 [n, H, W, 3], got {images.dtype} {images.shape}")
    if labels.shape != (images.shape[0],) or per_shard < 1:
        raise ValueError("one label per image and per_shard >= 1")
    os.makedirs(directory, exist_ok=True)
    count = 0
    for k, a in enumerate(range(0, images.shape[0], per_shard)):
        np.save(os.path.join(directory, f"images_{k:05d}.npy"), images[a:a + per_shard])
        np.save(os.path.join(directory, f"labels_{k:05d}.npy"), labels[a:a + per_shard])
        count += 1
    return count


class _Shards:
    """The memory-mapped shards of one directory as one indexable set."""

    def __init__(self, directory: str):
        paths = sorted(glob.glob(os.path.join(directory, "images_*.npy")))
        if not paths:
            raise FileNotFoundError(f"no images_*.npy shard in {directory}")
        self.images, labels = [], []
        for p in paths:
            im = np.load(p, mmap_mode="r")
            lb = np.load(os.path.join(os.path.dirname(p), os.path.basename(p).replace("images_", "labels_")))
            if im.dtype != np.uint8 or im.ndim != 4 or im.shape[3] != 3 or lb.shape != (im.shape[0],):
                raise ValueError(f"{p}: expected uint8 [n, H, W, 3] with n int64 labels")
            if self.images and im.shape[1:] != self.images[0].shape[1:]:
                raise ValueError(f"{p}: {im.shape[1:3]} images in a directory of {self.images[0].shape[1:3]}")
            self.images.append(im)
            labels.append(lb.astype(np.int64))
        self.labels = np.concatenate(labels)
        self.starts = np.cumsum([0] + [im.shape[0] for im in self.images])
        self.n = int(self.starts[-1])
        self.H, self.W = (int(v) for v in self.images[0].shape[1:3])

    def gather(self, dst: np.ndarray, idx: np.ndarray) -> None:
        which = np.searchsorted(self.starts, idx, side="right") - 1
        for j, (s, i) in enumerate(zip(which, idx)):
            dst[j] = self.images[s][i - self.starts[s]]


class ImageBatches:
    def __init__(self, directory: str, batch: int, size: int, train: bool = True, model: str = "inception",
                 device="cpu", dtype=torch.float32, seed: int = 0, rank: int = 0, world: int = 1,
                 colour: str = "none"):
        if not 0 <= rank < world or batch < 1:
            raise ValueError(f"rank {rank} of {world}, batch {batch}")
        if colour not in ("none", "fast", "full"):
            raise ValueError(f"colour must be 'none', 'fast' or 'full', got {colour!r}")
        self.colour = colour if train else "none"  # evaluation never distorts
        self.shards = _Shards(directory)
        self.batch, self.size, self.train, self.dtype = int(batch), int(size), bool(train), dtype
        self.device = torch.device(device)
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.scale, self.bias = image.normalisation(model)
        self._boxes = image.inception_train_boxes if model == "inception" else image.resnet_train_boxes
        n = self.shards.n
        if train:
            self._share = n // world  # every rank the same number of samples per epoch: the remainder is dropped
            self._per_epoch = self._share // batch
            if self._per_epoch < 1:
                raise ValueError(f"{n} images over {world} ranks do not fill one batch of {batch}")
        else:
            self._eval_idx = np.arange(rank, n, world, dtype=np.int64)  # file order, dealt round-robin
            self._per_epoch = -(-len(self._eval_idx) // batch)
        self._perm = (None, None)
        self.wait_ms = 0.0
        self.backpressure_ms = 0.0
        self.fill_ms, self.filled = 0.0, 0  # the filler's own working time, and the batches it made
        self._gates = collections.deque(maxlen=8)  # (start, end) of the filler's waits for a slot still in flight
        self.t = 0
        H, W, on_gpu = self.shards.H, self.shards.W, self.device.type == "cuda"
        pin = dict(pin_memory=True) if on_gpu else {}
        self._stage = [torch.empty((batch, H, W, 3), dtype=torch.uint8, **pin) for _ in range(2)]
        self._stage_box = [torch.zeros((batch, 5), dtype=torch.int32, **pin) for _ in range(2)]
        self._stage_lab = [torch.zeros(batch, dtype=torch.int64, **pin) for _ in range(2)]
        self.x = torch.empty((batch, size, size, 3), dtype=dtype, device=self.device).permute(0, 3, 1, 2)
        self.y = torch.zeros(batch, dtype=torch.int64, device=self.device)
        self._stage_col = self._dev_col = self._scratch = None
        if self.colour != "none":  # the colour table travels as the boxes do
            self._stage_col = [torch.zeros((batch, 5), dtype=torch.float32, **pin) for _ in range(2)]
        if on_gpu:
            self._dev = [torch.empty((batch, H, W, 3), dtype=torch.uint8, device=self.device) for _ in range(2)]
            self._dev_box = [torch.zeros((batch, 5), dtype=torch.int32, device=self.device) for _ in range(2)]
            self._dev_lab = [torch.zeros(batch, dtype=torch.int64, device=self.device) for _ in range(2)]
            if self.colour != "none":
                self._dev_col = [torch.zeros((batch, 5), dtype=torch.float32, device=self.device) for _ in range(2)]
            if self.colour == "full":  # the contrast statistics of one launch
                self._scratch = torch.empty(image.colour_scratch_floats(batch, size, size), dtype=torch.float32,
                                            device=self.device)
            self._copy = torch.cuda.Stream(self.device)
            self._copied = [torch.cuda.Event() for _ in range(2)]  # slot k's host-to-device copy
            self._read = [None, None]  # slot k's device copy read by the preprocess launch
        self._pool = ThreadPoolExecutor(FILL_WORKERS, thread_name_prefix="tony-image-fill")
        self._thread: Optional[threading.Thread] = None
        self._closed = False
        self._start(0)

    def __len__(self) -> int:
        """Batches per epoch of this rank (the last evaluation batch may be short)."""
        return self._per_epoch

    # -- what batch t is ---------------------------------------------------------------------------------

    def plan(self, t: int) -> Tuple[np.ndarray, np.ndarray]:
        """(sample indices, box table) of batch ``t``: a pure function of (seed, rank, world, t)."""
        epoch, i = divmod(int(t), self._per_epoch)
        H, W = self.shards.H, self.shards.W
        if not self.train:
            idx = self._eval_idx[i * self.batch:(i + 1) * self.batch]
            return idx, image.central_boxes(len(idx), H, W, EVAL_FRACTION)
        if self._perm[0] != epoch:
            perm = np.random.default_rng([self.seed, epoch]).permutation(self.shards.n)
            self._perm = (epoch, perm[self.rank::self.world][:self._share])
        idx = self._perm[1][i * self.batch:(i + 1) * self.batch]
        rng = np.random.default_rng([self.seed, self.rank, self.world, int(t)])
        return idx, self._boxes(rng, len(idx), H, W)

    def plan_colour(self, t: int) -> Optional[np.ndarray]:
        """The colour table (``ops.image.inception_colour_params``) of batch ``t``, from an rng stream of its own:
        a pure function of (seed, rank, world, t).  ``None`` without colour distortion."""
        if self.colour == "none":
            return None
        rng = np.random.default_rng([self.seed, self.rank, self.world, int(t), 1])
        return image.inception_colour_params(rng, self.batch, fast=self.colour == "fast")  # training batches are full

    # -- the filler thread ---------------------------------------------------------------------------------

    def _start(self, t: int) -> None:
        self._free: "queue.Queue" = queue.Queue()
        self._ready: "queue.Queue" = queue.Queue()
        self._pending = None
        self.t = self._fill_t = int(t)
        for k in range(2):
            self._free.put((k, None))
        self._thread = threading.Thread(target=self._fill_loop, args=(self._free, self._ready),
                                        name="tony-image-filler", daemon=True)
        self._thread.start()

    def _stop(self) -> None:
        if self._thread is not None:
            self._free.put(None)
            self._thread.join()
            self._thread = None
        if self.device.type == "cuda":
            self._copy.synchronize()  # no copy still reads a staging slot

    def _fill_loop(self, free, ready) -> None:
        try:
            while True:
                item = free.get()
                if item is None:
                    return
                k, copied = item
                if copied is not None:
                    g0 = time.perf_counter()
                    copied.synchronize()  # the slot's previous batch has left the host
                    self._gates.append((g0, time.perf_counter()))
                f0 = time.perf_counter()
                t, self._fill_t = self._fill_t, self._fill_t + 1
                idx, boxes = self.plan(t)
                m = len(idx)
                dst = self._stage[k].numpy()
                if m >= 2 * FILL_WORKERS:
                    cuts = np.linspace(0, m, FILL_WORKERS + 1).astype(int)
                    jobs = [self._pool.submit(self.shards.gather, dst[a:b], idx[a:b]) for a, b in zip(cuts, cuts[1:])]
                    for j in jobs:
                        j.result()
                else:
                    self.shards.gather(dst[:m], idx)
                self._stage_box[k].numpy()[:m] = boxes
                if self.colour != "none":
                    self._stage_col[k].numpy()[:m] = self.plan_colour(t)
                self._stage_lab[k].numpy()[:m] = self.shards.labels[idx]
                self.fill_ms += (time.perf_counter() - f0) * 1e3
                self.filled += 1
                ready.put((t, k, m))
        except BaseException as e:  # noqa: BLE001 - handed to next(), which raises it on the caller's thread
            ready.put(e)

    def _stage_next(self) -> None:
        """Take the next filled slot (blocking on the filler: counted in ``wait_ms``) and, on a GPU, start its
        host-to-device copy on the copy stream."""
        t0 = time.perf_counter()
        item = self._ready.get()
        t1 = time.perf_counter()
        # of the time blocked, the part the filler itself spent waiting for the GPU to take a slot's last batch
        gated = sum(max(0.0, min(e, t1) - max(b, t0)) for b, e in list(self._gates))
        self.backpressure_ms += gated * 1e3
        self.wait_ms += max(0.0, t1 - t0 - gated) * 1e3
        if isinstance(item, BaseException):
            raise RuntimeError("the image filler thread failed") from item
        t, k, m = item
        if self.device.type == "cuda":
            with torch.cuda.stream(self._copy):
                if self._read[k] is not None:
                    self._copy.wait_event(self._read[k])  # the launch that read the slot's previous batch
                self._dev[k][:m].copy_(self._stage[k][:m], non_blocking=True)
                self._dev_box[k][:m].copy_(self._stage_box[k][:m], non_blocking=True)
                if self.colour != "none":
                    self._dev_col[k][:m].copy_(self._stage_col[k][:m], non_blocking=True)
                self._dev_lab[k][:m].copy_(self._stage_lab[k][:m], non_blocking=True)
                self._copied[k].record(self._copy)
            self._free.put((k, self._copied[k]))  # the filler refills the slot once the copy has read it
        self._pending = (t, k, m)

    # -- the caller's side ---------------------------------------------------------------------------------

    def next(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Batch ``self.t`` in the persistent ``(x, y)`` (views of their first rows for a short last batch)."""
        if self._closed:
            raise RuntimeError("ImageBatches is closed")
        if self._pending is None:
            self._stage_next()
        t, k, m = self._pending
        assert t == self.t, (t, self.t)
        x, y = (self.x, self.y) if m == self.batch else (self.x[:m], self.y[:m])
        if self.device.type == "cuda":
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._copied[k])
            image.preprocess(self._dev[k][:m], self._dev_box[k][:m], self.size, self.dtype, self.scale, self.bias,
                             out=x, **self._colour_args(self._dev_col, k, m))
            y.copy_(self._dev_lab[k][:m], non_blocking=True)
            if self._read[k] is None:
                self._read[k] = torch.cuda.Event()
            self._read[k].record(cur)
        else:
            image.preprocess(self._stage[k][:m], self._stage_box[k][:m], self.size, self.dtype, self.scale,
                             self.bias, out=x, **self._colour_args(self._stage_col, k, m))
            y.copy_(self._stage_lab[k][:m])
            self._free.put((k, None))
        self._pending = None
        self.t = t + 1
        self._stage_next()  # batch t+1's copy overlaps the step of batch t
        return x, y

    def _colour_args(self, slots, k: int, m: int) -> dict:
        """``preprocess``'s colour arguments for slot ``k``: none at all without colour distortion."""
        if self.colour == "none":
            return {}
        return dict(colour=slots[k][:m], colour_has_contrast=self.colour == "full", scratch=self._scratch)

    def __iter__(self):
        """One epoch of this rank from batch 0."""
        self.seek(0)
        for _ in range(self._per_epoch):
            yield self.next()

    def seek(self, t: int) -> None:
        """Continue with batch ``t`` (resume: the batches are a pure function of ``t``)."""
        if self._closed:
            raise RuntimeError("ImageBatches is closed")
        if int(t) == self.t:
            return
        self._stop()
        self._start(t)

    def close(self) -> None:
        """Join the filler thread and its pool."""
        if self._closed:
            return
        self._closed = True
        self._stop()
        self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter teardown
            pass
