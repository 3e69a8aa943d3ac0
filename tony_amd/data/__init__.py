"""Input pipelines of the image jobs (``images``: uint8 ``.npy`` shards -> device batches)."""
