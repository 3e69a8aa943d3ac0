"""The image jobs fed from shards (``--data-dir``) and evaluated with top-1 / top-5 (``--eval-dir``) through the
launcher in local mode on CPU (gloo).  In the dedicated topology the ps task must answer the workers' counter
all-reduce with zeros: a mismatched collective sequence hangs the gang.  The launcher helpers are
tests/test_jobs_local.py's."""
import numpy as np
import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


@pytest.fixture
def data_dir(tmp_path):
    from tony_amd.data.images import write_shards

    d = str(tmp_path / "shards")
    rng = np.random.default_rng(0)
    write_shards(d, rng.integers(0, 256, (8, 64, 64, 3), dtype=np.uint8), rng.integers(0, 1000, 8), per_shard=3)
    return d


def _check(m):
    assert m["eval_images"] == 8
    assert 0 <= m["top1"] <= m["top5"] <= 1
    assert m["images_per_sec"] > 0
    assert m["input_wait_ms_per_step"] >= 0


@pytest.mark.parametrize("mode", ["colocated", "dedicated"])
def test_inception_ps_from_shards_with_eval(conf, data_dir, mode):  # noqa: F811
    rc, client, _ = run_job(conf, "inception_ps.py", ["tony.ps.instances=1", "tony.worker.instances=2"],
                            f"--ps-mode {mode} --batch-size 2 --steps 2 --warmup 1 --data-dir {data_dir} "
                            f"--eval-dir {data_dir} --ema-decay 0.9")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["workers"] == 2 and ms[0]["ps_mode"] == mode
    _check(ms[0])


def test_resnet50_ddp_from_shards_with_eval(conf, data_dir):  # noqa: F811
    rc, client, _ = run_job(conf, "resnet50_ddp.py", ["tony.application.framework=pytorch", "tony.worker.instances=2",
                                                      "tony.ps.instances=0"],
                            f"--batch-size 2 --image-size 32 --steps 2 --warmup 1 --data-dir {data_dir} "
                            f"--eval-dir {data_dir}")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["world"] == 2
    _check(ms[0])
