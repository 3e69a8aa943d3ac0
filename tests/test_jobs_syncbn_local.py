"""jobs/resnet50_ddp.py and jobs/hvd_resnet50.py with ``--sync-bn`` through the launcher in local mode on two CPU
ranks (gloo) at the tiny shapes of tests/test_jobs_data_local.py and tests/test_jobs_layerwise_local.py: the jobs
exit 0, the choice is in the log and in the metrics, the loss is finite.  The launcher helpers are
tests/test_jobs_local.py's."""
import math

import pytest

from test_jobs_adasum_local import _stdout
from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


def test_resnet50_ddp_sync_bn_tiny(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "resnet50_ddp.py", ["tony.application.framework=pytorch", "tony.worker.instances=2",
                                                      "tony.ps.instances=0"],
                            "--batch-size 2 --image-size 32 --steps 2 --warmup 1 --sync-bn")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["world"] == 2 and ms[0]["sync_bn"] is True and ms[0]["images_per_sec"] > 0
    assert math.isfinite(ms[0]["loss"])
    assert "sync_bn=True: BatchNorm statistics over the batches of 2 ranks" in _stdout(client)


def test_hvd_resnet50_sync_bn_tiny(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "hvd_resnet50.py",
                            ["tony.application.framework=horovod", "tony.worker.instances=2", "tony.ps.instances=0"],
                            "--batch-size 2 --image-size 64 --steps 2 --warmup 1 --sync-bn")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["size"] == 2 and ms[0]["sync_bn"] is True and ms[0]["images_per_sec"] > 0
    assert math.isfinite(ms[0]["loss"])
    assert "sync_bn=True: BatchNorm statistics over the batches of 2 ranks" in _stdout(client)
