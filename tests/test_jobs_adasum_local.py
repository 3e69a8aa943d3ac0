"""jobs/hvd_mnist.py with ``--adasum`` through the launcher in local mode on two CPU ranks (gloo): the job passes
``op=hvd.Adasum``, says so in its log, does not scale the learning rate by the number of ranks, and trains (a finite,
falling loss).  The launcher helpers are tests/test_jobs_local.py's."""
import math
import os

import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


def _stdout(client):
    out = []
    for root, _, files in os.walk(os.path.join(client.job_dir, "logs")):
        for f in files:
            with open(os.path.join(root, f), errors="replace") as fh:
                out.append(fh.read())
    return "\n".join(out)


def test_hvd_mnist_adasum(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "hvd_mnist.py", ["tony.application.framework=horovod", "tony.worker.instances=2"],
                            "--steps 12 --adasum")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["size"] == 2 and ms[0]["op"] == "Adasum"
    assert "gradient reduction op=Adasum lr=0.001" in _stdout(client)  # the operator, and the rate as it was given
    first, last = ms[0]["first_loss"], ms[0]["avg_last_loss"]
    assert math.isfinite(first) and math.isfinite(last) and last < first
