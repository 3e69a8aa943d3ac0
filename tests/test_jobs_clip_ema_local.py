"""jobs/inception_ps.py with the full published recipe (``--optimizer rmsprop_tf --clip-norm 2 --ema-decay``)
through the launcher in local mode on CPU (gloo), in both PS topologies: the ps task and the workers must issue
matching collective sequences through the deferred applies, the partial-block all-reduce and ``ema_weights()``.
The launcher helpers are tests/test_jobs_local.py's."""
import os
import re

import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


def _stdout(client):
    out = []
    for root, _, files in os.walk(os.path.join(client.job_dir, "logs")):
        for f in files:
            if f in ("stdout", "stderr"):
                with open(os.path.join(root, f), errors="replace") as fh:
                    out.append(fh.read())
    return "\n".join(out)


@pytest.mark.parametrize("mode", ["colocated", "dedicated"])
def test_inception_ps_full_recipe_tiny(conf, mode):  # noqa: F811
    rc, client, _ = run_job(conf, "inception_ps.py", ["tony.ps.instances=1", "tony.worker.instances=2"],
                            f"--ps-mode {mode} --batch-size 2 --image-size 299 --steps 2 --warmup 1 "
                            "--optimizer rmsprop_tf --clip-norm 2 --ema-decay 0.9")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["workers"] == 2 and ms[0]["ps_mode"] == mode and ms[0]["images_per_sec"] > 0
    text = _stdout(client)
    losses = re.findall(r"loss on the EMA weights \(decay 0\.9\): ([0-9.]+|nan|inf)", text)
    assert len(losses) == 2, text[-2000:]  # one line per worker
    assert all(float(v) == float(v) and float(v) < 1e3 for v in losses)
    assert re.search(r"images/sec total over 2 workers \(%s PS\)" % mode, text)  # the final rate line, unchanged
