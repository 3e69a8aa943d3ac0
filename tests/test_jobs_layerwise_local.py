"""The image jobs with ``--optimizer lars`` through the launcher in local mode on CPU ranks (gloo) at tiny shapes:
jobs/inception_ps.py in both PS topologies (the ps task and the workers must issue matching collective sequences
through the deferred applies and the per-tensor all-reduce) and jobs/hvd_resnet50.py with the warm-up / polynomial
schedule.  The launcher helpers are tests/test_jobs_local.py's."""
import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


@pytest.mark.parametrize("mode", ["colocated", "dedicated"])
def test_inception_ps_lars_tiny(conf, mode):  # noqa: F811
    rc, client, _ = run_job(conf, "inception_ps.py", ["tony.ps.instances=1", "tony.worker.instances=2"],
                            f"--ps-mode {mode} --batch-size 2 --image-size 299 --steps 2 --warmup 1 "
                            "--optimizer lars")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["workers"] == 2 and ms[0]["ps_mode"] == mode and ms[0]["images_per_sec"] > 0


def test_hvd_resnet50_lars_with_the_schedule_tiny(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "hvd_resnet50.py",
                            ["tony.application.framework=horovod", "tony.worker.instances=2", "tony.ps.instances=0"],
                            "--batch-size 2 --image-size 64 --steps 2 --warmup 1 --optimizer lars "
                            "--warmup-steps 1 --decay-steps 3")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["size"] == 2 and ms[0]["images_per_sec"] > 0 and ms[0]["optimizer"] == "lars"
    # the last of the three steps: warm-up 1, decay to 0 at step 3, power 2 -> 0.2 * (1 - 1/2)^2
    assert ms[0]["lr"] == pytest.approx(0.1 * 2 * 0.25)
    assert ms[0]["loss"] == ms[0]["loss"]
