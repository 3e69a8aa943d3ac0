"""``inception_ps.py --colour``: the job fed from shards with the recipe's colour distortion through the launcher in
local mode on CPU (gloo), and the flag refused without ``--data-dir``.  The launcher helpers are
tests/test_jobs_local.py's, the shards tests/test_jobs_data_local.py's."""
import pytest

from test_jobs_data_local import data_dir  # noqa: F401 - a fixture
from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


def test_inception_ps_with_full_colour(conf, data_dir):  # noqa: F811
    rc, client, _ = run_job(conf, "inception_ps.py", ["tony.ps.instances=1", "tony.worker.instances=2"],
                            f"--ps-mode colocated --batch-size 2 --steps 2 --warmup 1 --data-dir {data_dir} "
                            f"--colour full")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert len(ms) == 1 and ms[0]["workers"] == 2
    assert ms[0]["colour"] == "full"
    assert ms[0]["images_per_sec"] > 0 and ms[0]["input_wait_ms_per_step"] >= 0


def test_colour_is_refused_without_data_dir():
    from tony_amd.jobs import inception_ps

    with pytest.raises(SystemExit) as e:
        inception_ps.main(["--colour", "full", "--steps", "1"])
    assert e.value.code == 2  # argparse's usage error, before any model is built
