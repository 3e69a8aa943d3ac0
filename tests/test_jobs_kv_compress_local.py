"""``mxnet_linreg.py --gradient-compression 2bit``: the kvstore job of tests/test_jobs_local.py through the launcher
on CPU ranks with 2-bit gradient compression (the words over gloo).  The job's gradients are sums over a batch of
1024 rows, so the threshold is of that size: at 1024 a simulation of this recipe (two workers summed as in sync
mode) reaches w = 3.0 and mse 1.0e-4 from the second epoch on; at 256 it reaches 3.0 and then overshoots on its
accumulated residual (mse 0.08 to 1.5 in later epochs).  The bound is the job's own 0.05."""
import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


def test_mxnet_kvstore_linreg_with_2bit_compression(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "mxnet_linreg.py",
                            ["tony.application.framework=mxnet", "tony.scheduler.instances=1",
                             "tony.server.instances=1", "tony.worker.instances=2", "tony.ps.instances=0"],
                            "--kvstore dist_sync --rows 8192 --epochs 4 --lr 0.5 --gradient-compression 2bit "
                            "--gc-threshold 1024")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert ms and all(m["mse"] < 0.05 for m in ms if m["epoch"] == 3)
    assert sorted(m["rank"] for m in ms if m["epoch"] == 3) == [0, 1]


def test_the_flag_takes_only_known_types():
    from tony_amd.jobs import mxnet_linreg

    with pytest.raises(SystemExit) as e:
        mxnet_linreg.main(["--gradient-compression", "1bit"])
    assert e.value.code == 2  # argparse's usage error, before any role runs
