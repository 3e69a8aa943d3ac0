"""``mxnet_linreg.py --optimizer rmsprop`` and ``mxnet_sparse_linear.py --optimizer ftrl | adagrad`` through the
launcher on CPU ranks (1 scheduler + 1 server + 2 workers, dist_sync, the payloads over gloo): the setting reaches the
server, the job logs and records its optimizer, finishes, and ends with a lower loss than it started with."""
import os

import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)

CONFS = ["tony.application.framework=mxnet", "tony.scheduler.instances=1", "tony.server.instances=1",
         "tony.worker.instances=2", "tony.ps.instances=0"]


def _logged(client, text):
    """Whether a task's stdout holds ``text``."""
    for root, _, files in os.walk(os.path.join(client.job_dir, "logs")):
        for f in files:
            if f == "stdout":
                with open(os.path.join(root, f), errors="replace") as fh:
                    if text in fh.read():
                        return True
    return False


def test_linreg_job_under_rmsprop(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "mxnet_linreg.py", CONFS,
                            "--kvstore dist_sync --rows 8192 --epochs 8 --lr 0.1 --optimizer rmsprop")
    assert rc == 0, _diag(client)  # (the job's own bound: a final mse under 0.05)
    ms = _metrics(client)
    assert ms and all(m["optimizer"] == "rmsprop" for m in ms)
    assert _logged(client, "optimizer rmsprop")
    for rank in (0, 1):
        mse = [m["mse"] for m in sorted((m for m in ms if m["rank"] == rank), key=lambda m: m["epoch"])]
        assert len(mse) == 8 and mse[-1] < mse[0] and mse[-1] < 0.05, mse


@pytest.mark.parametrize("opt,lr", [("ftrl", 0.5), ("adagrad", 0.1)])
def test_sparse_linear_job_under_lazy_kinds(conf, opt, lr):  # noqa: F811
    rc, client, _ = run_job(conf, "mxnet_sparse_linear.py", CONFS,
                            "--kvstore dist_sync --device cpu --features 512 --dim 8 --samples 4096 --batch-size 256 "
                            f"--epochs 3 --lr {lr} --optimizer {opt}")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert ms and all(m["optimizer"] == opt for m in ms)
    assert _logged(client, f"optimizer {opt}")
    for rank in (0, 1):
        loss = [m["loss"] for m in sorted((m for m in ms if m.get("rank") == rank and "epoch" in m),
                                          key=lambda m: m["epoch"])]
        assert len(loss) == 3 and loss[-1] < loss[0], loss
    final = {m["rank"]: m["table_sha256"] for m in ms if m.get("final")}
    assert sorted(final) == [0, 1] and final[0] == final[1]  # both workers pull the same table


def test_the_jobs_take_the_listed_optimizers_and_no_other(monkeypatch):
    """In process, on a local store: a listed kind gets past the argument parser and trains; an unlisted one is
    argparse's usage error before any role runs."""
    from tony_amd.jobs import mxnet_linreg, mxnet_sparse_linear

    monkeypatch.delenv("DMLC_ROLE", raising=False)
    assert mxnet_linreg.main(["--kvstore", "local", "--rows", "4096", "--epochs", "8", "--optimizer", "adagrad",
                              "--lr", "0.5"]) == 0
    assert mxnet_sparse_linear.main(["--kvstore", "local", "--device", "cpu", "--features", "256", "--dim", "4",
                                     "--samples", "1024", "--batch-size", "256", "--epochs", "2", "--optimizer",
                                     "ftrl", "--lr", "0.5"]) == 0
    for job in (mxnet_linreg, mxnet_sparse_linear):
        with pytest.raises(SystemExit) as e:
            job.main(["--optimizer", "adadelta"])
        assert e.value.code == 2
